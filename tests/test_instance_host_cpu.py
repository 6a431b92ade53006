"""CPU: the host side of instance inference (K17) -- the config flags `arch_from_cfg` now accepts and what it still refuses, the model's attributes, the
generalised `Instances`, the bindings and the wrappers' behaviour without a device."""
import pytest
import torch
import yaml

from rba_amd import arch as A


def _cfg(tmp_path, test=None, top=None, mask_former=None):
    from rba_amd.config import load_cfg
    cfg = {"MODEL": {"META_ARCHITECTURE": "MaskFormer", "BACKBONE": {"NAME": "D2SwinTransformer"},
                     "MASK_FORMER": dict({"TEST": test or {}}, **(mask_former or {}))}}
    cfg.update(top or {})
    (tmp_path / "config.yaml").write_text(yaml.safe_dump(cfg))
    return load_cfg(str(tmp_path / "config.yaml"))


def test_arch_accepts_the_instance_flags(tmp_path):
    a = A.arch_from_cfg(_cfg(tmp_path))
    assert a["semantic_on"] is True and a["instance_on"] is False and a["test_topk_per_image"] == 100 and a["postprocess_before_inference"] is False
    a = A.arch_from_cfg(_cfg(tmp_path, {"INSTANCE_ON": True}, {"TEST": {"DETECTIONS_PER_IMAGE": 37}}))
    assert a["instance_on"] is True and a["semantic_on"] is True and a["test_topk_per_image"] == 37
    assert a["postprocess_before_inference"] is True, "instance inference implies sem_seg_postprocess_before_inference (maskformer_model.py:205-209)"
    a = A.arch_from_cfg(_cfg(tmp_path, {"INSTANCE_ON": True, "SEMANTIC_ON": False, "PANOPTIC_ON": True}))
    assert a["instance_on"] and not a["semantic_on"] and a["panoptic_on"]
    d = A.complete(A.ARCHS["tiny1"])
    assert d["semantic_on"] is True and d["instance_on"] is False and d["test_topk_per_image"] == 100


def test_arch_still_refuses_what_it_refused(tmp_path):
    for kw in (dict(mask_former={"PRE_NORM": True}), dict(mask_former={"ENFORCE_INPUT_PROJ": True}), dict(top={"SOLVER": {"FORCE_REGION_PARTITION": True}})):
        with pytest.raises(NotImplementedError):
            A.arch_from_cfg(_cfg(tmp_path, {"INSTANCE_ON": True}, **kw))


def test_model_carries_the_flags():
    from rba_amd.maskformer_model import MaskFormer
    m = MaskFormer(dict(A.ARCHS["tiny1"], instance_on=True, semantic_on=False, test_topk_per_image=7))
    assert m.instance_on and not m.semantic_on and m.test_topk_per_image == 7 and m.sem_seg_postprocess_before_inference
    assert m.instance_boxes is False and m.instance_mask_dtype is torch.float32
    m = MaskFormer(A.ARCHS["tiny1"])
    assert not m.instance_on and m.semantic_on and not m.sem_seg_postprocess_before_inference
    with pytest.raises(NotImplementedError):
        m([{"image": torch.zeros(3, 8, 8)}], return_aux=True)


def test_instances_keeps_its_constructor_and_carries_prediction_fields():
    from rba_amd.dataset_mappers import Instances
    classes, masks = torch.tensor([0, 2]), torch.zeros(2, 4, 6, dtype=torch.bool)
    inst = Instances((4, 6), classes, masks)
    assert inst.image_size == (4, 6) and inst.gt_classes is classes and inst.gt_masks is masks and len(inst) == 2
    moved = inst.to("cpu")
    assert isinstance(moved, Instances) and moved.image_size == (4, 6) and torch.equal(moved.gt_classes, classes) and torch.equal(moved.gt_masks, masks)
    bare = Instances([4, 6])
    assert bare.gt_classes is None and bare.gt_masks is None and bare.image_size == (4, 6)
    bare.gt_classes = classes
    assert len(bare) == 2
    pred = Instances((4, 6), pred_masks=torch.zeros(3, 4, 6), scores=torch.zeros(3))
    pred.pred_classes = torch.zeros(3, dtype=torch.int64)
    pred.pred_boxes = torch.zeros(3, 4)
    assert len(pred) == 3 and pred.has("pred_boxes") and not pred.has("gt_masks")
    assert set(pred.get_fields()) == {"pred_masks", "scores", "pred_classes", "pred_boxes"}
    moved = pred.to("cpu")
    assert set(moved.get_fields()) == set(pred.get_fields()) and moved.gt_classes is None and len(moved) == 3


def test_k17_entry_points_are_bound_and_the_abi_version_stays():
    import ctypes
    from rba_amd import _lib
    from rba_amd.csrc import build
    names = ("rba_instance_stats_f32", "rba_instance_stats_up4_f32", "rba_instance_masks_f32", "rba_instance_masks_u8", "rba_instance_masks_up4_f32",
             "rba_instance_masks_up4_u8")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.SIGNATURES["rba_instance_masks_f32"][5] is ctypes.c_int64 and len(_lib.SIGNATURES["rba_instance_stats_up4_f32"]) == 11
    assert _lib.EXPECTED_ABI == 191 and _lib.load().rba_hip_version() == 191
    assert "instance_masks.hip" in build.SOURCES
    import rba_amd.instance_ops as iops
    import rba_amd.ops as ops
    assert not any(hasattr(ops, n) for n in iops.__all__ if n != "MAX_QUERIES"), "the K17 wrappers live outside rba_amd.ops"


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """hipErrorInvalidValue (1) before anything touches a device: null pointers, Q outside 1..255, no pixels, a crop outside the x4 map, misalignment"""
    from rba_amd import _lib
    lib = _lib.load()
    p = 1 << 20                                                            # never dereferenced
    assert lib.rba_instance_stats_f32(0, p, p, p, p, 3, 4, 5, None) == 1
    assert lib.rba_instance_stats_f32(p, p, p, p, p, 0, 4, 5, None) == 1
    assert lib.rba_instance_stats_f32(p, p, p, p, p, 256, 4, 5, None) == 1
    assert lib.rba_instance_stats_f32(p, p, p, p, p, 3, 0, 5, None) == 1
    assert lib.rba_instance_stats_f32(p, p, p, p, p, 3, 1 << 16, 1 << 15, None) == 1
    assert lib.rba_instance_stats_f32(p + 2, p, p, p, p, 3, 4, 5, None) == 1
    assert lib.rba_instance_stats_f32(p, p, p, p + 4, p, 3, 4, 5, None) == 1
    assert lib.rba_instance_stats_up4_f32(p, p, p, p, p, 3, 4, 5, 17, 20, None) == 1
    assert lib.rba_instance_stats_up4_f32(p, p, p, p, p, 3, 4, 5, 16, 0, None) == 1
    for fn in (lib.rba_instance_masks_f32, lib.rba_instance_masks_u8):
        assert fn(p, p, 0, 3, 2, 20, None) == 1 and fn(p, p, p, 0, 2, 20, None) == 1 and fn(p, p, p, 3, 0, 20, None) == 1
        assert fn(p, p, p, 3, 65536, 20, None) == 1 and fn(p, p, p, 3, 2, 0, None) == 1 and fn(p, p + 2, p, 3, 2, 20, None) == 1
    assert lib.rba_instance_masks_f32(p, p, p + 2, 3, 2, 20, None) == 1
    for fn in (lib.rba_instance_masks_up4_f32, lib.rba_instance_masks_up4_u8):
        assert fn(p, p, p, 3, 2, 4, 5, 16, 21, None) == 1 and fn(p, p, p, 3, 0, 4, 5, 16, 20, None) == 1


def test_wrappers_have_no_cpu_path():
    from rba_amd import instance_ops as iops
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError, match="no CPU path"):
        iops.instance_stats(torch.zeros(3, 4, 5), torch.ones(3, dtype=torch.uint8))
    with pytest.raises(RbaHipError, match="no CPU path"):
        iops.instance_masks(torch.zeros(3, 4, 5), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RbaHipError, match="no CPU path"):
        iops.instance_segments(torch.zeros(3, 5), torch.zeros(3, 4, 5), 2, 4)
