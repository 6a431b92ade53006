"""MaskFormerSemanticCocoMixDatasetMapper with device= a HIP device (K14 does the pixels) against the same mapper on the host, tensor for tensor, on
seeded draws; its gt_classes / gt_masks against np.unique of the host's sem_seg; the device path never reaching Pillow or K12b; and one fine-tune step
fed by the mapper: mapper -> finetune_outputs -> prepare_targets -> criterion_from_cfg -> backward on the tiny seeded model of the fine-tune tests."""
import copy
import random

import numpy as np
import pytest
import torch

from tests import _train_view_cases as C

pytestmark = pytest.mark.gpu


class _Objects(list):
    """what the mapper needs of CocoOodObjects: [i] -> (RGB uint8 [bh,bw,3], mask uint8 [bh,bw]) and the sized view box_hw"""

    @property
    def box_hw(self):
        return [m.shape[:2] for _, m in self]


def _objects():
    obj, mask = C.ood_object(20, 30, holes=True)
    small, small_mask = C.ood_object(6, 9)
    as_item = lambda o, m: (np.ascontiguousarray(o.numpy().transpose(1, 2, 0)), m.numpy())      # noqa: E731
    return _Objects([as_item(obj, mask), (np.zeros((0, 0, 3), np.uint8), np.zeros((0, 0), np.uint8)), as_item(small, small_mask)])


def _cfg(**inp):
    from rba_amd.config import CfgNode
    base = dict(MIN_SIZE_TRAIN=[24, 31, 48, 64, 96], MAX_SIZE_TRAIN=4096, CROP=CfgNode(ENABLED=True, TYPE="absolute", SIZE=[24, 48]), COLOR_AUG_SSD=True,
                FORMAT="RGB", OOD_PROB=0.8, REPEAT_INSTANCE_MASKS=1)
    base.update(inp)
    return CfgNode(INPUT=CfgNode(**base))


def _pair(cfg, seed):
    from rba_amd.dataset_mappers import MaskFormerSemanticCocoMixDatasetMapper as Mapper
    make = lambda device: Mapper(cfg, device=device, coco=_objects(), np_rng=np.random.RandomState(seed), py_rng=random.Random(seed))      # noqa: E731
    return make(None), make("cuda")


@pytest.mark.parametrize("seed", range(10))
def test_device_mapper_equals_the_host_mapper(seed):
    img, lab = C.frame(48, 96)
    cfg = _cfg(REPEAT_INSTANCE_MASKS=1 + seed % 2, SIZE_DIVISIBILITY=48 if seed % 3 == 0 else -1)
    host, dev = _pair(cfg, 100 + seed)
    for _ in range(2):
        a, b = host({"image": img, "sem_seg_gt": lab}), dev({"image": img, "sem_seg_gt": lab})
        assert set(a) == set(b) == {"image", "sem_seg", "outlier_mask", "instances"}
        for k in ("image", "sem_seg", "outlier_mask"):
            assert b[k].is_cuda and b[k].dtype == a[k].dtype and torch.equal(b[k].cpu(), a[k]), k
        ia, ib = a["instances"], b["instances"]
        assert ib.image_size == ia.image_size == tuple(a["image"].shape[-2:])
        assert torch.equal(ib.gt_classes, ia.gt_classes) and ib.gt_masks.dtype == ia.gt_masks.dtype and torch.equal(ib.gt_masks.cpu(), ia.gt_masks)
        # the reference's own construction on the host's sem_seg
        classes = np.unique(a["sem_seg"].numpy())
        classes = classes[(classes != 255) & (classes != 254)].repeat(cfg.INPUT.REPEAT_INSTANCE_MASKS)
        assert ib.gt_classes.tolist() == classes.tolist() and ib.gt_classes.dtype == torch.int64
        for k, cls in enumerate(classes.tolist()):
            assert torch.equal(ib.gt_masks[k].cpu(), a["sem_seg"] == cls)


def test_the_draws_cover_pastes_and_every_size():
    """the ten seeds above are not ten times the same path"""
    from rba_amd.dataset_mappers import mapper_settings, sample_train_view_params
    s, boxes = mapper_settings(_cfg()), _objects().box_hw
    seen = [sample_train_view_params(s, 48, 96, boxes, np.random.RandomState(100 + seed), random.Random(100 + seed)) for seed in range(10)]
    assert any(p.paste is not None for p in seen) and any(p.paste is None for p in seen) and any(p.flip for p in seen) and any(not p.flip for p in seen)
    assert len({p.new_h for p in seen}) >= 3 and any(p.color.hue for p in seen) and any(p.color.saturation for p in seen)


def test_device_path_reaches_neither_pillow_nor_k12b(monkeypatch):
    from rba_amd import dataset_mappers, ops
    img, lab = C.frame(48, 96)
    host, dev = _pair(_cfg(OOD_PROB=1.0), 7)
    want = host({"image": img, "sem_seg_gt": lab})

    def refuse(*a, **kw):
        raise AssertionError("the device path resized a whole frame")

    monkeypatch.setattr(ops, "resize_u8_pil_bilinear", refuse)
    monkeypatch.setattr(dataset_mappers, "_resize_u8_host", refuse)
    monkeypatch.setattr(dataset_mappers, "train_view_host", refuse)
    try:
        from PIL import Image
        monkeypatch.setattr(Image.Image, "resize", refuse)
    except ImportError:
        pass
    got = dev({"image": img, "sem_seg_gt": lab})
    assert torch.equal(got["image"].cpu(), want["image"]) and torch.equal(got["sem_seg"].cpu(), want["sem_seg"])
    with pytest.raises(AssertionError, match="whole frame"):        # the patch is live: the host path does go through it
        _pair(_cfg(OOD_PROB=1.0), 7)[0]({"image": img, "sem_seg_gt": lab})


def test_one_finetune_step_fed_by_the_mapper():
    from rba_amd.config import CfgNode
    from rba_amd.dataset_mappers import ColorAug, MaskFormerSemanticCocoMixDatasetMapper, TrainViewParams
    from rba_amd.modeling.criterion import criterion_from_cfg
    from tests.test_finetune_heads_gpu import _head_params, _tiny
    model, _, _ = _tiny()
    model = copy.deepcopy(model)
    pred = model.sem_seg_head.predictor
    pred.sparse_intermediate_heads = False
    from rba_amd import arch as A
    K = A.complete(A.ARCHS["tiny1"])["num_classes"]
    img, lab = C.frame(60, 90)
    lab = torch.where(lab == C.IGNORE, lab, lab % K)
    cfg = _cfg(MIN_SIZE_TRAIN=[72], CROP=CfgNode(ENABLED=True, TYPE="absolute", SIZE=[48, 64]))
    cfg["MODEL"] = CfgNode(SEM_SEG_HEAD=CfgNode(NUM_CLASSES=K, IGNORE_VALUE=255),
                           MASK_FORMER=CfgNode(DEC_LAYERS=2, DEEP_SUPERVISION=True, TRAIN_NUM_POINTS=112, OUTLIER_SUPERVISION=True, OUTLIER_LOSS_TARGET="nls",
                                               SCORE_NORM="tanh", OUTLIER_LOSS_FUNC="squared_hinge", CLASS_WEIGHT=2.0, MASK_WEIGHT=5.0, DICE_WEIGHT=5.0))
    mapper = MaskFormerSemanticCocoMixDatasetMapper(cfg, device="cuda", coco=_objects())
    params = TrainViewParams(new_h=72, new_w=108, crop=(10, 20, 48, 64), flip=True, ood_index=0, paste=(15, 30),
                             color=ColorAug(brightness=True, beta=9.5, order=True, saturation=True, saturation_alpha=1.2, hue=True, hue_delta=7))
    d = mapper({"image": img, "sem_seg_gt": lab}, params=params)
    assert int((d["outlier_mask"] == 1).sum()) > 0 and int((d["outlier_mask"] == 0).sum()) > 0 and len(d["instances"]) > 0
    for p in model.parameters():
        p.requires_grad_(True)
        p.grad = None
    outputs, sizes, padded = model.finetune_outputs([d])
    assert sizes == [(48, 64)]
    targets = model.prepare_targets([d], padded)
    assert tuple(targets[0]["masks"].shape[1:]) == tuple(padded) and targets[0]["masks"].is_cuda and torch.equal(targets[0]["outlier_masks"], d["outlier_mask"])
    criterion = criterion_from_cfg(cfg)
    losses = criterion(outputs, targets)
    weighted = criterion.weighted(losses)
    total = sum(v for v in weighted.values() if v.requires_grad)
    assert {"loss_ce", "loss_mask", "loss_dice", "outlier_loss"} <= set(weighted) and bool(torch.isfinite(total))
    total.backward()
    heads = _head_params(pred)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0 for p in heads.values())
