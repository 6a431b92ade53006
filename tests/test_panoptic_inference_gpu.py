"""GPU: MaskFormer.panoptic_inference and forward() with TEST.PANOPTIC_ON on the K16 kernels (docs/kernels/K16.md) against the oracle's restatement of
the reference (oracle.ref_ops.panoptic_inference, fp64), the up4 path against the materialised planes, and the memory the closed-set merge may take.

The scenarios come from tests/_panoptic_cases.py, which asserts the decision margins on the CPU: panoptic_seg and segments_info are compared exactly."""
import numpy as np
import pytest
import torch

from tests import _panoptic_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run rba_amd.panoptic_ops' allocations under the guard bands too"""
    import rba_amd.panoptic_ops as pops
    if canary is None:
        yield
        return
    real, pops.torch = pops.torch, canary._PROXY
    try:
        yield
    finally:
        pops.torch = real


@pytest.fixture(scope="module")
def model():
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS["tiny1"])
    m = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()
    m.thing_classes = C.THING_CLASSES
    return m


_ORACLE = {}


def _oracle(name, open_p):
    """the scenario and the oracle's answer, computed once per (scenario, open_p) and left unchanged"""
    from oracle import ref_ops
    if (name, open_p) not in _ORACLE:
        mask_cls, mask_pred = getattr(C, name)()
        _ORACLE[name, open_p] = (mask_cls, mask_pred) + tuple(ref_ops.panoptic_inference(
            mask_cls, mask_pred, set(C.THING_CLASSES), C.OBJECT_MASK_THRESHOLD, C.OVERLAP_THRESHOLD, open_p, -0.3, 50))
    return _ORACLE[name, open_p]


@pytest.mark.parametrize("open_p", [False, True])
@pytest.mark.parametrize("name", ["box_scenario", "many_query_scenario"])
def test_panoptic_inference_equals_the_oracle(model, name, open_p):
    mask_cls, mask_pred, pan, info, rba = _oracle(name, open_p)
    model.object_mask_threshold, model.overlap_threshold = C.OBJECT_MASK_THRESHOLD, C.OVERLAP_THRESHOLD
    out = model.panoptic_inference(mask_cls.cuda(), mask_pred.cuda(), open_p, -0.3, 50, return_ood_pred=open_p)
    assert out[0].dtype == torch.int32 and np.array_equal(out[0].cpu().numpy(), pan), f"{int((out[0].cpu().numpy() != pan).sum())} pixels differ"
    assert out[1] == info
    closed = [s for s in info if s["category_id"] != 255]
    if name == "box_scenario":
        assert sum(1 for s in closed if s["category_id"] == 3) == 1 and len(closed) == 5, "stuff merges; one query fails the overlap test, one has no intersection"
    else:
        assert len(closed) >= 20
    if open_p:
        assert (out[2].cpu().double() - rba).abs().max().item() < 1e-5
        if name == "box_scenario":
            assert any(s["category_id"] == 255 for s in info), "the scenario must exercise the open-set branch"
        # the RbA map handed over gives what the recomputed one gives
        again = model.panoptic_inference(mask_cls.cuda(), mask_pred.cuda(), True, -0.3, 50, return_ood_pred=True, ood_mask=out[2])
        assert torch.equal(again[0], out[0]) and again[1] == out[1] and again[2] is out[2]
        from rba_amd._lib import RbaHipError
        with pytest.raises(RbaHipError):
            model.panoptic_inference(mask_cls.cuda(), mask_pred.cuda(), True, -0.3, 50, ood_mask=out[2][:-1])


def test_no_kept_query_returns_an_empty_map(model):
    mask_cls, mask_pred, *_ = _oracle("box_scenario", False)
    model.object_mask_threshold = 2.0
    try:
        pan, info = model.panoptic_inference(mask_cls.cuda(), mask_pred.cuda(), True, -0.3, 50)
    finally:
        model.object_mask_threshold = C.OBJECT_MASK_THRESHOLD
    assert info == [] and pan.shape == mask_pred.shape[1:] and pan.dtype == torch.int32 and not bool(pan.any())


def test_forward_up4_path_equals_panoptic_inference_on_the_materialised_planes(model):
    from rba_amd import ops
    g = torch.Generator().manual_seed(13)
    K = model.arch["num_classes"]
    model.object_mask_threshold, model.overlap_threshold = 0.0, 0.0
    bias = model.sem_seg_head.predictor.class_embed.bias
    with torch.no_grad():                                                  # make some queries prefer a non-void class
        bias[:K] += 6.0
    try:
        for open_p in (False, True):
            model.panoptic_on, model.open_panoptic = True, open_p
            for size in ((60, 90), (64, 96)):                              # padded beyond the image / exactly the image: both are x4 of the logits
                im = torch.randint(0, 256, (3,) + size, generator=g, dtype=torch.uint8)
                r = model([{"image": im}], panoptic_ood_threshold=-0.3, panoptic_pixel_min=20, return_panoptic_ood=True)[0]
                mask_cls, mask_pred, sizes, padded = model.predict([{"image": im}])
                assert tuple(mask_pred.shape[-2:]) == (padded[0] // 4, padded[1] // 4) and sizes[0] == size
                mp = ops.resample_bilinear(mask_pred[0].contiguous(), padded)[:, :size[0], :size[1]].contiguous()
                want = model.panoptic_inference(mask_cls[0], mp, open_p, -0.3, 20, True)                       # K1 recomputed on the planes
                handed = model.panoptic_inference(mask_cls[0], mp, open_p, -0.3, 20, True, ood_mask=r["rba"])  # forward()'s map handed over
                got = r["panoptic_seg"]
                assert len(got) == len(want) == (3 if open_p else 2) and len(got[1]) >= 1
                assert got[0].shape == size and torch.equal(got[0], want[0]) and got[1] == want[1]
                assert torch.equal(handed[0], want[0]) and handed[1] == want[1]
                if open_p:
                    assert got[2] is r["rba"] and (got[2] - want[2]).abs().max().item() < 1e-5
        # a requested output size: the planes are materialised and resized a second time; the RbA map of that size is handed over as well (a model built
        # with TEST.PANOPTIC_ON scores the resized mask logits: sem_seg_postprocess_before_inference)
        model.sem_seg_postprocess_before_inference = True
        im = torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8)
        r = model([{"image": im, "height": 45, "width": 70}], panoptic_ood_threshold=-0.3, panoptic_pixel_min=20, return_panoptic_ood=True)[0]
        mask_cls, mask_pred, sizes, padded = model.predict([{"image": im}])
        mp = ops.resample_bilinear(ops.resample_bilinear(mask_pred[0].contiguous(), padded)[:, :60, :90].contiguous(), (45, 70))
        want = model.panoptic_inference(mask_cls[0], mp, True, -0.3, 20, True)
        got = r["panoptic_seg"]
        assert got[0].shape == (45, 70) and torch.equal(got[0], want[0]) and got[1] == want[1] and got[2] is r["rba"]
        assert (got[2] - want[2]).abs().max().item() < 1e-5
    finally:
        with torch.no_grad():
            bias[:K] -= 6.0
        model.panoptic_on = model.open_panoptic = model.sem_seg_postprocess_before_inference = False
        model.object_mask_threshold, model.overlap_threshold = C.OBJECT_MASK_THRESHOLD, C.OVERLAP_THRESHOLD


@pytest.mark.no_canary
def test_the_closed_set_merge_allocates_no_plane_sized_temporary(model):
    """Q = 32 at 256 x 512, every query kept: the peak of allocated device memory over the call rises by less than HALF of mask_pred's bytes (the
    sigmoid plane and the product plane of the torch composition took at least twice those bytes)."""
    g = torch.Generator().manual_seed(32)
    Q, K, H, W = 32, 19, 256, 512
    mask_cls = torch.randn(Q, K + 1, generator=g)
    mask_cls[:, K] -= 20.0
    mask_pred = (torch.randn(Q, H, W, generator=g) * 4).cuda()
    mask_cls = mask_cls.cuda()
    model.object_mask_threshold, model.overlap_threshold = 0.0, 0.0
    try:
        model.panoptic_inference(mask_cls, mask_pred)                      # warm: code objects, the allocator's pools
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        pan, info = model.panoptic_inference(mask_cls, mask_pred)
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
    finally:
        model.object_mask_threshold, model.overlap_threshold = C.OBJECT_MASK_THRESHOLD, C.OVERLAP_THRESHOLD
    plane_bytes = mask_pred.numel() * mask_pred.element_size()
    print(f"peak rise {rise} B, mask_pred {plane_bytes} B")
    assert pan.shape == (H, W) and len(info) >= 1
    assert rise < plane_bytes / 2, f"the merge allocated {rise} B beside mask_pred's {plane_bytes} B"
