"""GPU: instance inference end to end on the K17 kernels (docs/kernels/K17.md) -- instance_ops.instance_segments and MaskFormer.instance_inference against
the numpy fp64 restatement of the reference (tests/_instance_cases.py), forward() with TEST.INSTANCE_ON on the up4 path against the materialised planes,
include_void, return_separately, TEST.SEMANTIC_ON: False, and the memory the instance branch may take.

The scenarios assert their decision margins on the CPU: classes, masks and boxes are compared exactly after matching detections on the (query, class)
pair, scores within SCORE_BAR = 1e-6 (derived in tests/_instance_cases.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _instance_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run rba_amd.instance_ops' allocations under the guard bands too"""
    import rba_amd.instance_ops as iops
    if canary is None:
        yield
        return
    real, iops.torch = iops.torch, canary._PROXY
    try:
        yield
    finally:
        iops.torch = real


def _tiny(**arch):
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(dict(A.ARCHS["tiny1"], **arch))
    return load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()


@pytest.fixture(scope="module")
def model():
    return _tiny()


_REFERENCE = {}


def _reference(name, filtered):
    """the scenario and the restatement's answer, computed once per (scenario, filter) and left unchanged"""
    if (name, filtered) not in _REFERENCE:
        mask_cls, mask_pred, topk = C.scenario(name)
        things = C.SCENARIOS[name]["things"] if filtered else None
        _REFERENCE[name, filtered] = (mask_cls, mask_pred, topk, things, C.instance_reference(mask_cls.numpy(), mask_pred.numpy(), topk, things))
    return _REFERENCE[name, filtered]


def _check(masks, classes, scores, boxes, want, with_boxes, where):
    """one result against the restatement.  The result carries no query index; its documented order is descending class score, which is the
    restatement's, and the scenarios hold EVERY pair of neighbouring top-k scores GAP apart (assert_topk_margin): position i is the same (query, class)
    pair on both sides, which the classes and masks then confirm."""
    n = len(want["classes"])
    assert masks.shape[0] == classes.shape[0] == scores.shape[0] == boxes.shape[0] == n, f"{where}: {masks.shape[0]} detections, the restatement has {n}"
    assert classes.dtype == torch.int64 and scores.dtype == torch.float32 and boxes.dtype == torch.float32 and tuple(boxes.shape) == (n, 4)
    got_scores, got_boxes = scores.cpu().double().numpy(), boxes.cpu().double().numpy()
    assert np.array_equal(classes.cpu().numpy(), want["classes"]), f"{where}: classes"
    assert np.array_equal(masks.cpu().numpy() != 0, want["masks"]), f"{where}: masks"
    d = np.abs(got_scores - want["scores"]).max() if n else 0.0
    print(f"{where}: max |d scores| {d:.3g} (bar {C.SCORE_BAR})")
    assert d <= C.SCORE_BAR, f"{where}: scores {d:.3g} from fp64"
    assert np.array_equal(got_boxes, want["boxes"] if with_boxes else np.zeros((n, 4))), f"{where}: boxes"


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_instance_segments_and_instance_inference_equal_the_restatement(model, name, filtered):
    from rba_amd import instance_ops as iops
    mask_cls, mask_pred, topk, things, want = _reference(name, filtered)
    K = mask_cls.shape[1] - 1
    assert len(C.by_pair(want["qidx"], want["classes"])) == len(want["classes"])
    for boxes, dtype in ((False, torch.float32), (True, torch.uint8)):
        out = iops.instance_segments(mask_cls.cuda(), mask_pred.cuda(), topk, K, thing_classes=things, boxes=boxes, mask_dtype=dtype)
        assert out[0].dtype == dtype
        _check(*out, want, boxes, f"instance_segments[{name}, boxes={boxes}]")
    saved = model.test_topk_per_image, model.panoptic_on, model.thing_classes, model.instance_boxes
    try:
        model.test_topk_per_image, model.panoptic_on, model.instance_boxes = topk, filtered, True
        model.thing_classes = things if filtered else model.thing_classes
        r = model.instance_inference(mask_cls.cuda(), mask_pred.cuda())
        assert r.image_size == tuple(mask_pred.shape[-2:]) and len(r) == len(want["classes"]) and r.pred_masks.dtype == torch.float32
        _check(r.pred_masks, r.pred_classes, r.scores, r.pred_boxes, want, True, f"instance_inference[{name}]")
        model.instance_boxes = False
        r = model.instance_inference(mask_cls.cuda(), mask_pred.cuda())
        assert not bool(r.pred_boxes.any()) and tuple(r.pred_boxes.shape) == (len(r), 4), "zeros by default, as the reference"
    finally:
        model.test_topk_per_image, model.panoptic_on, model.thing_classes, model.instance_boxes = saved


def test_topk_beyond_the_scores_is_refused_by_name(model):
    from rba_amd import instance_ops as iops
    from rba_amd._lib import RbaHipError
    mask_cls, mask_pred, topk, _, _ = _reference("small", False)
    with pytest.raises(RbaHipError, match="topk"):
        iops.instance_segments(mask_cls.cuda(), mask_pred.cuda(), 16 * 8 + 1, 8)
    everything = iops.instance_segments(mask_cls.cuda(), mask_pred.cuda(), 16 * 8, 8)
    assert everything[0].shape[0] == 128 and bool((everything[2][:-1] * 0 == 0).all())


def _same_instances(a, b):
    return (a.image_size == b.image_size and torch.equal(a.pred_masks, b.pred_masks) and torch.equal(a.pred_classes, b.pred_classes)
            and torch.equal(a.scores, b.scores) and torch.equal(a.pred_boxes, b.pred_boxes))


def test_forward_with_instance_on(model):
    """the up4 path (padded size exactly x4 of the logits, no other output size asked for) gives the Instances of instance_inference on the
    materialised planes; sem_seg / rba are the bits of a model without instance_on; a requested output size takes the materialised planes"""
    from rba_amd import ops
    g = torch.Generator().manual_seed(23)
    saved = model.instance_on, model.instance_boxes, model.sem_seg_postprocess_before_inference
    try:
        for size in ((60, 90), (64, 96)):                              # padded beyond the image / exactly the image: both are x4 of the logits
            im = torch.randint(0, 256, (3,) + size, generator=g, dtype=torch.uint8)
            model.instance_on = False
            plain = model([{"image": im}])[0]
            assert set(plain) == {"sem_seg", "rba"}
            model.instance_on = model.instance_boxes = True
            r = model([{"image": im}])[0]
            assert set(r) == {"sem_seg", "rba", "instances"}
            assert torch.equal(r["sem_seg"], plain["sem_seg"]) and torch.equal(r["rba"], plain["rba"])
            mask_cls, mask_pred, sizes, padded = model.predict([{"image": im}])
            assert tuple(mask_pred.shape[-2:]) == (padded[0] // 4, padded[1] // 4) and sizes[0] == size
            mp = ops.resample_bilinear(mask_pred[0].contiguous(), padded)[:, :size[0], :size[1]].contiguous()
            want = model.instance_inference(mask_cls[0], mp)
            got = r["instances"]
            assert len(got) == model.test_topk_per_image == 100 and got.image_size == size and got.pred_masks.shape[1:] == size
            assert float(got.pred_masks.sum()) > 0 and float(got.pred_boxes.sum()) > 0, "the seeded model detects something"
            # the kernels' fused taps and the materialised planes are the same fp32 expression (rba_reduce_up4_kernel's), so the two paths see the same
            # logits bit for bit, and the sums are exact integers: everything is equal, the scores included
            print(f"{size}: max |d scores| between the two paths {(got.scores - want.scores).abs().max().item():.3g}")
            assert _same_instances(got, want)
            assert bool((got.scores[:-1] >= 0).all()) and bool((got.scores <= 1).all())
        # a requested output size: the planes are materialised, cropped and resized a second time (sem_seg_postprocess before inference, :316-320)
        model.sem_seg_postprocess_before_inference = True
        im = torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8)
        r = model([{"image": im, "height": 45, "width": 70}])[0]
        mask_cls, mask_pred, sizes, padded = model.predict([{"image": im}])
        mp = ops.resample_bilinear(ops.resample_bilinear(mask_pred[0].contiguous(), padded)[:, :60, :90].contiguous(), (45, 70))
        assert r["instances"].image_size == (45, 70) and _same_instances(r["instances"], model.instance_inference(mask_cls[0], mp))
        assert tuple(r["sem_seg"].shape[1:]) == (45, 70)
    finally:
        model.instance_on, model.instance_boxes, model.sem_seg_postprocess_before_inference = saved


def test_include_void_and_return_separately(model):
    from rba_amd import ops
    g = torch.Generator().manual_seed(29)
    im = torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8)
    K = model.arch["num_classes"]
    plain = model([{"image": im}])[0]
    void = model([{"image": im}], include_void=True)[0]
    assert tuple(void["sem_seg"].shape) == (K + 1, 60, 90) and torch.equal(void["rba"], plain["rba"]), "rba stays the score over the K real classes"
    assert (void["sem_seg"][:K] - plain["sem_seg"]).abs().max().item() < 1e-4
    mask_cls, mask_pred, sizes, padded = model.predict([{"image": im}])
    up = F.interpolate(mask_pred[0].double()[None].cpu(), size=padded, mode="bilinear", align_corners=False)[0][:, :60, :90]
    want = torch.einsum("qc,qhw->chw", F.softmax(mask_cls[0].double().cpu(), -1), up.sigmoid())     # semantic_inference_with_void (:388-392) in fp64
    assert (void["sem_seg"].cpu().double() - want).abs().max().item() < 1e-4
    assert float(want[K].max()) > 1e-3, "the void channel carries something to compare"
    # return_separately (:353-354): the last image's class logits and its mask logits at the resolution the heads saw
    results, cls_last, pred_last = model([{"image": im}, {"image": im[:, :32, :64]}], return_separately=True)
    assert len(results) == 2 and set(results[1]) == {"sem_seg", "rba"}
    mask_cls, mask_pred, sizes, padded = model.predict([{"image": im}, {"image": im[:, :32, :64]}])
    assert torch.equal(cls_last, mask_cls[1]) and tuple(pred_last.shape) == (model.num_queries, 32, 64)
    assert torch.equal(pred_last, ops.resample_bilinear(mask_pred[1].contiguous(), padded)[:, :32, :64].contiguous())
    with pytest.raises(NotImplementedError):
        model([{"image": im}], return_aux=True)


def test_semantic_off_drops_the_semantic_keys():
    m = _tiny(semantic_on=False, instance_on=True, test_topk_per_image=10)
    g = torch.Generator().manual_seed(31)
    im = torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8)
    r = m([{"image": im}])[0]
    assert set(r) == {"instances"} and len(r["instances"]) == 10
    m.semantic_on = True
    assert set(m([{"image": im}], return_argmax=True)[0]) == {"sem_seg", "rba", "argmax", "instances"}


@pytest.mark.no_canary
def test_the_instance_branch_allocates_little_beside_its_result():
    """256 x 512, Q = N = 100: over a forward, the peak of allocated device memory rises with instance_on by less than the result planes' own
    N * H * W * 4 bytes plus 10 % over the semantic-only forward's rise (the torch composition of the reference's lines -- the up-sampled [Q,H,W], its
    gather, the > 0 plane, the sigmoid, the product -- takes several times those bytes)."""
    m = _tiny(num_queries=100)
    g = torch.Generator().manual_seed(37)
    H, W, N = 256, 512, 100
    im = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).cuda()

    def peak_rise(instance_on):
        m.instance_on = instance_on
        m([{"image": im}])                                                 # warm: code objects, per-shape constants, the allocator's pools
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        r = m([{"image": im}])[0]
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        return rise, r

    base, _ = peak_rise(False)
    rise, r = peak_rise(True)
    planes = N * H * W * 4
    print(f"peak rise: semantic only {base} B, with instance_on {rise} B, the result planes {planes} B")
    assert len(r["instances"]) == N and r["instances"].pred_masks.dtype == torch.float32 and r["instances"].pred_masks.shape == (N, H, W)
    assert rise - base < planes * 1.1, f"the instance branch took {rise - base} B beside the semantic forward, its result is {planes} B"
