"""GPU: K16c (panoptic_ops.segment_pairs) against np.unique pair counts, exactly; the PQ evaluator's device path against its host path; one end-to-end
run of the tiny model with TEST.PANOPTIC_ON against synthetic ground truth."""
import math

import numpy as np
import pytest
import torch

from tests import _panoptic_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run the allocations of the two new modules under the guard bands too"""
    import rba_amd.panoptic_evaluation as pev
    import rba_amd.panoptic_ops as pops
    if canary is None:
        yield
        return
    real = pops.torch, pev.torch
    pops.torch = pev.torch = canary._PROXY
    try:
        yield
    finally:
        pops.torch, pev.torch = real


def _run(gt, pred, G, P, counts=None, bad=None):
    from rba_amd import panoptic_ops as pops
    counts = torch.zeros((G, P), dtype=torch.int64, device="cuda") if counts is None else counts
    bad = torch.zeros(1, dtype=torch.int64, device="cuda") if bad is None else bad
    pops.segment_pairs(gt, pred, G, P, counts, bad)
    return counts, bad


PAIR_SHAPES = [(1, 1), (5, 7), (40, 300), (1000, 600)]                   # four LDS copies, four, one, the global-atomic form


@pytest.mark.parametrize("G,P", PAIR_SHAPES)
@pytest.mark.parametrize("n", [1, 37 * 53, 300 * 500])
def test_segment_pairs_equal_np_unique(n, G, P):
    for kind in ("single", "random", "out_of_range"):
        gt, pred = C.pair_maps(kind, n, G, P, seed=n + G)
        want, want_bad = C.pair_counts_reference(gt, pred, G, P)
        counts, bad = _run(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, P)
        assert np.array_equal(counts.cpu().numpy(), want) and int(bad) == want_bad, kind
        assert int(counts.sum()) + int(bad) == n
        if kind == "out_of_range" and n > 1000:
            assert want_bad > 0
        if kind == "random":                                             # a second call accumulates; the same bits twice
            _run(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda(), G, P, counts, bad)
            assert np.array_equal(counts.cpu().numpy(), 2 * want) and int(bad) == 0


@pytest.mark.parametrize("G,P", [(5, 7), (1000, 600)])
def test_segment_pairs_on_unaligned_slices(G, P):
    n = 37 * 53
    gt, pred = C.pair_maps("out_of_range", n + 8, G, P, seed=5)
    big_g, big_p = torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda()
    for og, op, m in ((1, 1, n), (1, 2, n), (3, 0, n), (2, 2, n - 3), (0, 3, 5), (3, 3, 2)):     # equal phases: the 16-byte form with a head; others: element loads
        a, b = big_g[og:og + m], big_p[op:op + m]
        assert a.data_ptr() % 16 == 4 * og and b.data_ptr() % 16 == 4 * op
        want, want_bad = C.pair_counts_reference(gt[og:og + m], pred[op:op + m], G, P)
        counts, bad = _run(a, b, G, P)
        assert np.array_equal(counts.cpu().numpy(), want) and int(bad) == want_bad, (og, op, m)


def _tiny_categories():
    """the 19 classes the tiny model predicts and one more thing category that only the ground truth knows (held out as unknown)"""
    return [{"id": i, "name": f"class{i}", "isthing": int(i in C.THING_CLASSES), "supercategory": "s"} for i in range(19)] + \
        [{"id": 100, "name": "novel", "isthing": 1, "supercategory": "s"}]


def _same(a, b):
    assert a.pq_stat.as_ints() == b.pq_stat.as_ints()
    assert {k: c.iou for k, c in a.pq_stat.pq_per_cat.items()} == {k: c.iou for k, c in b.pq_stat.pq_per_cat.items()}
    assert a.evaluate() == b.evaluate()


def test_device_path_equals_host_path_on_the_fixtures():
    from rba_amd.panoptic_evaluation import PanopticOpenEvaluator
    images = [im for name in sorted(C.HAND) for im in C.HAND[name][0]]
    for seed in (1, 2):
        pan_gt, info = C.synthetic_ground_truth((45, 63), seed)
        ids = {s["id"]: i + 1 for i, s in enumerate(info)}
        pred = np.zeros_like(pan_gt, dtype=np.int32)
        for s in info:
            pred[pan_gt == s["id"]] = ids[s["id"]]
        pred = np.roll(pred, (2 * seed, 3), (0, 1))
        images.append((pred, [{"id": ids[s["id"]], "category_id": 255 if s["category_id"] == 3 else s["category_id"]} for s in info], pan_gt, info))
    host, dev = PanopticOpenEvaluator(C.CATEGORIES, C.UNKNOWN_NAMES), PanopticOpenEvaluator(C.CATEGORIES, C.UNKNOWN_NAMES, device="cuda")
    for i, (pred, seg, gt, info) in enumerate(images):
        host.process(pred, seg, gt, info)
        dev.process(torch.from_numpy(pred).cuda() if i % 2 else pred, seg, gt, info)        # tensors on the device or arrays
    _same(host, dev)
    assert dev.evaluate() == C.pq_reference(images)[0]
    with pytest.raises(KeyError):
        pred, seg, gt, info = C.HAND["perfect"][0][0]
        dev.process(pred, seg[:1], gt, info)             # a predicted id without segments_info lands in `bad`


def test_end_to_end_tiny_model_against_synthetic_ground_truth():
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    from rba_amd.panoptic_evaluation import PanopticOpenEvaluator
    a = A.complete(A.ARCHS["tiny1"])
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()
    model.panoptic_on, model.open_panoptic = True, True
    with torch.no_grad():
        model.sem_seg_head.predictor.class_embed.bias[:19] += 6.0
    cats = _tiny_categories()
    unknown = ["novel"]
    host, dev = PanopticOpenEvaluator(cats, unknown), PanopticOpenEvaluator(cats, unknown, device="cuda")
    g = torch.Generator().manual_seed(21)
    for seed in (1, 2):
        im = torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8)
        pan, info = model([{"image": im}], panoptic_ood_threshold=-0.3, panoptic_pixel_min=20)[0]["panoptic_seg"]
        # ground truth: the prediction's own segments under sparse ids (so that things match), one of them relabelled as the held-out class, one cell void
        pan_h = pan.cpu().numpy()
        pan_gt = np.zeros((60, 90), dtype=np.int64)
        gt_info = []
        for j, s in enumerate(info):
            gid = 70000 * (j + 1) + seed
            pan_gt[pan_h == s["id"]] = gid
            gt_info.append({"id": gid, "category_id": 100 if s["category_id"] == 255 else s["category_id"], "iscrowd": 0})
        pan_gt[:20, :30] = 0
        gt_info = [s for s in gt_info if (pan_gt == s["id"]).any()]
        assert len(info) >= 2
        host.process(pan_h, info, pan_gt, gt_info)
        dev.process(pan, info, pan_gt, gt_info)
    _same(host, dev)
    res = dev.evaluate()
    assert set(res) == {"All", "Known Things", "Unknown Things", "Stuff", "per_class"}
    for name in ("All", "Known Things", "Unknown Things", "Stuff"):
        assert set(res[name]) == {"pq", "sq", "rq", "n"} and all(math.isfinite(res[name][k]) and 0.0 <= res[name][k] <= 1.0 for k in ("pq", "sq", "rq")), name
    assert res["All"]["n"] >= 1 and res["All"]["pq"] > 0.5
