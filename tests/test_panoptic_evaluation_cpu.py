"""CPU: the open-set PQ evaluator's host path (rba_amd.panoptic_evaluation with device=None) against the dictionary restatement of the reference in
tests/_panoptic_cases.py and against numbers written down by hand; the fixtures' decision margins; the K16 bindings."""
import numpy as np
import pytest

from tests import _panoptic_cases as C


def _evaluator(**kw):
    from rba_amd.panoptic_evaluation import PanopticOpenEvaluator
    return PanopticOpenEvaluator(C.CATEGORIES, C.UNKNOWN_NAMES, **kw)


@pytest.mark.parametrize("name", sorted(C.HAND))
def test_hand_fixture_gives_the_pq_written_down_by_hand(name):
    images, expected, ints = C.HAND[name]
    ev = _evaluator()
    for im in images:
        ev.process(*im)
    got = ev.evaluate()
    assert got == expected, f"{got}\n!=\n{expected}"
    assert {k: v for k, v in ev.pq_stat.as_ints().items() if any(v)} == ints
    ref, _ = C.pq_reference(images)
    assert got == ref


def test_host_path_equals_the_restatement_on_all_fixtures_pooled_and_rank_pooling_adds_up():
    images = [im for name in sorted(C.HAND) for im in C.HAND[name][0]]
    for seed in (1, 2):                                                  # two larger images: synthetic ground truth against a shifted copy of itself
        pan_gt, info = C.synthetic_ground_truth((45, 63), seed)
        ids = {s["id"]: i + 1 for i, s in enumerate(info)}
        pred = np.zeros_like(pan_gt, dtype=np.int32)
        for s in info:
            pred[pan_gt == s["id"]] = ids[s["id"]]
        pred = np.roll(pred, (2 * seed, 3), (0, 1))
        seg = [{"id": ids[s["id"]], "category_id": 255 if s["category_id"] == 3 else s["category_id"]} for s in info]
        images.append((pred, seg, pan_gt, info))
    ev = _evaluator()
    for im in images:
        ev.process(*im)
    ref, stat = C.pq_reference(images)
    assert ev.evaluate() == ref
    assert {k: (c.iou, c.tp, c.fp, c.fn) for k, c in ev.pq_stat.pq_per_cat.items() if c.tp + c.fp + c.fn} == \
        {k: tuple(v) for k, v in stat.items() if v[1] + v[2] + v[3]}
    for name in ("All", "Known Things", "Unknown Things", "Stuff"):
        assert ref[name]["n"] >= 1 and 0.0 < ref[name]["pq"] < 1.0, "the pooled run must exercise every row"
    a, b = _evaluator(), _evaluator()
    for i, im in enumerate(images):
        (a if i % 2 == 0 else b).process(*im)
    a += b
    assert a.images == len(images) and a.pq_stat.as_ints() == ev.pq_stat.as_ints()
    for k, c in ev.pq_stat.pq_per_cat.items():
        assert a.pq_stat[k].iou == pytest.approx(c.iou, rel=1e-12)       # the same terms in another order


def test_closed_set_categories_are_left_alone_and_malformed_predictions_are_refused():
    from rba_amd.panoptic_evaluation import PanopticOpenEvaluator, rewrite_categories
    cats, unknown = rewrite_categories(C.CATEGORIES, None)
    assert list(cats) == [1, 2, 3, 4] and unknown == ()
    cats, unknown = rewrite_categories(C.CATEGORIES, C.UNKNOWN_NAMES)
    assert list(cats) == [1, 2, -4, 4, 255] and unknown == (3,) and cats[-4]["name"] == "unknown_dog" and cats[-4]["id"] == -4
    assert C.CATEGORIES[2]["id"] == 3, "the caller's list is not edited"
    images = C.HAND["perfect"][0]
    ev = PanopticOpenEvaluator(C.CATEGORIES, None)
    ev.process(*images[0])
    assert ev.evaluate()["All"]["n"] == 2 and ev.evaluate()["Unknown Things"]["n"] == 0
    pred, seg, gt, info = images[0]
    with pytest.raises(KeyError):
        _evaluator().process(pred, seg[:1], gt, info)                     # segment 2 is in the map and not in segments_info
    with pytest.raises(KeyError):
        _evaluator().process(pred, seg + [{"id": 3, "category_id": 1}], gt, info)       # segment 3 is in segments_info and not in the map
    with pytest.raises(KeyError):
        _evaluator().process(pred, [seg[0], {"id": 2, "category_id": 77}], gt, info)    # a category nobody knows
    with pytest.raises(ValueError):
        _evaluator().process(pred[:2], seg, gt, info)


def test_merge_segments_is_the_reference_loop_on_counts():
    from rba_amd.panoptic_ops import merge_segments
    #          q:  0    1    2    3    4    5
    won = [100, 50, 0, 30, 10, 40]
    own = [100, 100, 20, 0, 40, 40]
    inter = [90, 45, 0, 0, 0, 40]
    classes = [3, 3, 11, 12, 13, -1]                                     # two stuff queries of class 3; 5 is not kept
    table, info, n = merge_segments([won, own, inter], classes, C.THING_CLASSES, 0.6)
    # q0: kept (1.0); q1: 50 / 100 < 0.6 dropped; q2: won 0; q3: own 0; q4: intersection 0; q5: not kept
    assert table == [1, 0, 0, 0, 0, 0] and info == [{"id": 1, "isthing": False, "category_id": 3}] and n == 1
    table, info, n = merge_segments([won, own, inter], classes, C.THING_CLASSES, 0.5)
    assert table == [1, 1, 0, 0, 0, 0] and n == 1, "the second stuff query of class 3 joins the first segment"
    table, info, n = merge_segments([won, own, [90, 45, 0, 0, 5, 40]], [11, 3, 11, 12, 3, -1], C.THING_CLASSES, 0.25)
    assert table == [1, 2, 0, 0, 2, 0] and n == 2
    assert info == [{"id": 1, "isthing": True, "category_id": 11}, {"id": 2, "isthing": False, "category_id": 3}]


def test_fixtures_hold_their_decision_margins():
    """every parity fixture of the GPU tests, built here without a device: the builders assert the margins"""
    for Q, H, W in C.MERGE_SHAPES + [C.PLACED_SHAPE]:
        for mode in C.KEEP_MODES:
            mask, score, keep = C.merge_case(Q, H, W, mode)
            winner, counts = C.merge_reference(mask.numpy(), score.numpy(), keep.numpy())
            assert counts[0].sum() == H * W and (counts[2] <= counts[0]).all() and (counts[2] <= counts[1]).all()
    mask, score, keep = C.never_solid_case()
    winner, counts = C.merge_reference(mask.numpy(), score.numpy(), keep.numpy())
    assert (winner == C.NOBODY).all() and counts[:, 2].tolist() == [99, 0, 0]
    mask, score, keep = C.tie_case()
    winner, counts = C.merge_reference(mask.numpy(), score.numpy(), keep.numpy())
    assert counts[0][1] > 0 and counts[0][3] == 0 and (winner != 3).all(), "the lower of two equal queries wins"
    for h, w, crop in C.UP4_CASES:
        C.up4_case(h, w, crop)
    from oracle import ref_ops
    mask_cls, mask_pred = C.box_scenario()
    pan, info, _ = ref_ops.panoptic_inference(mask_cls, mask_pred, set(C.THING_CLASSES), C.OBJECT_MASK_THRESHOLD, C.OVERLAP_THRESHOLD)
    assert sum(1 for s in info if s["category_id"] == 3) == 1 and len(info) == 5, "stuff merges; queries 5 and 7 are dropped"
    mask_cls, mask_pred = C.many_query_scenario()
    pan, info, _ = ref_ops.panoptic_inference(mask_cls, mask_pred, set(C.THING_CLASSES), C.OBJECT_MASK_THRESHOLD, C.OVERLAP_THRESHOLD)
    assert len(info) >= 20


def test_k16_entry_points_are_bound_and_the_abi_version_stays():
    from rba_amd import _lib
    from rba_amd.csrc import build
    for name in ("rba_panoptic_merge_f32", "rba_panoptic_merge_up4_f32", "rba_panoptic_assign_i32", "rba_segment_pairs_accum"):
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    assert _lib.EXPECTED_ABI == 191 and _lib.load().rba_hip_version() == 191
    assert "panoptic_merge.hip" in build.SOURCES
    import rba_amd.ops as ops
    import rba_amd.panoptic_ops as pops
    assert not any(hasattr(ops, n) for n in pops.__all__), "the K16 wrappers live outside rba_amd.ops"
