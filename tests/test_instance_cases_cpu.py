"""CPU: the K17 fixtures hold their decision margins, and the numpy fp64 restatement of MaskFormer.instance_inference (tests/_instance_cases.py) agrees
with the reference's own lines typed as fp32 torch ops (maskformer_model.py:488-527) -- classes and masks exactly after matching on the (query, class)
pair, scores within the bar the GPU tests hold the kernels to.  The distance measured here is the one quoted in docs/kernels/K17.md."""
import numpy as np
import pytest
import torch

from tests import _instance_cases as C


@pytest.mark.parametrize("mode", C.KEEP_MODES)
@pytest.mark.parametrize("H,W", C.STATS_SHAPES)
@pytest.mark.parametrize("Q", C.STATS_QUERIES)
def test_stats_fixtures_hold_the_logit_margin(Q, H, W, mode):
    mask, keep = C.stats_case(Q, H, W, mode)
    count, ssum, box = C.stats_reference(mask.numpy(), keep.numpy())
    assert int(keep.sum()) == min(Q, {"all": Q, "three": 3, "one": 1}[mode]) and (count[~keep.numpy()] == 0).all()
    assert (count[keep.numpy()] > 0).all() and ((mask == 0).sum() > 0 or H * W < 100)
    assert np.all(ssum <= count) and np.all(ssum >= 0.5 * count)


def test_special_planes_and_the_box_rule():
    mask, keep = C.special_case()
    count, ssum, box = C.stats_reference(mask.numpy(), keep.numpy())
    assert count[0] == 0 and box[0].tolist() == [22, 13, -1, -1] and ssum[0] == 0
    assert count[1] == 13 * 22 and box[1].tolist() == [0, 0, 21, 12]
    assert 0 < count[2] < 13 * 22 and np.isfinite(ssum[2])
    assert count[3] == 1 and box[3].tolist() == [21, 12, 21, 12]
    assert ssum[4] == count[4] > 0
    b = C.boxes_of(np.asarray(mask.numpy() > 0))
    assert b[0].tolist() == [0, 0, 0, 0] and b[1].tolist() == [0, 0, 22, 13] and b[3].tolist() == [21, 12, 22, 13]


@pytest.mark.parametrize("h,w,crop", C.UP4_CASES)
def test_up4_fixtures_are_dyadic(h, w, crop):
    low, keep, up = C.up4_case(h, w, crop)
    assert tuple(up.shape) == (C.UP4_Q,) + tuple(crop) and torch.equal((up * 512).round(), up * 512)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("name", sorted(C.SCENARIOS))
def test_restatement_equals_the_reference_lines_in_fp32(name, filtered):
    mask_cls, mask_pred, topk = C.scenario(name)
    things = C.SCENARIOS[name]["things"] if filtered else None
    want = C.instance_reference(mask_cls.numpy(), mask_pred.numpy(), topk, things)
    got = C.reference_lines_fp32(mask_cls, mask_pred, topk, things)
    at = C.by_pair(want["qidx"], want["classes"])
    pairs = C.by_pair(got["qidx"].numpy(), got["classes"].numpy())
    assert set(at) == set(pairs) and (things is not None or len(at) == topk)
    order = [at[p] for p in pairs]                                          # position in the restatement of each of the reference's detections
    assert np.array_equal(got["masks"].numpy() > 0, want["masks"][order])
    d = np.abs(got["scores"].double().numpy() - want["scores"][order]).max()
    print(f"{name}: the reference's fp32 composition is {d:.3g} from fp64 (the bar is {C.SCORE_BAR})")
    assert d <= C.SCORE_BAR
    assert np.isfinite(want["scores"]).all() and (want["scores"] >= 0).all() and (want["scores"] <= 1).all()
    empty = ~want["masks"].reshape(len(order), -1).any(1)
    assert (want["scores"][empty] == 0).all() and (want["boxes"][empty] == 0).all()
    if things is None:
        assert empty.any() and len({int(q) for q in want["qidx"]}) < len(order), "the scenario has empty masks and a query under several classes"
    else:
        assert 0 < len(order) < topk and all(int(c) in things for c in want["classes"])
