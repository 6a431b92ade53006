"""K8 on the GPU: ops.point_sample, ops.mask_point_loss (+ backward), ops.match_cost, the matcher, the uncertainty selection and SetCriterion against the
fp64 restatement of tests/_point_loss_cases.py.  Bar (tests/_rba_bwd_cases.py): e(T) = max|T - T64| / max|T64| <= 4 max(b, 2^-20) per tensor, b = the
fp32-CPU error of the same case; a scalar loss: |l - l64| <= 4 max(|l32 - l64|, 2^-20 |l64|).  The mask gradient is summed with float atomics (the
header: "may differ from launch to launch"), so two runs are each held to the bar; everything else is compared bit for bit between runs."""
import pytest
import torch

from tests import _point_loss_cases as C

pytestmark = pytest.mark.gpu


def _cuda(*ts):
    return tuple(t.cuda() for t in ts)


# ---------------------------------------------------------------------------------------------------------------- ops.point_sample
@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
@pytest.mark.parametrize("shape", C.SAMPLE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_point_sample(shape, shared):
    from rba_amd import ops
    N = shape[0]
    planes, coords, centres = C.sample_inputs(shape, shared)
    assert centres and float(coords.min()) < 0 and float(coords.max()) > 1 and bool((coords == 0).any()) and bool((coords == C.BELOW_ONE).any())
    # a permutation of N of the N + 2 planes and one repeat; with per-row coordinates the repeated row repeats its points too
    index = torch.randperm(N + 2, generator=torch.Generator().manual_seed(1))[:N]
    index = torch.cat([index, index[:1]])
    rows = coords if shared else torch.cat([coords, coords[:1]])
    t64 = C.ref_point_sample(planes.double(), rows.double(), index)
    b = C.err(C.ref_point_sample(planes, rows, index), t64)
    got = ops.point_sample(planes.cuda(), rows.cuda(), index.cuda())
    assert got.shape == (N + 1, shape[3])
    C.check(f"point_sample {shape} index", got, t64, b)
    for p, y, x in centres:                                       # at pixel centres: the plane's bits
        assert torch.equal(got[:, p].cpu(), planes[index, y, x])
    assert torch.equal(got[N], got[0])
    first = planes[:N].contiguous()                               # no index: row n reads plane n
    t64p = C.ref_point_sample(first.double(), coords.double())
    C.check(f"point_sample {shape}", ops.point_sample(first.cuda(), coords.cuda()), t64p, C.err(C.ref_point_sample(first, coords), t64p))
    assert torch.equal(ops.point_sample(planes.cuda(), rows.cuda(), index.cuda()), got)


def test_point_sample_refusals():
    from rba_amd import ops
    planes, coords = torch.zeros(3, 4, 5).cuda(), torch.zeros(3, 6, 2).cuda()
    with pytest.raises(ops.RbaHipError):
        ops.point_sample(planes, coords[:2])
    with pytest.raises(ops.RbaHipError):
        ops.point_sample(planes, coords, torch.zeros(3, dtype=torch.int32).cuda())
    with pytest.raises(ops.RbaHipError):
        ops.point_sample(planes[0], coords)
    out = ops.point_sample(planes, coords, torch.tensor([0, 3, -1]).cuda())       # an index that names no plane: NaN, nothing read
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isnan(out[1:]).all())
    assert ops.point_sample(planes, torch.zeros(3, 0, 2).cuda()).shape == (3, 0)


# ---------------------------------------------------------------------------------------------------------------- the fused loss
def _run_loss(args, need_grad=True):
    from rba_amd.modeling.criterion import MaskPointLossFunction
    pred, index, coords, labels, num_masks = args
    p = pred.cuda().requires_grad_(need_grad)
    lm, ld = MaskPointLossFunction.apply(p, index.cuda(), coords.cuda(), labels.cuda(), num_masks)
    if need_grad:
        (C.W_MASK * lm + C.W_DICE * ld).backward()
    return lm.detach(), ld.detach(), p.grad


def _check_loss(what, args, truth, runs=2):
    pred, index = args[0], args[1]
    unmatched = torch.ones(pred.shape[0] * pred.shape[1], dtype=torch.bool)
    unmatched[index] = False
    first = None
    for r in range(runs):
        lm, ld, g = _run_loss(args)
        C.check_scalar(f"{what} loss_mask", lm, truth["l32"][0], truth["l64"][0])
        C.check_scalar(f"{what} loss_dice", ld, truth["l32"][1], truth["l64"][1])
        C.check(f"{what} grad run {r}", g.cpu(), truth["g64"], truth["b"])              # every run meets the bar (atomics: last bits may move)
        assert bool((g.flatten(0, 1)[unmatched.cuda()] == 0).all()) and bool(torch.isfinite(g).all())
        if first is None:
            first = (lm, ld)
        assert torch.equal(lm, first[0]) and torch.equal(ld, first[1])                  # the scalars: bit for bit


@pytest.mark.parametrize("shape", C.LOSS_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_point_loss(shape):
    """Measured on MI355X: see docs/kernels/K8.md."""
    args = C.loss_inputs(shape)
    labels = args[3]
    if shape[3] > 1:
        assert bool(((labels > 0) & (labels < 1)).any()), "fixture: fractional labels"
    _check_loss(f"loss {shape}", args, C.loss_truth(shape))


def test_mask_point_loss_direct_ops_and_three_runs():
    from rba_amd import ops
    pred, index, coords, labels, num_masks = C.loss_inputs((9, 32, 64, 448))
    p, i, c, t = _cuda(pred, index, coords, labels)
    runs = [ops.mask_point_loss(p, i, c, t, num_masks) for _ in range(3)]
    assert all(torch.equal(r[0], runs[0][0]) and torch.equal(r[1], runs[0][1]) for r in runs)
    losses, sums = runs[0]
    x = C.ref_point_sample(pred.double().flatten(0, 1), coords.double(), index)
    s = x.sigmoid()
    want = torch.stack([torch.nn.functional.binary_cross_entropy_with_logits(x, labels.double(), reduction="none").sum(1), (s * labels).sum(1), s.sum(1),
                        labels.double().sum(1)], 1)
    assert float(((sums.cpu().double() - want).abs() / want.abs().amax(0)).max()) < 4e-6
    one = torch.ones((), device="cuda")
    g_mask = ops.mask_point_loss_backward(p, i, c, t, sums, num_masks, grad_loss_mask=one)             # one upstream gradient absent = 0
    g_both = ops.mask_point_loss_backward(p, i, c, t, sums, num_masks, one, torch.zeros((), device="cuda"))
    assert float((g_mask - g_both).abs().max()) <= 1e-6 * float(g_both.abs().max())
    with pytest.raises(ops.RbaHipError):
        ops.mask_point_loss_backward(p, i, c, t, sums, num_masks)
    with pytest.raises(ops.RbaHipError):
        ops.mask_point_loss(p, i, c, t[:, :-1].contiguous(), num_masks)
    with pytest.raises(ops.RbaHipError):
        ops.mask_point_loss(p, i, c, t, 0.0)


def test_mask_point_loss_contention_all_points_identical():
    """every mask's 448 points are one point: maximal contention on four pixels"""
    shape = (9, 32, 64, 448)
    _check_loss("contend", C.loss_inputs(shape, "contend"), C.loss_truth(shape, "contend"))


def test_mask_point_loss_wide_logits_stay_finite():
    shape = (9, 32, 64, 448)
    args = C.loss_inputs(shape, "wide")
    assert float(args[0].abs().max()) == 120.0
    lm, ld, g = _run_loss(args)
    assert bool(torch.isfinite(lm)) and bool(torch.isfinite(ld)) and bool(torch.isfinite(g).all())
    truth = C.loss_truth(shape, "wide")
    C.check_scalar("wide loss_mask", lm, truth["l32"][0], truth["l64"][0])
    C.check_scalar("wide loss_dice", ld, truth["l32"][1], truth["l64"][1])


def test_mask_point_loss_no_backward_launch_without_a_gradient_consumer(monkeypatch):
    from rba_amd import ops
    from rba_amd.modeling.criterion import MaskPointLossFunction
    pred, index, coords, labels, num_masks = C.loss_inputs((3, 5, 7, 63))
    monkeypatch.setattr(ops, "mask_point_loss_backward", lambda *a, **k: pytest.fail("backward launched"))
    t = labels.cuda().requires_grad_(True)                        # a graph exists, but not towards pred_masks
    lm, ld = MaskPointLossFunction.apply(pred.cuda(), index.cuda(), coords.cuda(), t, num_masks)
    (lm + ld).backward()
    assert t.grad is None


def test_mask_point_loss_without_masks_is_zero_and_launches_nothing(monkeypatch):
    from rba_amd import ops
    from rba_amd.modeling.criterion import MaskPointLossFunction
    monkeypatch.setattr(ops, "_launch", lambda *a, **k: pytest.fail("a kernel was launched"))
    p = torch.randn(2, 3, 4, 5).cuda().requires_grad_(True)
    lm, ld = MaskPointLossFunction.apply(p, torch.zeros(0, dtype=torch.int64).cuda(), torch.zeros(0, 7, 2).cuda(), torch.zeros(0, 7).cuda(), 1.0)
    assert float(lm.detach()) == 0.0 and float(ld.detach()) == 0.0
    (lm + ld).backward()
    assert p.grad.shape == p.shape and float(p.grad.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- ops.match_cost, the matcher
@pytest.mark.parametrize("shape", C.COST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_match_cost(shape):
    from rba_amd import ops
    pred, tgt, coords, logits, ids = C.cost_inputs(shape)
    c64, b = C.cost_truth(shape)
    wm, wc, wd = C.COST_WEIGHTS
    args = _cuda(pred, tgt, coords, logits.softmax(-1), ids)
    runs = [ops.match_cost(*args, cost_mask=wm, cost_class=wc, cost_dice=wd) for _ in range(3)]
    assert runs[0].shape == c64.shape
    C.check(f"match_cost {shape}", runs[0].cpu(), c64, b)
    assert torch.equal(runs[1], runs[0]) and torch.equal(runs[2], runs[0])
    assert torch.equal(ops.match_cost(args[0], args[1], args[2][None], *args[3:], cost_mask=wm, cost_class=wc, cost_dice=wd), runs[0])   # [1,P,2]


def test_match_cost_refuses_bad_ids_and_shapes():
    from rba_amd import ops
    pred, tgt, coords, logits, ids = C.cost_inputs((3, 1, 64))
    args = list(_cuda(pred, tgt, coords, logits.softmax(-1), ids))
    for bad in (-1, C.COST_K + 1):
        with pytest.raises(ops.RbaHipError, match="tgt_ids"):
            ops.match_cost(*args[:4], torch.tensor([bad]).cuda())
    with pytest.raises(ops.RbaHipError):
        ops.match_cost(*args[:4], torch.zeros(2, dtype=torch.int64).cuda())
    with pytest.raises(ops.RbaHipError):
        ops.match_cost(args[0], args[1], args[2], args[3][:2].contiguous(), args[4])


def test_hungarian_matcher_returns_the_planted_assignment():
    from rba_amd.modeling.matcher import HungarianMatcher
    logits, pred, targets, coords = C.planted()
    c64, rows, margin, bound = C.planted_assignment(logits[0], pred[0], targets[0], coords)
    print(f"margin {margin:.3e} against {bound:.3e}")
    wm, wc, wd = C.COST_WEIGHTS
    matcher = HungarianMatcher(cost_class=wc, cost_mask=wm, cost_dice=wd, num_points=coords.shape[0])
    empty = {"labels": torch.zeros(0, dtype=torch.int64), "masks": torch.zeros(0, 128, 256)}
    outputs = {"pred_logits": torch.cat([logits, logits]).cuda(), "pred_masks": torch.cat([pred, pred]).cuda()}
    (i, j), (ei, ej) = matcher(outputs, [{k: v.cuda() for k, v in targets[0].items()}, empty], point_coords=coords.cuda())
    assert i.dtype == j.dtype == torch.int64 and not i.is_cuda
    assert sorted(zip(i.tolist(), j.tolist())) == sorted(zip(rows.tolist(), range(len(rows))))
    assert ei.numel() == 0 and ej.numel() == 0 and ei.dtype == torch.int64                                   # T = 0
    b32 = C.err(C.ref_match_cost(pred[0], targets[0]["masks"], coords, logits[0], targets[0]["labels"], wm, wc, wd), c64)
    C.check("matcher cost", matcher.cost_matrix(outputs["pred_logits"][0], outputs["pred_masks"][0], {k: v.cuda() for k, v in targets[0].items()},
                                                coords.cuda()).cpu(), c64, b32)
    g = torch.Generator(device="cuda").manual_seed(5)                                                        # its own random points: the same seed, the same answer
    a = matcher(outputs, [targets[0]], generator=g)
    b = matcher(outputs, [targets[0]], generator=g.manual_seed(5))
    assert torch.equal(a[0][0], b[0][0]) and torch.equal(a[0][1], b[0][1]) and a[0][0].numel() == len(rows)


# ---------------------------------------------------------------------------------------------------------------- the uncertainty oversampling
def test_select_uncertain_points():
    from rba_amd.modeling.criterion import select_uncertain_points
    pred, index, _, _, _ = C.loss_inputs((9, 32, 64, 448))
    R, k = 1344, 336
    cand = torch.rand(9, R, 2, generator=torch.Generator().manual_seed(17))
    idx64, mag = C.ref_select(pred.double(), index, cand.double(), k)
    got = select_uncertain_points(pred.cuda(), index.cuda(), cand.cuda(), k).cpu()
    assert got.shape == (9, k, 2)
    tol = 2.0 ** -18 * float(mag.max())
    for n in range(9):
        kth = float(mag[n, idx64[n]].max())
        close = set(torch.nonzero((mag[n] - kth).abs() <= tol).flatten().tolist())
        assert len(close) <= max(1, k // 100), "fixture: too many candidates at the k-th value"
        # candidates are distinct points, so a returned point names its candidate
        where = {tuple(c): r for r, c in enumerate(cand[n].tolist())}
        mine = {where[tuple(c)] for c in got[n].tolist()}
        assert len(mine) == k and (mine ^ set(idx64[n].tolist())) <= close


def test_uncertain_point_coords():
    from rba_amd.modeling.criterion import draw_point_candidates, select_uncertain_points, uncertain_point_coords
    pred, index, _, _, _ = C.loss_inputs((9, 32, 64, 448))
    p, i = pred.cuda(), index.cuda()
    P, over, ratio = 448, 3.0, 0.75
    g = torch.Generator(device="cuda")
    a = uncertain_point_coords(p, i, P, over, ratio, generator=g.manual_seed(7))
    assert a.shape == (9, P, 2) and float(a.min()) >= 0.0 and float(a.max()) < 1.0
    assert torch.equal(uncertain_point_coords(p, i, P, over, ratio, generator=g.manual_seed(7)), a)
    cand, rest = draw_point_candidates(9, P, over, ratio, p.device, g.manual_seed(7))
    k = int(ratio * P)
    assert cand.shape == (9, int(P * over), 2) and rest.shape == (9, P - k, 2)
    assert torch.equal(a[:, :k], select_uncertain_points(p, i, cand, k)) and torch.equal(a[:, k:], rest)


# ---------------------------------------------------------------------------------------------------------------- SetCriterion
def test_set_criterion_against_the_restatement():
    from rba_amd.modeling.criterion import SetCriterion
    from rba_amd.modeling.matcher import HungarianMatcher
    B, Q, T, K, P = 2, 20, 3, 5, 200
    logits, pred, targets, mcoords = C.planted(Q=Q, T=T, P=P, B=B, K=K, pred_hw=(16, 32), seed=8500)
    targets = [dict(t) for t in targets]
    gen = torch.Generator().manual_seed(8501)
    lcoords = torch.rand(B * T, P, 2, generator=gen)
    for t in targets:
        r = torch.rand(64, 128, generator=gen)
        t["outlier_masks"] = torch.where(r < 0.25, 1, torch.where(r < 0.6, 0, 255))
    pred = pred - 1.0                                              # scores between the two thresholds of the hinge
    aux_logits, aux_pred = logits + 0.1 * torch.randn(logits.shape, generator=gen), pred + 0.1 * torch.randn(pred.shape, generator=gen)
    wm, wc, wd = C.COST_WEIGHTS
    weights = {"loss_ce": wc, "loss_mask": wm, "loss_dice": wd, "outlier_loss": 1.0}
    weights.update({f"{k}_0": v for k, v in list(weights.items())})
    crit = SetCriterion(K, HungarianMatcher(wc, wm, wd, P), weights, 0.1, ["labels", "masks", "outlier"], P, 3.0, 0.75, target="nls", score_norm="tanh",
                        func="squared_hinge", inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)
    lg, pm = logits.cuda().requires_grad_(True), pred.cuda().requires_grad_(True)
    outputs = {"pred_logits": lg, "pred_masks": pm, "aux_outputs": [{"pred_logits": aux_logits.cuda(), "pred_masks": aux_pred.cuda()}]}
    losses = crit(outputs, [{k: v.cuda() for k, v in t.items()} for t in targets], matcher_point_coords=mcoords.cuda(), loss_point_coords=lcoords.cuda())
    base = ("loss_ce", "loss_mask", "loss_dice", "outlier_loss")
    assert set(losses) == set(base) | {k + "_0" for k in base}
    losses["accuracy"] = torch.zeros((), device="cuda")
    weighted = crit.weighted(losses)
    assert set(weighted) == set(weights) and all(torch.equal(weighted[k], losses[k] * weights[k]) for k in weights)
    sum(weighted[k] for k in base).backward()

    def planted_indices(lgt, prd):
        out = []
        for b in range(B):
            _, rows, _, _ = C.planted_assignment(lgt[b], prd[b], targets[b], mcoords)
            order = torch.argsort(rows)                           # scipy returns rows ascending
            out.append((rows[order], order))
        return out

    num_masks = float(B * T)

    def truth(dtype, lgt, prd):
        indices = planted_indices(lgt, prd)
        l, p = lgt.to(dtype).clone().requires_grad_(True), prd.to(dtype).clone().requires_grad_(True)
        tg = [{k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()} for t in targets]
        out = C.ref_criterion(l, p, tg, indices, num_masks, lcoords.to(dtype), K, 0.1)
        sum(out[k] * weights[k] for k in base).backward()
        return out, l.grad, p.grad

    t64, gl64, gp64 = truth(torch.float64, logits, pred)
    t32, gl32, gp32 = truth(torch.float32, logits, pred)
    a64, _, _ = truth(torch.float64, aux_logits, aux_pred)
    a32, _, _ = truth(torch.float32, aux_logits, aux_pred)
    for k in base:
        C.check_scalar(k, losses[k].detach(), t32[k], t64[k])
        C.check_scalar(k + "_0", losses[k + "_0"], a32[k], a64[k])
        assert not losses[k + "_0"].requires_grad                 # deep supervision stays detached
    C.check("grad pred_logits", lg.grad.cpu(), gl64, C.err(gl32, gl64))
    C.check("grad pred_masks", pm.grad.cpu(), gp64, C.err(gp32, gp64))
