"""Every torch restatement that the GPU suites use as truth -- tests/_rba_bwd_cases.py (``ref_outlier_loss``, ``ref_score``),
tests/_dense_hybrid_cases.py (``ref_tail``, ``ref_densehybrid_loss``), tests/_pebal_cases.py (``ref_gambler_loss``, ``ref_gambler_tail``,
``ref_smoothness``, ``ref_sparsity``, ``ref_pebal_entry``) and tests/_point_loss_cases.py (``ref_mask_losses``, ``ref_match_cost``,
``ref_loss_labels``, ``ref_criterion``, ``ref_point_sample``) -- held to tests/golden/g9_criterion.npz, which the reference's own
``criterion.py`` and ``matcher.py`` wrote (tests/golden/make_golden.py, ``--only g9_criterion``).

Both sides are the same torch operations in double on a CPU, so the bound is derived, not measured: relative ``REL64`` = 1e-12 in the metric
max|a - a64| / max|a64|.  Where the reference computes in float32 whatever it is given -- ``pred_logits.float()`` of loss_labels, the float32
target of the BCE outlier loss, the matcher's ``.float()`` -- the restatement runs under the same cast and is held to ``REL32`` = 2^-23.
(tests/_criterion_ref_cases.py derives both.)
"""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _criterion_ref_cases as G
from tests import _dense_hybrid_cases as D
from tests import _pebal_cases as P
from tests import _point_loss_cases as C
from tests import _rba_bwd_cases as R

MAKE_GOLDEN = os.path.join(os.path.dirname(G.FIXTURE), "make_golden.py")


def _close(what, a, a64, bound):
    e = G.rel(a, a64)
    print(f"{what}: rel = {e:.3e}  bound = {bound:.3e}")
    assert e <= bound, f"{what}: rel = {e:.3e} > {bound:.3e}"


def _autograd(fn, leaves, dtype=torch.float64):
    lv = {k: v.to(dtype).clone().requires_grad_(True) for k, v in leaves.items()}
    loss = fn(**lv)
    if loss.requires_grad:
        loss.backward()
    return loss.detach(), {k: (torch.zeros_like(v) if v.grad is None else v.grad) for k, v in lv.items()}


def _hold(key, fn, leaves, bound=G.REL64, sums=False):
    """the restatement's float64 loss and gradients against the fixture's entry ``key``"""
    z = G.load()
    loss, grads = _autograd(fn, leaves)
    _close(key + " loss", loss, z[key + "/l64"], max(bound, G.REL32) if bool(z[key + "/l64_is_f32"]) else bound)
    for k, g in grads.items():
        if sums:
            assert G.crc(leaves[k]) == z[f"{key}/crc_{k}"], f"{key}: the seeded draw of {k} has drifted"
            for ax, s in G.grad_sums(g).items():
                _close(f"{key} grad {k} {ax} sums", s, z[f"{key}/s_{k}_{ax}"], bound)
        else:
            ref = G.t(z[f"{key}/g_{k}"])
            if float(ref.abs().max()) == 0:
                assert float(g.abs().max()) == 0, f"{key}: the reference's gradient of {k} is zero"
            else:
                _close(f"{key} grad {k}", g, ref, bound)


def _inputs(key, names=("pred_logits", "pred_masks")):
    z = G.load()
    return {k: G.t(z[f"{key}/in_{k}"]) for k in names}


def _plane(key, name, n=1):
    z = G.load()
    return torch.stack([G.t(z[f"{key}/t{i}_{name}"]) for i in range(n)])


def _masks(key, i):
    z = G.load()
    shape = tuple(int(s) for s in z[f"{key}/t{i}_masks_shape"])
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(z[f"{key}/t{i}_masks_bits"])[:n].reshape(shape).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- the dense losses
@pytest.mark.parametrize("outliers", (True, False), ids=("out", "noout"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("combo", R.COMBOS, ids="_".join)
def test_outlier_loss_small(combo, func, outliers):
    key = f"small/outlier/{'_'.join(combo)}/{'out' if outliers else 'noout'}"
    labels = _plane(key, "outlier_masks")
    assert bool((labels == 1).any()) == outliers
    # binary_cross_entropy: the reference's target is float32 under a float64 score, and so is its result
    _hold(f"{key}/{func}", lambda pred_logits, pred_masks: R.ref_outlier_loss(pred_logits, pred_masks, labels, combo[0], combo[1], func, G.THR_IN, G.THR_OUT),
          _inputs(key), G.REL32 if func == "binary_cross_entropy" else G.REL64)


@pytest.mark.parametrize("score", ("nls", "energy"))
def test_smoothness_and_sparsity_small(score):
    leaves, om = _inputs("small/reg"), _plane("small/reg", "outlier_masks")
    s = lambda pred_logits, pred_masks: P.ref_smoothness_score(pred_logits, pred_masks, score)
    _hold(f"small/reg/{score}/smoothness", lambda **lv: P.ref_smoothness(s(**lv)), leaves)
    _hold(f"small/reg/{score}/sparsity", lambda **lv: P.ref_sparsity(s(**lv), om), leaves)
    _hold(f"small/reg/{score}/sparsity_unlabelled", lambda **lv: P.ref_sparsity(s(**lv), None), leaves)
    assert float(G.load()[f"small/reg/{score}/sparsity_unlabelled/l64"]) == 0.0


@pytest.mark.parametrize("case,B", (("small", G.SMALL[0]), ("k19", G.K19[0])))
def test_densehybrid_loss(case, B):
    key = f"{case}/densehybrid"
    labels = _plane(key, "sem_seg", B)
    assert (labels == D.OUTLIER).any() and (labels == 255).any()
    _hold(key, lambda pred_logits, pred_masks, ood_pred: D.ref_densehybrid_loss(pred_logits, pred_masks, ood_pred, labels, G.BETA),
          _inputs(key, ("pred_logits", "pred_masks", "ood_pred")))


def test_densehybrid_loss_without_an_outlier_pixel_is_not_finite_in_the_reference():
    """the reference divides by the numel() of an empty selection: recorded, nothing further asserted"""
    assert not bool(G.load()["small/densehybrid/no_outlier_pixel_finite"])


@pytest.mark.parametrize("branch", ("out", "noout"))
def test_gambler_loss_k19(branch):
    key, B = f"k19/gambler/{branch}", G.K19[0]
    om, ss = _plane(key, "outlier_masks", B), _plane(key, "sem_seg", B)
    assert bool((om == 1).any()) == (branch == "out")
    _hold(key, lambda pred_logits, pred_masks: P.ref_gambler_loss(pred_logits, pred_masks, om, ss, G.OOD_REG), _inputs("k19/gambler/out"))


# ---------------------------------------------------------------------------------------------------------------- labels, masks, the plain functions
def _set_case():
    z = G.load()
    targets = [{"labels": G.t(z[f"small/set/t{i}_labels"]), "masks": _masks("small/set", i)} for i in range(len(G.SET_T))]
    indices = [(G.t(z[f"small/set/idx{i}_i"]), G.t(z[f"small/set/idx{i}_j"])) for i in range(len(G.SET_T))]
    return targets, indices, G.t(z["small/set/coords"])


def _padded(targets, indices, dtype):
    """the matched target masks, each zero-padded bottom / right to the batch's largest size, in the order of the images' pairs"""
    H, W = max(t["masks"].shape[-2] for t in targets), max(t["masks"].shape[-1] for t in targets)
    return torch.cat([F.pad(t["masks"][j], (0, W - t["masks"].shape[-1], 0, H - t["masks"].shape[-2])) for t, (_, j) in zip(targets, indices)]).to(dtype)


def test_loss_labels_small():
    targets, indices, _ = _set_case()
    assert [len(t["labels"]) for t in targets] == list(G.SET_T)
    assert bool(G.load()["small/set/loss_ce/l64_is_f32"])
    # the reference casts pred_logits to float32: the restatement under the same cast
    _hold("small/set/loss_ce", lambda pred_logits: C.ref_loss_labels(pred_logits.float(), targets, indices, G.SMALL[2], G.EOS),
          {"pred_logits": G.t(G.load()["small/set/loss_ce/in_pred_logits"])}, G.REL32)


def test_loss_masks_small():
    targets, indices, coords = _set_case()
    masks = G.t(G.load()["small/set/loss_mask/in_pred_masks"])
    Q = masks.shape[1]
    plane_index = torch.cat([b * Q + i for b, (i, _) in enumerate(indices)])
    assert len({tuple(t["masks"].shape[-2:]) for t in targets}) > 1 and targets[0]["masks"].shape[-2:] != masks.shape[-2:]

    def losses(pred_masks):
        labels = C.ref_point_sample(_padded(targets, indices, pred_masks.dtype), coords.to(pred_masks.dtype))
        return C.ref_mask_losses(pred_masks, plane_index, coords.to(pred_masks.dtype), labels, G.SET_NUM_MASKS)

    _hold("small/set/loss_mask", lambda pred_masks: losses(pred_masks)[0], {"pred_masks": masks})
    _hold("small/set/loss_dice", lambda pred_masks: losses(pred_masks)[1], {"pred_masks": masks})


def _centres(P_, dtype):
    """coordinates of the P pixel centres of a 1 x P plane: sampling there returns the plane's values (to one rounding of the coordinate)"""
    return torch.stack([(torch.arange(P_, dtype=dtype) + 0.5) / P_, torch.full((P_,), 0.5, dtype=dtype)], dim=-1)


def test_module_level_loss_functions():
    """dice_loss / sigmoid_ce_loss against ref_mask_losses and batch_dice_loss / batch_sigmoid_ce_loss against ref_match_cost in float64, the
    [N,P] arrays read as 1 x P planes sampled at their pixel centres (exact to a rounding of the coordinate, 2^-53 P)."""
    dtype, tag, bound = torch.float64, "64", G.REL64
    z = G.load()
    x, y, xq, yt = (G.t(z["small/fn/" + k]).to(dtype) for k in ("x", "y", "xq", "yt"))
    N, P_ = x.shape
    pts = _centres(P_, dtype)
    lm, ld = C.ref_mask_losses(x.view(1, N, 1, P_), torch.arange(N), pts[None].expand(N, -1, -1), y, float(z["small/fn/num_masks"]))
    _close("sigmoid_ce_loss", lm, z["small/fn/sigmoid_ce_loss" + tag], bound)
    _close("dice_loss", ld, z["small/fn/dice_loss" + tag], bound)
    Q, T = xq.shape[0], yt.shape[0]
    logits, ids = torch.zeros(Q, 3, dtype=dtype), torch.zeros(T, dtype=torch.int64)
    cost = lambda wm, wd: C.ref_match_cost(xq.view(Q, 1, P_), yt.view(T, 1, P_), pts, logits, ids, wm, 0.0, wd)
    _close("batch_sigmoid_ce_loss", cost(1.0, 0.0), z["small/fn/batch_sigmoid_ce_loss" + tag], bound)
    _close("batch_dice_loss", cost(0.0, 1.0), z["small/fn/batch_dice_loss" + tag], bound)


# ---------------------------------------------------------------------------------------------------------------- the matcher
def _cost(logits, pred, target, pts, dtype):
    w = G.MATCHER_WEIGHTS
    return C.ref_match_cost(pred.to(dtype), target["masks"].to(dtype), pts.to(dtype), logits.to(dtype), target["labels"], w["cost_mask"], w["cost_class"],
                            w["cost_dice"])


@pytest.mark.parametrize("n", range(len(G.MATCHER_SHAPES)))
def test_matcher_cost_and_assignment(n):
    from scipy.optimize import linear_sum_assignment
    z, key = G.load(), f"matcher/{n}"
    Q, T, P_, h, w = G.MATCHER_SHAPES[n]
    logits, pred, pts = G.t(z[key + "/in_pred_logits"])[0], G.t(z[key + "/in_pred_masks"])[0], G.t(z[key + "/coords"])
    target = {"labels": G.t(z[key + "/t0_labels"]), "masks": _masks(key, 0)}
    assert pred.shape == (Q, h, w) and target["masks"].shape == (T, 4 * h, 4 * w) and pts.shape == (P_, 2)
    c64 = _cost(logits, pred, target, pts, torch.float64)
    _close(key + " C64", c64, z[key + "/C64"], G.REL64)
    # the reference's C is float32 (``.float()`` on both sampled maps): the restatement in float32 at the pixel centres, where both samplers
    # return the same bits (tests/_criterion_ref_cases.matcher_inputs says why not at the uniform points)
    assert z[key + "/C32"].dtype == np.float32 and z[key + "/C32_centres"].dtype == np.float32
    _close(key + " C32 at centres", _cost(logits, pred, target, G.t(z[key + "/centres"]), torch.float32), z[key + "/C32_centres"], G.REL32)
    c32 = _cost(logits, pred, target, pts, torch.float32)
    print(f"{key} C32 at the uniform points: rel = {G.rel(c32, z[key + '/C32']):.3e} (not asserted)")
    for c in (c64, c32):
        i, j = linear_sum_assignment(c.numpy())
        assert np.array_equal(i, z[key + "/idx_i"]) and np.array_equal(j, z[key + "/idx_j"])


def test_matcher_without_a_target_returns_an_empty_assignment_in_the_reference():
    z = G.load()
    assert not bool(z["matcher/empty/raises"]) and int(z["matcher/empty/idx_len"]) == 0


# ---------------------------------------------------------------------------------------------------------------- SetCriterion.forward
def _forward_case():
    z = G.load()
    leaves = {k[len("forward/in_"):]: G.t(z[k]) for k in z if k.startswith("forward/in_")}
    B = G.K19[0]
    targets = [{"labels": G.t(z[f"forward/t{i}_labels"]), "masks": _masks("forward", i), "outlier_masks": G.t(z[f"forward/t{i}_outlier_masks"]),
                "sem_seg": G.t(z[f"forward/t{i}_sem_seg"])} for i in range(B)]
    indices = [[(G.t(z[f"forward/idx{e}_{b}_i"]), G.t(z[f"forward/idx{e}_{b}_j"])) for b in range(B)] for e in range(G.FWD_AUX + 1)]
    return leaves, targets, indices, G.t(z["forward/matcher_coords"]), G.t(z["forward/loss_coords"])


def _entries(lv):
    return [(lv["pred_logits"], lv["pred_masks"])] + [(lv[f"aux{i}_pred_logits"], lv[f"aux{i}_pred_masks"]) for i in range(G.FWD_AUX)]


def _restated_forward(name, lv, targets, indices, lcoords):
    """the three recipes' criteria as the GPU suites restate them: every entry's losses under the key suffix ``_{i}``; DenseHybrid for the final
    outputs only"""
    K, dtype = G.K19[2], lv["pred_masks"].dtype
    om, ss = torch.stack([t["outlier_masks"] for t in targets]), torch.stack([t["sem_seg"] for t in targets])
    if name == "densehybrid":
        return {"densehybrid_loss": D.ref_densehybrid_loss(lv["pred_logits"], lv["pred_masks"], lv["ood_pred"], ss, G.BETA)}
    losses = {}
    for e, (lg, mk) in enumerate(_entries(lv)):
        if name == "pebal":
            entry = P.ref_pebal_entry(lg, mk, om, ss)
        else:
            tg = [{k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()} for t in targets]
            num_masks = float(max(sum(len(t["labels"]) for t in targets), 1))
            entry = C.ref_criterion(lg, mk, tg, indices[e], num_masks, lcoords.to(dtype), K, G.EOS)
            entry["loss_ce"] = C.ref_loss_labels(lg.float(), targets, indices[e], K, G.EOS)       # the reference's cast
        losses.update({(k if e == 0 else f"{k}_{e - 1}"): v for k, v in entry.items()})
    return losses


@pytest.mark.parametrize("name", sorted(G.FORWARDS))
def test_set_criterion_forward(name):
    z = G.load()
    leaves, targets, indices, mcoords, lcoords = _forward_case()
    names = G.forward_leaves(name)
    seen = {}

    def total(**lv):
        losses = _restated_forward(name, {**{k: v.double() for k, v in leaves.items()}, **lv}, targets, indices, lcoords)
        seen.update({k: v.detach() for k, v in losses.items()})
        return sum(v * G.weight_of(name, k) for k, v in losses.items())

    # loss_ce is float32 arithmetic in the reference: its share of the total and of d total / d pred_logits carries one float32 rounding
    _hold(f"forward/{name}/total", total, {k: leaves[k] for k in names}, G.REL32 if name == "mix" else G.REL64)
    assert sorted(seen) == list(z[f"forward/{name}/keys"])
    if name == "densehybrid":
        assert list(z["forward/densehybrid/keys"]) == ["densehybrid_loss"], "the reference skips the DenseHybrid loss for aux_outputs entries"
    for k, v in seen.items():
        _close(f"forward/{name}/{k}", v, z[f"forward/{name}/{k}/l64"], G.REL32 if k.startswith("loss_ce") else G.REL64)


def test_set_criterion_forward_matching_is_the_restated_costs_optimum():
    """every entry's and image's assignment in the fixture is the optimum of the restated cost, in float32 and in float64"""
    from scipy.optimize import linear_sum_assignment
    leaves, targets, indices, mcoords, _ = _forward_case()
    for e, (lg, mk) in enumerate(_entries(leaves)):
        for b, target in enumerate(targets):
            for dtype in (torch.float64, torch.float32):
                i, j = linear_sum_assignment(_cost(lg[b], mk[b], target, mcoords, dtype).numpy())
                assert np.array_equal(i, indices[e][b][0].numpy()) and np.array_equal(j, indices[e][b][1].numpy()), (e, b, dtype)


# ---------------------------------------------------------------------------------------------------------------- the recipe crop
def _crop(case):
    leaves, targets = G.crop_cases()[case]
    z = G.load()
    for i, tg in enumerate(targets):
        for k, v in tg.items():
            assert G.crc(v) == z[f"crop/{case}/crc_t{i}_{k}"], f"crop/{case}: the seeded draw of target {i} {k} has drifted"
    return leaves, targets


@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("combo", R.COMBOS, ids="_".join)
def test_outlier_loss_crop(combo, func):
    case = "outlier/" + "_".join(combo)
    leaves, targets = _crop(case)
    labels = torch.stack([t["outlier_masks"] for t in targets])
    _hold(f"crop/{case}/{func}", lambda pred_logits, pred_masks: R.ref_outlier_loss(pred_logits, pred_masks, labels, combo[0], combo[1], func, G.THR_IN, G.THR_OUT),
          leaves, G.REL32 if func == "binary_cross_entropy" else G.REL64, sums=True)


def test_densehybrid_loss_crop():
    leaves, targets = _crop("densehybrid")
    labels = torch.stack([t["sem_seg"] for t in targets])
    _hold("crop/densehybrid/loss", lambda pred_logits, pred_masks, ood_pred: D.ref_densehybrid_loss(pred_logits, pred_masks, ood_pred, labels, G.BETA), leaves,
          sums=True)


def test_pebal_losses_crop():
    leaves, targets = _crop("pebal")
    om, ss = torch.stack([t["outlier_masks"] for t in targets]), torch.stack([t["sem_seg"] for t in targets])
    _hold("crop/pebal/gambler", lambda pred_logits, pred_masks: P.ref_gambler_loss(pred_logits, pred_masks, om, ss, G.OOD_REG), leaves, sums=True)
    s = lambda pred_logits, pred_masks: P.ref_smoothness_score(pred_logits, pred_masks, "energy")
    _hold("crop/pebal/smoothness", lambda **lv: P.ref_smoothness(s(**lv)), leaves, sums=True)
    _hold("crop/pebal/sparsity", lambda **lv: P.ref_sparsity(s(**lv), om), leaves, sums=True)


# ---------------------------------------------------------------------------------------------------------------- the fixture itself
def _reference_tree():
    spec = importlib.util.spec_from_file_location("_make_golden_for_its_paths", MAKE_GOLDEN)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.REF


def test_fixture_regenerates_identically():
    """the generator, run again, builds the committed arrays bit for bit (in memory: ``--check`` writes nothing).  It runs in a process of its own:
    its stand-in modules (detectron2, torchvision, ...) must not be visible to the other tests."""
    ref = _reference_tree()
    if not os.path.isdir(os.path.join(ref, "mask2former")):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, MAKE_GOLDEN, "--only", "g9_criterion", "--check"], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, "g9_criterion.npz is not what the generator builds today"
