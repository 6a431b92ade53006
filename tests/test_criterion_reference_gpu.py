"""The product's criterion and matcher (rba_amd.modeling.criterion / .matcher on the HIP kernels) held to tests/golden/g9_criterion.npz, which the
reference's own ``criterion.py`` and ``matcher.py`` wrote: the "small", "k19", matcher and ``SetCriterion.forward`` cases.  Only the ``.npz`` is
read.  Bars: tensors ``4 max(b, 2^-20)`` (tests/_rba_bwd_cases.py) and scalars ``scalar_bar`` (tests/_point_loss_cases.py), with b, l32 and l64
taken from the fixture -- the float32 reference's distance from the float64 reference -- never from the code under test.  The matcher's
assignment and the criteria's key sets must equal the reference's exactly."""
import numpy as np
import pytest
import torch

from tests import _criterion_ref_cases as G
from tests import _point_loss_cases as C
from tests import _rba_bwd_cases as R
from tests.test_criterion_reference_cpu import _forward_case, _inputs, _masks, _plane, _set_case

pytestmark = pytest.mark.gpu


def _cuda(targets):
    return [{k: v.cuda() for k, v in t.items()} for t in targets]


def _hold(key, fn, leaves):
    """the product's float32 loss and gradients on the GPU against the fixture's entry ``key``"""
    z = G.load()
    lv = {k: v.cuda().requires_grad_(True) for k, v in leaves.items()}
    loss = fn(**lv)
    if loss.requires_grad:
        loss.backward()
    C.check_scalar(key, loss.detach(), z[key + "/l32"], z[key + "/l64"])
    for k, v in lv.items():
        ref = G.t(z[f"{key}/g_{k}"])
        if float(ref.abs().max()) == 0:
            assert v.grad is None or float(v.grad.abs().max()) == 0, f"{key}: the reference's gradient of {k} is zero"
        else:
            assert v.grad is not None, f"{key}: no gradient for {k}"
            R.check(f"{key} grad {k}", v.grad.cpu(), ref, float(z[f"{key}/b_{k}"]))


# ---------------------------------------------------------------------------------------------------------------- the dense losses
@pytest.mark.parametrize("outliers", (True, False), ids=("out", "noout"))
@pytest.mark.parametrize("func", R.FUNCS)
@pytest.mark.parametrize("combo", R.COMBOS, ids="_".join)
def test_outlier_loss_small(combo, func, outliers):
    from rba_amd.modeling.criterion import outlier_loss
    key = f"small/outlier/{'_'.join(combo)}/{'out' if outliers else 'noout'}"
    targets = _cuda([{"outlier_masks": x} for x in _plane(key, "outlier_masks")])
    _hold(f"{key}/{func}", lambda **lv: outlier_loss(lv, targets, target=combo[0], score_norm=combo[1], func=func, inlier_upper_threshold=G.THR_IN,
                                                     outlier_lower_threshold=G.THR_OUT)["outlier_loss"], _inputs(key))


@pytest.mark.parametrize("score", ("nls", "energy"))
def test_smoothness_and_sparsity_small(score):
    from rba_amd.modeling.criterion import smoothness_loss, sparsity_loss
    leaves = _inputs("small/reg")
    targets = _cuda([{"outlier_masks": x} for x in _plane("small/reg", "outlier_masks")])
    _hold(f"small/reg/{score}/smoothness", lambda **lv: smoothness_loss(lv, targets, score=score)["smoothness_loss"], leaves)
    _hold(f"small/reg/{score}/sparsity", lambda **lv: sparsity_loss(lv, targets, score=score)["sparsity_loss"], leaves)
    _hold(f"small/reg/{score}/sparsity_unlabelled", lambda **lv: sparsity_loss(lv, [{} for _ in targets], score=score)["sparsity_loss"], leaves)


@pytest.mark.parametrize("case,shape", (("small", G.SMALL), ("k19", G.K19)))
def test_densehybrid_loss(case, shape):
    from rba_amd.modeling.criterion import densehybrid_loss
    key = f"{case}/densehybrid"
    targets = _cuda([{"sem_seg": x} for x in _plane(key, "sem_seg", shape[0])])
    _hold(key, lambda **lv: densehybrid_loss(lv, targets, num_classes=shape[2], beta=G.BETA)["densehybrid_loss"],
          _inputs(key, ("pred_logits", "pred_masks", "ood_pred")))


@pytest.mark.parametrize("branch", ("out", "noout"))
def test_gambler_loss_k19(branch):
    from rba_amd.modeling.criterion import gambler_loss
    key, (B, _, K) = f"k19/gambler/{branch}", G.K19[:3]
    targets = _cuda([{"outlier_masks": a, "sem_seg": b} for a, b in zip(_plane(key, "outlier_masks", B), _plane(key, "sem_seg", B))])
    _hold(key, lambda **lv: gambler_loss(lv, targets, num_classes=K, ood_reg=G.OOD_REG)["gambler_loss"], _inputs("k19/gambler/out"))


# ---------------------------------------------------------------------------------------------------------------- labels and masks
def test_loss_labels_small():
    from rba_amd.modeling.criterion import loss_labels
    targets, indices, _ = _set_case()
    _hold("small/set/loss_ce", lambda **lv: loss_labels(lv, _cuda(targets), indices, num_classes=G.SMALL[2], eos_coef=G.EOS)["loss_ce"],
          {"pred_logits": G.t(G.load()["small/set/loss_ce/in_pred_logits"])})


@pytest.mark.parametrize("name", ("loss_mask", "loss_dice"))
def test_loss_masks_small(name):
    from rba_amd.modeling.criterion import loss_masks
    targets, indices, coords = _set_case()
    _hold(f"small/set/{name}", lambda **lv: loss_masks(lv, _cuda(targets), indices, G.SET_NUM_MASKS, num_points=G.SET_P, oversample_ratio=3.0,
                                                      importance_sample_ratio=0.75, point_coords=coords.cuda())[name],
          {"pred_masks": G.t(G.load()["small/set/loss_mask/in_pred_masks"])})


# ---------------------------------------------------------------------------------------------------------------- the matcher
def _matcher(num_points):
    from rba_amd.modeling.matcher import HungarianMatcher
    return HungarianMatcher(num_points=num_points, **G.MATCHER_WEIGHTS)


@pytest.mark.parametrize("n", range(len(G.MATCHER_SHAPES)))
def test_matcher_cost_and_assignment(n):
    z, key = G.load(), f"matcher/{n}"
    logits, pred, pts = G.t(z[key + "/in_pred_logits"]).cuda(), G.t(z[key + "/in_pred_masks"]).cuda(), G.t(z[key + "/coords"]).cuda()
    target = {"labels": G.t(z[key + "/t0_labels"]).cuda(), "masks": _masks(key, 0).cuda()}
    matcher = _matcher(G.MATCHER_SHAPES[n][2])
    cost = matcher.cost_matrix(logits[0], pred[0], target, point_coords=pts)
    R.check(key + " C", cost.cpu(), G.t(z[key + "/C64"]), float(z[key + "/b"]))
    empty = {"labels": target["labels"][:0], "masks": target["masks"][:0]}
    idx = matcher({"pred_logits": torch.cat([logits, logits]), "pred_masks": torch.cat([pred, pred])}, [target, empty], point_coords=pts)
    assert np.array_equal(idx[0][0].numpy(), z[key + "/idx_i"]) and np.array_equal(idx[0][1].numpy(), z[key + "/idx_j"])
    assert idx[1][0].numel() == idx[1][1].numel() == int(z["matcher/empty/idx_len"]) == 0       # the reference: an empty assignment, no error
    cost = matcher.cost_matrix(logits[0], pred[0], target, point_coords=G.t(z[key + "/centres"]).cuda())
    R.check(key + " C at the pixel centres", cost.cpu(), G.t(z[key + "/C32_centres"]).double(), R.FLOOR)      # a float32 truth: the floor alone


# ---------------------------------------------------------------------------------------------------------------- the three recipes' criteria
def _weights(name):
    w = dict(G.FORWARDS[name]["weights"])
    w.update({f"{k}_{i}": v for i in range(G.FWD_AUX) for k, v in G.FORWARDS[name]["weights"].items()})
    return w


def _criterion(name):
    from rba_amd.modeling import criterion as M
    K, s = G.K19[2], G.FORWARDS[name]["settings"]
    outlier = dict(target=s["outlier_loss_target"], score_norm=s["score_norm"], func=s["outlier_loss_func"], inlier_upper_threshold=G.THR_IN,
                   outlier_lower_threshold=G.THR_OUT)
    if name == "mix":
        return M.SetCriterion(K, _matcher(G.FWD_PM), _weights(name), G.EOS, G.FORWARDS[name]["losses"], G.FWD_PL, 3.0, 0.75, **outlier)
    if name == "pebal":
        return M.PebalCriterion(K, _weights(name), G.FORWARDS[name]["losses"], G.OOD_REG, s["smoothness_score"], **outlier)
    return None


@pytest.mark.parametrize("name", sorted(G.FORWARDS))
def test_criterion_forward(name):
    from rba_amd.modeling.criterion import densehybrid_loss
    z = G.load()
    leaves, targets, indices, mcoords, lcoords = _forward_case()
    targets, crit, seen = _cuda(targets), _criterion(name), {}

    def total(**lv):
        outputs = G.outputs_of({**{k: v.cuda() for k, v in leaves.items()}, **lv}, ood=(name == "densehybrid"))
        if name == "mix":
            losses = crit(outputs, targets, matcher_point_coords=mcoords.cuda(), loss_point_coords=lcoords.cuda())
        elif name == "pebal":
            losses = crit(outputs, targets)
        else:                                                       # the DenseHybrid recipe's criterion is the one loss, of the final outputs only
            losses = densehybrid_loss(outputs, targets, num_classes=G.K19[2], beta=G.BETA)
        seen.update(losses)
        return sum(v * G.weight_of(name, k) for k, v in losses.items())

    _hold(f"forward/{name}/total", total, {k: leaves[k] for k in G.forward_leaves(name)})
    assert sorted(seen) == list(z[f"forward/{name}/keys"])
    for k, v in seen.items():
        C.check_scalar(f"forward/{name}/{k}", v.detach(), z[f"forward/{name}/{k}/l32"], z[f"forward/{name}/{k}/l64"])


def test_set_criterion_matches_every_entry_as_the_reference_does():
    leaves, targets, indices, mcoords, _ = _forward_case()
    matcher, targets = _matcher(G.FWD_PM), _cuda(targets)
    entries = [{"pred_logits": leaves["pred_logits"], "pred_masks": leaves["pred_masks"]}] + G.outputs_of(leaves)["aux_outputs"]
    for e, entry in enumerate(entries):
        got = matcher({k: v.cuda() for k, v in entry.items()}, targets, point_coords=mcoords.cuda())
        for b, (i, j) in enumerate(got):
            assert torch.equal(i, indices[e][b][0]) and torch.equal(j, indices[e][b][1]), (e, b)
