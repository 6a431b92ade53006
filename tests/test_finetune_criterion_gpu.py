"""The fine-tune recipe's whole weighted loss -- labels + masks + outlier behind the Hungarian matcher (rba_amd.modeling.criterion.SetCriterion) -- on
rba_amd's own model with differentiable heads (the fixture model of tests/test_finetune_heads_gpu.py): the gradients of the ten head tensors against
fp64 CPU autograd of the restated heads (tests/_k4_bwd_cases.py) plus the restated criterion (tests/_point_loss_cases.py) under the same indices and
point coordinates, a step that lowers the loss, and inference untouched.  Bar: tests/_rba_bwd_cases.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import _k4_bwd_cases as K4
from tests import _point_loss_cases as C
from tests.test_finetune_heads_gpu import _captured_last_head_call, _head_params, _tiny

pytestmark = pytest.mark.gpu

T, P, EOS = 3, 112, 0.1
BASE = ("loss_ce", "loss_mask", "loss_dice", "outlier_loss")
WEIGHTS = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "outlier_loss": 1.0}
_STATE = {}


class _Frozen(torch.nn.Module):
    """a matcher that repeats a given assignment: the loss stays one fixed function of the parameters across a step"""

    def __init__(self, indices):
        super().__init__()
        self.indices = indices

    def forward(self, outputs, targets, point_coords=None, generator=None):
        return self.indices


def _criterion(K, matcher):
    from rba_amd.modeling.criterion import SetCriterion
    weights = dict(WEIGHTS)
    weights.update({f"{k}_0": v for k, v in WEIGHTS.items()})
    return SetCriterion(K, matcher, weights, EOS, ["labels", "masks", "outlier"], P, 3.0, 0.75, target="nls", score_norm="tanh", func="squared_hinge",
                        inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)


def _fixture():
    """(model, image, targets on the GPU, targets on the CPU, matcher points [P,2], loss points [T,P,2]): T targets that are thresholded enlargements of T
    of the model's own predicted masks, so that the matching is far from a tie"""
    if not _STATE:
        model, image, outlier = _tiny()
        model = copy.deepcopy(model)                              # the other file's model stays as it is
        # deep supervision needs every intermediate head's full mask logits (the inference shortcut leaves aux_outputs with pred_logits only)
        model.sem_seg_head.predictor.sparse_intermediate_heads = False
        with torch.no_grad():
            outputs, _, _ = model.finetune_outputs([{"image": image}])
        masks = outputs["pred_masks"].detach().cpu()
        Q, K = masks.shape[1], outputs["pred_logits"].shape[-1] - 1
        gen = torch.Generator().manual_seed(8600)
        rows = torch.randperm(Q, generator=gen)[:T]
        up = F.interpolate(masks[:, rows], size=tuple(outlier.shape), mode="bilinear", align_corners=False)[0]
        target = {"labels": torch.randint(0, K, (T,), generator=gen), "masks": (up > up.median()).float(), "outlier_masks": outlier.cpu()}
        coords = torch.rand(P, 2, generator=gen), torch.rand(T, P, 2, generator=gen)
        _STATE["f"] = (model, image, [{k: v.cuda() for k, v in target.items()}], [target], coords[0].cuda(), coords[1].cuda(), K)
    return _STATE["f"]


def _differentiable_total(crit, losses):
    """the weighted losses that carry a gradient: the final outputs' four (deep supervision stays detached)"""
    w = crit.weighted(losses)
    assert set(w) == set(crit.weight_dict)
    assert {k for k, v in w.items() if v.requires_grad} == set(BASE)
    return sum(w[k] for k in BASE)


def test_every_head_tensor_gets_the_restated_gradient():
    from rba_amd.modeling.matcher import HungarianMatcher
    model, image, targets, targets_cpu, mcoords, lcoords, K = _fixture()
    pred = model.sem_seg_head.predictor
    crit = _criterion(K, HungarianMatcher(WEIGHTS["loss_ce"], WEIGHTS["loss_mask"], WEIGHTS["loss_dice"], P))
    for p in model.parameters():
        p.requires_grad_(True)
        p.grad = None
    try:
        def run():
            outputs, _, _ = model.finetune_outputs([{"image": image}])
            indices = crit.matcher(outputs, targets, point_coords=mcoords)
            return crit(outputs, targets, matcher_point_coords=mcoords, loss_point_coords=lcoords), indices, outputs

        (losses, indices, outputs), (dec_out, feat) = _captured_last_head_call(pred, run)
        assert len(outputs["aux_outputs"]) == 1 and set(losses) == set(BASE) | {k + "_0" for k in BASE}
        assert indices[0][0].numel() == T
        total = _differentiable_total(crit, losses)
        total.backward()
        heads = _head_params(pred)
        assert {id(p) for p in model.parameters() if p.grad is not None} == {id(p) for p in heads.values()}

        def truth(dtype):
            p = {n: heads[n].detach().cpu().to(dtype).clone().requires_grad_(True) for n in K4.HEAD_TENSORS}
            cls, masks = K4.ref_heads(dec_out.detach().cpu().to(dtype), feat.detach().cpu().to(dtype), p)
            tg = [{k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()} for t in targets_cpu]
            out = C.ref_criterion(cls, masks, tg, indices, float(T), lcoords.cpu().to(dtype), K, EOS)
            sum(WEIGHTS[k] * out[k] for k in BASE).backward()
            return out, {n: t.grad for n, t in p.items()}

        l64, g64 = truth(torch.float64)
        l32, g32 = truth(torch.float32)
        for k in BASE:
            C.check_scalar(k, losses[k].detach(), l32[k], l64[k])
        assert all(float(g.abs().max()) > 0 for g in g64.values())
        for n in K4.HEAD_TENSORS:
            C.check(f"grad {n}", heads[n].grad.cpu(), g64[n], C.err(g32[n], g64[n]))
    finally:
        for p in model.parameters():
            p.grad = None


def test_step_lowers_the_total_and_inference_is_untouched():
    from rba_amd.modeling.matcher import HungarianMatcher
    model, image, targets, _, mcoords, lcoords, K = _fixture()
    batch = [{"image": image}]
    logits0, masks0, _, _ = model.predict(batch)                  # before anything of the criterion has run on this copy
    model = copy.deepcopy(model)
    pred = model.sem_seg_head.predictor
    heads = _head_params(pred)
    for p in heads.values():
        p.requires_grad_(True)
    outputs, _, _ = model.finetune_outputs(batch)
    assert torch.equal(outputs["pred_logits"], logits0) and torch.equal(outputs["pred_masks"], masks0)
    indices = HungarianMatcher(WEIGHTS["loss_ce"], WEIGHTS["loss_mask"], WEIGHTS["loss_dice"], P)(outputs, targets, point_coords=mcoords)
    crit = _criterion(K, _Frozen(indices))

    def total():
        out, _, _ = model.finetune_outputs(batch)
        return _differentiable_total(crit, crit(out, targets, loss_point_coords=lcoords))

    loss = total()
    loss.backward()
    before = float(loss.detach())
    sq = sum(float((p.grad.double() ** 2).sum()) for p in heads.values())
    lr = 0.01 * before / sq                                  # one SGD step sized for a first-order decrease of 1 % of the loss
    with torch.no_grad():
        for p in heads.values():
            p -= lr * p.grad
    after = float(total().detach())
    print(f"total {before:.6f} -> {after:.6f}")
    assert after < before
    pred.differentiable_heads = False                             # the flag off: predict is what it was before the flag existed, on the stepped weights too
    try:
        logits1, masks1, _, _ = model.predict(batch)
    finally:
        pred.differentiable_heads = True
    logits2, masks2, _, _ = model.predict(batch)
    assert torch.equal(logits1, logits2) and torch.equal(masks1, masks2) and not torch.equal(masks1, masks0)
