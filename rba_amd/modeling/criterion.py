"""The reference's outlier-supervision loss (``SetCriterion.outlier_loss``, mask2former/modeling/criterion.py:435-553) on the HIP kernels:
the score of criterion.py:449-465 -- softmax / sigmoid, ``einsum("bqc,bqhw->bchw")``, tanh-sum | logsumexp | sum -- is K1 at the mask
resolution (``ops.rba_reduce``), and its gradient is K1's backward kernel (``ops.rba_reduce_backward``).  Everything around it is small
and stays torch with autograd: the class softmax ([Q, K+1] per image), the ``align_corners=True`` upsample of the one-channel score map and
the masked means.  This is what the outlier-supervised fine-tune (``..._1dl_coco_mix_finetune.yaml``: backbone, pixel decoder and the
transformer decoder but its two heads frozen) differentiates; the matcher, the other losses and the trainer are not part of this library.
"""
import torch
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops

# (OUTLIER_LOSS_TARGET, SCORE_NORM) -> K1 score mode; SCORE_NORM is read only by the "nls" target (criterion.py:456-465)
_NLS_SCORES = {"tanh": "rba", "none": "neg_logit_sum"}
TARGETS = ("nls", "energy")
FUNCS = ("squared_hinge", "binary_cross_entropy", "mse", "l1")


class RbaScoreFunction(Function):
    """``RbaScoreFunction.apply(mask_pred [B,Q,h,w], cls_prob [B,Q,K], score) -> [B,h,w]``: ``ops.rba_reduce`` image by image (the very bits
    of a direct call), differentiable once with respect to both tensors through ``ops.rba_reduce_backward``.  ``score`` is one of
    ``ops.SCORE_MODES``.  Only the two inputs are saved; a gradient nobody asks for is not computed."""

    @staticmethod
    def forward(ctx, mask_pred, cls_prob, score="rba"):
        if mask_pred.dim() != 4 or cls_prob.dim() != 3 or cls_prob.shape[:2] != mask_pred.shape[:2]:
            raise ops.RbaHipError(f"RbaScoreFunction: mask_pred [B,Q,h,w] and cls_prob [B,Q,K], got {tuple(mask_pred.shape)} and {tuple(cls_prob.shape)}")
        mask_pred, cls_prob = mask_pred.contiguous(), cls_prob.contiguous()
        ctx.score = score
        ctx.save_for_backward(mask_pred, cls_prob)
        return torch.stack([ops.rba_reduce(m, p, score=score)[0] for m, p in zip(mask_pred, cls_prob)])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_score):
        mask_pred, cls_prob = ctx.saved_tensors
        need_mask, need_prob = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_mask or need_prob):
            return None, None, None
        grad_score = grad_score.contiguous()                 # `score.sum().backward()` hands an expanded (stride 0) gradient
        grads = [ops.rba_reduce_backward(m, p, g, score=ctx.score, need_mask=need_mask, need_prob=need_prob)
                 for m, p, g in zip(mask_pred, cls_prob, grad_score)]
        return (torch.stack([gm for gm, _ in grads]) if need_mask else None,
                torch.stack([gp for _, gp in grads]) if need_prob else None, None)


def _score_mode(target, score_norm):
    if target == "nls":
        if score_norm not in _NLS_SCORES:
            raise ValueError(f"outlier_loss: score_norm {score_norm!r} is not built for target 'nls' (built: {sorted(_NLS_SCORES)})")
        return _NLS_SCORES[score_norm]
    if target == "energy":
        return "energy"
    raise ValueError(f"outlier_loss: target {target!r} is not built (built: {list(TARGETS)})")


def outlier_loss(outputs, targets, *, target="nls", score_norm="tanh", func="squared_hinge", inlier_upper_threshold=-1.0,
                 outlier_lower_threshold=-0.1):
    """``SetCriterion.outlier_loss`` (criterion.py:435-553; the matcher's ``indices`` and ``num_masks`` are unused there and absent here).
    outputs["pred_logits"] [B,Q,K+1], outputs["pred_masks"] [B,Q,h,w]; targets[i]["outlier_masks"] [H,W] with 1 = outlier, 0 = inlier,
    anything else ignored -> {"outlier_loss": scalar}.  Kept from the reference: without an outlier pixel the inlier term is not halved
    (:483-487), and an empty inlier set gives NaN (the mean of nothing).  Not built (ValueError): target "softmax_entropy" / "sum_entropy",
    score_norm "sigmoid", func "kl"."""
    mode = _score_mode(target, score_norm)
    if func not in FUNCS:
        raise ValueError(f"outlier_loss: func {func!r} is not built (built: {list(FUNCS)})")
    labels = torch.stack([t["outlier_masks"] for t in targets])                      # [B,H,W]
    ood, ind = labels == 1, labels == 0
    cls_prob = F.softmax(outputs["pred_logits"], dim=-1)[..., :-1]
    score = RbaScoreFunction.apply(outputs["pred_masks"], cls_prob, mode)            # [B,h,w]
    score = F.interpolate(score[:, None], size=labels.shape[-2:], mode="bilinear", align_corners=True)[:, 0]
    if func == "binary_cross_entropy":
        return {"outlier_loss": 0.5 * F.binary_cross_entropy_with_logits(score, ood.to(score.dtype))}
    d_in, d_out = score[ind] - inlier_upper_threshold, outlier_lower_threshold - score[ood]
    if func == "squared_hinge":
        term = lambda d: F.relu(d).pow(2).mean()
    elif func == "mse":
        term = lambda d: d.pow(2).mean()
    else:
        term = lambda d: d.abs().mean()
    loss = term(d_in)
    if d_out.numel() > 0:
        loss = 0.5 * (loss + term(d_out))
    return {"outlier_loss": loss}


# mask2former/config.py:188-227, the values in force after the file's last assignment of each key
_CFG_DEFAULTS = {"OUTLIER_LOSS_TARGET": "none", "SCORE_NORM": "none", "OUTLIER_LOSS_FUNC": "squared_hinge", "INLIER_UPPER_THRESHOLD": -1.0,
                 "OUTLIER_LOWER_THRESHOLD": -0.1}


def outlier_loss_from_cfg(cfg):
    """The loss a config selects: reads OUTLIER_LOSS_TARGET, SCORE_NORM, OUTLIER_LOSS_FUNC, INLIER_UPPER_THRESHOLD and OUTLIER_LOWER_THRESHOLD
    under MODEL.MASK_FORMER of ``rba_amd.config.load_cfg``'s result (absent keys: the defaults of mask2former/config.py:188-227) and returns
    ``loss(outputs, targets)``, a closure over ``outlier_loss``; its ``.keywords`` holds the five settings.  A combination that is not built
    raises ValueError here, not at the first step."""
    import functools
    mf = cfg.get("MODEL", {}).get("MASK_FORMER", {})
    v = {k: mf.get(k, d) for k, d in _CFG_DEFAULTS.items()}
    kw = dict(target=str(v["OUTLIER_LOSS_TARGET"]), score_norm=str(v["SCORE_NORM"]), func=str(v["OUTLIER_LOSS_FUNC"]),
              inlier_upper_threshold=float(v["INLIER_UPPER_THRESHOLD"]), outlier_lower_threshold=float(v["OUTLIER_LOWER_THRESHOLD"]))
    _score_mode(kw["target"], kw["score_norm"])
    if kw["func"] not in FUNCS:
        raise ValueError(f"outlier_loss: func {kw['func']!r} is not built (built: {list(FUNCS)})")
    return functools.partial(outlier_loss, **kw)
