"""The fine-tune recipe's criterion (``SetCriterion``, mask2former/modeling/criterion.py) on the HIP kernels.

``outlier_loss`` (criterion.py:435-553): the score of criterion.py:449-465 -- softmax / sigmoid, ``einsum("bqc,bqhw->bchw")``, tanh-sum |
logsumexp | sum -- is K1 at the mask resolution (``ops.rba_reduce``), and its gradient is K1's backward kernel (``ops.rba_reduce_backward``).
The tail behind the score map (criterion.py:474-518) -- the ``align_corners=True`` upsample of the one-channel score map to the labels' size, the
per-class terms, the masked means and the halving rule -- is K9 (``ops.outlier_tail`` / ``ops.outlier_tail_backward`` behind
``OutlierTailFunction``): the counts and the "any outlier pixel" decision stay on the device, so the loss performs no host synchronisation.  Only
the class softmax ([Q, K+1] per image) stays torch.

``loss_masks`` (criterion.py:194-243): the uncertainty oversampling, the label sampling and the two point-sampled losses with their scatter
backward are K8 (``ops.point_sample``, ``ops.mask_point_loss``, ``ops.mask_point_loss_backward``); no ``grid_sample`` call.  ``loss_labels``
(criterion.py:174-192) is plain torch.  ``SetCriterion`` is the reference's ``forward`` over these three losses behind a matcher
(``rba_amd.modeling.matcher``), ``aux_outputs`` included: they carry a gradient when the decoder's ``deep_supervision`` is set beside
``differentiable_heads``.

``densehybrid_loss`` (criterion.py:390-433), the whole criterion of the DenseHybrid fine-tune recipe (its loss list is ``["densehybrid"]`` alone,
maskformer_model.py:166-169): the class map ``einsum("bqc,bqhw->bchw")`` is K1's ``sem_seg`` output at the mask resolution behind
``SemSegFunction`` (backward: K1's per-class adjoint, ``ops.sem_seg_backward``), and everything behind it -- the two ``align_corners=True``
upsamples to the labels' size, log_softmax, logsumexp, get_batch_avg and the two nll_loss -- is K10 (``ops.dense_hybrid_loss`` /
``ops.dense_hybrid_loss_backward`` behind ``DenseHybridLossFunction``); the up-sampled maps never exist.  ``SetCriterion`` does not take
"densehybrid": the function is called directly.

``gambler_loss``, ``smoothness_loss`` and ``sparsity_loss`` (criterion.py:245-388), with ``outlier_loss`` the loss list of the PEBAL fine-tune
recipe (maskformer_model.py:164-175): the gambler loss behind its (K+1)-channel class map -- the upsample, softmax, the squared-logsumexp
reward and its Gaussian blur (through which the gradient flows), the masked log terms and the host-side "any outlier pixel" branch -- is K11a
(``ops.gambler_loss`` / ``ops.gambler_loss_backward`` behind ``GamblerLossFunction``); the two regularisers behind K1's score map are K11b
(``ops.score_reg`` / ``ops.score_reg_backward`` behind ``ScoreRegFunction``).  ``pebal_criterion_from_cfg`` builds the recipe's whole criterion
(``PebalCriterion``: no matcher -- these losses ignore its indices); ``SetCriterion`` does not take the three names.  Data mappers and the
trainer are not part of this library.
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


class OutlierTailFunction(Function):
    """``OutlierTailFunction.apply(score [B,h,w], labels [B,H,W] int64 | uint8, func, thr_in, thr_out) -> loss`` (a scalar): ``ops.outlier_tail``
    (the very bits of a direct call), differentiable once with respect to ``score`` only through ``ops.outlier_tail_backward``.  Saved: score,
    labels and the four sums.  No host synchronisation in either direction."""

    @staticmethod
    def forward(ctx, score, labels, func, thr_in, thr_out):
        score, labels = score.contiguous(), labels.contiguous()
        loss, stats = ops.outlier_tail(score, labels, func, thr_in, thr_out)
        ctx.settings = (func, thr_in, thr_out)
        ctx.save_for_backward(score, labels, stats)
        return loss.view(())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        score, labels, stats = ctx.saved_tensors
        return ops.outlier_tail_backward(score, labels, stats, grad_loss.contiguous(), *ctx.settings), None, None, None, None


def _score_mode(target, score_norm):
    if target == "nls":
        if score_norm not in _NLS_SCORES:
            raise ValueError(f"outlier_loss: score_norm {score_norm!r} is not built for target 'nls' (built: {sorted(_NLS_SCORES)})")
        return _NLS_SCORES[score_norm]
    if target == "energy":
        return "energy"
    raise ValueError(f"outlier_loss: target {target!r} is not built (built: {list(TARGETS)})")


def outlier_loss(outputs, targets, *, target="nls", score_norm="tanh", func="squared_hinge", inlier_upper_threshold=-1.0,
                 outlier_lower_threshold=-0.1, score=None):
    """``SetCriterion.outlier_loss`` (criterion.py:435-553; the matcher's ``indices`` and ``num_masks`` are unused there and absent here).
    outputs["pred_logits"] [B,Q,K+1], outputs["pred_masks"] [B,Q,h,w]; targets[i]["outlier_masks"] [H,W] with 1 = outlier, 0 = inlier,
    anything else ignored -> {"outlier_loss": scalar}.  Kept from the reference: without an outlier pixel the inlier term is not halved
    (:483-487), and an empty inlier set gives NaN (the mean of nothing).  Not built (ValueError): target "softmax_entropy" / "sum_entropy",
    score_norm "sigmoid", func "kl".  ``score`` [B,h,w]: the K1 score of this (target, score_norm), computed by the caller (``k1_score``) and shared
    with other losses; None = computed here."""
    mode = _score_mode(target, score_norm)
    if func not in FUNCS:
        raise ValueError(f"outlier_loss: func {func!r} is not built (built: {list(FUNCS)})")
    labels = torch.stack([t["outlier_masks"] for t in targets])                      # [B,H,W]
    if labels.dtype not in (torch.int64, torch.uint8):
        labels = torch.where(labels == 0, 0, torch.where(labels == 1, 1, 255)).to(torch.uint8)      # on the device, nothing read back
    if score is None:
        cls_prob = F.softmax(outputs["pred_logits"], dim=-1)[..., :-1]
        score = RbaScoreFunction.apply(outputs["pred_masks"], cls_prob, mode)        # [B,h,w]
    return {"outlier_loss": OutlierTailFunction.apply(score, labels, func, inlier_upper_threshold, outlier_lower_threshold)}


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


# ---------------------------------------------------------------------------------------------------------------- the DenseHybrid loss (K10)
class SemSegFunction(Function):
    """``SemSegFunction.apply(mask_pred [B,Q,h,w], cls_prob [B,Q,K]) -> [B,K,h,w]``: the class map of ``ops.rba_reduce(..., want_sem_seg=True)``
    image by image (the very bits of a direct call), differentiable once with respect to both tensors through ``ops.sem_seg_backward``.  Only
    the two inputs are saved; a gradient nobody asks for is not computed."""

    @staticmethod
    def forward(ctx, mask_pred, cls_prob):
        if mask_pred.dim() != 4 or cls_prob.dim() != 3 or cls_prob.shape[:2] != mask_pred.shape[:2]:
            raise ops.RbaHipError(f"SemSegFunction: mask_pred [B,Q,h,w] and cls_prob [B,Q,K], got {tuple(mask_pred.shape)} and {tuple(cls_prob.shape)}")
        mask_pred, cls_prob = mask_pred.contiguous(), cls_prob.contiguous()
        ctx.save_for_backward(mask_pred, cls_prob)
        return torch.stack([ops.rba_reduce(m, p, want_sem_seg=True)[1] for m, p in zip(mask_pred, cls_prob)])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_sem):
        mask_pred, cls_prob = ctx.saved_tensors
        need_mask, need_prob = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_mask or need_prob):
            return None, None
        grad_sem = grad_sem.contiguous()
        grads = [ops.sem_seg_backward(m, p, g, need_mask=need_mask, need_prob=need_prob) for m, p, g in zip(mask_pred, cls_prob, grad_sem)]
        return (torch.stack([gm for gm, _ in grads]) if need_mask else None,
                torch.stack([gp for _, gp in grads]) if need_prob else None)


class DenseHybridLossFunction(Function):
    """``DenseHybridLossFunction.apply(sem [B,K,h,w], ood [B,2,h,w], labels [B,H,W] int64 | uint8, beta) -> loss`` (a scalar):
    ``ops.dense_hybrid_loss`` (losses[0], the very bits of a direct call), differentiable once with respect to ``sem`` and ``ood`` through
    ``ops.dense_hybrid_loss_backward``.  Saved: the three inputs, the sums and the [B,H,W] logsumexp map.  No host synchronisation in either
    direction."""

    @staticmethod
    def forward(ctx, sem, ood, labels, beta):
        sem, ood, labels = sem.contiguous(), ood.contiguous(), labels.contiguous()
        losses, stats, lse = ops.dense_hybrid_loss(sem, ood, labels, beta)
        ctx.beta = beta
        ctx.save_for_backward(sem, ood, labels, stats, lse)
        return losses[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        need_sem, need_ood = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_sem or need_ood):
            return None, None, None, None
        sem, ood, labels, stats, lse = ctx.saved_tensors
        grad_sem, grad_ood = ops.dense_hybrid_loss_backward(sem, ood, labels, stats, lse, grad_loss.contiguous(), ctx.beta)
        return grad_sem if need_sem else None, grad_ood if need_ood else None, None, None


def densehybrid_loss(outputs, targets, *, num_classes, beta=0.03):
    """``SetCriterion.densehybrid_loss`` (criterion.py:390-433; the matcher's ``indices`` and ``num_masks`` are unused there and absent here).
    outputs["pred_logits"] [B,Q,K+1], outputs["pred_masks"] [B,Q,h,w], outputs["ood_pred"] [B,2,h,w]; targets[i]["sem_seg"] [H,W] with a value
    < K = that class, 254 = outlier, anything else void (the reference takes 255 only and relabels its targets in place; here they are not
    written) -> {"densehybrid_loss": scalar}.  ``num_classes`` = K is checked against ``pred_logits``.  Kept from the reference: without a class
    pixel or without an outlier pixel the loss is NaN (the mean of nothing)."""
    K = outputs["pred_logits"].shape[-1] - 1
    if K != num_classes:
        raise ValueError(f"densehybrid_loss: pred_logits has {K} classes (and no-object), num_classes is {num_classes}")
    labels = torch.stack([t["sem_seg"] for t in targets])                            # [B,H,W]
    if labels.dtype not in (torch.int64, torch.uint8):
        keep = ((labels >= 0) & (labels < K)) | (labels == 254)
        labels = torch.where(keep, labels, 255).to(torch.uint8)                      # on the device, nothing read back
    cls_prob = F.softmax(outputs["pred_logits"], dim=-1)[..., :-1]
    sem = SemSegFunction.apply(outputs["pred_masks"], cls_prob)                      # [B,K,h,w]
    return {"densehybrid_loss": DenseHybridLossFunction.apply(sem, outputs["ood_pred"], labels, float(beta))}


def densehybrid_loss_from_cfg(cfg):
    """The loss the DenseHybrid recipe's config selects: reads MODEL.MASK_FORMER.DENSE_HYBRID_BETA (absent: 0.03, mask2former/config.py) and
    MODEL.SEM_SEG_HEAD.NUM_CLASSES of ``rba_amd.config.load_cfg``'s result and returns ``loss(outputs, targets)``, a closure over
    ``densehybrid_loss``; its ``.keywords`` holds the two settings."""
    import functools
    model = cfg.get("MODEL", {})
    return functools.partial(densehybrid_loss, num_classes=int(model.get("SEM_SEG_HEAD", {}).get("NUM_CLASSES", 19)),
                             beta=float(model.get("MASK_FORMER", {}).get("DENSE_HYBRID_BETA", 0.03)))


# ---------------------------------------------------------------------------------------------------------------- the PEBAL fine-tune losses (K11)
class GamblerLossFunction(Function):
    """``GamblerLossFunction.apply(sem [B,K+1,h,w], labels [B,H,W] int64 | uint8, ood_reg) -> loss`` (a scalar): ``ops.gambler_loss``
    (losses[0], the very bits of a direct call), differentiable once with respect to ``sem`` through ``ops.gambler_loss_backward``.  Saved: the two
    inputs, the sums and the [B,H,W] blurred reward.  No host synchronisation in either direction."""

    @staticmethod
    def forward(ctx, sem, labels, ood_reg):
        sem, labels = sem.contiguous(), labels.contiguous()
        losses, stats, R = ops.gambler_loss(sem, labels, ood_reg)
        ctx.ood_reg = ood_reg
        ctx.save_for_backward(sem, labels, stats, R)
        return losses[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        sem, labels, stats, R = ctx.saved_tensors
        return ops.gambler_loss_backward(sem, labels, stats, R, grad_loss.contiguous(), ctx.ood_reg), None, None


class ScoreRegFunction(Function):
    """``ScoreRegFunction.apply(score [B,h,w], labels [B,H,W] int64 | uint8 | None) -> (smoothness, sparsity)`` (two scalars): ``ops.score_reg``
    (the very bits of a direct call), differentiable once with respect to ``score`` through ``ops.score_reg_backward``; the two upstream gradients
    reach the kernel as two device scalars.  Saved: score, labels and the two sums.  No host synchronisation in either direction."""

    @staticmethod
    def forward(ctx, score, labels):
        score = score.contiguous()
        labels = None if labels is None else labels.contiguous()
        losses, stats = ops.score_reg(score, labels)
        ctx.has_labels = labels is not None
        ctx.save_for_backward(*((score, stats, labels) if ctx.has_labels else (score, stats)))
        return losses[0], losses[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_smoothness, grad_sparsity):
        if not ctx.needs_input_grad[0]:
            return None, None
        score, stats = ctx.saved_tensors[:2]
        labels = ctx.saved_tensors[2] if ctx.has_labels else None
        return ops.score_reg_backward(score, labels, stats, grad_smoothness.contiguous(), grad_sparsity.contiguous()), None


# SMOOTHNESS_SCORE -> K1 score mode (criterion.py:260-268; the third branch there tests another attribute and is not built)
_SMOOTHNESS_SCORES = {"nls": "neg_logit_sum", "energy": "energy"}


def k1_score(outputs, mode):
    """The K1 score [B,h,w] of an outputs entry at the mask resolution (criterion.py:254-263, 449-465): ``mode`` is one of ``ops.SCORE_MODES``."""
    return RbaScoreFunction.apply(outputs["pred_masks"], F.softmax(outputs["pred_logits"], dim=-1)[..., :-1], mode)


def _smoothness_score(outputs, score, who):
    if isinstance(score, torch.Tensor):
        return score
    if score not in _SMOOTHNESS_SCORES:
        raise ValueError(f"{who}: score {score!r} is not built (built: {sorted(_SMOOTHNESS_SCORES)})")
    return k1_score(outputs, _SMOOTHNESS_SCORES[score])


def _outlier_plane(targets):
    """targets[i]["outlier_masks"] stacked to [B,H,W] int64 | uint8 (another dtype: reduced on the device to 1 / 255), or None without that key"""
    if "outlier_masks" not in targets[0]:
        return None
    labels = torch.stack([t["outlier_masks"] for t in targets])
    if labels.dtype not in (torch.int64, torch.uint8):
        labels = torch.where(labels == 1, 1, 255).to(torch.uint8)
    return labels


def smoothness_loss(outputs, targets, *, score="energy"):
    """``SetCriterion.smoothness_loss`` (criterion.py:245-281; ``indices`` and ``num_masks`` are unused there and absent here; so are the targets).
    ``score``: SMOOTHNESS_SCORE "energy" | "nls" (K1 at the mask resolution), or that score map [B,h,w] computed by the caller
    -> {"smoothness_loss": half the sum of the squared forward differences along both axes}."""
    s = _smoothness_score(outputs, score, "smoothness_loss")
    return {"smoothness_loss": ScoreRegFunction.apply(s, None)[0]}


def sparsity_loss(outputs, targets, *, score="energy"):
    """``SetCriterion.sparsity_loss`` (criterion.py:283-321).  ``score`` as in ``smoothness_loss``; targets[i]["outlier_masks"] [H,W] with 1 =
    outlier -> {"sparsity_loss": the 2-norm of the ``align_corners=True`` upsampled score over the outlier pixels}; 0 (with a zero gradient)
    without an outlier pixel or without that key."""
    s = _smoothness_score(outputs, score, "sparsity_loss")
    return {"sparsity_loss": ScoreRegFunction.apply(s, _outlier_plane(targets))[1]}


def gambler_loss(outputs, targets, *, num_classes, ood_reg=0.1):
    """``SetCriterion.gambler_loss`` (criterion.py:323-388; ``indices`` and ``num_masks`` are unused there and absent here).
    outputs["pred_logits"] [B,Q,K+1], outputs["pred_masks"] [B,Q,h,w]; targets[i]["outlier_masks"] [H,W] (1 = outlier, 255 = void, anything else
    inlier) and targets[i]["sem_seg"] [H,W] (the inlier pixels' classes) -> {"gambler_loss": scalar}.  The one label plane is built on the
    device -- outlier 1 -> 254, 255 -> 255, otherwise the ``sem_seg`` value if < K, else 255 -- and neither target is written (the reference
    relabels both in place).  One departure: an inlier pixel whose label is not a class is an index error in the reference and void here, as in
    ``densehybrid_loss``.  Kept from the reference: without an inlier pixel the loss is NaN.  ``self.pebal_reward`` there is dead code (the
    reward map always has elements) and is not built."""
    K = outputs["pred_logits"].shape[-1] - 1
    if K != num_classes:
        raise ValueError(f"gambler_loss: pred_logits has {K} classes (and no-object), num_classes is {num_classes}")
    om = torch.stack([t["outlier_masks"] for t in targets])                          # [B,H,W]
    ss = torch.stack([t["sem_seg"] for t in targets])
    labels = torch.where(om == 1, 254, torch.where((om != 255) & (ss >= 0) & (ss < K), ss, 255)).to(torch.uint8)      # nothing read back
    sem = SemSegFunction.apply(outputs["pred_masks"], F.softmax(outputs["pred_logits"], dim=-1))      # [B,K+1,h,w]: the no-object column stays (:327)
    return {"gambler_loss": GamblerLossFunction.apply(sem, labels, float(ood_reg))}


class PebalCriterion(torch.nn.Module):
    """The criterion of the PEBAL fine-tune recipe: the loss list maskformer_model.py:164-175 produces with GAMBLER_LOSS -- "gambler", then
    "smoothness", "sparsity" and "outlier" as configured -- over the final outputs and every ``aux_outputs`` entry i (key suffix ``_{i}``), as
    ``SetCriterion.forward`` does.  No matcher is called: these four losses ignore its indices.  The K1 score of an entry is computed once and
    shared by the losses that select the same K1 mode (the recipe: energy for all three).  ``outlier`` = the keyword settings of
    ``outlier_loss``."""

    def __init__(self, num_classes, weight_dict, losses, ood_reg=0.1, smoothness_score="energy", **outlier):
        super().__init__()
        for name in losses:
            if name not in ("gambler", "smoothness", "sparsity", "outlier"):
                raise ValueError(f"PebalCriterion: loss {name!r} is not one of gambler, smoothness, sparsity, outlier")
        if smoothness_score not in _SMOOTHNESS_SCORES:
            raise ValueError(f"PebalCriterion: smoothness score {smoothness_score!r} is not built (built: {sorted(_SMOOTHNESS_SCORES)})")
        unknown = set(outlier) - {"target", "score_norm", "func", "inlier_upper_threshold", "outlier_lower_threshold"}
        if unknown:
            raise TypeError(f"PebalCriterion: unknown outlier settings {sorted(unknown)}")
        self.num_classes, self.weight_dict, self.losses, self.ood_reg = num_classes, dict(weight_dict), list(losses), float(ood_reg)
        self.smoothness_score, self.outlier = smoothness_score, dict(outlier)

    def _entry(self, outputs, targets):
        scores = {}                                          # K1 mode -> score map of this entry

        def score(mode):
            if mode not in scores:
                scores[mode] = k1_score(outputs, mode)
            return scores[mode]

        losses = {}
        reg = [name for name in self.losses if name in ("smoothness", "sparsity")]
        if reg:                                              # one K11b call serves both regularisers
            labels = _outlier_plane(targets) if "sparsity" in reg else None
            smooth, sparse = ScoreRegFunction.apply(score(_SMOOTHNESS_SCORES[self.smoothness_score]), labels)
        for name in self.losses:
            if name == "gambler":
                losses.update(gambler_loss(outputs, targets, num_classes=self.num_classes, ood_reg=self.ood_reg))
            elif name == "smoothness":
                losses["smoothness_loss"] = smooth
            elif name == "sparsity":
                losses["sparsity_loss"] = sparse
            else:
                mode = _score_mode(self.outlier.get("target", "nls"), self.outlier.get("score_norm", "tanh"))
                losses.update(outlier_loss(outputs, targets, score=score(mode), **self.outlier))
        return losses

    def forward(self, outputs, targets):
        final = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        losses = self._entry(final, targets)
        for i, aux in enumerate(outputs.get("aux_outputs", ())):
            losses.update({f"{k}_{i}": v for k, v in self._entry(aux, targets).items()})
        return losses

    def weighted(self, losses):
        """maskformer_model.py:283-288: every loss times its weight; a loss without a weight is dropped"""
        return {k: v * self.weight_dict[k] for k, v in losses.items() if k in self.weight_dict}


def pebal_criterion_from_cfg(cfg):
    """The criterion the PEBAL recipe's config selects (maskformer_model.py:112-195 with GAMBLER_LOSS): ``PebalCriterion`` with the loss list,
    weight_dict (with the ``_{i}`` copies of DEEP_SUPERVISION), PEBAL_OOD_REG, SMOOTHNESS_SCORE and, with OUTLIER_SUPERVISION,
    ``outlier_loss_from_cfg``'s settings.  GAMBLER_LOSS unset, DENSE_HYBRID_LOSS beside it (the reference then drops the gambler loss), or a
    score that is not built raises ValueError here."""
    model = cfg.get("MODEL", {})
    mf = model.get("MASK_FORMER", {})
    v = {k: mf.get(k, d) for k, d in _CRITERION_DEFAULTS.items()}
    if not v["GAMBLER_LOSS"]:
        raise ValueError("pebal_criterion_from_cfg: GAMBLER_LOSS is not set; criterion_from_cfg builds the other recipes")
    if v["DENSE_HYBRID_LOSS"]:
        raise ValueError("pebal_criterion_from_cfg: DENSE_HYBRID_LOSS beside GAMBLER_LOSS selects the densehybrid recipe (densehybrid_loss_from_cfg)")
    weight_dict = {"loss_ce": v["CLASS_WEIGHT"], "loss_mask": v["MASK_WEIGHT"], "loss_dice": v["DICE_WEIGHT"], "smoothness_loss": v["SMOOTHNESS_WEIGHT"],
                   "sparsity_loss": v["SPARSITY_WEIGHT"], "outlier_loss": v["OUTLIER_WEIGHT"], "gambler_loss": v["GAMBLER_WEIGHT"],
                   "densehybrid_loss": v["DENSE_HYBRID_WEIGHT"]}
    if v["DEEP_SUPERVISION"]:
        weight_dict.update({f"{k}_{i}": w for i in range(int(v["DEC_LAYERS"]) - 1) for k, w in list(weight_dict.items())})
    losses = ["gambler"]
    if v["SMOOTHNESS_LOSS"]:
        losses.append("smoothness")
    if v["SPARSITY_LOSS"]:
        losses.append("sparsity")
    outlier = {}
    if v["OUTLIER_SUPERVISION"]:
        losses.append("outlier")
        outlier = outlier_loss_from_cfg(cfg).keywords
    return PebalCriterion(int(model.get("SEM_SEG_HEAD", {}).get("NUM_CLASSES", 19)), weight_dict, losses, float(mf.get("PEBAL_OOD_REG", 0.1)),
                          str(mf.get("SMOOTHNESS_SCORE", "energy")), **outlier)


# ---------------------------------------------------------------------------------------------------------------- the point-sampled mask losses (K8)
class MaskPointLossFunction(Function):
    """``MaskPointLossFunction.apply(pred_masks [B,Q,h,w], plane_index [N], point_coords [N,P,2], point_labels [N,P], num_masks) ->
    (loss_mask, loss_dice)``: ``ops.mask_point_loss`` (the very bits of a direct call), differentiable once with respect to ``pred_masks`` only
    through ``ops.mask_point_loss_backward``.  Mask n is plane ``plane_index[n]`` of ``pred_masks.view(B * Q, h, w)``.  Saved: the inputs and
    the per-mask sums [N,4].  N = 0: both losses are 0, the gradient is zeros, and no kernel is launched."""

    @staticmethod
    def forward(ctx, pred_masks, plane_index, point_coords, point_labels, num_masks):
        if pred_masks.dim() != 4:
            raise ops.RbaHipError(f"MaskPointLossFunction: pred_masks [B,Q,h,w], got {tuple(pred_masks.shape)}")
        ctx.num_masks, ctx.empty = float(num_masks), plane_index.numel() == 0
        if ctx.empty:
            ctx.like = (pred_masks.shape, pred_masks.device)
            zero = torch.zeros((), dtype=torch.float32, device=pred_masks.device)
            return zero, zero.clone()
        pred_masks, point_coords, point_labels = pred_masks.contiguous(), point_coords.contiguous(), point_labels.contiguous()
        losses, sums = ops.mask_point_loss(pred_masks, plane_index, point_coords, point_labels, ctx.num_masks)
        ctx.save_for_backward(pred_masks, plane_index, point_coords, point_labels, sums)
        return losses[0], losses[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_mask, grad_dice):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if ctx.empty:
            return torch.zeros(ctx.like[0], dtype=torch.float32, device=ctx.like[1]), None, None, None, None
        pred_masks, plane_index, point_coords, point_labels, sums = ctx.saved_tensors
        grad = ops.mask_point_loss_backward(pred_masks, plane_index, point_coords, point_labels, sums, ctx.num_masks,
                                            grad_mask.contiguous(), grad_dice.contiguous())
        return grad, None, None, None, None


def select_uncertain_points(pred_masks, plane_index, candidates, num_uncertain):
    """The selection of detectron2's ``get_uncertain_point_coords_with_randomness`` with the reference's uncertainty -|x| (criterion.py:76-90):
    mask n = plane ``plane_index[n]`` of pred_masks [B,Q,h,w] is sampled at candidates[n] [N,R,2] (``ops.point_sample``) and the
    ``num_uncertain`` candidates of smallest |logit| are returned, most uncertain first -> [N, num_uncertain, 2]."""
    with torch.no_grad():
        logits = ops.point_sample(pred_masks.detach().contiguous(), candidates.contiguous(), plane_index)
        idx = torch.topk(-logits.abs(), k=num_uncertain, dim=1)[1]
        return torch.gather(candidates, 1, idx[:, :, None].expand(-1, -1, 2))


def draw_point_candidates(N, num_points, oversample_ratio, importance_sample_ratio, device, generator=None):
    """The random numbers of ``uncertain_point_coords``, drawn before anything is selected -> (candidates [N, int(num_points * oversample_ratio), 2],
    random points [N, num_points - int(importance_sample_ratio * num_points), 2]), uniform in [0, 1)."""
    num_uncertain = int(importance_sample_ratio * num_points)
    candidates = torch.rand(N, int(num_points * oversample_ratio), 2, device=device, generator=generator)
    return candidates, torch.rand(N, num_points - num_uncertain, 2, device=device, generator=generator)


def uncertain_point_coords(pred_masks, plane_index, num_points, oversample_ratio, importance_sample_ratio, generator=None):
    """detectron2's ``get_uncertain_point_coords_with_randomness`` (point_rend/point_features.py) for the matched masks: of
    ``int(num_points * oversample_ratio)`` uniform candidates per mask the ``int(importance_sample_ratio * num_points)`` most uncertain, followed by
    uniform points up to ``num_points`` -> [N, num_points, 2] in [0, 1)."""
    if oversample_ratio < 1 or not 0 <= importance_sample_ratio <= 1:
        raise ValueError("uncertain_point_coords: oversample_ratio >= 1 and 0 <= importance_sample_ratio <= 1")
    candidates, rest = draw_point_candidates(plane_index.numel(), num_points, oversample_ratio, importance_sample_ratio, pred_masks.device, generator)
    chosen = select_uncertain_points(pred_masks, plane_index, candidates, int(importance_sample_ratio * num_points))
    return torch.cat([chosen, rest], dim=1)


def _flat_rows(per_image, sizes, device):
    """one int64 index vector per image into that image's `sizes[b]` rows -> their rows in the images' concatenation"""
    offs = [0]
    for n in sizes:
        offs.append(offs[-1] + int(n))
    return torch.cat([i.to(torch.int64) + o for i, o in zip(per_image, offs)]).to(device)


def _padded_masks(masks, dtype, device):
    """nested_tensor_from_tensor_list (utils/misc.py) on the images' [T_i,H_i,W_i] masks: one [sum T_i, max H, max W] tensor, zero-padded bottom / right"""
    H, W = max(m.shape[-2] for m in masks), max(m.shape[-1] for m in masks)
    out = torch.zeros((sum(m.shape[0] for m in masks), H, W), dtype=dtype, device=device)
    o = 0
    for m in masks:
        out[o:o + m.shape[0], :m.shape[-2], :m.shape[-1]] = m.to(device=device, dtype=dtype)
        o += m.shape[0]
    return out


def loss_masks(outputs, targets, indices, num_masks, *, num_points, oversample_ratio, importance_sample_ratio, point_coords=None, generator=None):
    """``SetCriterion.loss_masks`` (criterion.py:194-243).  outputs["pred_masks"] [B,Q,h,w]; targets[i]["masks"] [T_i,H_i,W_i] (zero-padded to the
    batch's largest H x W); indices = the matcher's [(idx_i, idx_j)]; ``point_coords`` [N,P,2] replaces the random oversampling (tests)
    -> {"loss_mask", "loss_dice"}.  No matched mask in the batch: both are 0 with a zero gradient and no kernel is launched."""
    pred = outputs["pred_masks"]
    B, Q = pred.shape[:2]
    dev = pred.device
    plane_index = _flat_rows([i for i, _ in indices], [Q] * B, dev)
    if plane_index.numel() == 0:
        lm, ld = MaskPointLossFunction.apply(pred, plane_index, None, None, num_masks)
        return {"loss_mask": lm, "loss_dice": ld}
    with torch.no_grad():
        tgt_index = _flat_rows([j for _, j in indices], [t["masks"].shape[0] for t in targets], dev)
        tgt = _padded_masks([t["masks"] for t in targets], pred.dtype, dev)
        if point_coords is None:
            point_coords = uncertain_point_coords(pred, plane_index, num_points, oversample_ratio, importance_sample_ratio, generator)
        point_coords = point_coords.contiguous()
        point_labels = ops.point_sample(tgt, point_coords, tgt_index)
    lm, ld = MaskPointLossFunction.apply(pred, plane_index, point_coords, point_labels, num_masks)
    return {"loss_mask": lm, "loss_dice": ld}


def loss_labels(outputs, targets, indices, *, num_classes, eos_coef):
    """``SetCriterion.loss_labels`` (criterion.py:174-192), plain torch: cross entropy over all B Q queries against the matched targets' labels
    (unmatched: the no-object class ``num_classes``, weighted ``eos_coef``) -> {"loss_ce"}."""
    logits = outputs["pred_logits"].float()
    dev = logits.device
    classes = torch.full(logits.shape[:2], num_classes, dtype=torch.int64, device=dev)
    for b, (t, (i, j)) in enumerate(zip(targets, indices)):
        classes[b, i.to(dev)] = t["labels"].to(dev)[j.to(dev)]
    weight = torch.ones(num_classes + 1, dtype=logits.dtype, device=dev)
    weight[-1] = eos_coef
    return {"loss_ce": F.cross_entropy(logits.transpose(1, 2), classes, weight)}


BUILT_LOSSES = ("labels", "masks", "outlier")
REFERENCE_LOSSES = BUILT_LOSSES + ("smoothness", "sparsity", "gambler", "densehybrid")


class SetCriterion(torch.nn.Module):
    """The reference's ``SetCriterion`` (criterion.py:99-172, 569-624) over the losses built here: "labels", "masks" and "outlier"; "smoothness",
    "sparsity", "gambler" and "densehybrid" raise ValueError.  ``outlier`` = the keyword settings of ``outlier_loss``.  ``forward(outputs,
    targets)`` matches the final outputs, computes num_masks (all-reduced over the process group when one is initialised, clamped to 1), runs
    every loss, then the same per ``aux_outputs`` entry i with the key suffix ``_{i}``."""

    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses, num_points, oversample_ratio, importance_sample_ratio, **outlier):
        super().__init__()
        for name in losses:
            if name not in BUILT_LOSSES:
                raise ValueError(f"SetCriterion: loss {name!r} is " + ("not built" if name in REFERENCE_LOSSES else "unknown") + f" (built: {list(BUILT_LOSSES)})")
        unknown = set(outlier) - {"target", "score_norm", "func", "inlier_upper_threshold", "outlier_lower_threshold"}
        if unknown:
            raise TypeError(f"SetCriterion: unknown outlier settings {sorted(unknown)}")
        self.num_classes, self.matcher, self.weight_dict, self.eos_coef, self.losses = num_classes, matcher, dict(weight_dict), eos_coef, list(losses)
        self.num_points, self.oversample_ratio, self.importance_sample_ratio = num_points, oversample_ratio, importance_sample_ratio
        self.outlier = dict(outlier)

    def get_loss(self, loss, outputs, targets, indices, num_masks, point_coords=None, generator=None):
        if loss == "labels":
            return loss_labels(outputs, targets, indices, num_classes=self.num_classes, eos_coef=self.eos_coef)
        if loss == "masks":
            if "pred_masks" not in outputs:
                raise ValueError("SetCriterion: an outputs entry without pred_masks")
            return loss_masks(outputs, targets, indices, num_masks, num_points=self.num_points, oversample_ratio=self.oversample_ratio,
                              importance_sample_ratio=self.importance_sample_ratio, point_coords=point_coords, generator=generator)
        return outlier_loss(outputs, targets, **self.outlier)

    def forward(self, outputs, targets, matcher_point_coords=None, loss_point_coords=None, generator=None):
        """``matcher_point_coords`` [P,2] and ``loss_point_coords`` [N,P,2] replace the random points of the matcher and of loss_masks (tests)."""
        final = {k: v for k, v in outputs.items() if k != "aux_outputs"}
        if "pred_masks" not in final:
            raise ValueError("SetCriterion: outputs without pred_masks")
        for i, aux in enumerate(outputs.get("aux_outputs", ())):
            if "pred_masks" not in aux:
                raise ValueError(f"SetCriterion: aux_outputs[{i}] has no pred_masks")
        match = lambda out: self.matcher(out, targets, point_coords=matcher_point_coords, generator=generator)
        indices = match(final)
        dev = final["pred_masks"].device
        num_masks = torch.as_tensor([sum(len(t["labels"]) for t in targets)], dtype=torch.float, device=dev)
        world = 1
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            torch.distributed.all_reduce(num_masks)
            world = torch.distributed.get_world_size()
        num_masks = torch.clamp(num_masks / world, min=1).item()
        losses = {}
        for loss in self.losses:
            losses.update(self.get_loss(loss, final, targets, indices, num_masks, loss_point_coords, generator))
        for i, aux in enumerate(outputs.get("aux_outputs", ())):
            indices = match(aux)
            for loss in self.losses:
                losses.update({f"{k}_{i}": v for k, v in self.get_loss(loss, aux, targets, indices, num_masks, loss_point_coords, generator).items()})
        return losses

    def weighted(self, losses):
        """maskformer_model.py:283-288: every loss times its weight; a loss without a weight is dropped"""
        return {k: v * self.weight_dict[k] for k, v in losses.items() if k in self.weight_dict}


# mask2former/config.py (add_maskformer2_config), the values in force after the file's last assignment of each key
_CRITERION_DEFAULTS = {"DEEP_SUPERVISION": True, "NO_OBJECT_WEIGHT": 0.1, "CLASS_WEIGHT": 1.0, "DICE_WEIGHT": 1.0, "MASK_WEIGHT": 20.0, "DEC_LAYERS": 6,
                       "TRAIN_NUM_POINTS": 112 * 112, "OVERSAMPLE_RATIO": 3.0, "IMPORTANCE_SAMPLE_RATIO": 0.75, "OUTLIER_SUPERVISION": False,
                       "OUTLIER_WEIGHT": 1.0, "MATCHER": "HungarianMatcher", "SMOOTHNESS_LOSS": False, "SMOOTHNESS_WEIGHT": 3e-6, "SPARSITY_LOSS": False,
                       "SPARSITY_WEIGHT": 5e-4, "GAMBLER_LOSS": False, "GAMBLER_WEIGHT": 1.0, "DENSE_HYBRID_LOSS": False, "DENSE_HYBRID_WEIGHT": 1.0,
                       "NUM_OBJECT_QUERIES": 100}


def criterion_from_cfg(cfg):
    """The criterion a config selects (maskformer_model.py:112-195): matcher, weight_dict (with the ``_{i}`` copies of DEEP_SUPERVISION), the list of
    losses, the point-sampling settings and, with OUTLIER_SUPERVISION, ``outlier_loss_from_cfg``'s settings.  A loss that is not built raises
    ValueError here."""
    from .matcher import FixedMatcher, HungarianMatcher
    model = cfg.get("MODEL", {})
    mf = model.get("MASK_FORMER", {})
    v = {k: mf.get(k, d) for k, d in _CRITERION_DEFAULTS.items()}
    num_classes = int(model.get("SEM_SEG_HEAD", {}).get("NUM_CLASSES", 19))
    if v["MATCHER"] == "HungarianMatcher":
        matcher = HungarianMatcher(cost_class=v["CLASS_WEIGHT"], cost_mask=v["MASK_WEIGHT"], cost_dice=v["DICE_WEIGHT"], num_points=int(v["TRAIN_NUM_POINTS"]))
    elif v["MATCHER"] == "FixedMatcher":
        if num_classes != int(v["NUM_OBJECT_QUERIES"]):
            raise ValueError("When using FixedMatcher, number of object queries must be equal to number of classes")
        matcher = FixedMatcher()
    else:
        raise ValueError(f"Given Matcher ({v['MATCHER']}) is not defined")
    weight_dict = {"loss_ce": v["CLASS_WEIGHT"], "loss_mask": v["MASK_WEIGHT"], "loss_dice": v["DICE_WEIGHT"], "smoothness_loss": v["SMOOTHNESS_WEIGHT"],
                   "sparsity_loss": v["SPARSITY_WEIGHT"], "outlier_loss": v["OUTLIER_WEIGHT"], "gambler_loss": v["GAMBLER_WEIGHT"],
                   "densehybrid_loss": v["DENSE_HYBRID_WEIGHT"]}
    if v["DEEP_SUPERVISION"]:
        weight_dict.update({f"{k}_{i}": w for i in range(int(v["DEC_LAYERS"]) - 1) for k, w in list(weight_dict.items())})
    losses = ["labels", "masks"]
    if v["GAMBLER_LOSS"]:
        losses = ["gambler"]
    if v["DENSE_HYBRID_LOSS"]:
        losses = ["densehybrid"]
    if v["SMOOTHNESS_LOSS"]:
        losses.append("smoothness")
    if v["SPARSITY_LOSS"]:
        losses.append("sparsity")
    outlier = {}
    if v["OUTLIER_SUPERVISION"]:
        losses.append("outlier")
        outlier = outlier_loss_from_cfg(cfg).keywords
    return SetCriterion(num_classes, matcher, weight_dict, float(v["NO_OBJECT_WEIGHT"]), losses, int(v["TRAIN_NUM_POINTS"]), float(v["OVERSAMPLE_RATIO"]),
                        float(v["IMPORTANCE_SAMPLE_RATIO"]), **outlier)
