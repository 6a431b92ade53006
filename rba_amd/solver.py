"""The optimizer and the schedule of the reference's fine-tune recipes: ``Trainer.build_optimizer`` / ``build_lr_scheduler`` (train_net.py:211-333)
restated for this library's model, with the step on K15 (docs/kernels/K15.md).

``build_optimizer(cfg, model)`` applies the ``MODEL.FREEZE_*`` flags, switches the predictor's differentiable paths on to match, builds one group per
trainable parameter by the reference's rules and returns a ``ClipAdamW``: full-model gradient clipping + AdamW over ONE flat gradient buffer -- two
launches and, across ranks, one ``all_reduce`` per step, nothing read back.  ``WarmupPolyLR(cfg)`` is Detectron2's DeepLab schedule in closed form.
Detectron2 is not installed where this was written: its scheduler and its SOLVER defaults are restated from its published source, parity unpinned.

By default this library trains the prediction heads (``class_embed``, ``mask_embed``, ``decoder_norm``) and the ``ood_pred`` head only; a cfg that leaves
anything else trainable is refused by name, as is every solver setting the step does not implement.  ``build_optimizer(..., differentiable_decoder=True)``
opts in to training the transformer decoder itself (the released PEBAL recipe); backbone and pixel decoder have no backward here and stay refused.  ``SOLVER.AMP`` is ignored (one logged line): the
fine-tune path is fp32 by design.
"""
import logging
import math

import torch
from torch import nn

from . import ops

logger = logging.getLogger(__name__)

# train_net.py:228-240
NORM_MODULE_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm, nn.GroupNorm, nn.InstanceNorm1d, nn.InstanceNorm2d,
                     nn.InstanceNorm3d, nn.LayerNorm, nn.LocalResponseNorm)
# what has a backward here: MultiScaleMaskedTransformerDecoder.differentiable_heads (+ deep_supervision), .differentiable_ood_head and, opt-in,
# .differentiable_decoder (every other predictor parameter)
HEAD_MODULES = ("class_embed", "mask_embed", "decoder_norm")
OOD_HEAD_MODULE = "ood_pred"
PREDICTOR = "sem_seg_head.predictor."


def apply_freeze_flags(cfg, model):
    """train_net.py:242-273: the flags only ever clear ``requires_grad``; of the four decoder flags the first one set wins (the reference's elif chain)."""
    m = cfg.MODEL
    if m.get("FREEZE_BACKBONE", False):
        for p in model.backbone.parameters():
            p.requires_grad = False
    if m.get("FREEZE_PIXEL_DECODER", False):
        for p in model.sem_seg_head.pixel_decoder.parameters():
            p.requires_grad = False
    keep = None
    if m.get("FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES", False):
        keep = ("query_embed", "query_feat")
    elif m.get("FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP_AND_OOD_PRED", False):
        keep = ("class_embed", "mask_embed", "ood_pred")
    elif m.get("FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP", False):
        keep = ("class_embed", "mask_embed")
    elif m.get("FREEZE_TRANSFORMER_DECODER", False):
        keep = ()
    if keep is not None:
        for name, p in model.sem_seg_head.predictor.named_parameters():
            if not any(k in name for k in keep):
                p.requires_grad = False


def _flag_that_would_freeze(name):
    if name.startswith("backbone."):
        return "MODEL.FREEZE_BACKBONE"
    if name.startswith("sem_seg_head.pixel_decoder."):
        return "MODEL.FREEZE_PIXEL_DECODER"
    if "query_embed" in name or "query_feat" in name:
        return "MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES"
    return "MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP"


def param_groups(cfg, model):
    """train_net.py:276-300: one group per trainable parameter, in ``named_modules`` order -> [(name, parameter, lr multiplier, weight decay)].
    The learning rate of a group is ``lr * multiplier``; the reference stores BASE_LR times it."""
    s = cfg.SOLVER
    groups, memo = [], set()
    for module_name, module in model.named_modules():
        for param_name, value in module.named_parameters(recurse=False):
            if not value.requires_grad or value in memo:
                continue
            memo.add(value)
            mult, wd = 1.0, float(s.WEIGHT_DECAY)
            if "backbone" in module_name:
                mult = float(s.BACKBONE_MULTIPLIER)
            if "relative_position_bias_table" in param_name or "absolute_pos_embed" in param_name:
                wd = 0.0
            if isinstance(module, NORM_MODULE_TYPES):
                wd = float(s.WEIGHT_DECAY_NORM)
            if isinstance(module, nn.Embedding):
                wd = float(s.WEIGHT_DECAY_EMBED)
            groups.append((f"{module_name}.{param_name}" if module_name else param_name, value, mult, wd))
    return groups


def check_solver_settings(cfg):
    """-> max_norm of the full-model clip (0.0: none).  Everything the step does not implement raises ValueError naming the value."""
    s = cfg.SOLVER
    if s.OPTIMIZER != "ADAMW":
        raise ValueError(f"SOLVER.OPTIMIZER {s.OPTIMIZER!r}: only 'ADAMW' is built (the three fine-tune recipes use it; SGD has no kernel here)")
    c = s.CLIP_GRADIENTS
    if not c.ENABLED:
        return 0.0
    if c.CLIP_TYPE != "full_model":
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.CLIP_TYPE {c.CLIP_TYPE!r}: only 'full_model' is built (per-parameter clipping is Detectron2's "
                         "maybe_add_gradient_clipping, which the recipes do not use)")
    if float(c.NORM_TYPE) != 2.0:
        raise ValueError(f"SOLVER.CLIP_GRADIENTS.NORM_TYPE {c.NORM_TYPE!r}: only the 2-norm is built")
    return max(float(c.CLIP_VALUE), 0.0)           # train_net.py:306-310: a value <= 0 disables the clip


def build_optimizer(cfg, model, differentiable_decoder=False):
    """``Trainer.build_optimizer`` (train_net.py:220-333) -> ClipAdamW.  Side effects, as in the reference: ``requires_grad`` of the frozen parameters is
    cleared; and, this library's own: the predictor's ``differentiable_heads`` / ``deep_supervision`` / ``differentiable_ood_head`` /
    ``differentiable_decoder`` are set to what the trainable set and ``MASK_FORMER.DEEP_SUPERVISION`` ask for.

    ``differentiable_decoder`` (opt-in; ``train_net --differentiable_decoder``): any trainable subset of ``sem_seg_head.predictor.*`` is accepted --
    the released PEBAL recipe (FREEZE_BACKBONE + FREEZE_PIXEL_DECODER: the whole transformer decoder) and
    FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES -- and the predictor's ``differentiable_decoder`` is set iff a trainable parameter lies outside
    the heads and ``ood_pred``.  A trainable backbone or pixel-decoder parameter is refused either way."""
    max_norm = check_solver_settings(cfg)
    if cfg.SOLVER.get("AMP", {}).get("ENABLED", False):
        logger.info("SOLVER.AMP.ENABLED is ignored: the fine-tune path of this library is fp32 by design")
    apply_freeze_flags(cfg, model)
    groups = param_groups(cfg, model)
    heads = ood = layers = False
    for name, _, _, _ in groups:
        part = name[len(PREDICTOR):].split(".")[0] if name.startswith(PREDICTOR) else None
        if part in HEAD_MODULES:
            heads = True
        elif part == OOD_HEAD_MODULE:
            ood = True
        elif part is not None and differentiable_decoder:
            layers = True
        else:
            raise ValueError(f"{name} would be trained, but this library has backward kernels for the prediction heads ({', '.join(HEAD_MODULES)}) and "
                             f"the {OOD_HEAD_MODULE} head only: set {_flag_that_would_freeze(name)}: True (the COCO-mix and DenseHybrid recipes set such flags)"
                             + ("" if part is None or differentiable_decoder else
                                "; or train the transformer decoder itself with build_optimizer(..., differentiable_decoder=True) / "
                                "train_net --differentiable_decoder"))
    if not groups:
        raise ValueError("the MODEL.FREEZE_* flags leave no trainable parameter")
    predictor = model.sem_seg_head.predictor
    predictor.differentiable_heads = True          # the ood head's graph hangs off the differentiable head call too
    predictor.deep_supervision = bool((heads or layers) and cfg.MODEL.MASK_FORMER.get("DEEP_SUPERVISION", True))
    predictor.differentiable_ood_head = ood
    predictor.differentiable_decoder = layers
    return ClipAdamW([(n, p) for n, p, _, _ in groups], [m for _, _, m, _ in groups], [w for _, _, _, w in groups], max_norm=max_norm)


class ClipAdamW:
    """clip_grad_norm_(all parameters, max_norm) + torch.optim.AdamW(amsgrad=False) over flat fp32 state.

    ``grad`` is one flat buffer and every parameter's ``.grad`` a view of its slice (autograd accumulates into an existing ``.grad`` in place, which
    keeps the view); ``exp_avg`` / ``exp_avg_sq`` have the same layout.  On HIP parameters ``step`` is K15's two launches and synchronises nothing; on
    CPU parameters the same class runs the same formulas in plain torch, so the host logic around it is testable without a device.  Departures from
    torch, both stated in docs/kernels/K15.md: the clipped gradient is not written back (``.grad`` keeps the unclipped, unscaled sum), and a parameter
    that received no gradient is stepped with a zero gradient, not skipped."""

    def __init__(self, named_params, lr_mults, weight_decays, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0, chunk=None):
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        if not self.params or len(set(self.names)) != len(self.names):
            raise ValueError("ClipAdamW needs at least one parameter and distinct names")
        self.lr_mults, self.weight_decays = [float(m) for m in lr_mults], [float(w) for w in weight_decays]
        self.betas, self.eps, self.max_norm = (float(betas[0]), float(betas[1])), float(eps), float(max_norm)
        self.step_count, self.grad_scale = 0, 1.0
        dev = self.params[0].device
        if any(p.device != dev or p.dtype != torch.float32 or not p.is_contiguous() for p in self.params):
            raise ValueError("ClipAdamW needs contiguous fp32 parameters on one device")
        self.on_device = dev.type == "cuda"
        if self.on_device:
            self.plan = ops.adamw_plan([p.detach() for p in self.params], self.lr_mults, self.weight_decays, chunk=chunk)
            self.offsets, total, self.stats = self.plan.offsets, self.plan.total, self.plan.stats
            self.grad, self.exp_avg, self.exp_avg_sq = (ops.adamw_flat(self.plan) for _ in range(3))
        else:
            self.offsets, total = [], 0
            for p in self.params:
                self.offsets.append(total)
                total += (p.numel() + 3) // 4 * 4
            self.grad, self.exp_avg, self.exp_avg_sq = (torch.zeros(total) for _ in range(3))
            self.stats = torch.zeros(1)
        for p, off in zip(self.params, self.offsets):
            p.grad = self.grad[off:off + p.numel()].view_as(p)

    # ---- the three calls of an iteration
    def zero_grad(self):
        """one memset: every ``.grad`` is a view of the flat buffer"""
        self.grad.zero_()

    def all_reduce_grads(self, group=None):
        """one all_reduce(SUM) of the flat buffer; the 1 / world factor goes into the step's grad_scale instead of a pass over the buffer"""
        import torch.distributed as dist
        world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if world > 1:
            dist.all_reduce(self.grad, op=dist.ReduceOp.SUM, group=group)
        self.grad_scale = 1.0 / world

    def _slices(self, flat):
        return [flat[off:off + p.numel()].view_as(p) for p, off in zip(self.params, self.offsets)]

    @torch.no_grad()
    def step(self, lr):
        """One step at learning rate ``lr`` for a group with multiplier 1 (WarmupPolyLR.lr(iteration)); a group's own is ``lr * multiplier``."""
        for p, off in zip(self.params, self.offsets):
            if p.grad is None or p.grad.data_ptr() != self.grad.data_ptr() + 4 * off:
                raise RuntimeError("ClipAdamW: a parameter's .grad no longer is its slice of the flat buffer (zero_grad(set_to_none=True) or an "
                                   "assignment replaced it); use this optimizer's zero_grad()")
        self.step_count += 1
        lr = float(lr)
        if self.on_device:
            ops.grad_sqnorm(self.plan, self.grad, self.grad_scale)
            ops.clip_adamw_step(self.plan, self.grad, self.exp_avg, self.exp_avg_sq, self.step_count, lr, betas=self.betas, eps=self.eps,
                                max_norm=self.max_norm, grad_scale=self.grad_scale)
            return
        beta1, beta2 = self.betas
        bc1, bc2_sqrt = 1.0 - beta1 ** self.step_count, (1.0 - beta2 ** self.step_count) ** 0.5
        g = self.grad * self.grad_scale
        total = torch.linalg.vector_norm(g)
        self.stats[0] = total
        if self.max_norm > 0.0:
            g = g * torch.clamp(self.max_norm / (total + 1e-6), max=1.0)          # clamp keeps NaN, as clip_grad_norm_'s does
        for p, gt, m, v, mult, wd in zip(self.params, self._slices(g), self._slices(self.exp_avg), self._slices(self.exp_avg_sq), self.lr_mults,
                                         self.weight_decays):
            lr_t = lr * mult
            p.mul_(1.0 - lr_t * wd)
            m.lerp_(gt, 1.0 - beta1)
            v.mul_(beta2).addcmul_(gt, gt, value=1.0 - beta2)
            p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(self.eps), value=-(lr_t / bc1))

    @property
    def grad_norm(self):
        """the last step's gradient norm (before clipping, after the 1 / world scale): a one-element tensor where the parameters live, not read back"""
        return self.stats

    # ---- checkpointing: tensors and numbers only
    def state_dict(self):
        return {"step": self.step_count,
                "exp_avg": {n: t.detach().clone().cpu() for n, t in zip(self.names, self._slices(self.exp_avg))},
                "exp_avg_sq": {n: t.detach().clone().cpu() for n, t in zip(self.names, self._slices(self.exp_avg_sq))}}

    @torch.no_grad()
    def load_state_dict(self, state):
        for key, flat in (("exp_avg", self.exp_avg), ("exp_avg_sq", self.exp_avg_sq)):
            have = state[key]
            if set(have) != set(self.names):
                raise ValueError(f"optimizer state '{key}' names {sorted(set(have) ^ set(self.names))[:4]} do not match the trainable parameters")
            for n, t in zip(self.names, self._slices(flat)):
                if tuple(have[n].shape) != tuple(t.shape):
                    raise ValueError(f"optimizer state '{key}' of {n}: shape {tuple(have[n].shape)} vs parameter {tuple(t.shape)}")
                t.copy_(have[n])
        self.step_count = int(state["step"])


class WarmupPolyLR:
    """Detectron2's ``WarmupPolyLR`` (projects/DeepLab/deeplab/lr_scheduler.py behind ``build_lr_scheduler``) in closed form:
    ``lr(it) = BASE_LR * warmup(it) * (1 - it / MAX_ITER) ** POLY_LR_POWER``, with ``warmup(it)`` = 1 from WARMUP_ITERS on, WARMUP_FACTOR
    ("constant") or ``WARMUP_FACTOR * (1 - it / WARMUP_ITERS) + it / WARMUP_ITERS`` ("linear") before; with POLY_LR_CONSTANT_ENDING > 0, past the
    warm-up, the rate stays at ``BASE_LR * POLY_LR_CONSTANT_ENDING`` once the polynomial falls below it.  ``it`` counts finished iterations: the
    first step runs at ``lr(0)``.  Restated from the published source, parity unpinned."""

    def __init__(self, cfg):
        s = cfg.SOLVER
        if s.LR_SCHEDULER_NAME != "WarmupPolyLR":
            raise ValueError(f"SOLVER.LR_SCHEDULER_NAME {s.LR_SCHEDULER_NAME!r}: only 'WarmupPolyLR' is built (the Cityscapes recipes use it)")
        if s.WARMUP_METHOD not in ("linear", "constant"):
            raise ValueError(f"SOLVER.WARMUP_METHOD {s.WARMUP_METHOD!r}: 'linear' or 'constant'")
        self.base_lr, self.max_iter = float(s.BASE_LR), int(s.MAX_ITER)
        self.warmup_factor, self.warmup_iters, self.warmup_method = float(s.WARMUP_FACTOR), int(s.WARMUP_ITERS), s.WARMUP_METHOD
        self.power, self.constant_ending = float(s.POLY_LR_POWER), float(s.POLY_LR_CONSTANT_ENDING)

    def lr(self, iteration, multiplier=1.0):
        """the learning rate of a group with ``multiplier`` (its base rate is BASE_LR * multiplier, train_net.py:289) at ``iteration``, the products in
        Detectron2's order; ``ClipAdamW.step`` takes the multiplier-1 value"""
        it, base = int(iteration), self.base_lr * multiplier
        if it >= self.warmup_iters:
            warmup = 1.0
        elif self.warmup_method == "constant":
            warmup = self.warmup_factor
        else:
            alpha = it / self.warmup_iters
            warmup = self.warmup_factor * (1 - alpha) + alpha
        poly = math.pow(1.0 - it / self.max_iter, self.power)
        if self.constant_ending > 0 and warmup == 1.0 and poly < self.constant_ending:
            return base * self.constant_ending
        return base * warmup * poly
