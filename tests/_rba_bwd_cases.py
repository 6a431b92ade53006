"""Shared by tests/test_rba_backward_cpu.py and tests/test_rba_backward_gpu.py: the torch restatement of the reference's outlier loss, the
case table of K1's backward, the error metric and its bar.

The restatement below (``ref_score``, ``ref_outlier_loss``) is written from mask2former/modeling/criterion.py:443-518 of the reference.  Its parity
is PINNED BY REFERENCE CODE: tests/golden/g9_criterion.npz holds what the reference's own ``SetCriterion.outlier_loss`` computes (loss and float64
gradients, three targets x four functions, with and without outlier pixels, at the "small" and "crop" shapes below), and
tests/test_criterion_reference_cpu.py holds this restatement to it at relative 1e-12 (2^-23 for ``binary_cross_entropy``, whose target the reference
casts to float32).  It is also checked against the mathematics (torch.autograd.gradcheck in double, test_rba_backward_cpu.py), and it is the truth
the GPU tests use.
"""
import functools

import torch
import torch.nn.functional as F

SCORES = ("rba", "energy", "neg_logit_sum")                      # ops.SCORE_MODES 0, 1, 2
COMBOS = (("nls", "tanh"), ("nls", "none"), ("energy", "none"))  # (target, score_norm) that are built
FUNCS = ("squared_hinge", "binary_cross_entropy", "mse", "l1")
SCORE_OF = {("nls", "tanh"): "rba", ("nls", "none"): "neg_logit_sum", ("energy", "none"): "energy"}
FLOOR = 2.0 ** -20


def ref_score(mask, prob, score):
    """criterion.py:452-465.  mask [B,Q,h,w] logits, prob [B,Q,K] -> [B,h,w]"""
    sem = torch.einsum("bqc,bqhw->bchw", prob, mask.sigmoid())   # :452, :454
    if score == "rba":
        return -sem.tanh().sum(dim=1)                            # :460, :463
    if score == "neg_logit_sum":
        return -sem.sum(dim=1)                                   # :462-463
    assert score == "energy"
    return -torch.logsumexp(sem, dim=1)                          # :465


def ref_outlier_loss(pred_logits, pred_masks, labels, target="nls", score_norm="tanh", func="squared_hinge", thr_in=-1.0, thr_out=-0.1):
    """criterion.py:443-503 (+ the l1 branch :506-518).  pred_logits [B,Q,K+1], pred_masks [B,Q,h,w], labels [B,H,W] -> scalar"""
    ood, ind = labels == 1, labels == 0                                                              # :446-447
    prob = F.softmax(pred_logits, dim=-1)[..., :-1]                                                  # :451
    score = ref_score(pred_masks, prob, SCORE_OF[(target, score_norm)])
    score = F.interpolate(score.unsqueeze(1), size=labels.shape[-2:], mode="bilinear", align_corners=True).squeeze(1)   # :474-475
    s_out, s_in = score[ood], score[ind]                                                             # :477-478
    if func == "binary_cross_entropy":
        return 0.5 * F.binary_cross_entropy_with_logits(score, ood.to(score.dtype))                  # :489
    if func == "squared_hinge":
        f_in, f_out = F.relu(s_in - thr_in).pow(2).mean(), F.relu(thr_out - s_out).pow(2).mean()     # :481-486
    elif func == "mse":
        f_in, f_out = F.mse_loss(s_in, torch.full_like(s_in, thr_in)), F.mse_loss(s_out, torch.full_like(s_out, thr_out))   # :492-502
    else:
        assert func == "l1"
        f_in, f_out = F.l1_loss(s_in, torch.full_like(s_in, thr_in)), F.l1_loss(s_out, torch.full_like(s_out, thr_out))     # :507-517
    if int(ood.sum()) > 0:                                                                           # :483 / :497 / :512
        return 0.5 * (f_in + f_out)
    return f_in                                                                                      # not halved


# ---- K1 backward: (name, Q, K, N, modes, logit scale, clip)
CASES = (
    ("base", 100, 19, 4096, SCORES, 6.0, None),
    ("odd", 7, 3, 130, SCORES, 6.0, None),
    ("one", 1, 1, 1, SCORES, 6.0, None),
    ("mapillary", 33, 65, 1000, SCORES, 6.0, None),
    ("kmax", 100, 160, 257, SCORES, 6.0, None),
    ("bigq", 250, 19, 515, SCORES, 6.0, None),
    ("quarter", 100, 19, 131072, ("rba",), 6.0, None),
    ("saturated", 100, 19, 4096, SCORES, 40.0, 120.0),
    ("k27", 100, 27, 515, SCORES, 6.0, None),                   # 20 < K <= 32: the launcher's third template instantiation, chunked (Q + K > 124)
)
CASE = {c[0]: c for c in CASES}
CASE_MODES = [(c[0], s) for c in CASES for s in c[4]]


def inputs_for(Q, K, N, scale, seed, clip=None):
    """(mask [Q,N], prob [Q,K], g [N]) fp32 on the CPU for any shape, seeded: the named cases and the random-shape sweep draw here"""
    gen = torch.Generator().manual_seed(seed)
    mask = scale * torch.randn(Q, N, generator=gen)
    if clip is not None:
        mask = mask.clamp(-clip, clip)
    prob = F.softmax(2.0 * torch.randn(Q, K + 1, generator=gen), dim=-1)[:, :-1].contiguous()
    g = torch.randn(N, generator=gen)
    return mask, prob, g


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(mask [Q,N], prob [Q,K], g [N]) fp32 on the CPU, seeded by the case"""
    _, Q, K, N, _, scale, clip = CASE[name]
    return inputs_for(Q, K, N, scale, 1000 + [c[0] for c in CASES].index(name), clip)


def _autograd(mask, prob, g, score):
    m, p = mask.detach().clone().requires_grad_(True), prob.detach().clone().requires_grad_(True)
    (ref_score(m[None, :, None, :], p[None], score)[0, 0] * g).sum().backward()
    return m.grad, p.grad


@functools.lru_cache(maxsize=None)
def case_truth(name, score):
    """fp64 CPU autograd on .double() of the very inputs, and b = the same metric for fp32 CPU autograd: (grad_mask64, grad_prob64, b_mask, b_prob)"""
    mask, prob, g = case_inputs(name)
    gm64, gp64 = _autograd(mask.double(), prob.double(), g.double(), score)
    gm32, gp32 = _autograd(mask, prob, g, score)
    return gm64, gp64, err(gm32, gm64), err(gp32, gp64)


def err(t, t64):
    """e(T) = max|T - T64| / max|T64|"""
    return float((t.detach().cpu().double() - t64).abs().max() / t64.abs().max())


def bar(b):
    return 4.0 * max(b, FLOOR)


def check(what, t, t64, b):
    e = err(t, t64)
    print(f"{what}: e = {e:.3e}  b = {b:.3e}  e/b = {e / max(b, 1e-300):.2f}  bar = {bar(b):.3e}")
    assert torch.isfinite(t).all(), f"{what}: not finite"
    assert e <= bar(b), f"{what}: e = {e:.3e} > 4 max(b, 2^-20) = {bar(b):.3e} (b = {b:.3e})"


# ---- the loss: (B, Q, K, h, w, H, W, mask-logit shift).  The shift puts the scores around the two thresholds so that both terms of every
# loss function are active (a 6 randn logit field of 100 queries sums to a score near -K, far below both)
LOSS_SHAPES = {"crop": (2, 100, 19, 32, 64, 128, 256, -7.1), "small": (1, 20, 5, 7, 9, 25, 33, -5.0)}
KINK = 1e-3


@functools.lru_cache(maxsize=None)
def loss_inputs(shape, combo, outliers=True):
    """(pred_logits, pred_masks, labels) on the CPU.  Labels: 0 / 1 / 255 at random (no 1 with outliers=False); a labelled pixel whose fp64 score lies
    within KINK of the threshold of its class is relabelled 255, so the kink of l1 (and the corner of the hinge) is never sampled -- asserted."""
    B, Q, K, h, w, H, W, shift = LOSS_SHAPES[shape]
    gen = torch.Generator().manual_seed(77 + 13 * sorted(LOSS_SHAPES).index(shape) + COMBOS.index(combo))
    logits = 2.0 * torch.randn(B, Q, K + 1, generator=gen)
    masks = 3.0 * torch.randn(B, Q, h, w, generator=gen) + shift
    r = torch.rand(B, H, W, generator=gen)
    labels = torch.full((B, H, W), 255, dtype=torch.int64)
    labels[r < 0.6] = 0
    if outliers:
        labels[r < 0.25] = 1
    prob = F.softmax(logits.double(), dim=-1)[..., :-1]
    s = F.interpolate(ref_score(masks.double(), prob, SCORE_OF[combo]).unsqueeze(1), size=(H, W), mode="bilinear", align_corners=True).squeeze(1)
    labels[(labels == 0) & ((s + 1.0).abs() < KINK)] = 255
    labels[(labels == 1) & ((s + 0.1).abs() < KINK)] = 255
    assert ((s[labels == 0] + 1.0).abs() >= KINK).all() and ((s[labels == 1] + 0.1).abs() >= KINK).all()
    assert (labels == 0).any() and (labels == 255).any() and bool((labels == 1).any()) == outliers
    return logits, masks, labels


def _loss_autograd(logits, masks, labels, combo, func):
    lg, mk = logits.detach().clone().requires_grad_(True), masks.detach().clone().requires_grad_(True)
    loss = ref_outlier_loss(lg, mk, labels, combo[0], combo[1], func)
    loss.backward()
    return loss.detach(), lg.grad, mk.grad


@functools.lru_cache(maxsize=None)
def loss_truth(shape, combo, func, outliers=True):
    """(loss64, grad_logits64, grad_masks64, b_logits, b_masks)"""
    logits, masks, labels = loss_inputs(shape, combo, outliers)
    l64, gl64, gm64 = _loss_autograd(logits.double(), masks.double(), labels, combo, func)
    _, gl32, gm32 = _loss_autograd(logits, masks, labels, combo, func)
    return l64, gl64, gm64, err(gl32, gl64), err(gm32, gm64)
