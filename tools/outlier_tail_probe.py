#!/usr/bin/env python3
"""Time K9 (csrc/outlier_tail.hip) at the fine-tune recipe's crop -- B = 2, score 128 x 256 -> labels 512 x 1024 (int64; 60 % inlier, 25 % outlier,
15 % ignored), squared_hinge -- forward + backward, beside the torch tail it replaced on the same GPU: F.interpolate(align_corners=True), the two
boolean-mask gathers (a nonzero with a read-back each), relu / pow / mean, the host-side `numel() > 0` decision, and autograd's backward of all
of it.  The torch side is kept here as it stood in criterion.outlier_loss; its read-backs sit inside its window.

Then one whole SetCriterion forward + backward (labels + masks + outlier behind the Hungarian matcher) on the Swin-B 1dl shapes -- B = 2, Q = 100,
masks 128 x 256, 19 targets per image, P = 12544 -- on the final outputs alone and with the recipe's one deep-supervision entry beside them
(a measurement, no bar).

HIP events around batches of 10 launches queued behind a long kernel; the median of 6 rounds after 2 warm-up rounds; the candidates alternate."""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops
from rba_amd.modeling.criterion import OutlierTailFunction, SetCriterion
from rba_amd.modeling.matcher import HungarianMatcher

BATCH, ROUNDS, WARM = 10, 6, 2
B, h, w, H, W = 2, 128, 256, 512, 1024
Q, K, T, P = 100, 19, 19, 12544
THR_IN, THR_OUT = -1.0, -0.1
busy = torch.randn(8192, 8192, device="cuda")


def timed(fns, batch=BATCH):
    """{name: median us per call}: the candidates alternate round by round, each round = `batch` calls bracketed by events behind a long kernel"""
    ts = {k: [] for k in fns}
    for i in range(WARM + ROUNDS):
        for k, fn in fns.items():
            busy @ busy
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= WARM:
                ts[k].append(e0.elapsed_time(e1) * 1e3 / batch)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def torch_tail(score, labels):
    """the tail of criterion.outlier_loss before K9 (squared_hinge)"""
    ood, ind = labels == 1, labels == 0
    s = F.interpolate(score[:, None], size=labels.shape[-2:], mode="bilinear", align_corners=True)[:, 0]
    d_in, d_out = s[ind] - THR_IN, THR_OUT - s[ood]
    term = lambda d: F.relu(d).pow(2).mean()
    loss = term(d_in)
    if d_out.numel() > 0:
        loss = 0.5 * (loss + term(d_out))
    return loss


g = torch.Generator(device="cuda").manual_seed(0)
coarse = torch.randn(B, 1, 17, 33, device="cuda", generator=g)
score0 = (-0.55 + 0.5 * F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)[:, 0]).contiguous()
r = torch.rand(B, H, W, device="cuda", generator=g)
labels = torch.full((B, H, W), 255, dtype=torch.int64, device="cuda")
labels[r < 0.85] = 0
labels[r < 0.25] = 1
labels8 = labels.to(torch.uint8)
score_t, score_h = score0.clone().requires_grad_(True), score0.clone().requires_grad_(True)
one = torch.ones((), device="cuda")
loss_h, stats = ops.outlier_tail(score0, labels, "squared_hinge", THR_IN, THR_OUT)


def hip_pair(lab=labels):
    return torch.autograd.grad(OutlierTailFunction.apply(score_h, lab, "squared_hinge", THR_IN, THR_OUT), score_h)[0]


t = timed({
    "hip fwd+bwd": hip_pair, "torch fwd+bwd": lambda: torch.autograd.grad(torch_tail(score_t, labels), score_t)[0],
    "hip fwd+bwd uint8": lambda: hip_pair(labels8),
    "hip fwd": lambda: ops.outlier_tail(score0, labels, "squared_hinge", THR_IN, THR_OUT),
    "hip bwd": lambda: ops.outlier_tail_backward(score0, labels, stats, one, "squared_hinge", THR_IN, THR_OUT),
    "torch fwd": lambda: torch_tail(score0, labels),
})
rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
frac = [float((labels == v).float().mean()) for v in (0, 1, 255)]
print(f"B={B} score {h}x{w} -> labels {H}x{W} int64 (inlier {frac[0]:.2f}, outlier {frac[1]:.2f}, ignored {frac[2]:.2f}) squared_hinge")
print(f"  tail fwd+bwd  : hip {t['hip fwd+bwd']:8.1f} us   torch {t['torch fwd+bwd']:8.1f} us   hip / torch = {t['hip fwd+bwd'] / t['torch fwd+bwd']:.3f}")
print(f"  hip fwd alone {t['hip fwd']:.1f} us, bwd alone {t['hip bwd']:.1f} us, fwd+bwd on uint8 labels {t['hip fwd+bwd uint8']:.1f} us; torch fwd alone {t['torch fwd']:.1f} us")
print(f"  bytes the forward must read: {(labels.numel() * 8 + score0.numel() * 4) / 1e6:.2f} MB")
print(f"  max rel difference hip vs torch: loss {rel(loss_h[0], torch_tail(score0, labels)):.1e}  grad "
      f"{rel(hip_pair(), torch.autograd.grad(torch_tail(score_t, labels), score_t)[0]):.1e}")

# ---- one whole SetCriterion forward + backward, with and without the deep-supervision entry
pred = lambda: (4.0 * F.interpolate(torch.randn(B * Q, 1, 17, 33, device="cuda", generator=g), size=(h, w), mode="bilinear",
                                    align_corners=True)[:, 0] - 5.0).view(B, Q, h, w).contiguous().requires_grad_(True)
logit = lambda: torch.randn(B, Q, K + 1, device="cuda", generator=g).requires_grad_(True)
final, aux = {"pred_logits": logit(), "pred_masks": pred()}, {"pred_logits": logit(), "pred_masks": pred()}
targets = [{"labels": torch.randint(0, K, (T,), device="cuda", generator=g),
            "masks": (F.interpolate(torch.randn(T, 1, 17, 33, device="cuda", generator=g), size=(H, W), mode="bilinear", align_corners=True)[:, 0] > 0).float(),
            "outlier_masks": labels[b]} for b in range(B)]
weights = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "outlier_loss": 1.0}
weights.update({k + "_0": v for k, v in list(weights.items())})
crit = SetCriterion(K, HungarianMatcher(2.0, 5.0, 5.0, P), weights, 0.1, ["labels", "masks", "outlier"], P, 3.0, 0.75, target="nls", score_norm="tanh",
                    func="squared_hinge", inlier_upper_threshold=THR_IN, outlier_lower_threshold=THR_OUT)


def step(outputs):
    leaves = [outputs["pred_logits"], outputs["pred_masks"]] + [v for a in outputs["aux_outputs"] for v in a.values()]
    return torch.autograd.grad(sum(crit.weighted(crit(outputs, targets)).values()), leaves)


c = timed({"final only": lambda: step({**final, "aux_outputs": []}), "final + 1 aux": lambda: step({**final, "aux_outputs": [aux]})}, batch=3)
print(f"SetCriterion fwd+bwd, B={B} Q={Q} masks {h}x{w} T={T}/image P={P} (matcher's host solve inside the window):")
print(f"  final outputs only {c['final only']:.0f} us   with the deep-supervision entry {c['final + 1 aux']:.0f} us   ratio {c['final + 1 aux'] / c['final only']:.2f}")
