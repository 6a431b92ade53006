#!/usr/bin/env python3
"""Time criterion.densehybrid_loss (K1's class map and its per-class adjoint around K10, csrc/dense_hybrid_loss.hip) at the DenseHybrid recipe's
crop -- B = 2, Q = 100, K = 19, masks 128 x 256 -> labels 512 x 1024 (int64; classes, 15 % outlier, 10 % void) -- forward + backward, beside the
torch restatement of the reference's criterion.py:390-433 (tests/_dense_hybrid_cases.py) on the same GPU and the same inputs: softmax, sigmoid,
einsum, the two F.interpolate(align_corners=True) to the label size, log_softmax, logsumexp, the global mean, the two nll_loss, and autograd's
backward of all of it.  That is what a user of this library ran before K10.  Also: K10's forward alone, its backward alone, and uint8 labels.

HIP events around batches of 10 calls queued behind a long kernel; the median of 6 rounds after 2 warm-up rounds; the candidates alternate."""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops
from rba_amd.modeling.criterion import SemSegFunction, densehybrid_loss
from tests._dense_hybrid_cases import ref_densehybrid_loss

BATCH, ROUNDS, WARM = 10, 6, 2
B, Q, K, h, w, H, W = 2, 100, 19, 128, 256, 512, 1024
BETA = 0.03
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


g = torch.Generator(device="cuda").manual_seed(0)
smooth = lambda n: F.interpolate(torch.randn(n, 1, 17, 33, device="cuda", generator=g), size=(h, w), mode="bilinear", align_corners=True)[:, 0]
logits = (2.0 * torch.randn(B, Q, K + 1, device="cuda", generator=g)).requires_grad_(True)
masks = (4.0 * smooth(B * Q) - 2.0).view(B, Q, h, w).contiguous().requires_grad_(True)
ood = (1.5 * smooth(B * 2)).view(B, 2, h, w).contiguous().requires_grad_(True)
leaves = [logits, masks, ood]
labels = torch.randint(0, K, (B, H, W), device="cuda", generator=g)
r = torch.rand(B, H, W, device="cuda", generator=g)
labels[r < 0.15] = 254
labels[(r >= 0.15) & (r < 0.25)] = 255
labels8 = labels.to(torch.uint8)
outputs = {"pred_logits": logits, "pred_masks": masks, "ood_pred": ood}
targets, targets8 = [{"sem_seg": l} for l in labels], [{"sem_seg": l} for l in labels8]

hip_loss = lambda tg=targets: densehybrid_loss(outputs, tg, num_classes=K, beta=BETA)["densehybrid_loss"]
torch_loss = lambda: ref_densehybrid_loss(logits, masks, ood, labels, BETA)
with torch.no_grad():
    sem0 = SemSegFunction.apply(masks, F.softmax(logits, dim=-1)[..., :-1]).contiguous()
    ood0 = ood.detach()
    _, stats, lse = ops.dense_hybrid_loss(sem0, ood0, labels, BETA)
one = torch.ones((), device="cuda")

t = timed({
    "hip fwd+bwd": lambda: torch.autograd.grad(hip_loss(), leaves), "torch fwd+bwd": lambda: torch.autograd.grad(torch_loss(), leaves),
    "hip fwd+bwd uint8": lambda: torch.autograd.grad(hip_loss(targets8), leaves),
    "hip fwd": hip_loss, "torch fwd": torch_loss,
    "K10 fwd": lambda: ops.dense_hybrid_loss(sem0, ood0, labels, BETA),
    "K10 bwd": lambda: ops.dense_hybrid_loss_backward(sem0, ood0, labels, stats, lse, one, BETA),
    "K1 sem_seg fwd": lambda: [ops.rba_reduce(m, p, want_sem_seg=True) for m, p in zip(masks.detach(), F.softmax(logits.detach(), dim=-1)[..., :-1].contiguous())],
    "K1 sem_seg bwd": lambda: [ops.sem_seg_backward(m, p, s) for m, p, s in zip(masks.detach(), F.softmax(logits.detach(), dim=-1)[..., :-1].contiguous(), sem0)],
})
rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
frac = [float(((labels < K)).float().mean()), float((labels == 254).float().mean()), float((labels == 255).float().mean())]
print(f"B={B} Q={Q} K={K} masks {h}x{w} -> labels {H}x{W} int64 (class {frac[0]:.2f}, outlier {frac[1]:.2f}, void {frac[2]:.2f}) beta={BETA}")
print(f"  densehybrid_loss fwd+bwd : hip {t['hip fwd+bwd']:8.1f} us   torch {t['torch fwd+bwd']:8.1f} us   hip / torch = {t['hip fwd+bwd'] / t['torch fwd+bwd']:.3f}")
print(f"  densehybrid_loss fwd     : hip {t['hip fwd']:8.1f} us   torch {t['torch fwd']:8.1f} us")
print(f"  hip fwd+bwd on uint8 labels {t['hip fwd+bwd uint8']:.1f} us")
print(f"  kernels alone: K10 fwd {t['K10 fwd']:.1f} us, K10 bwd {t['K10 bwd']:.1f} us, K1 class map (2 images) {t['K1 sem_seg fwd']:.1f} us, "
      f"its per-class adjoint (2 images) {t['K1 sem_seg bwd']:.1f} us")
print(f"  bytes K10's forward must read: {(labels.numel() * 8 + sem0.numel() * 4 + ood0.numel() * 4) / 1e6:.2f} MB")
gh, gt = torch.autograd.grad(hip_loss(), leaves), torch.autograd.grad(torch_loss(), leaves)
print(f"  max rel difference hip vs torch: loss {rel(hip_loss().detach(), torch_loss().detach()):.1e}  grads "
      + "  ".join(f"{n} {rel(a, b):.1e}" for n, a, b in zip(("pred_logits", "pred_masks", "ood_pred"), gh, gt)))
ok = t["hip fwd+bwd"] < t["torch fwd+bwd"]
print(f"condition (kernel path's median below the torch side's): {'holds' if ok else 'FAILS'}")
sys.exit(0 if ok else 1)
