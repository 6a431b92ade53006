#!/usr/bin/env python3
"""Time the PEBAL fine-tune recipe's losses (K1 in front of K11, csrc/pebal_loss.hip) at the recipe's crop -- B = 2, Q = 100, K = 19, masks
128 x 256 -> labels 512 x 1024 (int64; 75 % class, 15 % outlier, 10 % void) -- forward + backward, beside the torch restatements of the
reference's criterion.py:245-388 and :435-518 (tests/_pebal_cases.py, tests/_rba_bwd_cases.py) on the same GPU and the same inputs:
(a) criterion.gambler_loss alone, (b) the whole recipe's criterion (gambler + smoothness + sparsity + outlier, weighted) on one outputs entry.
Also the kernels alone: K11a forward / backward, the blur of the B planes and its adjoint, K11b forward / backward.

HIP events around batches of 10 calls queued behind a long kernel; the median of 6 rounds after 2 warm-up rounds; the candidates alternate."""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops
from rba_amd.modeling.criterion import PebalCriterion, SemSegFunction, gambler_loss, k1_score
from tests._pebal_cases import OOD_REG, RECIPE_WEIGHTS, ref_gambler_loss, ref_pebal_entry

BATCH, ROUNDS, WARM = 10, 6, 2
B, Q, K, h, w, H, W = 2, 100, 19, 128, 256, 512, 1024
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
leaves = [logits, masks]
sem_seg = torch.randint(0, K, (B, H, W), device="cuda", generator=g)
r = torch.rand(B, H, W, device="cuda", generator=g)
outlier_masks = torch.zeros_like(sem_seg)
outlier_masks[r < 0.15] = 1
outlier_masks[(r >= 0.15) & (r < 0.25)] = 255
outputs = {"pred_logits": logits, "pred_masks": masks}
targets = [{"outlier_masks": o, "sem_seg": s} for o, s in zip(outlier_masks, sem_seg)]
criterion = PebalCriterion(K, RECIPE_WEIGHTS, ["gambler", "smoothness", "sparsity", "outlier"], OOD_REG, "energy", target="energy", score_norm="none",
                           func="squared_hinge", inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)

hip_gambler = lambda: gambler_loss(outputs, targets, num_classes=K, ood_reg=OOD_REG)["gambler_loss"]
torch_gambler = lambda: ref_gambler_loss(logits, masks, outlier_masks, sem_seg, OOD_REG)
hip_recipe = lambda: sum(criterion.weighted(criterion(outputs, targets)).values())
torch_recipe = lambda: sum(v * RECIPE_WEIGHTS[k] for k, v in ref_pebal_entry(logits, masks, outlier_masks, sem_seg).items())
with torch.no_grad():
    sem0 = SemSegFunction.apply(masks, F.softmax(logits, dim=-1)).contiguous()
    score0 = k1_score(outputs, "energy").contiguous()
    labels = torch.where(outlier_masks == 1, 254, torch.where(outlier_masks == 255, 255, sem_seg))
    _, gstats, R = ops.gambler_loss(sem0, labels, OOD_REG)
    _, sstats = ops.score_reg(score0, outlier_masks)
one = torch.ones((), device="cuda")

t = timed({
    "hip gambler": lambda: torch.autograd.grad(hip_gambler(), leaves), "torch gambler": lambda: torch.autograd.grad(torch_gambler(), leaves),
    "hip recipe": lambda: torch.autograd.grad(hip_recipe(), leaves), "torch recipe": lambda: torch.autograd.grad(torch_recipe(), leaves),
    "hip gambler fwd": hip_gambler, "torch gambler fwd": torch_gambler, "hip recipe fwd": hip_recipe, "torch recipe fwd": torch_recipe,
    "K11a fwd": lambda: ops.gambler_loss(sem0, labels, OOD_REG), "K11a bwd": lambda: ops.gambler_loss_backward(sem0, labels, gstats, R, one, OOD_REG),
    "blur": lambda: ops.gaussian_blur_planes(R), "blur adjoint": lambda: ops.gaussian_blur_planes_adjoint(R),
    "K11b fwd": lambda: ops.score_reg(score0, outlier_masks), "K11b bwd": lambda: ops.score_reg_backward(score0, outlier_masks, sstats, one, one),
})
rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
frac = [float((outlier_masks == 0).float().mean()), float((outlier_masks == 1).float().mean()), float((outlier_masks == 255).float().mean())]
print(f"B={B} Q={Q} K={K} masks {h}x{w} -> labels {H}x{W} int64 (class {frac[0]:.2f}, outlier {frac[1]:.2f}, void {frac[2]:.2f}) ood_reg={OOD_REG}")
for name in ("gambler", "recipe"):
    print(f"  {name:8s} fwd+bwd : hip {t['hip ' + name]:8.1f} us   torch {t['torch ' + name]:8.1f} us   hip / torch = {t['hip ' + name] / t['torch ' + name]:.3f}")
    print(f"  {name:8s} fwd     : hip {t['hip ' + name + ' fwd']:8.1f} us   torch {t['torch ' + name + ' fwd']:8.1f} us")
print(f"  kernels alone: K11a fwd {t['K11a fwd']:.1f} us, K11a bwd {t['K11a bwd']:.1f} us, blur of {B} planes {t['blur']:.1f} us, its adjoint "
      f"{t['blur adjoint']:.1f} us, K11b fwd {t['K11b fwd']:.1f} us, K11b bwd {t['K11b bwd']:.1f} us")
print(f"  bytes K11a's forward must move: labels {labels.numel() * 8 / 1e6:.2f} MB, class map 2 x {sem0.numel() * 4 / 1e6:.2f} MB, "
      f"reward / R maps 4 x {R.numel() * 4 / 1e6:.2f} MB")
for name, hip, ref in (("gambler", hip_gambler, torch_gambler), ("recipe", hip_recipe, torch_recipe)):
    gh, gt = torch.autograd.grad(hip(), leaves), torch.autograd.grad(ref(), leaves)
    print(f"  {name}: max rel difference hip vs torch: loss {rel(hip().detach(), ref().detach()):.1e}  grads "
          + "  ".join(f"{n} {rel(a, b):.1e}" for n, a, b in zip(("pred_logits", "pred_masks"), gh, gt)))
ok_g, ok_r = t["hip gambler"] < t["torch gambler"], t["hip recipe"] < t["torch recipe"]
print(f"condition (kernel path's median below the torch side's): gambler_loss {'holds' if ok_g else 'FAILS'}, recipe criterion {'holds' if ok_r else 'FAILS'}")
sys.exit(0 if ok_g and ok_r else 1)
