#!/usr/bin/env python3
"""Time K8 (csrc/point_loss.hip) at the fine-tune recipe's shape -- B = 2, Q = 100, masks 128 x 256, targets 512 x 1024, 19 targets per image,
P = 12544 points, oversampling 3 -- leg by leg beside the torch composition of the same steps on the same GPU (grid_sample, einsum, autograd):

  matcher cost    ops.match_cost per image                      | grid_sample of Q + T planes, BCE pos / neg, two einsums per term
  oversampling    select_uncertain_points (ops.point_sample)    | grid_sample of the gathered matched masks + topk + gather
  labels          ops.point_sample of the target masks          | grid_sample of the gathered target masks
  loss fwd + bwd  MaskPointLossFunction forward and backward    | gather + grid_sample + BCE / dice + autograd (grid_sample's scatter backward)

HIP events around batches of launches queued behind a long kernel; median over 60 launches after 20 warm-ups; the two sides alternate.  Prints
the scatter's added bytes / time against the chip-wide float-atomic rate, and each leg's difference from the torch side."""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops
from rba_amd.modeling.criterion import MaskPointLossFunction, select_uncertain_points

ATOMIC_RATE = 1.3e12                     # bytes / s of well-shaped global float atomic adds, chip-wide
BATCH, ROUNDS, WARM = 10, 6, 2
B, Q, h, w, H, W, T, P, OVER, K = 2, 100, 128, 256, 512, 1024, 19, 12544, 3, 19
busy = torch.randn(8192, 8192, device="cuda")


def timed(fns):
    """{name: median us per call}: the candidates alternate round by round, each round = BATCH launches bracketed by events behind a long kernel"""
    ts = {k: [] for k in fns}
    for i in range(WARM + ROUNDS):
        for k, fn in fns.items():
            busy @ busy
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= WARM:
                ts[k].append(e0.elapsed_time(e1) * 1e3 / BATCH)
    return {k: sorted(v)[len(v) // 2] for k, v in ts.items()}


def grid(x, c):
    """detectron2's point_sample: x [N,1,h,w], c [N,P,2] -> [N,P]"""
    return F.grid_sample(x, 2.0 * c[:, :, None] - 1.0, mode="bilinear", padding_mode="zeros", align_corners=False)[:, 0, :, 0]


g = torch.Generator(device="cuda").manual_seed(0)
coarse = torch.randn(B * Q, 1, 17, 33, device="cuda", generator=g)
pred = (4.0 * F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)[:, 0]).view(B, Q, h, w).contiguous()
tgt = (F.interpolate(torch.randn(B * T, 1, 17, 33, device="cuda", generator=g), size=(H, W), mode="bilinear", align_corners=True)[:, 0] > 0).float()
prob = torch.softmax(torch.randn(B, Q, K + 1, device="cuda", generator=g), -1)
ids = torch.randint(0, K, (B, T), device="cuda", generator=g)
mcoords = torch.rand(P, 2, device="cuda", generator=g)
N = B * T
plane_index = torch.cat([b * Q + torch.randperm(Q, device="cuda", generator=g)[:T] for b in range(B)])
tgt_index = torch.arange(N, device="cuda")
cand = torch.rand(N, OVER * P, 2, device="cuda", generator=g)
lcoords = torch.rand(N, P, 2, device="cuda", generator=g)
labels = ops.point_sample(tgt, lcoords, tgt_index)
num_masks = float(N)
wm, wc, wd = 5.0, 2.0, 5.0


def torch_cost(b):
    c = mcoords[None]
    x = grid(pred[b][:, None], c.expand(Q, -1, -1))
    t = grid(tgt[b * T:(b + 1) * T][:, None], c.expand(T, -1, -1))
    pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    cm = (torch.einsum("nc,mc->nm", pos, t) + torch.einsum("nc,mc->nm", neg, 1 - t)) / P
    s = x.sigmoid()
    cd = 1 - (2 * torch.einsum("nc,mc->nm", s, t) + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None] + 1)
    return wm * cm + wc * -prob[b][:, ids[b]] + wd * cd


def hip_cost(b):
    return ops.match_cost(pred[b], tgt[b * T:(b + 1) * T], mcoords, prob[b], ids[b], wm, wc, wd)


def torch_select():
    src = pred.flatten(0, 1)[plane_index][:, None]
    idx = torch.topk(-grid(src, cand).abs(), k=int(0.75 * P), dim=1)[1]
    return torch.gather(cand, 1, idx[:, :, None].expand(-1, -1, 2))


pred_t = pred.clone().requires_grad_(True)
pred_h = pred.clone().requires_grad_(True)


def torch_loss():
    x = grid(pred_t.flatten(0, 1)[plane_index][:, None], lcoords)
    lm = F.binary_cross_entropy_with_logits(x, labels, reduction="none").mean(1).sum() / num_masks
    s = x.sigmoid()
    ld = (1 - (2 * (s * labels).sum(-1) + 1) / (s.sum(-1) + labels.sum(-1) + 1)).sum() / num_masks
    return torch.autograd.grad(wm * lm + wd * ld, pred_t)[0]


def hip_loss():
    lm, ld = MaskPointLossFunction.apply(pred_h, plane_index, lcoords, labels, num_masks)
    return torch.autograd.grad(wm * lm + wd * ld, pred_h)[0]


losses, sums = ops.mask_point_loss(pred, plane_index, lcoords, labels, num_masks)
one = torch.ones((), device="cuda")
t = timed({
    "hip cost": lambda: [hip_cost(b) for b in range(B)], "torch cost": lambda: [torch_cost(b) for b in range(B)],
    "hip oversampling": lambda: select_uncertain_points(pred, plane_index, cand, int(0.75 * P)), "torch oversampling": torch_select,
    "hip labels": lambda: ops.point_sample(tgt, lcoords, tgt_index), "torch labels": lambda: grid(tgt[tgt_index][:, None], lcoords),
    "hip loss fwd+bwd": hip_loss, "torch loss fwd+bwd": torch_loss,
    "hip loss fwd": lambda: ops.mask_point_loss(pred, plane_index, lcoords, labels, num_masks),
    "hip loss bwd": lambda: ops.mask_point_loss_backward(pred, plane_index, lcoords, labels, sums, num_masks, one, one),
    "zero fill": lambda: torch.zeros_like(pred),
})
rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())
print(f"B={B} Q={Q} masks {h}x{w} targets {H}x{W} T={T}/image P={P} oversample {OVER}  (N = {N} matched masks)")
for leg in ("cost", "oversampling", "labels", "loss fwd+bwd"):
    a, b = t["hip " + leg], t["torch " + leg]
    print(f"  {leg:14s}: hip {a:8.1f} us   torch {b:8.1f} us   hip / torch = {a / b:.2f}")
print(f"  loss fwd alone {t['hip loss fwd']:.1f} us, bwd alone {t['hip loss bwd']:.1f} us, of which a zero fill of [{B},{Q},{h},{w}] is ~{t['zero fill']:.1f} us")
added = N * P * 4 * 4
scatter = max(t["hip loss bwd"] - t["zero fill"], 1e-3)
print(f"  scatter: {added / 1e6:.1f} MB of added bytes in ~{scatter:.1f} us = {added / scatter / 1e6:.3f} TB/s against {ATOMIC_RATE / 1e12:.1f} TB/s for well-shaped atomics")
print(f"  max rel difference hip vs torch: cost {max(rel(hip_cost(b), torch_cost(b)) for b in range(B)):.1e}  labels "
      f"{rel(ops.point_sample(tgt, lcoords, tgt_index), grid(tgt[tgt_index][:, None], lcoords)):.1e}  grad {rel(hip_loss(), torch_loss()):.1e}")
