#!/usr/bin/env python3
"""Time K4's backward (rba_mask_logits_bwd_f32: grad_embed alone, grad_feat alone, both in one call) at the fine-tune's shapes, beside what a
user got before it for the same gradients: torch autograd's backward of torch.einsum("bqc,bchw->bqhw") on the same tensors (library GEMMs).
HIP events around batches of launches queued behind a long kernel; median over >= 50 launches after >= 10 warm-ups; the two sides alternate.
Prints each kernel's fraction of its larger floor (traffic at 8 TB/s, padded MFMA work at 157 TFLOP/s) and checks the results against fp64."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops

HBM, MFMA = 8e12, 157e12
BATCH, ROUNDS, WARM = 10, 6, 2           # 10 launches per event pair, 6 timed rounds (60 launches) after 2 warm-up rounds (20 launches)
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


def floors(Q, C, N):
    """(us of traffic, us of padded MFMA work) per gradient: one pass over its two inputs and its output; 16-padded rows of the MFMA tile"""
    qp, cp = (Q + 15) // 16 * 16, (C + 15) // 16 * 16
    return {"embed": (4 * (C * N + Q * N + Q * C) / HBM * 1e6, 2 * qp * cp * N / MFMA * 1e6),
            "feat": (4 * (Q * N + Q * C + C * N) / HBM * 1e6, 2 * ((Q + 3) // 4 * 4) * cp * N / MFMA * 1e6)}


for B, Q, C, h, w in ((1, 100, 256, 128, 256), (1, 100, 256, 256, 512)):
    N = h * w
    g = torch.Generator(device="cuda").manual_seed(0)
    E = torch.randn(B, Q, C, device="cuda", generator=g)
    F = 0.25 * torch.randn(B, C, h, w, device="cuda", generator=g)
    G = torch.randn(B, Q, h, w, device="cuda", generator=g) * 1e-3
    Ea, Fa = E.clone().requires_grad_(True), F.clone().requires_grad_(True)
    Eo, Fo = E.clone().requires_grad_(True), F.clone()
    out_both = torch.einsum("bqc,bchw->bqhw", Ea, Fa)
    out_embed = torch.einsum("bqc,bchw->bqhw", Eo, Fo)
    Ff, Ef = F.clone().requires_grad_(True), E.clone()
    out_feat = torch.einsum("bqc,bchw->bqhw", Ef, Ff)
    t = timed({
        "hip embed": lambda: ops.mask_logits_backward(None, F, G, need_feat=False),
        "torch embed": lambda: torch.autograd.grad(out_embed, Eo, G, retain_graph=True),
        "hip feat": lambda: ops.mask_logits_backward(E, None, G, need_embed=False),
        "torch feat": lambda: torch.autograd.grad(out_feat, Ff, G, retain_graph=True),
        "hip both": lambda: ops.mask_logits_backward(E, F, G),
        "torch both": lambda: torch.autograd.grad(out_both, (Ea, Fa), G, retain_graph=True),
    })
    ge, gf = ops.mask_logits_backward(E, F, G)
    ge64 = torch.einsum("bqn,bcn->bqc", G.flatten(2).double(), F.flatten(2).double())
    gf64 = torch.einsum("bqc,bqn->bcn", E.double(), G.flatten(2).double())
    te, tf = torch.autograd.grad(out_both, (Ea, Fa), G, retain_graph=True)
    rel = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    fl = floors(Q, C, N)
    print(f"B={B} Q={Q} C={C} N={N}")
    for k in ("embed", "feat"):
        floor = max(fl[k])
        print(f"  grad_{k}: hip {t['hip ' + k]:7.1f} us  torch {t['torch ' + k]:7.1f} us   floors: traffic {fl[k][0]:.1f} us, MFMA {fl[k][1]:.1f} us"
              f"  -> {floor / t['hip ' + k]:.2f} of the larger floor")
    print(f"  both      : hip {t['hip both']:7.1f} us  torch {t['torch both']:7.1f} us")
    print(f"  max rel err vs fp64: hip embed {rel(ge, ge64):.1e} feat {rel(gf.flatten(2), gf64):.1e} | torch embed {rel(te, ge64):.1e} "
          f"feat {rel(tf.flatten(2), gf64):.1e}")
