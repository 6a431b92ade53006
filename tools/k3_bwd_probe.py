#!/usr/bin/env python3
"""Time K3's backward (rba_masked_xattn_bwd_f32: row pass + key pass, all three gradients) against the backward of the torch composition the
reference runs -- softmax(q k^T scale + mask) v with the [B*nH, Q, S] tensors materialised -- in the same process, alternating the two.
HIP events around each call after warm-up; median, min and max of 20 per side; two rounds so the spread between runs is visible.
    python tools/k3_bwd_probe.py [--out profiles/k3_backward_probe.txt]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops  # noqa: E402

SHAPES = [(1, 100, 512, 8, True), (2, 100, 512, 8, True), (1, 100, 2048, 8, True), (1, 100, 8192, 8, True), (1, 100, 100, 8, False)]
REPS, WARM = 20, 5


def composition(q, k, v, blocked):
    """the reference's arithmetic between the projections: materialised scores, masked_fill, softmax, P V"""
    B, Q, nH, hd = q.shape
    att = (q * hd ** -0.5).permute(0, 2, 1, 3) @ k.permute(0, 2, 3, 1)
    if blocked is not None:
        att = att.masked_fill(blocked[:, None], float("-inf"))
    return (torch.softmax(att, -1) @ v.permute(0, 2, 1, 3)).permute(0, 2, 1, 3).reshape(B, Q, nH * hd)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3, r


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[0], ts[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = [f"K3 backward probe on {torch.cuda.get_device_name(0)}: us per call, median [min .. max] of {REPS} after {WARM} warm-up calls, two rounds",
             "kernel = ops.masked_xattn_backward (dq, dk, dv; statistics pass included); composition = autograd backward of the materialised torch form",
             f"{'B,Q,S,nH':>16} {'mask':>5} | {'kernel r1':>24} {'kernel r2':>24} | {'composition r1':>24} {'composition r2':>24} | ratio (comp / kernel, medians)"]
    for B, Q, S, nH, masked in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(S)
        q, k, v = (torch.randn(B, n, nH, 32, device="cuda", generator=g) for n in (Q, S, S))
        go = torch.randn(B, Q, nH * 32, device="cuda", generator=g)
        ml = torch.randn(B, Q, S, device="cuda", generator=g) * 3 if masked else None
        blocked = None
        if masked:
            blocked = ml.sigmoid() < 0.5
            blocked[blocked.all(-1)] = False
        qa, ka, va = (t.clone().requires_grad_(True) for t in (q, k, v))
        out = composition(qa, ka, va, blocked)

        def kernel():
            return ops.masked_xattn_backward(q, k, v, ml, go)

        def comp():
            return torch.autograd.grad(out, (qa, ka, va), go, retain_graph=True)

        for _ in range(WARM):
            kernel()
            comp()
        torch.cuda.synchronize()
        rounds = {"kernel": [], "comp": []}
        for _ in range(2):
            tk, tc = [], []
            for _ in range(REPS):                      # alternating: both sides see the same machine
                tk.append(timed(kernel)[0])
                tc.append(timed(comp)[0])
            rounds["kernel"].append(stats(tk))
            rounds["comp"].append(stats(tc))
        gk, gc = kernel(), comp()
        diff = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(gk, gc))
        fmt = lambda s: f"{s[0]:8.1f} [{s[1]:6.1f} ..{s[2]:7.1f}]"      # noqa: E731
        mk = sum(r[0] for r in rounds["kernel"]) / 2
        mc = sum(r[0] for r in rounds["comp"]) / 2
        lines.append(f"{f'{B},{Q},{S},{nH}':>16} {'yes' if masked else 'no':>5} | {fmt(rounds['kernel'][0])} {fmt(rounds['kernel'][1])} | "
                     f"{fmt(rounds['comp'][0])} {fmt(rounds['comp'][1])} | {mc / mk:5.2f}   (max rel. difference of the gradients {diff:.1e})")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
