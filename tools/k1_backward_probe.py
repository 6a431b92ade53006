#!/usr/bin/env python3
"""A probe, not a benchmark: device-event timing of K1's backward at the two mask resolutions of the outlier-supervised fine-tune,
(Q, K, h x w) = (100, 19, 128 x 256) (the training crop at quarter resolution) and (100, 19, 256 x 512), per shape
  * the backward launch (the whole entry point: the tile kernel and the second reduction stage), and its share of the 8 Q HW-byte traffic floor
    (one read of the mask logits, one write of their gradient) at 8 TB/s;
  * forward + backward through RbaScoreFunction (torch allocations and autograd bookkeeping included);
  * the torch-op formulation of criterion.py:449-463 (sigmoid, einsum, tanh, sum, autograd backward) on the same GPU, the same inputs and
    the same grad_score -- the yardstick, since the library had no such capability before;
  * each path's peak extra device memory (torch's allocator high-water mark above what is live before the call);
and the e / b table of the cases of tests/_rba_bwd_cases.py (e = max|T_gpu - T64| / max|T64|, b = the same for fp32 CPU autograd,
bar = 4 max(b, 2^-20)).  The record goes to profiles/k1_backward_probe.json (--out).
`python tools/k1_backward_probe.py [--samples 20] [--batch 10] [--out FILE]`

Protocol (docs/measurements.md): >= 1 s of back-to-back launches of the timed form, then `--samples` windows of `--batch` launches between
two device events (samples x batch >= 200 launches); median, min, p90 per launch."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from rba_amd import _lib, ops  # noqa: E402
from rba_amd.modeling.criterion import RbaScoreFunction  # noqa: E402

HBM = 8.0e12
SHAPES = {"128x256": (100, 19, 128, 256), "256x512": (100, 19, 256, 512)}


def time_launches(fn, samples, batch, warmup_s=1.0):
    t0 = time.time()
    while time.time() - t0 < warmup_s:
        for _ in range(batch):
            fn()
        torch.cuda.synchronize()
    us = []
    for _ in range(samples):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(batch):
            fn()
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3 / batch)
    us.sort()
    return {"median_us": round(statistics.median(us), 2), "min_us": round(us[0], 2), "p90_us": round(us[int(0.9 * (len(us) - 1))], 2)}


def peak_extra_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def torch_ops_step(mask, prob, g):
    """criterion.py:449-463 for one image, written in torch ops, and its autograd backward"""
    m, p = mask.detach().requires_grad_(True), prob.detach().requires_grad_(True)
    sem = torch.einsum("qc,qhw->chw", p, m.sigmoid())
    score = -sem.tanh().sum(dim=0)
    score.backward(g)
    return m.grad, p.grad


def fused_step(mask, prob, g):
    m, p = mask.detach().requires_grad_(True), prob.detach().requires_grad_(True)
    RbaScoreFunction.apply(m[None], p[None], "rba").backward(g[None])
    return m.grad, p.grad


def timings(args):
    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for name, (Q, K, h, w) in SHAPES.items():
        gen = torch.Generator().manual_seed(0)
        mask = (6.0 * torch.randn(Q, h, w, generator=gen)).cuda()
        prob = torch.softmax(2.0 * torch.randn(Q, K + 1, generator=gen), -1)[:, :-1].contiguous().cuda()
        g = torch.randn(h, w, generator=gen).cuda()
        HW = h * w
        n = torch.zeros(1, dtype=torch.int64)
        _lib.check(lib.rba_reduce_bwd_workspace_f32(Q, K, HW, n.data_ptr()), "workspace")
        ws = torch.empty(int(n) // 4, device="cuda")
        gm, gp = torch.empty_like(mask), torch.empty_like(prob)

        def bwd():
            _lib.check(lib.rba_reduce_bwd_f32(mask.data_ptr(), prob.data_ptr(), g.data_ptr(), gm.data_ptr(), gp.data_ptr(), Q, K, HW, 0,
                                              ws.data_ptr(), int(n), st), "bwd")

        floor_us = 8.0 * Q * HW / HBM * 1e6
        r = {"Q": Q, "K": K, "h": h, "w": w, "traffic_floor_bytes": 8 * Q * HW, "traffic_floor_us": round(floor_us, 2),
             "workspace_bytes": int(n)}
        r["backward_launch"] = time_launches(bwd, args.samples, args.batch)
        r["backward_launch"]["fraction_of_floor_at_8TBps"] = round(floor_us / r["backward_launch"]["median_us"], 3)
        r["fused_forward_backward"] = time_launches(lambda: fused_step(mask, prob, g), args.samples, args.batch)
        r["torch_ops_forward_backward"] = time_launches(lambda: torch_ops_step(mask, prob, g), args.samples, args.batch)
        r["torch_ops_over_fused"] = round(r["torch_ops_forward_backward"]["median_us"] / r["fused_forward_backward"]["median_us"], 2)
        r["fused_forward_backward"]["peak_extra_bytes"] = peak_extra_bytes(lambda: fused_step(mask, prob, g))
        r["torch_ops_forward_backward"]["peak_extra_bytes"] = peak_extra_bytes(lambda: torch_ops_step(mask, prob, g))
        a, b = fused_step(mask, prob, g), torch_ops_step(mask, prob, g)
        r["fused_vs_torch_ops_max_rel_diff"] = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(a, b)]
        out[name] = r
    return out


def errors():
    from tests import _rba_bwd_cases as C
    rows, worst = [], 0.0
    for name, score in C.CASE_MODES:
        _, Q, K, N, *_ = C.CASE[name]
        mask, prob, g = (t.cuda() for t in C.case_inputs(name))
        gm64, gp64, b_mask, b_prob = C.case_truth(name, score)
        gm, gp = ops.rba_reduce_backward(mask.view(Q, 1, N), prob, g.view(1, N), score=score)
        row = {"case": name, "Q": Q, "K": K, "N": N, "score": score}
        for tn, t, t64, b in (("grad_mask", gm.cpu().view(Q, N), gm64, b_mask), ("grad_prob", gp.cpu(), gp64, b_prob)):
            e = C.err(t, t64)
            row[tn] = {"e": e, "b": b, "bar": C.bar(b)}
            worst = max(worst, e / C.bar(b))
        rows.append(row)
    return rows, worst


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=20)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "k1_backward_probe.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a HIP device"
    assert a.samples * a.batch >= 200
    rec = {"probe": "k1_backward", "device": torch.cuda.get_device_name(0), "samples": a.samples, "launches_per_sample": a.batch,
           "hbm_rate_assumed_TBps": HBM / 1e12, "shapes": timings(a)}
    rows, worst = errors()
    rec["errors"] = {"metric": "e = max|T_gpu - T64| / max|T64|; b = the same for fp32 CPU autograd; bar = 4 max(b, 2^-20)", "cases": rows,
                     "worst_e_over_bar": worst}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"probe": "k1_backward", "out": a.out, "worst_e_over_bar": worst,
                      **{k: {"backward_us": v["backward_launch"]["median_us"], "of_floor": v["backward_launch"]["fraction_of_floor_at_8TBps"],
                             "fused_us": v["fused_forward_backward"]["median_us"], "torch_ops_us": v["torch_ops_forward_backward"]["median_us"]}
                         for k, v in rec["shapes"].items()}}))
