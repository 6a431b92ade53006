#!/usr/bin/env python3
"""A probe, not a benchmark: device-event timing of K2 forward, K2 backward (model form) and K2 backward (generic form) at the C2 encoder
shape (1 level, 2 048 tokens) and the C5 encoder shape (3 levels, 19 320 tokens); one JSON line with the times, the grad_value atomic bytes
(counted from the inputs: in-map taps of in-window samples x 128 B) and atomic bytes / time as a fraction of the 1.3 TB/s chip-wide rate of
global float atomic adds.  `python tools/k2_backward_probe.py [--samples 30] [--batch 10] [--out FILE]`

Protocol (docs/measurements.md): >= 1 s of warm-up launches of the timed form, then `--samples` timed windows of `--batch` back-to-back
launches between two device events (outputs preallocated, the C ABI called directly: the host stays ahead of the device); median, min, p90
per launch.  A backward launch is the whole entry point: the zero-fill of grad_value and the kernel.

`--errors` instead runs the cases of tests/_msda_cases.py (the GPU test file's helper) and writes the measured e / b record per case and
gradient tensor (default profiles/k2_backward_errors.json): e = max|T_gpu - T64| / max|T64| against fp64 CPU autograd through the oracle,
b = the same for the oracle's fp32 CPU autograd, bar = 4 max(b, 2^-20) (fp64: 1e-10)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _knobs  # noqa: F401,E402  (knob-writing tool: run on librba_hip_knobs.so)
from rba_amd import _lib, ops  # noqa: E402

ATOMIC_RATE = 1.3e12        # bytes/s of added bytes, chip-wide (global float atomic adds, MI355X)
M, D, P = 8, 32, 4
SHAPES = {"C2": [(32, 64)], "C5": [(92, 160), (46, 80), (23, 40)]}


def encoder_inputs(hw, seed=0):
    """encoder self-attention: one query per pixel, reference point on its centre, offsets of about 1.5 pixels, softmaxed weights"""
    g = torch.Generator().manual_seed(seed)
    L = len(hw)
    sh = torch.tensor(hw, dtype=torch.int64)
    S = int(sh.prod(1).sum())
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    ref = torch.cat([torch.stack(((torch.arange(w, dtype=torch.float32) + 0.5).repeat(h) / w,
                                  (torch.arange(h, dtype=torch.float32) + 0.5).repeat_interleave(w) / h), -1) for h, w in hw], 0)
    wh = torch.tensor(hw, dtype=torch.float32).flip(-1).view(1, 1, 1, L, 1, 2)
    loc = ref.view(1, S, 1, 1, 1, 2) + torch.randn(1, S, M, L, P, 2, generator=g) * 1.5 / wh
    w = torch.softmax(torch.randn(1, S, M, L * P, generator=g), -1).view(1, S, M, L, P)
    value = torch.randn(1, S, M, D, generator=g)
    go = torch.randn(1, S, M * D, generator=g)
    # grad_value atomic traffic: every in-map tap of every in-window sample is one 128-byte (32 x fp32) segment
    pix = loc * wh - 0.5
    inside = ((pix > -1) & (pix < wh)).all(-1)
    f = pix.floor()
    taps = torch.zeros_like(inside, dtype=torch.int64)
    for dy in (0, 1):
        for dx in (0, 1):
            x, y = f[..., 0] + dx, f[..., 1] + dy
            taps += (inside & (x >= 0) & (x <= wh[..., 0] - 1) & (y >= 0) & (y <= wh[..., 1] - 1)).long()
    return dict(value=value, shapes=sh, lsi=lsi, loc=loc, w=w, go=go, S=S, L=L, atomic_bytes=int(taps.sum()) * D * 4,
                atomic_bytes_all_taps=S * M * L * P * 4 * D * 4)


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


def probe(args):
    lib = _lib.load()
    knob = _lib.knob("rba_k2_bwd_variant")
    st = torch.cuda.current_stream().cuda_stream
    res = {"probe": "k2_backward", "device": torch.cuda.get_device_name(0), "samples": args.samples, "launches_per_sample": args.batch,
           "atomic_rate_assumed_TBps": ATOMIC_RATE / 1e12, "shapes": {}}
    for name, hw in SHAPES.items():
        inp = encoder_inputs(hw)
        S, L = inp["S"], inp["L"]
        t = {k: inp[k].cuda().contiguous() for k in ("value", "shapes", "lsi", "loc", "w", "go")}
        out = torch.empty(1, S, M * D, device="cuda")
        gv, gl, ga = torch.empty_like(t["value"]), torch.empty_like(t["loc"]), torch.empty_like(t["w"])
        p = [x.data_ptr() for x in (t["value"], t["shapes"], t["lsi"], t["loc"], t["w"])]

        def fwd():
            _lib.check(lib.rba_ms_deform_attn_fwd_f32(*p, out.data_ptr(), 1, S, M, D, L, S, P, st), "fwd")

        def bwd():
            _lib.check(lib.rba_ms_deform_attn_bwd_f32(*p, t["go"].data_ptr(), gv.data_ptr(), gl.data_ptr(), ga.data_ptr(), 1, S, M, D, L, S, P, st), "bwd")

        r = {"tokens": S, "levels": L, "grad_value_atomic_bytes": inp["atomic_bytes"], "grad_value_atomic_bytes_if_all_taps_in_map": inp["atomic_bytes_all_taps"],
             "atomic_floor_us": round(inp["atomic_bytes"] / ATOMIC_RATE * 1e6, 1)}
        r["forward"] = time_launches(fwd, args.samples, args.batch)
        knob.value = 0
        r["backward_model_form"] = time_launches(bwd, args.samples, args.batch)
        model = [x.clone() for x in (gv, gl, ga)]
        knob.value = 1
        try:
            r["backward_generic_form"] = time_launches(bwd, args.samples, args.batch)
        finally:
            knob.value = 0
        # the two forms computed the same thing (reordered fp32 sums)
        r["forms_max_rel_diff"] = [float((a - b).abs().max() / a.abs().max()) for a, b in zip(model, (gv, gl, ga))]
        for k in ("backward_model_form", "backward_generic_form"):
            r[k]["fraction_of_atomic_rate"] = round(inp["atomic_bytes"] / (r[k]["median_us"] * 1e-6) / ATOMIC_RATE, 3)
        r["backward_over_forward"] = round(r["backward_model_form"]["median_us"] / r["forward"]["median_us"], 1)
        res["shapes"][name] = r
    print(json.dumps(res))


def errors(args):
    from tests import _msda_cases as C
    knob = _lib.knob("rba_k2_bwd_variant")
    rec = {"metric": "e = max|T_gpu - T64| / max|T64|; b = the same for fp32 CPU autograd of the oracle; bar = 4 max(b, 2^-20), fp64 bar 1e-10",
           "device": torch.cuda.get_device_name(0), "cases": []}
    runs = [(n, torch.float32, v) for n in C.FP32_CASES for v in ((0, 1) if C.CASES[n][2] == 32 and C.CASES[n][5] == 4 else (0,))]
    runs += [(n, torch.float64, 0) for n in C.FP64_CASES]
    worst = 0.0
    for name, dt, variant in runs:
        inp = C.make(name, dt)
        t64 = C.cpu_grads(inp, torch.float64)
        b = [C.err(t, r) for t, r in zip(C.cpu_grads(inp, torch.float32), t64)] if dt == torch.float32 else [None] * 3
        knob.value = variant
        try:
            got = ops.ms_deform_attn_backward(*[inp[k].cuda().contiguous() for k in ("value", "shapes", "lsi", "loc", "w", "go")])
        finally:
            knob.value = 0
        e = [C.err(t, r) for t, r in zip(got, t64)]
        bars = [C.FP64_BAR if dt == torch.float64 else C.bar(x) for x in b]
        worst = max(worst, max(x / y for x, y in zip(e, bars)))
        rec["cases"].append({"case": name, "dtype": str(dt).replace("torch.", ""), "form": "generic (forced)" if variant else "dispatch",
                             "outside_share": round(float(C.outside(inp["loc"], inp["shape_list"]).float().mean()), 3),
                             **{tn: {"e": e[i], "b": b[i], "bar": bars[i]} for i, tn in enumerate(C.NAMES)}})
    rec["worst_e_over_bar"] = worst
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"probe": "k2_backward_errors", "cases": len(rec["cases"]), "worst_e_over_bar": worst, "out": args.out}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--errors", action="store_true")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "k2_backward_errors.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this probe needs a HIP device"
    assert a.samples >= 20
    (errors if a.errors else probe)(a)
