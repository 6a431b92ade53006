"""K15 beside torch: one optimizer step -- clip_grad_norm_(params, 0.01) + AdamW -- at the Swin-B recipe's head shapes, between HIP events.

    python tools/optimizer_step_probe.py [--steps 300] [--warmup 50] [--big 67108864] [--out FILE]

Three forms on the same ten tensors (decoder_norm 2 x 256, class_embed 20 x 256 + 20, mask_embed 3 x (256 x 256 + 256): 203 028 elements), alternated round by
round so that clock and neighbours hit all three alike: K15 (ClipAdamW.step), torch.optim.AdamW(foreach=True) and AdamW(fused=True), the last two behind
torch.nn.utils.clip_grad_norm_.  A timed round is `steps` steps between two events; the figure is the median over rounds of (round time / steps), with min and
max.  Launches per step are counted from the kineto trace of one step of each form (K15's are also the two recorded entry points).  Then the streaming form
once: a single tensor of `--big` elements, K15a + K15b, achieved bytes/s at 28 B per element (K15a reads 4; K15b reads 16 and writes 12) against 8 TB/s.
One JSON object on stdout (and in --out).
"""
import argparse
import json
import os
import statistics
import sys

import torch

HEAD_SHAPES = [(256,), (256,), (20, 256), (20,), (256, 256), (256,), (256, 256), (256,), (256, 256), (256,)]
WEIGHT_DECAYS = [0.0, 0.0] + [0.05] * 8
PEAK_BYTES_PER_S = 8.0e12


def _params(shapes, seed=0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=gen).cuda().requires_grad_(True) for s in shapes]


def _torch_step(params, **kw):
    opt = torch.optim.AdamW([{"params": [p], "weight_decay": wd} for p, wd in zip(params, WEIGHT_DECAYS)], lr=1e-4, **kw)

    def step():
        torch.nn.utils.clip_grad_norm_(params, 0.01)
        opt.step()
    return step


def _timed(step, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / steps          # us per step


def _launches(step):
    """device kernels of one step from the kineto trace; None (= not measured) where the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile
    step()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            step()
            torch.cuda.synchronize()
    except Exception as e:                                   # noqa: BLE001 -- a tracer that does not start must not lose the timings
        print(f"launch count not measured: {e}", file=sys.stderr)
        return None
    n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name and "Memset" not in e.name)
    return n or None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--big", type=int, default=64 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("optimizer_step_probe needs a HIP device: a time taken anywhere else says nothing about it")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from rba_amd.solver import ClipAdamW

    forms = {}
    gen = torch.Generator().manual_seed(1)
    grads = [1e-2 * torch.randn(s, generator=gen).cuda() for s in HEAD_SHAPES]
    for name in ("k15", "foreach", "fused"):
        params = _params(HEAD_SHAPES)
        if name == "k15":
            opt = ClipAdamW([(str(i), p) for i, p in enumerate(params)], [1.0] * 10, WEIGHT_DECAYS, max_norm=0.01)
            step = lambda opt=opt: opt.step(1e-4)
        else:
            step = _torch_step(params, **{name: True})
        for p, g in zip(params, grads):
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)
        forms[name] = (step, params)
    result = {"elements": sum(p.numel() for p in forms["k15"][1]), "steps_per_round": args.steps, "rounds": args.rounds, "forms": {}}
    for name, (step, _) in forms.items():
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    times = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, (step, _) in forms.items():
            times[name].append(_timed(step, args.steps))
    for name, (step, _) in forms.items():
        t = times[name]
        result["forms"][name] = {"us_per_step_median": round(statistics.median(t), 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2),
                                 "device_launches_per_step": _launches(step)}
    # (clip_grad_norm_ scales .grad in place, so the torch forms' gradients shrink round by round while K15's stay: the work per step is the same)

    n = int(args.big)
    p = torch.randn(n, generator=torch.Generator().manual_seed(2)).cuda().requires_grad_(True)
    big = ClipAdamW([("big", p)], [1.0], [0.05], max_norm=0.01)
    p.grad.normal_(0.0, 1e-3)
    for _ in range(5):
        big.step(1e-4)
    torch.cuda.synchronize()
    t = [_timed(lambda: big.step(1e-4), 20) for _ in range(args.rounds)]
    us = statistics.median(t)
    result["streaming"] = {"elements": n, "chunk": big.plan.chunk, "partials": big.plan.n_partials, "us_per_step_median": round(us, 1), "us_min": round(min(t), 1),
                           "us_max": round(max(t), 1), "bytes_per_step": 28 * n, "achieved_TB_per_s": round(28 * n / us * 1e-6, 3),
                           "share_of_8TB_per_s": round(28 * n / us * 1e6 / PEAK_BYTES_PER_S, 3),
                           # with K15a's own read of the gradient counted too (4 + 16 + 12 B per element)
                           "share_of_8TB_per_s_at_32B": round(32 * n / us * 1e6 / PEAK_BYTES_PER_S, 3)}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
