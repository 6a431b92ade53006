"""Bootstrap timing probe (docs/kernels/K18.md, docs/measurements.md § K18).

    python tools/bootstrap_probe.py [--pixels 200000000] [--images 1000] [--trials 64] [--ratio 0.5] [--calls 5] [--warmup 2]
                                    [--no-kernel] [--no-yardstick] [--no-tiny] [--arch swin_b_1dl] [--full-images 6] [--out FILE]

Runs on an MI355X only.  Every line is JSON.

  1. the kernels alone, on a synthetic pooled set of --pixels labelled pixels from --images images (3 % positives, fp32 scores, sorted once):
     bootstrap_ops.subset_curves per chunk size (one HIP event pair per call, --warmup calls, --calls timed: median and minimum), the sort beside it, and the
     yardstick: the torch composition on the device -- per trial, the compaction of the sorted arrays by the trial's membership plus metrics.ood_metrics on
     the compacted pair -- run once over all trials (host clock around a synchronise), with the largest difference between the two sets of metrics.
  2. OODEvaluator.evaluate_ood_bootstrapped on the same images and draws, the re-scoring loop (one_pass=False: what the parent commit runs) against
     one_pass=True: the tiny model on 16 images of 256 x 512, and --arch on --full-images images of 1024 x 2048 (seeded weights, synthetic images and
     labels; host clock around a synchronise, one run each after one warm-up run of one trial)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3)}


def timed(fn, calls, warmup):
    """one event pair per call -> {"median", "min"} in ms"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) for a, b in ev])


def emit(out, **row):
    line = json.dumps(row)
    print(line, flush=True)
    if out is not None:
        out.write(line + "\n")
        out.flush()


def synthetic_pool(pixels, images, seed=0):
    """-> (score fp32 [n], tag int32 [n]) on the device, unsorted"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    label = (torch.rand(pixels, device="cuda", generator=g) < 0.03).to(torch.int32)
    score = torch.randn(pixels, device="cuda", generator=g) + 1.5 * label
    image = torch.randint(0, images, (pixels,), device="cuda", generator=g, dtype=torch.int32)
    return score, (image << 1) | label


def kernel_part(args, out):
    from rba_amd import bootstrap_ops as B
    from rba_amd import metrics
    from rba_amd.evaluate_ood import bootstrap_members
    score, tag = synthetic_pool(args.pixels, args.images)
    members = bootstrap_members(args.images, args.trials, args.ratio, 0)
    words = B.member_words(members[:64], "cuda")
    T = min(args.trials, 64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s, order = torch.sort(score, descending=True)
    t = tag[order].contiguous()
    del order
    torch.cuda.synchronize()
    emit(out, part="sort", pixels=args.pixels, ms=round((time.perf_counter() - t0) * 1e3, 1), note="first call: includes the sort's workspace allocation")
    for chunk in (1024, 2048, 4096, 8192, 16384):
        r = timed(lambda: B.subset_curves(s, t, words, T, chunk=chunk), args.calls, args.warmup)
        emit(out, part="subset_curves", pixels=args.pixels, images=args.images, trials=T, chunk=chunk, ms=r,
             bytes_per_pixel_read=2 * 8, gb_per_s=round(2 * 8 * args.pixels / (r["median"] * 1e-3) / 1e9, 1))
    if args.no_yardstick:
        return
    got = {k: v.cpu().numpy() for k, v in B.subset_curves(s, t, words, T).items()}
    # the yardstick: 64 compactions and 64 curve builds as torch ops
    member_dev = torch.from_numpy(members[:64]).cuda()
    image = (t >> 1).to(torch.int64)
    label = (t & 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = []
    for k in range(T):
        keep = member_dev[k][image]
        want.append(metrics.ood_metrics(s[keep], label[keep]))
    torch.cuda.synchronize()
    torch_ms = (time.perf_counter() - t0) * 1e3
    k18 = timed(lambda: B.subset_curves(s, t, words, T), args.calls, args.warmup)
    with np.errstate(divide="ignore", invalid="ignore"):
        P, N = got["P"].astype(np.float64), got["N"].astype(np.float64)
        mine = {"auroc": got["auroc2"].astype(np.float64) / (2.0 * P * N), "aupr": got["ap"] / P, "fpr95": got["fp95"] / N}
    diff = {m: float(np.max(np.abs(mine[m] - np.array([w[m] for w in want])))) for m in mine}
    emit(out, part="k18_vs_torch_composition", pixels=args.pixels, trials=T, k18_ms=k18, default_chunk=B.default_chunk(args.pixels), torch_composition_ms=round(torch_ms, 1),
         ratio=round(torch_ms / k18["median"], 1), max_abs_difference=diff, note="torch composition: one run over all trials, host clock")


class _Synthetic(torch.utils.data.Dataset):
    def __init__(self, n, h, w, seed=0):
        rng = np.random.RandomState(seed)
        self.items = []
        for _ in range(n):
            lab = np.full((h, w), 255, dtype=np.int64)
            inner = (rng.rand(h - 16, w - 16) < 0.05).astype(np.int64)
            inner[0, 0] = 1
            lab[8:-8, 8:-8] = inner
            self.items.append((torch.from_numpy(rng.randint(0, 256, (3, h, w), dtype=np.uint8)), torch.from_numpy(lab)))

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def evaluator_part(args, out, arch_name, n_images, h, w):
    from rba_amd import arch as A
    from rba_amd import evaluate_ood as E
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    from rba_amd.support import OODEvaluator
    a = A.complete(A.ARCHS[arch_name])
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).to("cuda:0").eval()
    ev = OODEvaluator(model, E.get_logits, E.get_RbA)
    data = _Synthetic(n_images, h, w)
    res = {}
    for one_pass in (False, True):
        np.random.seed(0)
        ev.evaluate_ood_bootstrapped(data, ratio=args.ratio, trials=1, device=torch.device("cuda"), num_workers=0, one_pass=one_pass)      # warm-up
        np.random.seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res[one_pass] = ev.evaluate_ood_bootstrapped(data, ratio=args.ratio, trials=args.trials, device=torch.device("cuda"), num_workers=0, one_pass=one_pass)
        torch.cuda.synchronize()
        res[one_pass] = (res[one_pass], time.perf_counter() - t0)
    (loop, loop_s), (one, one_s) = res[False], res[True]
    diff = max(abs(a_[k] - b_[k]) for a_, b_ in zip(loop, one) for k in a_)
    emit(out, part="evaluate_ood_bootstrapped", arch=arch_name, images=n_images, shape=[h, w], trials=args.trials, ratio=args.ratio,
         rescoring_loop_s=round(loop_s, 3), one_pass_s=round(one_s, 3), speedup=round(loop_s / one_s, 1), max_abs_difference_percent=diff,
         means_percent={k: round(v, 4) for k, v in one[0].items()})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--pixels", type=int, default=200_000_000)
    p.add_argument("--images", type=int, default=1000)
    p.add_argument("--trials", type=int, default=64)
    p.add_argument("--ratio", type=float, default=0.5)
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--no-kernel", action="store_true")
    p.add_argument("--no-tiny", action="store_true")
    p.add_argument("--no-yardstick", action="store_true", help="the kernels alone without the torch composition (for a kernel trace)")
    p.add_argument("--arch", default="swin_b_1dl", help="'' skips the full-size model")
    p.add_argument("--full-images", type=int, default=6)
    p.add_argument("--out", default=None)
    args = p.parse_args()
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    out = open(args.out, "w") if args.out else None
    emit(out, part="device", name=torch.cuda.get_device_name(0), torch=torch.__version__)
    if not args.no_kernel:
        kernel_part(args, out)
        torch.cuda.empty_cache()
    if not args.no_tiny:
        evaluator_part(args, out, "tiny1", 16, 256, 512)
    if args.arch:
        evaluator_part(args, out, args.arch, args.full_images, 1024, 2048)


if __name__ == "__main__":
    main()
