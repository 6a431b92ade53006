"""K13 timing probe (docs/kernels/K13.md): ops.confusion_accumulate at 1024 x 2048, K = 19, on three maps, against the torch composition on the same tensors.

    python tools/confusion_probe.py [--launches 200] [--warmup 20] [--out FILE]

Runs on an MI355X only.  Each launch is bracketed by its own pair of HIP events on the current stream; after a warm-up, `--launches` (>= 200) timed launches,
the median and the minimum are reported.  Maps: "blocks" (block-constant, Cityscapes-like: what real use looks like), "uniform" (random pairs: no run to
merge), "single" (one (pred, gt) pair everywhere: the worst contention on one counter).  The torch composition is what the evaluator would otherwise run on
the device: bincount((K + 1) * pred.long() + gt.long() with the ignore fill, minlength=(K + 1)^2), added into the matrix.  Both results are compared
(exactly) before anything is timed.  Algorithmic traffic: 8 MiB of int32 predictions + 2 MiB of uint8 labels read, 3.2 KB of matrix updated."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

H, W, K, IGNORE = 1024, 2048, 19, 255


def maps(kind, seed=0):
    rng = np.random.default_rng(seed)
    n = H * W
    if kind == "single":
        return np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
    if kind == "uniform":
        return rng.integers(0, K, n, dtype=np.int32), rng.integers(0, K, n).astype(np.uint8)
    # blocks: 64 x 128 pixel cells of one class (rows of a cell are runs of 128 pixels), road in the lower third, 3 % ignored, 5 % of the predictions wrong
    cells = rng.integers(0, K, (H // 64, W // 128))
    cells[(H // 64) * 2 // 3:, :] = 0
    gt = np.kron(cells, np.ones((64, 128), dtype=np.int64)).astype(np.uint8)
    pred = gt.astype(np.int32)
    wrong = np.kron(rng.random((H // 8, W // 16)) < 0.05, np.ones((8, 16), dtype=bool))
    pred[wrong] = (pred[wrong] + 1) % K
    gt[np.kron(rng.random((H // 16, W // 32)) < 0.03, np.ones((16, 32), dtype=bool))] = IGNORE
    return pred.reshape(-1), gt.reshape(-1)


def torch_composition(pred, gt, conf):
    g = gt.long()
    g[g == IGNORE] = K
    conf += torch.bincount((K + 1) * pred.long() + g, minlength=(K + 1) ** 2).reshape(K + 1, K + 1)


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return {"median_us": round(float(np.median(us)), 2), "min_us": round(float(us.min()), 2), "p90_us": round(float(np.percentile(us, 90)), 2)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = p.parse_args(argv)
    if args.launches < 200:
        raise SystemExit("--launches must be at least 200")
    from rba_amd import ops
    dev = torch.device("cuda")
    lines = []
    for kind in ("blocks", "uniform", "single"):
        pred_h, gt_h = maps(kind)
        pred, gt = torch.from_numpy(pred_h).to(dev), torch.from_numpy(gt_h).to(dev)
        conf, bad = torch.zeros((K + 1, K + 1), dtype=torch.int64, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
        ref = torch.zeros_like(conf)
        ops.confusion_accumulate(pred, gt, K, conf, bad, IGNORE)
        torch_composition(pred, gt, ref)
        if not torch.equal(conf, ref) or int(bad.sum()):
            raise SystemExit(f"{kind}: K13 and the torch composition disagree")
        k13 = timed(lambda: ops.confusion_accumulate(pred, gt, K, conf, bad, IGNORE), args.launches, args.warmup)
        tc = timed(lambda: torch_composition(pred, gt, ref), args.launches, args.warmup)
        lines.append({"map": kind, "pixels": H * W, "K": K, "launches": args.launches, "k13": k13, "torch_composition": tc,
                      "speedup_median": round(tc["median_us"] / k13["median_us"], 2), "bytes_read": 5 * H * W})
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
