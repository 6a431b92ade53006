"""Panoptic-inference timing probe (docs/kernels/K16.md, docs/measurements.md).

    python tools/panoptic_probe.py [--calls 20] [--warmup 3] [--launches 200] [--arch swin_b_1dl] [--no-forward] [--out FILE]

Runs on an MI355X only.  Part 1 uses nothing but `MaskFormer.panoptic_inference` and `MaskFormer.forward` with TEST.PANOPTIC_ON, so the same file runs
on a tree from before K16: `panoptic_inference` (closed-set and open-set) on synthetic logits with Q = 100 queries of which 40 are kept, at 1024 x 2048 and
800 x 1216, and `forward` of --arch on a uint8 image of each size.  A call ends in host read-backs, so each call is timed by a pair of HIP events AND the
host clock around it, after a synchronise; --warmup calls, then --calls timed ones, median and minimum.  Part 2 (only where rba_amd.panoptic_ops exists):
the kernels alone, each launch bracketed by its own pair of events, 20 warm-up launches, --launches (>= 200) timed: K16a in both forms with the time
HBM needs for the planes it reads (kept queries x H x W x 4 B at 8 TB/s; K1 reaches 0.65 of that rate), K16b, and K16c against the host np.unique on the
same maps.  Every line is JSON."""
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

SHAPES = [(1024, 2048), (800, 1216)]
Q, KEPT, K = 100, 40, 19
HBM_BYTES_PER_S = 8.0e12


def scenario(H, W, lowres=False):
    """mask_cls [Q,K+1], mask_pred [Q,H,W] (or the quarter-resolution [Q,H/4,W/4]): 40 kept queries as an 5 x 8 grid of overlapping cells"""
    g = torch.Generator().manual_seed(H + W)
    mask_cls = torch.randn(Q, K + 1, generator=g)
    mask_cls[:, K] -= 2.0
    for q in range(KEPT):
        mask_cls[q, (3 * q) % K] += 6.0 + 0.45 * (q % 9) + 0.04 * q
    mask_cls[KEPT:, K] += 9.0
    h, w = (H // 4, W // 4) if lowres else (H, W)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    mask_pred = torch.empty(Q, h, w)
    ch, cw = h // 5, w // 8
    for q in range(Q):
        mask_pred[q] = -6.0 - 0.02 * q
        if q < KEPT:
            cy, cx = divmod(q, 8)
            mask_pred[q][(yy >= cy * ch) & (yy < (cy + 1) * ch) & (xx >= cx * cw) & (xx < (cx + 1) * cw + cw // 3)] = 6.0 - 0.1 * q
    mask_pred += 0.05 * torch.randn(Q, h, w, generator=g)
    return mask_cls, mask_pred


def stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3), "p90": round(float(np.percentile(v, 90)), 3)}


def timed_calls(fn, calls, warmup):
    """calls that synchronise themselves: device span (events) and host wall time per call, in ms"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    dev_ms, host_ms = [], []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        host_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(a.elapsed_time(b))
    return {"events_ms": stats(dev_ms), "host_ms": stats(host_ms)}


def timed_launches(fn, launches, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) * 1e3 for a, b in ev])


def build_model(arch, dev):
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS[arch])
    return load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).to(dev).eval()


def part1(args, emit):
    dev = torch.device("cuda")
    model = build_model("tiny1", dev)                                     # panoptic_inference uses the model's thresholds and thing classes only
    model.object_mask_threshold, model.overlap_threshold = 0.5, 0.6
    for H, W in SHAPES:
        mask_cls, mask_pred = scenario(H, W)
        mask_cls, mask_pred = mask_cls.to(dev), mask_pred.to(dev)
        for open_p in (False, True):
            out = model.panoptic_inference(mask_cls, mask_pred, open_p, -0.3, 300)
            t = timed_calls(lambda: model.panoptic_inference(mask_cls, mask_pred, open_p, -0.3, 300), args.calls, args.warmup)
            emit({"what": "panoptic_inference", "H": H, "W": W, "Q": Q, "kept": KEPT, "open_set": open_p, "segments": len(out[1]),
                  "checksum": int(out[0].long().sum()), **t})
        del mask_pred
        torch.cuda.empty_cache()
    if args.no_forward:
        return
    model = build_model(args.arch, dev)
    model.panoptic_on, model.open_panoptic = True, True
    K_ = model.arch["num_classes"]
    with torch.no_grad():
        model.sem_seg_head.predictor.class_embed.bias[:K_] += 6.0          # seeded weights predict void everywhere: let queries prefer classes
    for H, W in SHAPES:
        g = torch.Generator().manual_seed(H)
        image = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
        r = model([{"image": image}])[0]["panoptic_seg"]
        t = timed_calls(lambda: model([{"image": image}]), args.calls, args.warmup)
        emit({"what": "forward(panoptic_on, open_panoptic)", "arch": args.arch, "H": H, "W": W, "segments": len(r[1]), "checksum": int(r[0].long().sum()), **t})
        model.panoptic_on = False
        t0 = timed_calls(lambda: model([{"image": image}]), args.calls, args.warmup)
        model.panoptic_on = True
        emit({"what": "forward(semantic only)", "arch": args.arch, "H": H, "W": W, **t0})


def part2(args, emit):
    try:
        from rba_amd import ops, panoptic_ops as pops
    except ImportError:
        emit({"what": "kernels", "skipped": "this tree has no rba_amd.panoptic_ops"})
        return
    dev = torch.device("cuda")
    for H, W in SHAPES:
        mask_cls, mask_pred = scenario(H, W)
        prob = torch.softmax(mask_cls, -1)
        score, labels = prob.max(-1)
        keep = (labels.ne(K) & (score > 0.5))
        kept = int(keep.sum())
        m, s, k = mask_pred.to(dev), score.to(dev), keep.to(torch.uint8).to(dev)
        winner, counts = pops.panoptic_merge(m, s, k, kept=kept)
        floor_us = kept * H * W * 4 / HBM_BYTES_PER_S * 1e6
        t = timed_launches(lambda: ops._launch("rba_panoptic_merge_f32", m.data_ptr(), s.data_ptr(), k.data_ptr(), winner.data_ptr(), counts.data_ptr(), Q, H * W),
                           args.launches)
        emit({"what": "K16a full resolution", "H": H, "W": W, "Q": Q, "kept": kept, "us": t, "bytes_read": kept * H * W * 4, "hbm_floor_us": round(floor_us, 2),
              "fraction_of_8TBps": round(floor_us / t["median"], 3)})
        low = torch.nn.functional.interpolate(mask_pred[None], size=(H // 4, W // 4), mode="bilinear", align_corners=False)[0].contiguous().to(dev)
        w4, c4 = pops.panoptic_merge_up4(low, s, k, (H, W), kept=kept)
        t = timed_launches(lambda: ops._launch("rba_panoptic_merge_up4_f32", low.data_ptr(), s.data_ptr(), k.data_ptr(), w4.data_ptr(), c4.data_ptr(), Q,
                                               H // 4, W // 4, H, W), args.launches)
        emit({"what": "K16a up4", "H": H, "W": W, "Q": Q, "kept": kept, "us": t, "bytes_read": kept * (H // 4) * (W // 4) * 4,
              "virtual_plane_hbm_floor_us": round(floor_us, 2), "fraction_of_8TBps_on_the_virtual_planes": round(floor_us / t["median"], 3)})
        table = torch.arange(Q, dtype=torch.int32, device=dev)
        pan = pops.panoptic_assign(winner, table)
        t = timed_launches(lambda: ops._launch("rba_panoptic_assign_i32", winner.data_ptr(), table.data_ptr(), pan.data_ptr(), Q, H * W), args.launches)
        emit({"what": "K16b", "H": H, "W": W, "us": t})
        # K16c: a ground truth of 40 segments with sparse ids against the merge's own map
        G, P = 41, Q + 1
        pred_h = pan.cpu().numpy()
        gt_sparse = (np.roll(pred_h, (7, 13), (0, 1)).astype(np.int64) * 70001) % 16000000
        t0 = time.perf_counter()
        for _ in range(3):
            np.unique(gt_sparse.astype(np.uint64) * np.uint64(256 ** 3) + pred_h.astype(np.uint64), return_counts=True)
        host_unique_ms = (time.perf_counter() - t0) / 3 * 1e3
        t0 = time.perf_counter()
        ids, dense = np.unique(gt_sparse.reshape(-1), return_inverse=True)
        densify_ms = (time.perf_counter() - t0) * 1e3
        G = len(ids) + 1
        gt_d = torch.from_numpy(dense.astype(np.int32)).to(dev)
        buf = torch.zeros(G * P + 1, dtype=torch.int64, device=dev)
        pred_d = pan.reshape(-1)
        t = timed_launches(lambda: ops._launch("rba_segment_pairs_accum", gt_d.data_ptr(), pred_d.data_ptr(), H * W, G, P, buf.data_ptr(),
                                               buf[G * P:].data_ptr()), args.launches)
        emit({"what": "K16c", "H": H, "W": W, "G": G, "P": P, "us": t, "host_np_unique_pairs_ms": round(host_unique_ms, 2),
              "host_np_unique_densify_gt_ms": round(densify_ms, 2)})
        del m, low
        torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--launches", type=int, default=200)
    p.add_argument("--arch", default="swin_b_1dl")
    p.add_argument("--no-forward", action="store_true")
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = p.parse_args(argv)
    if args.launches < 200:
        raise SystemExit("--launches must be at least 200")
    if not torch.cuda.is_available():
        raise SystemExit("panoptic_probe needs a HIP device: timings are taken on the GPU only")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(ln) + "\n" for ln in lines)
    part1(args, emit)
    part2(args, emit)


if __name__ == "__main__":
    main()
