"""Instance-inference timing probe (docs/kernels/K17.md, docs/measurements.md).

    python tools/instance_probe.py [--calls 15] [--warmup 3] [--arch swin_b_1dl] [--no-forward] [--out FILE]

Runs on an MI355X only.  The docs/measurements.md protocol: one pair of HIP events per call, --warmup calls, then --calls timed ones, median and minimum.
At 1024 x 2048 and 800 x 1216 with Q = 100 queries, K = 19 classes and topk = 100 (panoptic_probe's synthetic logits: 40 queries with a class of their
own, the rest of the top-k from the others):

  1. `MaskFormer.instance_inference` on the materialised [Q,H,W] logits, `instance_ops.instance_segments` on the quarter-resolution logits (the up4 forms,
     what forward() runs), and the yardstick: the reference's lines maskformer_model.py:488-527 typed as torch ops on the device, from the same
     materialised logits and -- as forward() would have to run them -- with F.interpolate (:294-299) in front.
  2. `forward` of --arch with instance_on, and the semantic-only forward (this part runs on a tree from before K17 too: it is skipped there
     with a note, the semantic-only line still comes out).
  3. the kernels alone: K17a in both forms beside K16a's up4 form on the same 40 kept planes, K17b in both element types and forms with the
     fraction of 8 TB/s its written bytes reach.
Every line is JSON."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from tools.panoptic_probe import K, KEPT, Q, SHAPES, build_model, scenario  # noqa: E402

TOPK = 100
HBM_BYTES_PER_S = 8.0e12


def stats(v):
    v = np.asarray(v)
    return {"median": round(float(np.median(v)), 3), "min": round(float(v.min()), 3)}


def timed(fn, calls, warmup, scale=1.0):
    """one event pair per call -> {"median", "min"} in ms * scale"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return stats([a.elapsed_time(b) * scale for a, b in ev])


def reference_lines(mask_cls, mask_pred, topk):
    """maskformer_model.py:488-527 as the reference types them (panoptic_on off)"""
    num_classes, num_queries = mask_cls.shape[1] - 1, mask_cls.shape[0]
    scores = F.softmax(mask_cls, dim=-1)[:, :-1]
    labels = torch.arange(num_classes, device=mask_cls.device).unsqueeze(0).repeat(num_queries, 1).flatten(0, 1)
    scores_per_image, topk_indices = scores.flatten(0, 1).topk(topk, sorted=False)
    labels_per_image = labels[topk_indices]
    topk_indices = topk_indices // num_classes
    mask_pred = mask_pred[topk_indices]
    pred_masks = (mask_pred > 0).float()
    mask_scores_per_image = (mask_pred.sigmoid().flatten(1) * pred_masks.flatten(1)).sum(1) / (pred_masks.flatten(1).sum(1) + 1e-6)
    return pred_masks, labels_per_image, scores_per_image * mask_scores_per_image


def part1(args, emit):
    from rba_amd import instance_ops as iops
    dev = torch.device("cuda")
    model = build_model("tiny1", dev)                                     # instance_inference uses the model's top-k and flags only
    model.test_topk_per_image = TOPK
    for H, W in SHAPES:
        mask_cls, low = scenario(H, W, lowres=True)
        mask_cls, low = mask_cls.to(dev), low.to(dev).contiguous()
        full = F.interpolate(low[None], size=(H, W), mode="bilinear", align_corners=False)[0].contiguous()
        planes = int(torch.unique(torch.topk(F.softmax(mask_cls, -1)[:, :-1].flatten(), TOPK).indices // K).numel())
        common = {"H": H, "W": W, "Q": Q, "topk": TOPK, "planes_in_topk": planes}
        r = model.instance_inference(mask_cls, full)
        emit({"what": "instance_inference (materialised logits)", **common, "checksum": float(r.scores.sum()),
              "ms": timed(lambda: model.instance_inference(mask_cls, full), args.calls, args.warmup)})
        out = iops.instance_segments(mask_cls, low, TOPK, K, crop=(H, W))
        emit({"what": "instance_segments (quarter-resolution logits, up4 forms)", **common, "checksum": float(out[2].sum()),
              "ms": timed(lambda: iops.instance_segments(mask_cls, low, TOPK, K, crop=(H, W)), args.calls, args.warmup)})
        emit({"what": "instance_segments (up4 forms, uint8 planes)", **common,
              "ms": timed(lambda: iops.instance_segments(mask_cls, low, TOPK, K, crop=(H, W), mask_dtype=torch.uint8), args.calls, args.warmup)})
        ref = reference_lines(mask_cls, full, TOPK)
        emit({"what": "reference lines :488-527 as torch ops (materialised logits)", **common, "checksum": float(ref[2].sum()),
              "ms": timed(lambda: reference_lines(mask_cls, full, TOPK), args.calls, args.warmup)})
        del ref, full, out, r
        torch.cuda.empty_cache()
        emit({"what": "reference lines :294-299 + :488-527 as torch ops (quarter-resolution logits)", **common,
              "ms": timed(lambda: reference_lines(mask_cls, F.interpolate(low[None], size=(H, W), mode="bilinear", align_corners=False)[0], TOPK),
                          args.calls, args.warmup)})
        torch.cuda.empty_cache()


def part2(args, emit):
    dev = torch.device("cuda")
    model = build_model(args.arch, dev)
    with torch.no_grad():
        model.sem_seg_head.predictor.class_embed.bias[:model.arch["num_classes"]] += 6.0   # seeded weights predict void everywhere
    for H, W in SHAPES:
        g = torch.Generator().manual_seed(H)
        image = torch.randint(0, 256, (3, H, W), generator=g, dtype=torch.uint8).to(dev)
        emit({"what": "forward(semantic only)", "arch": args.arch, "H": H, "W": W, "ms": timed(lambda: model([{"image": image}]), args.calls, args.warmup)})
        if not hasattr(model, "instance_on"):
            emit({"what": "forward(instance_on)", "skipped": "this tree has no instance inference"})
            continue
        model.instance_on = True
        n = len(model([{"image": image}])[0]["instances"])
        emit({"what": "forward(instance_on)", "arch": args.arch, "H": H, "W": W, "detections": n,
              "ms": timed(lambda: model([{"image": image}]), args.calls, args.warmup)})
        model.instance_on = False


def part3(args, emit):
    from rba_amd import instance_ops as iops, ops, panoptic_ops as pops
    dev = torch.device("cuda")
    for H, W in SHAPES:
        mask_cls, low = scenario(H, W, lowres=True)
        low = low.to(dev).contiguous()
        score, labels = torch.softmax(mask_cls, -1).max(-1)
        keep = (labels.ne(K) & (score > 0.5))
        kept = int(keep.sum())
        k, s = keep.to(torch.uint8).to(dev), score.to(dev)
        full = ops.resample_bilinear(low, (H, W))
        h, w = H // 4, W // 4
        floor_us = kept * H * W * 4 / HBM_BYTES_PER_S * 1e6
        count, ssum, box = iops.instance_stats(full, k)
        t = timed(lambda: ops._launch("rba_instance_stats_f32", full.data_ptr(), k.data_ptr(), count.data_ptr(), ssum.data_ptr(), box.data_ptr(), Q, H, W),
                  args.calls, args.warmup, 1e3)
        emit({"what": "K17a full resolution", "H": H, "W": W, "kept": kept, "us": t, "hbm_floor_us": round(floor_us, 2),
              "fraction_of_8TBps": round(floor_us / t["median"], 3)})
        t = timed(lambda: ops._launch("rba_instance_stats_up4_f32", low.data_ptr(), k.data_ptr(), count.data_ptr(), ssum.data_ptr(), box.data_ptr(), Q, h, w,
                                      H, W), args.calls, args.warmup, 1e3)
        emit({"what": "K17a up4", "H": H, "W": W, "kept": kept, "us": t})
        winner, counts = pops.panoptic_merge_up4(low, s, k, (H, W), kept=kept)
        t = timed(lambda: ops._launch("rba_panoptic_merge_up4_f32", low.data_ptr(), s.data_ptr(), k.data_ptr(), winner.data_ptr(), counts.data_ptr(), Q, h, w,
                                      H, W), args.calls, args.warmup, 1e3)
        emit({"what": "K16a up4 (the same kept planes)", "H": H, "W": W, "kept": kept, "us": t})
        qidx = (torch.arange(TOPK, dtype=torch.int32, device=dev) * 7) % Q
        for dtype, suffix in ((torch.float32, "f32"), (torch.uint8, "u8")):
            out = torch.empty((TOPK, H, W), dtype=dtype, device=dev)
            written = out.numel() * out.element_size()
            for name, call in ((f"K17b {suffix}", lambda: ops._launch("rba_instance_masks_" + suffix, full.data_ptr(), qidx.data_ptr(), out.data_ptr(), Q,
                                                                       TOPK, H * W)),
                               (f"K17b up4 {suffix}", lambda: ops._launch("rba_instance_masks_up4_" + suffix, low.data_ptr(), qidx.data_ptr(), out.data_ptr(),
                                                                           Q, TOPK, h, w, H, W))):
                t = timed(call, args.calls, args.warmup, 1e3)
                emit({"what": name, "H": H, "W": W, "N": TOPK, "us": t, "bytes_written": written,
                      "fraction_of_8TBps_on_bytes_written": round(written / HBM_BYTES_PER_S * 1e6 / t["median"], 3)})
            del out
        del full
        torch.cuda.empty_cache()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--calls", type=int, default=15)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--arch", default="swin_b_1dl")
    p.add_argument("--no-forward", action="store_true")
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("instance_probe needs a HIP device: timings are taken on the GPU only")
    lines = []

    def emit(d):
        lines.append(d)
        print(json.dumps(d), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.writelines(json.dumps(ln) + "\n" for ln in lines)
    if not args.no_forward:
        part2(args, emit)
    try:
        import rba_amd.instance_ops  # noqa: F401
    except ImportError:
        emit({"what": "instance inference", "skipped": "this tree has no rba_amd.instance_ops"})
        return
    part1(args, emit)
    part3(args, emit)


if __name__ == "__main__":
    main()
