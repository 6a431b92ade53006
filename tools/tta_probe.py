#!/usr/bin/env python3
"""Time test-time augmentation (K12, csrc/tta_merge.hip + csrc/resize_u8.hip) at the Cityscapes recipe -- MIN_SIZES 512 .. 1792, FLIP: twelve views of a
1024 x 2048 image, K = 19 -- beside what a user composed before it existed, on the same GPU and the same inputs:
 1. ops.tta_merge against the torch composition on the twelve class maps: ops.resample_bilinear per view, flip, +=, / n, -tanh().sum(0);
 2. K12b (ops.resize_u8_pil_bilinear) against Pillow on the host, for the six sizes (the host side: wall clock, and it still has its upload ahead);
 3. one image through SemanticSegmentorWithTTA.rba_scores against the same protocol on the public API without it: host Pillow views,
    MaskFormer.forward with height / width per view, torch merge (wall clock around a synchronised call: the host's resizes are inside the window).
HIP events around batches of calls queued behind a long kernel (rows 1, 2); the median of 6 rounds after 2 warm-up rounds; the sides alternate.
`python tools/tta_probe.py [--arch swin_b_1dl] [--rows 123] > profiles/tta_probe.txt`"""
import argparse, os, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import arch as A, ops
from rba_amd.config import CfgNode
from rba_amd.test_time_augmentation import DatasetMapperTTA, SemanticSegmentorWithTTA

ap = argparse.ArgumentParser()
ap.add_argument("--arch", default="swin_b_1dl")
ap.add_argument("--rows", default="123")
args = ap.parse_args()
ROUNDS, WARM = 6, 2
K, H, W = 19, 1024, 2048
SIZES = (512, 768, 1024, 1280, 1536, 1792)
cfg = CfgNode(TEST=CfgNode(AUG=CfgNode(ENABLED=True, MIN_SIZES=list(SIZES), MAX_SIZE=4096, FLIP=True)))
busy = torch.randn(8192, 8192, device="cuda")
median = lambda v: sorted(v)[len(v) // 2]
rel = lambda a, b: float((a.double() - b.double()).abs().max() / b.double().abs().max())


def timed_events(fns, batch):
    """{name: median us per call}: the candidates alternate round by round, each round = `batch` calls bracketed by events behind a long kernel"""
    ts = {k: [] for k in fns}
    for i in range(WARM + ROUNDS):
        for k, fn in fns.items():
            busy @ busy
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(batch):
                fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= WARM:
                ts[k].append(e0.elapsed_time(e1) * 1e3 / batch)
    return {k: median(v) for k, v in ts.items()}


def timed_wall(fns):
    """{name: median us per call} by the wall clock around one synchronised call; the candidates alternate"""
    ts = {k: [] for k in fns}
    for i in range(WARM + ROUNDS):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= WARM:
                ts[k].append((time.perf_counter() - t0) * 1e6)
    return {k: median(v) for k, v in ts.items()}


def torch_merge(sems, flips, size):
    total = None
    for sem, f in zip(sems, flips):
        r = ops.resample_bilinear(sem, size)
        if f:
            r = r.flip(dims=[2])
        if total is None:
            total = r
        else:
            total += r
    return total / len(sems)


ok = True
g = torch.Generator(device="cuda").manual_seed(0)
print(f"K = {K}, output {H} x {W}, views {[(s, 2 * s) for s in SIZES]} each unflipped then flipped (twelve)")
if "1" in args.rows:
    sems = [torch.rand(K, s, 2 * s, device="cuda", generator=g) for s in SIZES for _ in (0, 1)]
    flips = [bool(i % 2) for i in range(len(sems))]
    hip = lambda: ops.tta_merge(sems, flips, (H, W))[0]
    ref = lambda: -torch_merge(sems, flips, (H, W)).tanh().sum(0)
    t = timed_events({"hip": hip, "torch": ref}, batch=2)
    tf = timed_events({"hip sem": lambda: ops.tta_merge(sems, flips, (H, W), True, True)}, batch=2)
    print(f"row 1  merge of twelve class maps -> score      : ops.tta_merge {t['hip']:9.1f} us   torch composition {t['torch']:9.1f} us   "
          f"kernel / torch = {t['hip'] / t['torch']:.3f}   (with sem_seg and argmax outputs: {tf['hip sem']:.1f} us)")
    print(f"       class maps read {sum(s.numel() for s in sems) * 4 / 1e6:.0f} MB, score written {H * W * 4 / 1e6:.1f} MB; max rel difference of the scores {rel(hip(), ref()):.1e}")
    ok &= t["hip"] < t["torch"]
    del sems
if "2" in args.rows:
    from PIL import Image
    img = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device="cuda", generator=g)
    host = Image.fromarray(np.ascontiguousarray(img.cpu().numpy().transpose(1, 2, 0)))
    for s in SIZES:
        td = timed_events({"plain": lambda: ops.resize_u8_pil_bilinear(img, (s, 2 * s)), "flip": lambda: ops.resize_u8_pil_bilinear(img, (s, 2 * s), True)}, batch=5)
        tp = []
        for i in range(WARM + ROUNDS):
            t0 = time.perf_counter()
            out = host.resize((2 * s, s), Image.BILINEAR)
            tp.append((time.perf_counter() - t0) * 1e6)
        same = torch.equal(ops.resize_u8_pil_bilinear(img, (s, 2 * s)).cpu(), torch.from_numpy(np.asarray(out).transpose(2, 0, 1).copy()))
        print(f"row 2  view {s:4d} x {2 * s:4d}: K12b {td['plain']:8.1f} us (flipped {td['flip']:8.1f} us)   Pillow on the host {median(tp[WARM:]):9.1f} us   "
              f"every byte equal: {same}")
        ok &= same
if "3" in args.rows:
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS[args.arch])
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()
    image = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    wrapper = SemanticSegmentorWithTTA(cfg, model)
    host_mapper = DatasetMapperTTA(cfg)

    def composed():
        total = None
        for v in host_mapper({"image": image, "height": H, "width": W}):
            sem = model([{"image": v["image"], "height": H, "width": W}])[0]["sem_seg"]
            if any(t[0] == "hflip" for t in v["transforms"]):
                sem = sem.flip(dims=[2])
            if total is None:
                total = sem
            else:
                total += sem
        return -(total / 12).tanh().sum(0)

    t = timed_wall({"hip": lambda: wrapper.rba_scores([{"image": image}])[0], "composed": composed})
    print(f"row 3  one image, {args.arch}, twelve views -> score    : SemanticSegmentorWithTTA.rba_scores {t['hip'] / 1e3:9.1f} ms   composition on the public API "
          f"{t['composed'] / 1e3:9.1f} ms   wrapper / composition = {t['hip'] / t['composed']:.3f}")
    print(f"       max rel difference of the scores {rel(wrapper.rba_scores([{'image': image}])[0], composed()):.1e}")
    ok &= t["hip"] < t["composed"]
print(f"condition (the kernel path's median below the composition's in rows 1 and 3; K12b's bytes equal Pillow's): {'holds' if ok else 'FAILS'}")
sys.exit(0 if ok else 1)
