#!/usr/bin/env python3
"""Time the training view of the COCO-mix mapper (K14, csrc/train_view.hip) at the recipe's shape -- a 1024 x 2048 frame, a 200 x 300 object pasted, the
short edge resized to --size (512, 1228 or 2048), a 512 x 1024 crop, every colour leg on, flipped -- beside what a user composed before it existed, on
the same GPU and the same inputs:
  device composition: the paste with torch on the uploaded frame, ops.resize_u8_pil_bilinear (K12b) of the WHOLE frame, torch crop and flip,
      F.interpolate(mode="nearest") of the labels, the colour legs in torch, the mask compares and torch.bincount;
  host composition: dataset_mappers.train_view_host (numpy, Pillow, torch on the CPU), by the wall clock.
HIP events around batches of calls queued behind a long kernel; the median of 6 rounds after 2 warm-up rounds; the sides alternate.  One process per row:
`for s in 512 1228 2048; do python tools/train_view_probe.py --size $s; done > profiles/train_view_probe.txt`"""
import argparse, os, sys, time
import numpy as np
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rba_amd import ops
from rba_amd.dataset_mappers import ColorAug, TrainViewParams, train_view_host, _HDIV, _SDIV, _SECTOR

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1228)
args = ap.parse_args()
ROUNDS, WARM = 6, 2
H, W, CH, CW, IGNORE, OOD = 1024, 2048, 512, 1024, 255, 254
busy = torch.randn(8192, 8192, device="cuda")
median = lambda v: sorted(v)[len(v) // 2]


def timed_events(fns, batch):
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


# ---------------------------------------------------------------------------------------------------------------- the colour legs in torch, on [3,h,w] RGB
SDIV, HDIV, SECTOR = (torch.from_numpy(np.asarray(t)).cuda() for t in (_SDIV, _HDIV, _SECTOR))


def t_convert(x, alpha=1.0, beta=0.0):
    return (x.float() * alpha + beta).clamp_(0, 255).to(torch.uint8)


def t_bgr2hsv(b, g, r):
    b, g, r = b.long(), g.long(), r.long()
    v = torch.maximum(torch.maximum(b, g), r)
    diff = v - torch.minimum(torch.minimum(b, g), r)
    s = (diff * SDIV[v] + 2048) >> 12
    h = torch.where(v == r, g - b, torch.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + 2048) >> 12
    return torch.where(h < 0, h + 180, h), s, v


def t_hsv2bgr(H_, S_, V_):
    s, v = S_.float() * (1.0 / 255.0), V_.float() * (1.0 / 255.0)
    hh = H_.float() * (6.0 / 180.0)
    fl = hh.floor()
    f = hh - fl
    t = torch.stack([v, v * (1 - s), v * (1 - s * f), v * (1 - s * (1 - f))])
    pick = SECTOR[fl.long()].permute(2, 0, 1)
    out = torch.gather(t, 0, pick)
    out = torch.where((S_ == 0)[None], v[None], out)
    return (out * 255.0).round_().clamp_(0, 255).to(torch.uint8)


def t_color(rgb, c):
    r, g, b = rgb[0], rgb[1], rgb[2]
    img = torch.stack([b, g, r])
    if c.brightness:
        img = t_convert(img, beta=c.beta)
    for leg in (("contrast", "saturation", "hue") if c.order else ("saturation", "hue", "contrast")):
        if not getattr(c, leg):
            continue
        if leg == "contrast":
            img = t_convert(img, alpha=c.contrast_alpha)
        else:
            h, s, v = t_bgr2hsv(img[0], img[1], img[2])
            if leg == "saturation":
                s = t_convert(s, alpha=c.saturation_alpha).long()
            else:
                h = (h + c.hue_delta) % 180
            img = t_hsv2bgr(h, s, v)
    return img.flip(0)


def composed(img, lab, p, obj, objmask):
    m = objmask == OOD
    py, px = p.paste
    bh, bw = m.shape
    frame, sem = img.clone(), lab.clone()
    frame[:, py:py + bh, px:px + bw] = torch.where(m[None], obj, frame[:, py:py + bh, px:px + bw])
    sem[py:py + bh, px:px + bw] = torch.where(m, torch.full_like(objmask, OOD), sem[py:py + bh, px:px + bw])
    view = ops.resize_u8_pil_bilinear(frame, (p.new_h, p.new_w))
    sem = F.interpolate(sem[None, None].double(), size=(p.new_h, p.new_w), mode="nearest")[0, 0]
    y0, x0, ch, cw = p.crop
    view, sem = view[:, y0:y0 + ch, x0:x0 + cw], sem[y0:y0 + ch, x0:x0 + cw].long()
    view = t_color(view, p.color)
    if p.flip:
        view, sem = view.flip(2), sem.flip(1)
    view, sem = view.contiguous(), sem.contiguous()
    outlier = torch.zeros_like(sem)
    outlier[(sem == OOD) & (sem != IGNORE)] = 1
    outlier[sem == IGNORE] = IGNORE
    return view, sem, outlier, torch.bincount(sem.reshape(-1), minlength=256).to(torch.int32)


g = torch.Generator().manual_seed(0)
img = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, generator=g)
lab = torch.randint(0, 19, (H // 16, W // 16), dtype=torch.uint8, generator=g).repeat_interleave(16, 0).repeat_interleave(16, 1).contiguous()
lab[torch.rand(H, W, generator=g) < 0.05] = IGNORE
obj = torch.randint(0, 256, (3, 200, 300), dtype=torch.uint8, generator=g)
objmask = torch.where(torch.rand(200, 300, generator=g) < 0.8, torch.tensor(OOD, dtype=torch.uint8), torch.tensor(0, dtype=torch.uint8))
s = args.size
color = ColorAug(brightness=True, beta=-20.75, order=True, contrast=True, contrast_alpha=1.3127, saturation=True, saturation_alpha=0.6113, hue=True, hue_delta=-11)
p = TrainViewParams(new_h=s, new_w=2 * s, crop=((s - CH) // 2, (2 * s - CW) // 2, CH, CW), flip=True, color=color, ood_index=0, paste=(400, 850))
dev = [t.cuda() for t in (img, lab, obj, objmask)]
hip = lambda: ops.train_view(dev[0], dev[1], p, dev[2], dev[3], None, IGNORE, OOD)
ref = lambda: composed(dev[0], dev[1], p, dev[2], dev[3])
a, b = hip(), ref()
same_dev = all(torch.equal(x, y) for x, y in zip(a, b))
t = timed_events({"hip": hip, "composed": ref}, batch=5)
tw = []
for i in range(WARM + 3):
    t0 = time.perf_counter()
    host = train_view_host(img, lab, p, obj, objmask, None, IGNORE, OOD)
    tw.append((time.perf_counter() - t0) * 1e6)
same_host = all(torch.equal(x.cpu(), y) for x, y in zip(a, host))
ok = t["hip"] < t["composed"]
print(f"short edge {s:4d} ({s} x {2 * s}) -> crop {CH} x {CW}: K14 {t['hip']:8.1f} us   device composition {t['composed']:9.1f} us   K14 / composition = "
      f"{t['hip'] / t['composed']:.3f}   host composition {median(tw[WARM:]) / 1e3:7.1f} ms (wall)   every element equal: device composition {same_dev}, "
      f"host composition {same_host}   condition (K14's median below the device composition's): {'holds' if ok else 'FAILS'}", flush=True)
sys.exit(0 if ok and same_host else 1)
