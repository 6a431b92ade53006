"""Shared by the K14 / COCO-mix mapper tests (test_train_view_cpu.py, test_train_view_gpu.py, test_coco_mix_mapper_gpu.py): seeded inputs and the plain
restatement of one training view, written the way the reference executes it (mask_former_semantic_coco_mix_dataset_mapper.py over Detectron2's
transforms): numpy paste on the full frame, Image.resize(BILINEAR) of the whole frame (Pillow itself where it is installed, else the loop restatement
of tests/_tta_cases.py), F.interpolate(mode="nearest") of the float64 labels, slices, the colour legs in numpy fp32, [..., ::-1], F.pad, the mask rules.
The colour legs are restated here on their own, pixel formulas written out, independently of rba_amd.dataset_mappers.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests._tta_cases import pil_bilinear_resize

IGNORE, OOD = 255, 254


# ---------------------------------------------------------------------------------------------------------------- the colour legs, restated
def convert(img, alpha=1.0, beta=0.0):
    out = img.astype(np.float32)
    out = out * np.float32(alpha)
    out = out + np.float32(beta)
    return np.clip(out, 0, 255).astype(np.uint8)


def _round_half_even(x):
    fl = np.floor(x)
    d = x - fl
    up = (d > 0.5) | ((d == 0.5) & (fl % 2 == 1))
    return (fl + up).astype(np.int64)


SDIV = [0] + [int(_round_half_even(np.float64((255 << 12) / i))) for i in range(1, 256)]
HDIV = [0] + [int(_round_half_even(np.float64((180 << 12) / (6 * i)))) for i in range(1, 256)]


def bgr2hsv(bgr):
    sdiv, hdiv = np.array(SDIV), np.array(HDIV)
    b, g, r = bgr[..., 0].astype(np.int64), bgr[..., 1].astype(np.int64), bgr[..., 2].astype(np.int64)
    v = np.max(np.stack([b, g, r]), axis=0)
    diff = v - np.min(np.stack([b, g, r]), axis=0)
    s = (diff * sdiv[v] + 2048) >> 12
    h = r - g + 4 * diff
    h[v == g] = (b - r + 2 * diff)[v == g]
    h[v == r] = (g - b)[v == r]
    h = (h * hdiv[diff] + 2048) >> 12
    h[h < 0] += 180
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


def hsv2bgr(hsv):
    f32 = np.float32
    H, S, V = (hsv[..., i] for i in range(3))
    s = S.astype(f32) * (f32(1.0) / f32(255.0))
    v = V.astype(f32) * (f32(1.0) / f32(255.0))
    hh = H.astype(f32) * (f32(6.0) / f32(180.0))
    hh[hh < 0] += f32(6.0)
    hh[hh >= 6] -= f32(6.0)
    sector = np.floor(hh)
    f = (hh - sector).astype(f32)
    sector = sector.astype(np.int64)
    t0 = v
    t1 = v * (f32(1.0) - s)
    t2 = v * (f32(1.0) - s * f)
    t3 = v * (f32(1.0) - s * (f32(1.0) - f))
    t = [t0, t1, t2, t3]
    table = [[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]]
    out = np.empty(hsv.shape, dtype=f32)
    for k in range(6):
        sel = sector == k
        for ch in range(3):
            out[..., ch][sel] = t[table[k][ch]][sel]
    gray = S == 0
    for ch in range(3):
        out[..., ch][gray] = v[gray]
    scaled = (out * f32(255.0)).astype(np.float64)                    # the fp32 product, rounded half to even and clipped
    return np.clip(_round_half_even(scaled), 0, 255).astype(np.uint8)


def color_legs(rgb, c):
    """ColorAugSSDTransform(img_format="RGB").apply_image with the draws of ``c`` (a ColorAug)"""
    img = rgb[:, :, [2, 1, 0]]
    if c.brightness:
        img = convert(img, beta=c.beta)

    def contrast(im):
        return convert(im, alpha=c.contrast_alpha) if c.contrast else im

    def saturation(im):
        if not c.saturation:
            return im
        hsv = bgr2hsv(im)
        hsv[:, :, 1] = convert(hsv[:, :, 1], alpha=c.saturation_alpha)
        return hsv2bgr(hsv)

    def hue(im):
        if not c.hue:
            return im
        hsv = bgr2hsv(im)
        hsv[:, :, 0] = (hsv[:, :, 0].astype(int) + c.hue_delta) % 180
        return hsv2bgr(hsv)

    img = hue(saturation(contrast(img))) if c.order else contrast(hue(saturation(img)))
    return img[:, :, [2, 1, 0]]


# ---------------------------------------------------------------------------------------------------------------- one training view, restated
def _pillow_resize(hwc, nh, nw):
    try:
        from PIL import Image
    except ImportError:
        return pil_bilinear_resize(np.ascontiguousarray(hwc.transpose(2, 0, 1)), (nh, nw)).transpose(1, 2, 0)
    return np.asarray(Image.fromarray(hwc).resize((nw, nh), Image.BILINEAR))


def ref_view(img, lab, params, obj=None, objmask=None, lut=None, ignore_label=IGNORE, ood_label=OOD, pad_size=None):
    """img uint8 [3,h,w], lab uint8 [h,w] (tensors) -> (image uint8 [3,ph,pw], sem_seg int64 [ph,pw], outlier_mask int64 [ch,cw], hist int32 [256])"""
    image = np.ascontiguousarray(img.numpy().transpose(1, 2, 0))
    sem = lab.numpy()
    if lut is not None:
        sem = lut.numpy()[sem]
    sem = sem.astype("double")
    if params.paste is not None:
        cut_mask, cut_image = objmask.numpy(), obj.numpy().transpose(1, 2, 0)
        py, px = params.paste
        idx = np.transpose(np.repeat(np.expand_dims(cut_mask, axis=0), 3, axis=0), (1, 2, 0))
        image = image.copy()
        image[py:py + cut_mask.shape[0], px:px + cut_mask.shape[1], :][np.where(idx == ood_label)] = cut_image[np.where(idx == ood_label)]
        sem = sem.copy()
        sem[py:py + cut_mask.shape[0], px:px + cut_mask.shape[1]][np.where(cut_mask == ood_label)] = cut_mask[np.where(cut_mask == ood_label)]
    nh, nw = params.new_h, params.new_w
    image = _pillow_resize(image, nh, nw)
    sem = F.interpolate(torch.from_numpy(sem)[None, None], size=(nh, nw), mode="nearest")[0, 0].numpy()
    y0, x0, ch, cw = params.crop
    image, sem = image[y0:y0 + ch, x0:x0 + cw], sem[y0:y0 + ch, x0:x0 + cw]
    if params.color is not None:
        image = color_legs(image, params.color)
    if params.flip:
        image, sem = image[:, ::-1], sem[:, ::-1]
    image = torch.as_tensor(np.ascontiguousarray(image.transpose(2, 0, 1)))
    sem = torch.as_tensor(sem.astype("long"))
    outlier = torch.zeros_like(sem).contiguous()
    outlier[(sem == ood_label) & (sem != ignore_label)] = 1
    outlier[sem == ignore_label] = ignore_label
    hist = torch.bincount(sem.reshape(-1), minlength=256).to(torch.int32)
    if pad_size is not None:
        padding = [0, pad_size[1] - cw, 0, pad_size[0] - ch]
        image = F.pad(image, padding, value=128).contiguous()
        sem = F.pad(sem, padding, value=ignore_label).contiguous()
    return image, sem.long(), outlier.long(), hist


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
@functools.lru_cache(maxsize=None)
def frame(h, w, seed=0, raw_ids=False):
    """(img uint8 [3,h,w], lab uint8 [h,w]): random pixels with planted 0 / 255 stripes (the clip), labels in blocks of classes 0..18 with some void
    (255); ``raw_ids``: labels 0..33, to be read through a table"""
    g = np.random.default_rng(7000 + 131 * h + w + seed)
    img = g.integers(0, 256, (3, h, w), dtype=np.uint8)
    img[0, : max(1, h // 4)] = 255
    img[1, :, : max(1, w // 5)] = 0
    coarse = g.integers(0, 34 if raw_ids else 19, ((h + 3) // 4, (w + 4) // 5), dtype=np.uint8)
    lab = np.kron(coarse, np.ones((4, 5), dtype=np.uint8))[:h, :w].copy()
    if not raw_ids:
        lab[g.random((h, w)) < 0.1] = IGNORE
    return torch.from_numpy(img), torch.from_numpy(np.ascontiguousarray(lab))


@functools.lru_cache(maxsize=None)
def ood_object(bh, bw, holes=False, seed=0):
    """(obj uint8 [3,bh,bw], objmask uint8 [bh,bw]) as CocoOodObjects hands them out: the mask's ood_label box is the whole array (its first and last
    row and column hold an ood pixel); ``holes``: a third of the inside is 0"""
    g = np.random.default_rng(7100 + 17 * bh + bw + seed)
    obj = g.integers(0, 256, (3, bh, bw), dtype=np.uint8)
    m = np.full((bh, bw), OOD, dtype=np.uint8)
    if holes:
        m[g.random((bh, bw)) < 0.33] = 0
        m[0, 0] = m[-1, -1] = OOD
    return torch.from_numpy(obj), torch.from_numpy(m)


def lattice():
    """(img uint8 [3,376,374], lab): every triple of {0,5,..,255}^3 once (52^3 = 140608 pixels, the rest zero)"""
    v = np.arange(0, 256, 5, dtype=np.uint8)
    trip = np.stack(np.meshgrid(v, v, v, indexing="ij"), axis=0).reshape(3, -1)
    flat = np.zeros((3, 376 * 374), dtype=np.uint8)
    flat[:, :trip.shape[1]] = trip
    return torch.from_numpy(flat.reshape(3, 376, 374)), torch.zeros((376, 374), dtype=torch.uint8)


def primaries():
    """(img uint8 [3,2,4]): black, white and the six primaries / secondaries"""
    cols = [(0, 0, 0), (255, 255, 255), (255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255)]
    return torch.tensor(cols, dtype=torch.uint8).T.reshape(3, 2, 4).contiguous(), torch.zeros((2, 4), dtype=torch.uint8)


def check_equal(got, want, what=""):
    names = ("image", "sem_seg", "outlier_mask", "hist")
    for n, a, b in zip(names, got, want):
        a = a.cpu()
        assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape), (what, n, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
        bad = int((a != b).sum())
        assert bad == 0, f"{what}: {n} differs in {bad} of {a.numel()} elements"


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> (source (h, w), resized (new_h, new_w), crop (y0, x0, ch, cw)).  Source (24, 48) to the short edges 12 (ksize 5), 17 (non-integer down), 24 (no
# pass on either axis), 31 (non-integer up) and 48 (the >> 1 label rule), by Detectron2's shortest-edge rule; a (12, 24) crop at offset 0, at the maximum
# and inside, and -- where the resized frame is no larger than the crop -- the crop clipped to the whole frame, as RandomCrop clips it.
GEOMETRY = {
    "e12_whole": ((24, 48), (12, 24), (0, 0, 12, 24)),
    "e17_whole": ((24, 48), (17, 34), (0, 0, 17, 34)),
    "e17_first": ((24, 48), (17, 34), (0, 0, 12, 24)),
    "e17_last": ((24, 48), (17, 34), (5, 10, 12, 24)),
    "e17_inside": ((24, 48), (17, 34), (2, 7, 12, 24)),
    "e24_first": ((24, 48), (24, 48), (0, 0, 12, 24)),
    "e24_last": ((24, 48), (24, 48), (12, 24, 12, 24)),
    "e24_inside": ((24, 48), (24, 48), (5, 11, 12, 24)),
    "e31_first": ((24, 48), (31, 62), (0, 0, 12, 24)),
    "e31_last": ((24, 48), (31, 62), (19, 38, 12, 24)),
    "e31_inside": ((24, 48), (31, 62), (7, 13, 12, 24)),
    "e48_first": ((24, 48), (48, 96), (0, 0, 12, 24)),
    "e48_last": ((24, 48), (48, 96), (36, 72, 12, 24)),
    "e48_inside": ((24, 48), (48, 96), (10, 33, 12, 24)),
    "x_only_down": ((24, 48), (24, 31), (6, 3, 12, 24)),
    "x_only_up": ((24, 48), (24, 70), (6, 41, 12, 24)),
    "y_only_down": ((24, 48), (17, 48), (2, 20, 12, 24)),
    "y_only_up": ((24, 48), (37, 48), (21, 20, 12, 24)),
    "odd_first": ((23, 47), (31, 63), (0, 0, 11, 21)),
    "odd_last": ((23, 47), (31, 63), (20, 42, 11, 21)),
    "odd_inside": ((23, 47), (31, 63), (9, 17, 11, 21)),
    "odd_down": ((23, 47), (13, 27), (1, 3, 11, 21)),
    "wide": ((6, 1100), (5, 1070), (1, 17, 3, 1040)),                 # several workgroups per row, word stores
    "tall_to_10": ((80, 48), (10, 24), (1, 2, 8, 20)),                # ksize 17: the source rows of a tile do not fit the staging buffer
    "two_row_tiles": ((40, 48), (61, 73), (3, 5, 37, 52)),            # more than one tile of rows, staged, ragged in both directions
}
# every (in, out) size pair of an axis above: the label rule is held against F.interpolate at each
SIZE_PAIRS = sorted({(s[i], n[i]) for s, n, _ in GEOMETRY.values() for i in (0, 1)})

# name -> (box (bh, bw), holes, position (py, px) in the (24, 48) source, the GEOMETRY case it is seen through); the e31_inside crop shows source
# rows ~5..15 and columns ~10..29, the e31_last crop the source's bottom-right corner
PASTES = {
    "interior": ((6, 9), False, (7, 14), "e31_inside"),
    "bottom_right": ((7, 11), False, (17, 37), "e31_last"),
    "straddle": ((10, 12), False, (1, 3), "e31_inside"),
    "holes": ((9, 13), True, (6, 12), "e31_inside"),
    "covers_crop": ((20, 40), True, (2, 4), "e17_inside"),
}


def params_of(name, flip=False, color=None, paste=None):
    from rba_amd.dataset_mappers import TrainViewParams
    _, new, crop = GEOMETRY[name]
    return TrainViewParams(new_h=new[0], new_w=new[1], crop=crop, flip=flip, color=color, ood_index=None if paste is None else 0, paste=paste)


def color_cases():
    from rba_amd.dataset_mappers import ColorAug
    c = {}
    for beta in (-32.0, 32.0, 13.37):
        c[f"brightness_{beta}"] = ColorAug(brightness=True, beta=beta)
    for alpha in (0.5, 1.5, 0.8318):
        c[f"contrast_{alpha}"] = ColorAug(contrast=True, contrast_alpha=alpha)
        c[f"saturation_{alpha}"] = ColorAug(saturation=True, saturation_alpha=alpha)
    for delta in (-18, 0, 18):
        c[f"hue_{delta}"] = ColorAug(hue=True, hue_delta=delta)
    for order in (False, True):
        c[f"all_order{int(order)}"] = ColorAug(brightness=True, beta=-20.75, order=order, contrast=True, contrast_alpha=1.3127, saturation=True,
                                               saturation_alpha=0.6113, hue=True, hue_delta=-11)
    c["none_on"] = ColorAug()
    return c
