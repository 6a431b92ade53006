"""Shared by the test-time-augmentation tests (test_tta_cpu.py, test_tta_merge_gpu.py, test_resize_u8_gpu.py, test_tta_model_gpu.py): seeded inputs, the
numpy restatement of Pillow's Image.resize(BILINEAR), and the torch restatement of the reference's multi-view merge
(mask2former/test_time_augmentation.py:83-97 over sem_seg_postprocess, maskformer_model.py:330-332) in fp64 and in fp32 on the CPU.

The Pillow restatement is written from Pillow's src/libImaging/Resample.c (precompute_coeffs, normalize_coeffs_8bpc, ImagingResampleHorizontal_8bpc /
Vertical_8bpc) in plain loops, independently of rba_amd.ops.pil_bilinear_coeffs; test_tta_cpu.py holds both against Pillow itself.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests._rba_bwd_cases import FLOOR, bar, check, err  # noqa: F401  (the project's metric e = max|T - T64| / max|T64| and bar 4 max(b, 2^-20))

# ---------------------------------------------------------------------------------------------------------------- Pillow's bilinear resize
RESIZE_SHAPES = (((7, 9), (13, 20)), ((32, 64), (16, 32)), ((32, 64), (24, 48)), ((30, 61), (53, 107)), ((33, 70), (12, 25)), ((5, 5), (1, 1)),
                 ((17, 40), (17, 23)), ((40, 17), (23, 17)), ((11, 14), (11, 14)))
PRECISION_BITS = 32 - 8 - 2


def pil_axis_table(n_in, n_out):
    """-> (ksize, [(xmin, [kk_0 .. kk_{n-1}])] per output index) for one axis"""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    rows = []
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        n = min(int(c + support + 0.5), n_in) - xmin
        w = []
        ww = 0.0
        for j in range(n):
            t = abs((j + xmin - c + 0.5) * ss)
            v = 1.0 - t if t < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        rows.append((xmin, [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w]))
    return ksize, rows


def _pil_pass(img, rows):
    """img [..., n_in] uint8 -> [..., n_out]: clip(((1 << 21) + sum kk_j pixel_j) >> 22, 0, 255) along the last axis"""
    out = np.empty(img.shape[:-1] + (len(rows),), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, kk) in enumerate(rows):
        acc = np.full(img.shape[:-1], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for j, k in enumerate(kk):
            acc = acc + src[..., xmin + j] * k
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def pil_bilinear_resize(image, size):
    """uint8 [C,h,w] numpy -> [C,H,W]: columns first, then rows on the rounded uint8 intermediate; an axis whose size does not change is skipped"""
    H, W = size
    img = np.ascontiguousarray(image)
    if img.shape[2] != W:
        img = _pil_pass(img, pil_axis_table(img.shape[2], W)[1])
    if img.shape[1] != H:
        img = np.ascontiguousarray(_pil_pass(np.ascontiguousarray(img.transpose(0, 2, 1)), pil_axis_table(img.shape[1], H)[1]).transpose(0, 2, 1))
    return img


@functools.lru_cache(maxsize=None)
def resize_case(i):
    """(image uint8 [3,h,w], expected [3,H,W]) of RESIZE_SHAPES[i], seeded; the extremes 0 and 255 are planted so that the clip is exercised"""
    (h, w), (H, W) = RESIZE_SHAPES[i]
    rng = np.random.default_rng(500 + i)
    img = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    img[0, : max(1, h // 3)] = 255
    img[1, :, : max(1, w // 3)] = 0
    return img, pil_bilinear_resize(img, (H, W))


# ---------------------------------------------------------------------------------------------------------------- the multi-view merge
RECIPE = tuple((h, w, f) for h, w in ((8, 16), (12, 24), (16, 32), (20, 40), (24, 48), (28, 56)) for f in (0, 1))
# name -> (K, (H, W), ((h_a, w_a, flip_a), ...))
MERGE_CASES = {
    "identity_flip_ragged": (3, (5, 7), ((5, 7, 0), (5, 7, 1))),
    "recipe": (19, (16, 32), RECIPE),
    "k20": (20, (9, 13), ((7, 10, 1), (13, 21, 0))),
    "k21": (21, (6, 9), ((4, 5, 0), (11, 17, 1))),
    "k32": (32, (6, 9), ((4, 5, 0), (11, 17, 1))),
    "one_pixel_view": (1, (4, 4), ((1, 1, 1),)),
    "one_pixel_out": (2, (1, 1), ((3, 5, 0),)),
    "one_column": (2, (3, 1), ((2, 1, 1),)),
    "sixteen_views": (5, (7, 10), tuple((3 + a, 4 + 2 * a, a % 3 == 1) for a in range(16))),
    "one_view": (19, (6, 9), ((9, 14, 1),)),
    # several workgroups along a row (more than 256 four-column groups) and a row width that is a multiple of four: the 16-byte stores
    "wide": (4, (3, 1040), ((2, 700, 1), (5, 1300, 0))),
}
MODES = ("rba", "energy", "neg_logit_sum")


@functools.lru_cache(maxsize=None)
def merge_inputs(name):
    """the views of a case: fp32 class maps U[0,1) on the CPU, seeded by the case"""
    K, _, views = MERGE_CASES[name]
    gen = torch.Generator().manual_seed(9000 + sorted(MERGE_CASES).index(name))
    return tuple(torch.rand(K, h, w, generator=gen) for h, w, _ in views)


def ref_merge(views, flips, size):
    """test_time_augmentation.py:83-97: per view sem_seg_postprocess = F.interpolate(size, bilinear, align_corners=False), .flip(dims=[2]) for a flipped
    view, the first view's result and then `+=` in order, `/ count`"""
    total = None
    for v, f in zip(views, flips):
        r = F.interpolate(v[None], size=size, mode="bilinear", align_corners=False)[0]
        if f:
            r = r.flip(dims=[2])
        if total is None:
            total = r.clone()
        else:
            total += r
    return total / len(views)


def ref_score(sem, mode):
    if mode == "rba":
        return -sem.tanh().sum(dim=0)
    if mode == "energy":
        return -torch.logsumexp(sem, dim=0)
    assert mode == "neg_logit_sum"
    return -sem.sum(dim=0)


@functools.lru_cache(maxsize=None)
def merge_truth(name):
    """{"sem64", "b_sem", "score64": {mode}, "b_score": {mode}, "argmax64", "decided": pixels whose fp64 top-two gap exceeds 8 2^-20 max|sem64|}.
    The fixture's own conditions are asserted here: the undecided pixels are at most 1 % of the map (for U[0,1) maps their expected share is of the
    order of 1e-4), and the fp32 CPU restatement has no argmax flip on a decided pixel."""
    K, size, spec = MERGE_CASES[name]
    views, flips = merge_inputs(name), [bool(f) for _, _, f in spec]
    sem64 = ref_merge([v.double() for v in views], flips, size)
    sem32 = ref_merge(list(views), flips, size)
    t = {"sem64": sem64, "b_sem": err(sem32, sem64), "score64": {}, "b_score": {}}
    for mode in MODES:
        t["score64"][mode] = ref_score(sem64, mode)
        t["b_score"][mode] = err(ref_score(sem32, mode), t["score64"][mode])
    t["argmax64"] = sem64.argmax(0)
    if K > 1:
        top2 = sem64.topk(2, dim=0).values
        t["decided"] = (top2[0] - top2[1]) > 8.0 * FLOOR * float(sem64.abs().max())
    else:
        t["decided"] = torch.ones(size, dtype=torch.bool)
    undecided = int((~t["decided"]).sum())
    assert undecided <= 0.01 * t["decided"].numel(), (name, undecided)
    assert not ((sem32.argmax(0) != t["argmax64"]) & t["decided"]).any(), name
    return t


# ---------------------------------------------------------------------------------------------------------------- the model test's image and settings
MODEL_IMAGE_HW = (48, 96)
MODEL_AUG = {"MIN_SIZES": (32, 48, 64), "MAX_SIZE": 4096, "FLIP": True}


def model_image():
    g = torch.Generator().manual_seed(4321)
    return torch.randint(0, 256, (3,) + MODEL_IMAGE_HW, generator=g, dtype=torch.uint8)


def aug_cfg(min_sizes, max_size, flip, enabled=False):
    from rba_amd.config import CfgNode
    return CfgNode(TEST=CfgNode(AUG=CfgNode(ENABLED=enabled, MIN_SIZES=list(min_sizes), MAX_SIZE=max_size, FLIP=flip)))
