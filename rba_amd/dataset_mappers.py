"""The fine-tune recipes' input pipeline: INPUT.DATASET_MAPPER_NAME "mask_former_semantic_coco_mix" (reference:
mask2former/data/dataset_mappers/mask_former_semantic_coco_mix_dataset_mapper.py and coco.py, over Detectron2's ResizeShortestEdge, RandomCrop,
ColorAugSSDTransform and RandomFlip).

``MaskFormerSemanticCocoMixDatasetMapper(cfg, device=None)`` turns one dataset dict into the reference's training dict: ``image`` uint8 [3,H,W],
``sem_seg`` int64, ``outlier_mask`` int64 and ``instances`` (``gt_classes``, ``gt_masks``).  Every random decision is made on the host by
``sample_train_view_params`` in the reference's draw order and recorded in a ``TrainViewParams``; the pixels are then a pure function of the decoded
frame, the out-of-distribution object and those parameters:

  device = a HIP device: the frame and the object are uploaded once and ONE kernel (K14, ops.train_view; docs/kernels/K14.md) writes the finished view --
      paste, Pillow's resize of the crop's pixels only, nearest-neighbour labels, colour legs, flip, pad, outlier mask and the label histogram that
      gives ``gt_classes`` (one 1 KB read-back per image).
  device = None: ``train_view_host``, the same function the way the reference executes it (numpy paste, Pillow's resize of the whole frame,
      F.interpolate for the labels, slices) -- what the CPU tests hold the logic against, and what the kernel equals in every element.

The two 8-bit colour conversions of the saturation and hue legs are OpenCV's as this module restates them, and the sampler follows Detectron2's draw
order as read from its sources; neither OpenCV nor Detectron2 is a dependency, so byte parity with cv2 and draw-for-draw parity with Detectron2 are
NOT pinned by a test against them (docs/kernels/K14.md).
"""
import copy
import os
import random as _random
from dataclasses import dataclass, field
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .h2d import to_device
from .test_time_augmentation import _resize_u8_host, resize_shortest_edge_shape

__all__ = ["ColorAug", "TrainViewParams", "MapperSettings", "mapper_settings", "sample_train_view_params", "train_view_host", "CocoOodObjects",
           "extract_bbox", "Instances", "MaskFormerSemanticCocoMixDatasetMapper", "bgr_to_hsv_u8", "hsv_to_bgr_u8", "color_aug_ssd"]


# ---------------------------------------------------------------------------------------------------------------- the sampled decisions
@dataclass
class ColorAug:
    """ColorAugSSDTransform's draws: each leg on / off with its value; ``order`` set: contrast, saturation, hue -- else saturation, hue, contrast"""
    brightness: bool = False
    beta: float = 0.0
    order: bool = False
    contrast: bool = False
    contrast_alpha: float = 1.0
    saturation: bool = False
    saturation_alpha: float = 1.0
    hue: bool = False
    hue_delta: int = 0


@dataclass
class TrainViewParams:
    """Every sampled decision of one training view.  ``ood_index``: the drawn object or None; ``paste``: (py, px), the box's top-left corner in the
    source frame, or None (no object drawn, an object without an ood pixel, or a box larger than the frame); ``crop``: (y0, x0, ch, cw) in the resized
    frame; ``color``: None when colour augmentation is off."""
    new_h: int
    new_w: int
    crop: Tuple[int, int, int, int]
    flip: bool = False
    color: Optional[ColorAug] = None
    ood_index: Optional[int] = None
    paste: Optional[Tuple[int, int]] = None


@dataclass
class MapperSettings:
    min_sizes: Tuple[int, ...] = (800,)
    max_size: int = 1333
    sampling: str = "choice"
    crop_enabled: bool = False
    crop_type: str = "relative_range"
    crop_size: Tuple[float, float] = (0.9, 0.9)
    single_category_max_area: float = 1.0
    color_aug: bool = False
    image_format: str = "RGB"
    size_divisibility: int = -1
    ignore_label: int = 255
    ood_label: int = 254
    ood_prob: float = 0.2
    coco_root: str = "coco/"
    coco_proxy_size: Optional[int] = 300
    repeat_instance_masks: int = 1
    mapper_name: str = "mask_former_semantic_coco_mix"
    random_flip: str = "horizontal"
    extra: dict = field(default_factory=dict)


def mapper_settings(cfg):
    """The INPUT.* keys (and MODEL.SEM_SEG_HEAD.IGNORE_VALUE) the mapper reads -> MapperSettings; a cfg without INPUT gets config.py's defaults"""
    from .config import _DEFAULTS
    inp = copy.deepcopy(_DEFAULTS["INPUT"])
    given = cfg.get("INPUT", {}) or {}
    for k, v in given.items():
        if k == "CROP":
            inp["CROP"].update(v)
        else:
            inp[k] = v
    ms = inp["MIN_SIZE_TRAIN"]
    ms = (ms,) if isinstance(ms, (int, float)) else tuple(ms)
    if len(ms) == 1 and isinstance(ms[0], str):
        # the Cityscapes base config's python/eval tag, which config.py reads as a string: "[int(x * 0.1 * 1024) for x in range(5, 21)]".  That one
        # form is computed here; nothing is evaluated.
        import re
        m = re.fullmatch(r"\s*\[\s*int\(x \* ([0-9.]+) \* ([0-9]+)\) for x in range\(([0-9]+), ([0-9]+)\)\s*\]\s*", ms[0])
        if m is None:
            raise ValueError(f"INPUT.MIN_SIZE_TRAIN {ms[0]!r} is not a list of sizes; give the sizes as a list")
        ms = tuple(int(x * float(m.group(1)) * int(m.group(2))) for x in range(int(m.group(3)), int(m.group(4))))
    if isinstance(inp["CROP"]["SIZE"], str):                             # "(512, 1024)": a tuple literal is a string to the YAML reader
        import ast
        inp["CROP"]["SIZE"] = ast.literal_eval(inp["CROP"]["SIZE"])
    return MapperSettings(
        min_sizes=tuple(int(s) for s in ms), max_size=int(inp["MAX_SIZE_TRAIN"]), sampling=str(inp["MIN_SIZE_TRAIN_SAMPLING"]),
        crop_enabled=bool(inp["CROP"]["ENABLED"]), crop_type=str(inp["CROP"]["TYPE"]), crop_size=tuple(inp["CROP"]["SIZE"]),
        single_category_max_area=float(inp["CROP"]["SINGLE_CATEGORY_MAX_AREA"]), color_aug=bool(inp["COLOR_AUG_SSD"]), image_format=str(inp["FORMAT"]),
        size_divisibility=int(inp["SIZE_DIVISIBILITY"]),
        ignore_label=int(cfg.get("MODEL", {}).get("SEM_SEG_HEAD", {}).get("IGNORE_VALUE", 255)), ood_label=int(inp["OOD_LABEL"]),
        ood_prob=float(inp["OOD_PROB"]), coco_root=str(inp["COCO_ROOT"]),
        coco_proxy_size=None if inp["COCO_PROXY_SIZE"] is None else int(inp["COCO_PROXY_SIZE"]),
        repeat_instance_masks=int(inp["REPEAT_INSTANCE_MASKS"]), mapper_name=str(inp["DATASET_MAPPER_NAME"]), random_flip=str(inp["RANDOM_FLIP"]))


def _check_settings(s):
    """the cases this mapper does not provide raise here, before any draw"""
    if s.sampling != "choice":
        raise NotImplementedError(f"INPUT.MIN_SIZE_TRAIN_SAMPLING {s.sampling!r}: only 'choice' is provided")
    if s.crop_enabled and s.crop_type != "absolute":
        raise NotImplementedError(f"INPUT.CROP.TYPE {s.crop_type!r}: only 'absolute' is provided")
    if s.crop_enabled and s.single_category_max_area < 1.0:
        raise NotImplementedError("INPUT.CROP.SINGLE_CATEGORY_MAX_AREA < 1.0 (the category-area-constrained crop) is not provided")
    if s.color_aug and s.image_format != "RGB":
        raise NotImplementedError(f"INPUT.FORMAT {s.image_format!r}: the colour legs are provided for 'RGB' frames")
    if s.random_flip != "horizontal":
        raise NotImplementedError(f"INPUT.RANDOM_FLIP {s.random_flip!r}: only 'horizontal' is provided")
    if not 0.0 <= s.ood_prob <= 1.0:
        raise ValueError(f"OOD Probability should be between [0,1], given was {s.ood_prob}")
    if s.repeat_instance_masks < 1:
        raise ValueError(f"Number of times to repeat a mask cannot be less than one, given was {s.repeat_instance_masks}")


def _pad_size(s, ch, cw):
    """the output canvas: the crop's size, or SIZE_DIVISIBILITY x SIZE_DIVISIBILITY (the reference pads to that size, not to a multiple)"""
    d = s.size_divisibility
    if d <= 0:
        return ch, cw
    if ch > d or cw > d:
        raise NotImplementedError(f"INPUT.SIZE_DIVISIBILITY {d} with a {ch} x {cw} crop: the reference's F.pad goes negative there")
    return d, d


def sample_train_view_params(settings, h, w, ood_box_hw=None, np_rng=None, py_rng=None):
    """The reference's draws for one h x w frame, on the host, in its order -> TrainViewParams.

    ``np_rng`` (np.random or a RandomState) and ``py_rng`` (random or a random.Random): the reference draws from both global generators.
      np_rng: rand() for ood_p; with a paste randint(0, len(coco)); choice(MIN_SIZE_TRAIN); randint(new_h - ch + 1), randint(new_w - cw + 1);
              uniform(0, 1) < 0.5 for the flip.
      py_rng: with a paste that fits randint(0, h - bh), randint(0, w - bw); then ColorAugSSDTransform: randrange(2) + uniform(-32, 32) for
              brightness, randrange(2) for the order, and per leg in that order randrange(2) and its uniform(0.5, 1.5) or randint(-18, 18).
    ``ood_box_hw``: the objects' ood_label boxes -- len() of them, [i] -> (bh, bw), (0, 0) for an object without an ood pixel -- or None / empty:
    no object is ever drawn (the draw for ood_p is still made)."""
    np_rng = np.random if np_rng is None else np_rng
    py_rng = _random if py_rng is None else py_rng
    s = settings
    _check_settings(s)
    ood_index = paste = None
    ood_p = np_rng.rand()
    if ood_p < s.ood_prob and ood_box_hw is not None and len(ood_box_hw) > 0:
        ood_index = int(np_rng.randint(0, len(ood_box_hw)))
        bh, bw = (int(v) for v in ood_box_hw[ood_index])
        if bh > 0 and bw > 0 and bh <= h and bw <= w:                     # mix_object: no ood pixel -> no paste, no draw; too large -> unchanged, no draw
            py = py_rng.randint(0, h - bh)
            paste = (py, py_rng.randint(0, w - bw))
    size = int(np_rng.choice(s.min_sizes))
    new_h, new_w = resize_shortest_edge_shape(h, w, size, s.max_size)
    if s.crop_enabled:
        ch, cw = min(int(s.crop_size[0]), new_h), min(int(s.crop_size[1]), new_w)
        y0 = int(np_rng.randint(new_h - ch + 1))
        crop = (y0, int(np_rng.randint(new_w - cw + 1)), ch, cw)
    else:
        crop = (0, 0, new_h, new_w)
    _pad_size(s, crop[2], crop[3])
    color = None
    if s.color_aug:
        color = ColorAug()
        if py_rng.randrange(2):
            color.brightness, color.beta = True, py_rng.uniform(-32, 32)
        color.order = bool(py_rng.randrange(2))
        for leg in (("contrast", "saturation", "hue") if color.order else ("saturation", "hue", "contrast")):
            if py_rng.randrange(2):
                setattr(color, leg, True)
                if leg == "hue":
                    color.hue_delta = py_rng.randint(-18, 18)
                else:
                    setattr(color, leg + "_alpha", py_rng.uniform(0.5, 1.5))
    flip = bool(np_rng.uniform(0, 1) < 0.5)
    return TrainViewParams(new_h=new_h, new_w=new_w, crop=crop, flip=flip, color=color, ood_index=ood_index, paste=paste)


# ---------------------------------------------------------------------------------------------------------------- the colour legs on the host
def _convert(img, alpha=1.0, beta=0.0):
    """ColorAugSSDTransform.convert: one fp32 multiply, one fp32 add, clip, truncate"""
    v = img.astype(np.float32) * np.float32(alpha) + np.float32(beta)
    return np.clip(v, 0, 255).astype(np.uint8)


def _round_half_even_div(num, den):
    return np.rint(num / den).astype(np.int64)


_SDIV = np.zeros(256, dtype=np.int64)
_HDIV = np.zeros(256, dtype=np.int64)
_SDIV[1:] = _round_half_even_div(float(255 << 12), np.arange(1, 256, dtype=np.float64))
_HDIV[1:] = _round_half_even_div(float(180 << 12), 6.0 * np.arange(1, 256, dtype=np.float64))


def bgr_to_hsv_u8(bgr):
    """uint8 [...,3] BGR -> uint8 [...,3] HSV with H in 0..179: OpenCV's 8-bit conversion as docs/kernels/K14.md restates it"""
    b, g, r = (bgr[..., i].astype(np.int64) for i in range(3))
    v = np.maximum(np.maximum(b, g), r)
    diff = v - np.minimum(np.minimum(b, g), r)
    s = (diff * _SDIV[v] + 2048) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * _HDIV[diff] + 2048) >> 12
    h = np.where(h < 0, h + 180, h)
    return np.stack([h, s, v], axis=-1).astype(np.uint8)


_SECTOR = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def hsv_to_bgr_u8(hsv):
    """uint8 [...,3] HSV (H in 0..179) -> uint8 [...,3] BGR in fp32, every operation rounded on its own"""
    f32 = np.float32
    H, S, V = hsv[..., 0], hsv[..., 1], hsv[..., 2]
    s = S.astype(f32) * (f32(1) / f32(255))
    v = V.astype(f32) * (f32(1) / f32(255))
    hh = H.astype(f32) * (f32(6) / f32(180))
    hh = np.where(hh < 0, hh + f32(6), hh)
    hh = np.where(hh >= 6, hh - f32(6), hh).astype(f32)
    fl = np.floor(hh)
    sector = fl.astype(np.int64)
    f = hh - fl
    one = f32(1)
    t = np.stack([v, v * (one - s), v * (one - s * f), v * (one - s * (one - f))], axis=-1)
    pick = _SECTOR[sector]                                                        # [..., 3]
    bgr = np.take_along_axis(t, pick, axis=-1)
    bgr = np.where((S == 0)[..., None], v[..., None], bgr).astype(f32)
    return np.clip(np.rint(bgr * f32(255)), 0, 255).astype(np.uint8)


def color_aug_ssd(rgb, color):
    """ColorAugSSDTransform(img_format="RGB").apply_image with the draws of ``color``: uint8 [...,3] RGB -> the same"""
    img = rgb[..., ::-1]
    if color.brightness:
        img = _convert(img, beta=color.beta)
    for leg in (("contrast", "saturation", "hue") if color.order else ("saturation", "hue", "contrast")):
        if not getattr(color, leg):
            continue
        if leg == "contrast":
            img = _convert(img, alpha=color.contrast_alpha)
        else:
            hsv = bgr_to_hsv_u8(img)
            if leg == "saturation":
                hsv[..., 1] = _convert(hsv[..., 1], alpha=color.saturation_alpha)
            else:
                hsv[..., 0] = (hsv[..., 0].astype(int) + int(color.hue_delta)) % 180
            img = hsv_to_bgr_u8(hsv)
    return np.ascontiguousarray(img[..., ::-1])


# ---------------------------------------------------------------------------------------------------------------- the host composition
def _np(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def train_view_host(img, lab, params, obj=None, objmask=None, lut=None, ignore_label=255, ood_label=254, pad_size=None):
    """ops.train_view's contract on the host, executed the way the reference executes it -> the same four CPU tensors"""
    image = np.ascontiguousarray(_np(img).transpose(1, 2, 0))                    # HWC, RGB
    sem = _np(lab)
    if lut is not None:
        sem = _np(lut)[sem]
    sem = sem.astype("double")
    h, w = sem.shape
    if params.paste is not None:                                                  # mix_object behind its draws
        m = _np(objmask) == ood_label
        py, px = params.paste
        bh, bw = m.shape
        if py < 0 or px < 0 or py + bh > h or px + bw > w:
            raise ValueError(f"the {bh} x {bw} box at {(py, px)} does not lie inside the {h} x {w} frame")
        image = image.copy()
        image[py:py + bh, px:px + bw][m] = _np(obj).transpose(1, 2, 0)[m]
        sem = sem.copy()
        sem[py:py + bh, px:px + bw][m] = ood_label
    nh, nw = int(params.new_h), int(params.new_w)
    y0, x0, ch, cw = (int(v) for v in params.crop)
    if min(ch, cw) < 1 or y0 < 0 or x0 < 0 or y0 + ch > nh or x0 + cw > nw:
        raise ValueError(f"the crop {params.crop} does not lie inside the {nh} x {nw} resized frame")
    image = _resize_u8_host(np.ascontiguousarray(image.transpose(2, 0, 1)), (nh, nw)).transpose(1, 2, 0)      # ResizeTransform: Pillow for uint8 ...
    sem = F.interpolate(torch.from_numpy(np.ascontiguousarray(sem))[None, None], size=(nh, nw), mode="nearest")[0, 0].numpy()      # ... ATen for the rest
    image, sem = image[y0:y0 + ch, x0:x0 + cw], sem[y0:y0 + ch, x0:x0 + cw]
    if params.color is not None:
        image = color_aug_ssd(image, params.color)
    if params.flip:
        image, sem = image[:, ::-1], sem[:, ::-1]
    image = torch.as_tensor(np.ascontiguousarray(image.transpose(2, 0, 1)))
    sem = torch.as_tensor(np.ascontiguousarray(sem).astype("long"))
    outlier = torch.zeros_like(sem)
    outlier[(sem == ood_label) & (sem != ignore_label)] = 1
    outlier[sem == ignore_label] = ignore_label
    hist = torch.bincount(sem.reshape(-1), minlength=256).to(torch.int32)
    if pad_size is not None:
        ph, pw = int(pad_size[0]), int(pad_size[1])
        if ph < ch or pw < cw:
            raise ValueError(f"the canvas {(ph, pw)} is smaller than the {ch} x {cw} crop")
        image = F.pad(image, [0, pw - cw, 0, ph - ch], value=128).contiguous()
        sem = F.pad(sem, [0, pw - cw, 0, ph - ch], value=ignore_label).contiguous()
    return image, sem, outlier, hist


# ---------------------------------------------------------------------------------------------------------------- the COCO objects
def extract_bbox(mask):
    """(y1, x1, y2, x2) of a boolean mask, y2 / x2 exclusive; zeros for an empty mask (the reference's extract_bboxes for one instance)"""
    cols, rows = np.where(np.any(mask, axis=0))[0], np.where(np.any(mask, axis=1))[0]
    if cols.shape[0] == 0:
        return 0, 0, 0, 0
    return int(rows[0]), int(cols[0]), int(rows[-1]) + 1, int(cols[-1]) + 1


class CocoOodObjects:
    """The reference's COCO listing (data/dataset_mappers/coco.py): annotations/ood_seg_train<year>/*.png <-> train<year>/*.jpg under ``root``, shuffled
    with ``py_rng`` (random.shuffle in the reference) and cut to the first ``proxy_size`` (5000 when None).  ``[i]`` -> (RGB uint8 [bh,bw,3], mask uint8
    [bh,bw]) cropped to the ood_label bounding box on the host (the box size is needed for the position draw); an object without an ood pixel gives
    empty arrays.  ``box_hw`` is the sized view ``sample_train_view_params`` takes."""
    min_image_size = 480

    def __init__(self, root, proxy_size, split="train", year="2017", shuffle=True, py_rng=None, ood_label=254, cache=64):
        self.root, self.split, self.ood_label = root, split + year, int(ood_label)
        images, targets = [], []
        for d, _, filenames in os.walk(os.path.join(root, "annotations", "ood_seg_" + self.split)):
            for filename in filenames:
                if os.path.splitext(filename)[-1] == ".png":
                    targets.append(os.path.join(d, filename))
                    images.append(os.path.join(root, self.split, filename.split(".")[0] + ".jpg"))
        if shuffle and images:
            zipped = list(zip(images, targets))
            (_random if py_rng is None else py_rng).shuffle(zipped)
            images, targets = zip(*zipped)
        n = 5000 if proxy_size is None else int(proxy_size)
        self.images, self.targets = list(images[:n]), list(targets[:n])
        self._cache, self._cache_size = {}, int(cache)
        self.box_hw = _BoxSizes(self)

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        hit = self._cache.get(i)
        if hit is None:
            from PIL import Image
            image = np.array(Image.open(self.images[i]).convert("RGB"))
            target = np.array(Image.open(self.targets[i]).convert("L"))
            y1, x1, y2, x2 = extract_bbox(target == self.ood_label)
            hit = (np.ascontiguousarray(image[y1:y2, x1:x2]), np.ascontiguousarray(target[y1:y2, x1:x2]))
            if len(self._cache) >= self._cache_size:
                self._cache.pop(next(iter(self._cache)))
            self._cache[i] = hit
        return hit

    def __repr__(self):
        return "Number of COCO Images: %d" % len(self.images)


class _BoxSizes:
    def __init__(self, objects):
        self.objects = objects

    def __len__(self):
        return len(self.objects)

    def __getitem__(self, i):
        return self.objects[i][1].shape[:2]


# ---------------------------------------------------------------------------------------------------------------- the mapper
class Instances:
    """The part of Detectron2's Instances the model uses: an image size and per-instance fields, each a tensor whose first dimension is the number of
    instances -- ``gt_classes`` / ``gt_masks`` in training (what the model reads), ``pred_masks`` / ``pred_classes`` / ``scores`` / ``pred_boxes`` from
    instance inference (``pred_boxes`` is a plain [N,4] tensor, XYXY).  Fields are attributes; any name may be set."""

    def __init__(self, image_size, gt_classes=None, gt_masks=None, **fields):
        self.image_size, self.gt_classes, self.gt_masks = tuple(image_size), gt_classes, gt_masks
        for name, value in fields.items():
            setattr(self, name, value)

    def get_fields(self):
        """{name: value} of the fields that are set"""
        return {k: v for k, v in vars(self).items() if k != "image_size" and v is not None}

    def has(self, name):
        return name in self.get_fields()

    def to(self, device):
        return Instances(self.image_size, **{k: to_device(v, device) for k, v in self.get_fields().items()})

    def __len__(self):
        if self.gt_classes is not None:
            return int(self.gt_classes.shape[0])
        for v in self.get_fields().values():
            return int(v.shape[0])
        raise NotImplementedError("empty Instances does not support __len__")


class MaskFormerSemanticCocoMixDatasetMapper:
    """``mapper(dataset_dict)`` -> the reference's training dict.  ``dataset_dict`` names the files (``file_name``, ``sem_seg_file_name``) or carries
    the decoded frame (``image`` uint8 [3,h,w], ``sem_seg_gt`` uint8 [h,w]; ``lut`` of raw-id labels is given at construction).  The labels are 8-bit.
    ``coco``: the objects (CocoOodObjects or anything with its two-array items and ``box_hw``); by default the listing under
    $DETECTRON2_DATASETS/INPUT.COCO_ROOT.  ``np_rng`` / ``py_rng``: the two generators of the draws (the globals by default, as in the reference).
    ``mapper(dataset_dict, params=...)`` applies given decisions instead of drawing."""

    def __init__(self, cfg, device=None, coco=None, np_rng=None, py_rng=None, lut=None, labels_mapping=None):
        if labels_mapping is not None:
            raise NotImplementedError("labels_mapping (the Mapillary path of the reference's mapper) is not provided")
        self.settings = s = mapper_settings(cfg)
        _check_settings(s)
        self.device = torch.device(device) if device is not None else None
        if coco is None:
            coco = CocoOodObjects(os.path.join(os.getenv("DETECTRON2_DATASETS", "datasets"), s.coco_root), s.coco_proxy_size, py_rng=py_rng,
                                  ood_label=s.ood_label)
        self.coco, self.np_rng, self.py_rng = coco, np_rng, py_rng
        self.lut = None if lut is None else torch.as_tensor(lut, dtype=torch.uint8)
        self._lut_dev = None

    @property
    def on_device(self):
        return self.device is not None and self.device.type == "cuda"

    def _decode(self, d):
        if "image" in d:
            image, sem = d.pop("image"), d.pop("sem_seg_gt", None)
        else:
            from .datasets import read_image, read_label
            image = torch.from_numpy(np.ascontiguousarray(np.asarray(read_image(d["file_name"])).transpose(2, 0, 1)))
            sem = torch.from_numpy(np.ascontiguousarray(np.asarray(read_label(d.pop("sem_seg_file_name"))))) if "sem_seg_file_name" in d else None
        if sem is None:
            raise ValueError("Cannot find 'sem_seg_file_name' for semantic segmentation dataset {}.".format(d.get("file_name")))
        image, sem = torch.as_tensor(image), torch.as_tensor(sem)
        if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[0] != 3:
            raise ValueError(f"the mapper needs a uint8 [3,h,w] frame, got {image.dtype} {tuple(image.shape)}")
        if sem.dtype != torch.uint8 or tuple(sem.shape) != tuple(image.shape[1:]):
            raise ValueError(f"the mapper needs uint8 [h,w] labels of the frame's size, got {sem.dtype} {tuple(sem.shape)}")
        return image, sem

    def __call__(self, dataset_dict, params=None):
        s = self.settings
        d = copy.copy(dataset_dict)
        if "annotations" in d:
            raise ValueError("Semantic segmentation dataset should not have 'annotations'.")
        image, sem = self._decode(d)
        h, w = int(image.shape[1]), int(image.shape[2])
        if params is None:
            params = sample_train_view_params(s, h, w, getattr(self.coco, "box_hw", None), self.np_rng, self.py_rng)
        obj = objmask = None
        if params.paste is not None:
            o, m = self.coco[params.ood_index]
            obj, objmask = torch.from_numpy(np.ascontiguousarray(np.asarray(o).transpose(2, 0, 1))), torch.from_numpy(np.ascontiguousarray(m))
        pad = _pad_size(s, params.crop[2], params.crop[3])
        if self.on_device:
            dev = self.device
            if self.lut is not None and self._lut_dev is None:
                self._lut_dev = self.lut.to(dev)
            up = [None if t is None else to_device(t, dev).contiguous() for t in (image, sem, obj, objmask)]
            out_image, out_sem, outlier, hist = ops.train_view(up[0], up[1], params, up[2], up[3], self._lut_dev, s.ignore_label, s.ood_label, pad)
        else:
            out_image, out_sem, outlier, hist = train_view_host(image, sem, params, obj, objmask, self.lut, s.ignore_label, s.ood_label, pad)
        # per-category binary masks: the classes present are the histogram's non-zero bins (np.unique of the reference), one 1 KB read-back
        counts = hist.cpu()
        classes = torch.nonzero(counts, as_tuple=False).reshape(-1)
        classes = classes[(classes != s.ignore_label) & (classes != s.ood_label)].repeat_interleave(s.repeat_instance_masks)
        inst = Instances((int(out_image.shape[-2]), int(out_image.shape[-1])))
        inst.gt_classes = classes.to(torch.int64)
        if classes.numel() == 0:                                                  # some image does not have annotation (all ignored)
            inst.gt_masks = torch.zeros((0, out_sem.shape[-2], out_sem.shape[-1]), device=out_sem.device)
        else:
            inst.gt_masks = out_sem[None] == classes.to(out_sem.device)[:, None, None]
        d["image"], d["sem_seg"], d["outlier_mask"], d["instances"] = out_image, out_sem, outlier, inst
        return d
