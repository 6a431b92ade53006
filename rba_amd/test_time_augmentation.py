"""Test-time augmentation: multi-scale and flip inference (reference: mask2former/test_time_augmentation.py::SemanticSegmentorWithTTA, used at
train_net.py:336-348, over Detectron2's DatasetMapperTTA; recipe: TEST.AUG of configs/cityscapes/semantic-segmentation/Base-Cityscapes-SemanticSegmentation.yaml).

``DatasetMapperTTA(cfg)`` turns one dataset dict into its views -- per entry of TEST.AUG.MIN_SIZES the image resized by Detectron2's shortest-edge rule and,
with TEST.AUG.FLIP, its horizontally flipped twin.  ``SemanticSegmentorWithTTA(cfg, model)`` runs the model on every view, brings each view's class map back
to the input's ``height`` x ``width``, un-flips, averages: ``wrapper(batched_inputs) -> [{"sem_seg": [K,H,W]}]`` as the reference, and
``wrapper.rba_scores(...)`` with MaskFormer.rba_scores' contract for the evaluators.

On a HIP device the views are made on the device from ONE upload of the image (K12b, ops.resize_u8_pil_bilinear: Pillow's fixed-point bilinear resize, byte for
byte) and the per-view resize, flip, sum, division and score are ONE kernel behind the forwards (K12a, ops.tta_merge); docs/kernels/K12.md.
"""
import copy

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from ._lib import TTA_MAX_VIEWS
from .h2d import to_device

__all__ = ["DatasetMapperTTA", "SemanticSegmentorWithTTA", "resize_shortest_edge_shape", "tta_enabled"]


def resize_shortest_edge_shape(h, w, size, max_size):
    """Detectron2's ResizeShortestEdge.get_output_shape: the short edge becomes ``size``, the whole is scaled down again when the long edge would
    exceed ``max_size``, then int(v + 0.5) -> (new_h, new_w)."""
    size = size * 1.0
    scale = size / min(h, w)
    newh, neww = (size, scale * w) if h < w else (scale * h, size)
    if max(newh, neww) > max_size:
        scale = max_size * 1.0 / max(newh, neww)
        newh, neww = newh * scale, neww * scale
    return int(newh + 0.5), int(neww + 0.5)


def pil_bilinear_resize_numpy(image, size):
    """Pillow's Image.resize(BILINEAR) of a uint8 [C,h,w] array in numpy: the horizontal pass, then the vertical pass on its rounded uint8 result,
    with the integer tables of ops.pil_bilinear_coeffs -- the arithmetic K12b runs on the device.  For hosts without Pillow, and the tests."""
    img = np.ascontiguousarray(image)
    H, W = int(size[0]), int(size[1])
    for axis, n_out in ((2, W), (1, H)):
        n_in = img.shape[axis]
        if n_in == n_out:
            continue
        kk, bounds, ksize = ops.pil_bilinear_coeffs(n_in, n_out)
        src = np.moveaxis(img, axis, -1).astype(np.int64)
        idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(ksize)[None, :], n_in - 1)          # weights beyond the count are 0
        acc = (src[..., idx] * kk.astype(np.int64)).sum(-1) + (1 << 21)
        img = np.ascontiguousarray(np.moveaxis(np.clip(acc >> 22, 0, 255).astype(np.uint8), -1, axis))
    return img


def _resize_u8_host(image, size):
    """uint8 [C,h,w] numpy -> [C,H,W]: Pillow itself where it is installed (what Detectron2 calls), its numpy restatement otherwise"""
    H, W = int(size[0]), int(size[1])
    try:
        from PIL import Image
    except ImportError:
        return pil_bilinear_resize_numpy(image, (H, W))
    hwc = np.ascontiguousarray(image.transpose(1, 2, 0))
    if hwc.shape[2] == 1:
        out = np.asarray(Image.fromarray(hwc[:, :, 0], mode="L").resize((W, H), Image.BILINEAR))[:, :, None]
    else:
        out = np.asarray(Image.fromarray(hwc).resize((W, H), Image.BILINEAR))
    return np.ascontiguousarray(out.transpose(2, 0, 1))


def tta_enabled(cfg):
    """TEST.AUG.ENABLED of a config (False where the config has no TEST.AUG)"""
    return bool(cfg.get("TEST", {}).get("AUG", {}).get("ENABLED", False))


class DatasetMapperTTA:
    """Detectron2's DatasetMapperTTA (detectron2/modeling/test_time_augmentation.py): dataset dict with "image" ([C,h,w] tensor, uint8 or float) ->
    one dict per view, for each of TEST.AUG.MIN_SIZES the ResizeShortestEdge(min_size, MAX_SIZE) view and then, with TEST.AUG.FLIP, its flipped twin.
    Every view keeps the input's other keys (``height`` / ``width``: the size results are asked at) and carries ``"transforms"``: a list of
    ("resize", h, w, new_h, new_w) / ("hflip", width) tuples; as in Detectron2 the list starts with the resize from the image's size to ``height`` x ``width``
    when the two differ, and -- as in Detectron2 -- that one is recorded for the consumer, not applied to the pixels: the views are cut from the image
    as it is.

    device=None: views are made on the host (uint8: Pillow, as Detectron2's ResizeTransform; float: F.interpolate bilinear, as Detectron2 does for
    float images) and stay there.  device=a HIP device: the image is uploaded once and every view is made on the device -- uint8 by K12b
    (ops.resize_u8_pil_bilinear, flip folded in), equal to the host views in every byte; float by ops.resample_bilinear and torch.flip."""

    def __init__(self, cfg, device=None):
        aug = cfg.TEST.AUG
        self.min_sizes = tuple(int(s) for s in aug.MIN_SIZES)
        self.max_size = int(aug.MAX_SIZE)
        self.flip = bool(aug.FLIP)
        self.device = torch.device(device) if device is not None else None

    def view_shapes(self, h, w):
        """[(new_h, new_w, flipped)] in the order the views are emitted"""
        out = []
        for s in self.min_sizes:
            nh, nw = resize_shortest_edge_shape(h, w, s, self.max_size)
            out.append((nh, nw, False))
            if self.flip:
                out.append((nh, nw, True))
        return out

    def _view(self, image, host, nh, nw, flipped):
        if self.device is not None and self.device.type == "cuda":
            if image.dtype == torch.uint8:
                return ops.resize_u8_pil_bilinear(image, (nh, nw), flip=flipped)
            v = ops.resample_bilinear(image, (nh, nw)) if tuple(image.shape[-2:]) != (nh, nw) else image
            return torch.flip(v, dims=[2]).contiguous() if flipped else v
        if image.dtype == torch.uint8:
            v = torch.from_numpy(_resize_u8_host(host, (nh, nw)))
        else:
            v = F.interpolate(image[None].float(), size=(nh, nw), mode="bilinear", align_corners=False)[0].to(image.dtype)
        return torch.flip(v, dims=[2]).contiguous() if flipped else v

    def __call__(self, dataset_dict):
        image = dataset_dict["image"]
        if not torch.is_tensor(image) or image.dim() != 3:
            raise ValueError("DatasetMapperTTA needs dataset_dict['image'] as a [C,h,w] tensor")
        h, w = int(image.shape[1]), int(image.shape[2])
        height, width = int(dataset_dict.get("height", h)), int(dataset_dict.get("width", w))
        pre = [("resize", h, w, height, width)] if (h, w) != (height, width) else []
        rest = {k: v for k, v in dataset_dict.items() if k != "image"}
        host = None
        if self.device is not None and self.device.type == "cuda":
            image = to_device(image, self.device).contiguous()
            if image.dtype not in (torch.uint8, torch.float32):
                image = image.float()
        elif image.dtype == torch.uint8:
            host = image.cpu().numpy()
        ret = []
        for nh, nw, flipped in self.view_shapes(h, w):
            dic = copy.deepcopy(rest)
            dic["transforms"] = pre + [("resize", h, w, nh, nw)] + ([("hflip", nw)] if flipped else [])
            dic["image"] = self._view(image, host, nh, nw, flipped)
            ret.append(dic)
        return ret


def _flipped(tfms):
    return any(t[0] == "hflip" for t in tfms)


class SemanticSegmentorWithTTA(nn.Module):
    """A semantic segmentor with test-time augmentation (mask2former/test_time_augmentation.py:21-103).  ``wrapper(batched_inputs)`` has MaskFormer.forward's
    input and output format (``[{"sem_seg": [K,H,W]}]``, H x W = the input's ``height`` x ``width``); ``wrapper.rba_scores(batched_inputs,
    return_argmax, score)`` has MaskFormer.rba_scores', so OODEvaluator and evaluate_ood.get_RbA / get_energy / get_neg_logit_sum take the wrapper as they
    take the model.

    Per view: ``model.predict`` and ``model._post(..., want_sem_seg=True)`` = the view's class map at the view's size; then ONE ops.tta_merge (K12a)
    resizes every class map to H x W, un-flips, adds in view order, divides by the number of views and takes the score -- the reference's
    ``sem_seg_postprocess`` per view, ``.flip(dims=[2])``, ``+=`` and ``/ count`` (:83-97) without their K x H x W intermediates.  More than
    K = 32 classes or more than 16 views: the same arithmetic from ops.resample_bilinear and torch, view by view.
    Forwards run eagerly: graph replay across views is not provided, and the wrapper has no ``graph_replay`` attribute for an evaluator to set."""

    def __init__(self, cfg, model, tta_mapper=None, batch_size=1):
        super().__init__()
        if isinstance(model, nn.parallel.DistributedDataParallel):
            model = model.module
        self.cfg = copy.deepcopy(cfg)
        self.model = model
        if tta_mapper is None:
            dev = model.device
            tta_mapper = DatasetMapperTTA(cfg, device=dev if dev.type == "cuda" else None)
        self.tta_mapper = tta_mapper
        self.batch_size = max(1, int(batch_size))

    @property
    def device(self):
        return self.model.device

    @staticmethod
    def _complete(dataset_dict):
        ret = copy.copy(dataset_dict)
        if "image" not in ret:
            raise KeyError("SemanticSegmentorWithTTA needs the decoded 'image' in every input dict")
        if "height" not in ret and "width" not in ret:
            ret["height"], ret["width"] = int(ret["image"].shape[1]), int(ret["image"].shape[2])
        return ret

    def _view_class_maps(self, inp):
        """-> ([sem_a [K,h_a,w_a]], [flip_a]) in view order"""
        if getattr(self.model, "sem_seg_postprocess_before_inference", False):
            raise NotImplementedError("test-time augmentation is provided for semantic inference only (no TEST.PANOPTIC_ON / "
                                      "SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE)")
        views = self.tta_mapper(inp)
        flips = [_flipped(v["transforms"]) for v in views]
        sems = []
        for i in range(0, len(views), self.batch_size):
            chunk = [{"image": v["image"]} for v in views[i:i + self.batch_size]]
            mask_cls, mask_pred, sizes, padded = self.model.predict(chunk)
            for j in range(len(chunk)):
                sems.append(self.model._post(mask_cls[j], mask_pred[j], sizes[j], padded, True, False)[1])
        return sems, flips

    @staticmethod
    def _fused(sems):
        return len(sems) <= TTA_MAX_VIEWS and sems[0].shape[0] <= 32

    @staticmethod
    def _unfused_mean(sems, flips, size):
        """the reference's own sequence: sem_seg_postprocess (resize), flip, +=, / count"""
        total = None
        for sem, flipped in zip(sems, flips):
            r = ops.resample_bilinear(sem.contiguous(), size) if tuple(sem.shape[-2:]) != tuple(size) else sem
            if flipped:
                r = torch.flip(r, dims=[2])
            if total is None:
                total = r.clone() if r is sem else r
            else:
                total += r
        return total / len(sems)

    @torch.no_grad()
    def _merged(self, inp, want_sem_seg, want_argmax, score):
        """one input dict -> (score map, sem_seg | None, argmax | None) at height x width"""
        inp = self._complete(inp)
        size = (int(inp["height"]), int(inp["width"]))
        sems, flips = self._view_class_maps(inp)
        if self._fused(sems):
            return ops.tta_merge(sems, flips, size, want_sem_seg, want_argmax, score)
        mean = self._unfused_mean(sems, flips, size)
        ops._mode(score)
        s = -mean.tanh().sum(0) if score == "rba" else (-torch.logsumexp(mean, dim=0) if score == "energy" else -mean.sum(0))
        return s, (mean if want_sem_seg else None), (mean.argmax(0).to(torch.int32) if want_argmax else None)

    def forward(self, batched_inputs):
        """Same input / output format as MaskFormer.forward's semantic branch: [{"sem_seg": [K,height,width]}]"""
        return [{"sem_seg": self._merged(x, True, False, "rba")[1]} for x in batched_inputs]

    def rba_scores(self, batched_inputs, return_argmax=False, score="rba"):
        """MaskFormer.rba_scores' contract: per input the score map [height,width] of the averaged class map -- "rba", "energy" or "neg_logit_sum" --
        or (score map, int32 argmax map) with ``return_argmax``; the averaged sem_seg itself is never stored."""
        out = []
        for x in batched_inputs:
            s, _, arg = self._merged(x, False, return_argmax, score)
            out.append((s, arg) if return_argmax else s)
        return out
