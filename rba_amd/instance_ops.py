"""Python entry points of K17 (csrc/instance_masks.hip, docs/kernels/K17.md): MaskFormer.instance_inference (mask2former/maskformer_model.py:488-527)
on the mask logits -- the per-query mask statistics in one pass over the planes of the top-k queries, and the result planes written once.

Written in rba_amd.ops' style with its decorator, validators and launch line (as rba_amd.panoptic_ops): a wrapper reads top to bottom as its checks, its
output allocation, one `_launch` line; a bad argument raises RbaHipError before anything is allocated or enqueued; there is no fallback path."""
import torch

from . import ops
from ._lib import RbaHipError
from .ops import _chk, _hip_op, _launch, _p

MAX_QUERIES = 255             # K17_MAX_Q
MAX_DETECTIONS = 65535        # K17B_MAX_N: one grid row per result plane
SSUM_ONE = 1 << 32            # ssum counts sigmoids in units of 2^-32
MASK_DTYPES = {torch.float32: "f32", torch.uint8: "u8"}


# ---------------------------------------------------------------------------------------------------------------- argument contracts, each written once
def _kept(keep, Q):
    """keep uint8 [Q] of 1 <= Q <= 255 queries (none kept is served: every output stays neutral)"""
    if not 1 <= Q <= MAX_QUERIES:
        raise RbaHipError(f"the instance statistics need 1 <= Q <= {MAX_QUERIES} queries, got {Q}")
    _chk(keep, "keep", dtype=torch.uint8, dim=1)
    if keep.numel() != Q:
        raise RbaHipError(f"keep must have {Q} elements, got {keep.numel()}")


def _crop(crop, h, w):
    ch, cw = int(crop[0]), int(crop[1])
    if h < 1 or w < 1 or not (1 <= ch <= 4 * h and 1 <= cw <= 4 * w):
        raise RbaHipError(f"crop {(ch, cw)} must lie inside the x4 map {(4 * h, 4 * w)} and hold at least one pixel")
    return ch, cw


def _detections(qidx, dtype):
    """qidx int32 [N] of 1 <= N <= 65535 detections, and the result planes' element type -> the entry points' suffix"""
    _chk(qidx, "qidx", dtype=torch.int32, dim=1)
    if not 1 <= qidx.numel() <= MAX_DETECTIONS:
        raise RbaHipError(f"qidx must name 1 <= N <= {MAX_DETECTIONS} detections, got {qidx.numel()}")
    if dtype not in MASK_DTYPES:
        raise RbaHipError(f"the result planes are torch.float32 (the reference's) or torch.uint8, got {dtype}")
    return MASK_DTYPES[dtype]


def _stats_outputs(Q, H, W, device):
    """count int32 [Q] and ssum int64 [Q] zeroed, box int32 [Q,4] = (W, H, -1, -1): the neutral elements of the kernels' add / min / max"""
    box = torch.empty((Q, 4), dtype=torch.int32, device=device)
    box[:, 0], box[:, 1], box[:, 2:] = W, H, -1                                       # fills: nothing is copied from the host
    return torch.zeros(Q, dtype=torch.int32, device=device), torch.zeros(Q, dtype=torch.int64, device=device), box


@_hip_op
def instance_stats(mask, keep):
    """K17a.  mask [Q,H,W] mask logits at the output resolution, keep uint8 [Q] (non-zero: the query is in the top-k) ->
    (count int32 [Q], ssum int64 [Q], box int32 [Q,4]).  For every kept q over its pixels with logit m > 0: count = their number, ssum = the exact sum of
    their fp32 sigmoids in units of 2^-32 (bitwise reproducible), box = (min x, min y, max x, max y), (W, H, -1, -1) where there is none
    (maskformer_model.py:517-524 and the boxes of :520 for every query of the top-k in one pass).  1 <= Q <= 255, 1 <= H * W < 2^31."""
    _chk(mask, "mask", dim=3)
    Q, H, W = mask.shape
    _kept(keep, Q)
    if not 1 <= H * W < 1 << 31:
        raise RbaHipError(f"instance_stats needs 1 <= H * W < 2^31 pixels, got {H} x {W}")
    count, ssum, box = _stats_outputs(Q, H, W, mask.device)
    _launch("rba_instance_stats_f32", _p(mask), _p(keep), _p(count), _p(ssum), _p(box), Q, H, W)
    return count, ssum, box


@_hip_op
def instance_stats_up4(mask_lowres, keep, crop):
    """K17a fused with the x4 upsample (maskformer_model.py:294-299) and the crop (:330-332), panoptic_ops.panoptic_merge_up4's contract: mask_lowres [Q,h,w];
    the rule of `instance_stats` on the [crop_h, crop_w] window of the virtual [Q,4h,4w] map."""
    _chk(mask_lowres, "mask_lowres", dim=3)
    Q, h, w = mask_lowres.shape
    _kept(keep, Q)
    ch, cw = _crop(crop, h, w)
    count, ssum, box = _stats_outputs(Q, ch, cw, mask_lowres.device)
    _launch("rba_instance_stats_up4_f32", _p(mask_lowres), _p(keep), _p(count), _p(ssum), _p(box), Q, h, w, ch, cw)
    return count, ssum, box


@_hip_op
def instance_masks(mask, qidx, dtype=torch.float32):
    """K17b.  mask [Q,H,W] mask logits, qidx int32 [N] (the query of each detection; a query may appear several times) -> out [N,H,W] of `dtype`
    (torch.float32, the reference's, or torch.uint8): out[n] = mask[qidx[n]] > 0 (maskformer_model.py:503, :517).  A qidx outside [0, Q) gives a plane
    of zeros: the kernel refuses it on the device, nothing is read back here."""
    _chk(mask, "mask", dim=3)
    Q, H, W = mask.shape
    suffix = _detections(qidx, dtype)
    if Q < 1 or not 1 <= H * W < 1 << 31:
        raise RbaHipError(f"instance_masks needs Q >= 1 and 1 <= H * W < 2^31 pixels, got mask {tuple(mask.shape)}")
    out = torch.empty((qidx.numel(), H, W), dtype=dtype, device=mask.device)
    _launch("rba_instance_masks_" + suffix, _p(mask), _p(qidx), _p(out), Q, qidx.numel(), H * W)
    return out


@_hip_op
def instance_masks_up4(mask_lowres, qidx, crop, dtype=torch.float32):
    """K17b on the [crop_h, crop_w] window of the virtual x4 map of mask_lowres [Q,h,w] (instance_stats_up4's taps: planes and counts agree pixel by
    pixel) -> out [N,crop_h,crop_w]."""
    _chk(mask_lowres, "mask_lowres", dim=3)
    Q, h, w = mask_lowres.shape
    suffix = _detections(qidx, dtype)
    if Q < 1:
        raise RbaHipError("instance_masks_up4 needs Q >= 1")
    ch, cw = _crop(crop, h, w)
    out = torch.empty((qidx.numel(), ch, cw), dtype=dtype, device=mask_lowres.device)
    _launch("rba_instance_masks_up4_" + suffix, _p(mask_lowres), _p(qidx), _p(out), Q, qidx.numel(), h, w, ch, cw)
    return out


def mask_scores(count, ssum):
    """The reference's fp32 expression (:523-524) from K17a's integers: fp32(ssum * 2^-32) / (fp32(count) + 1e-6f) -- one rounding for the sum (the
    int64 -> fp32 conversion; the power of two is exact), one for the denominator, one for the division."""
    return (ssum.to(torch.float32) * (1.0 / SSUM_ONE)) / (count.to(torch.float32) + 1e-6)


def boxes_xyxy(count, box):
    """K17a's (min x, min y, max x, max y) -> Detectron2's BitMasks.get_bounding_boxes convention: fp32 (xmin, ymin, xmax + 1, ymax + 1), zeros for an
    empty mask."""
    b = box.to(torch.float32)
    b[:, 2:] += 1.0
    return torch.where((count > 0)[:, None], b, torch.zeros_like(b))


@_hip_op
def instance_segments(mask_cls, mask, topk, num_classes, crop=None, thing_classes=None, boxes=False, mask_dtype=torch.float32):
    """MaskFormer.instance_inference (maskformer_model.py:488-527) end to end.  mask_cls [Q,K+1] class logits, mask [Q,H,W] mask logits at the output
    resolution (``crop`` = (H, W) given: the quarter-resolution [Q,h,w], and everything runs on that window of their virtual x4 up-sampling -- the
    full-resolution planes are never written) -> (pred_masks [N,H,W] of ``mask_dtype``, pred_classes int64 [N], scores fp32 [N], pred_boxes fp32 [N,4]).

    The [Q,K] scores (rba_softmax_drop_last_f32), torch.topk over the flat Q * K scores, class = index % K, query = index // K, the kept queries
    scattered on the device, K17a, score = class score * mask score in fp32 as the reference writes it, K17b.  The reference asks topk for
    ``sorted=False`` and so leaves the order of the detections unspecified; HERE THE DETECTIONS COME IN DESCENDING CLASS SCORE (``sorted=True``).
    ``thing_classes`` (the reference's `panoptic_on` filter, :506-513): only detections of these classes are returned -- one device table lookup and
    one boolean index, which is this function's only read-back; without it nothing is read back.  ``boxes``: K17a's boxes in Detectron2's
    BitMasks.get_bounding_boxes convention instead of the reference's zeros (:518)."""
    _chk(mask_cls, "mask_cls", dim=2)
    _chk(mask, "mask", dim=3)
    Q, K = mask_cls.shape[0], int(num_classes)
    if mask_cls.shape[1] != K + 1:
        raise RbaHipError(f"mask_cls must have num_classes + 1 = {K + 1} columns, got {mask_cls.shape[1]}")
    if not 1 <= Q <= MAX_QUERIES or not 1 <= K <= 63:
        raise RbaHipError(f"instance_segments needs 1 <= Q <= {MAX_QUERIES} queries and 1 <= K <= 63 classes, got Q = {Q}, K = {K}")
    if mask.shape[0] != Q:
        raise RbaHipError(f"mask_cls has {Q} queries, mask {mask.shape[0]}")
    if crop is not None:
        _crop(crop, mask.shape[1], mask.shape[2])
    elif not 1 <= mask.shape[1] * mask.shape[2] < 1 << 31:
        raise RbaHipError(f"instance_segments needs 1 <= H * W < 2^31 pixels, got mask {tuple(mask.shape)}")
    topk = int(topk)
    if not 1 <= topk <= Q * K:
        raise RbaHipError(f"topk must satisfy 1 <= topk <= Q * K = {Q * K}, got {topk}")
    if mask_dtype not in MASK_DTYPES:
        raise RbaHipError(f"mask_dtype is torch.float32 (the reference's) or torch.uint8, got {mask_dtype}")
    device = mask.device
    scores = ops.softmax_drop_last(mask_cls)                                        # [Q,K] (:493)
    cls_score, index = torch.topk(scores.flatten(), topk, sorted=True)              # (:497-498)
    labels, qidx = index % K, index // K                                            # (:494-501)
    keep = torch.zeros(Q, dtype=torch.uint8, device=device).index_fill_(0, qidx, 1)
    count, ssum, box = instance_stats(mask, keep) if crop is None else instance_stats_up4(mask, keep, crop)
    if thing_classes is not None:                                                   # (:506-513)
        is_thing = torch.zeros(K, dtype=torch.bool, device=device)
        things = [int(c) for c in thing_classes if 0 <= int(c) < K]
        if things:
            is_thing[torch.tensor(things, dtype=torch.int64, device=device)] = True
        sel = is_thing[labels]
        cls_score, labels, qidx = cls_score[sel], labels[sel], qidx[sel]
    out_scores = cls_score * mask_scores(count, ssum)[qidx]                         # (:523-525)
    n = qidx.numel()
    pred_boxes = boxes_xyxy(count, box)[qidx] if boxes else torch.zeros((n, 4), dtype=torch.float32, device=device)
    if n == 0:
        H, W = mask.shape[-2:] if crop is None else (int(crop[0]), int(crop[1]))
        return torch.zeros((0, H, W), dtype=mask_dtype, device=device), labels, out_scores, pred_boxes
    q32 = qidx.to(torch.int32)
    planes = instance_masks(mask, q32, mask_dtype) if crop is None else instance_masks_up4(mask, q32, crop, mask_dtype)
    return planes, labels, out_scores, pred_boxes


__all__ = ["instance_stats", "instance_stats_up4", "instance_masks", "instance_masks_up4", "instance_segments", "mask_scores", "boxes_xyxy",
           "MAX_QUERIES", "MAX_DETECTIONS", "SSUM_ONE"]
