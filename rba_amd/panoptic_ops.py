"""Python entry points of K16 (csrc/panoptic_merge.hip, docs/kernels/K16.md): the closed-set panoptic merge of MaskFormer.panoptic_inference
(mask2former/maskformer_model.py:394-452) and the segment-pair histogram of the open-set PQ evaluation (mask2former/evaluation/evaluation.py:152-159).

Written in rba_amd.ops' style with its decorator, validators and launch line: a wrapper reads top to bottom as its checks, its output allocation, one
`_launch` line; a bad argument raises RbaHipError before anything is allocated or enqueued; there is no fallback path."""
import torch

from ._lib import RbaHipError
from .ops import _chk, _hip_op, _launch, _p

MAX_QUERIES = 255             # K16_MAX_Q: 0xFF is the "nobody" byte of `winner`
NOBODY = 0xFF
MAX_PAIRS = 1 << 24           # K16C_MAX_PAIRS


# ---------------------------------------------------------------------------------------------------------------- argument contracts, each written once
def _queries(score, keep, Q, kept):
    """score fp32 [Q] and keep uint8 [Q] of 1 <= Q <= 255 queries, at least one of them kept.  `kept`: the number of kept queries when the caller has read
    it already (a call under graph capture must pass it); None: it is read here, the wrapper's one read-back, before anything is allocated."""
    if not 1 <= Q <= MAX_QUERIES:
        raise RbaHipError(f"the panoptic merge needs 1 <= Q <= {MAX_QUERIES} queries (0xFF marks a pixel nobody owns), got {Q}")
    _chk(score, "score", dim=1)
    _chk(keep, "keep", dtype=torch.uint8, dim=1)
    for t, name in ((score, "score"), (keep, "keep")):
        if t.numel() != Q:
            raise RbaHipError(f"{name} must have {Q} elements, got {t.numel()}")
    if (int(keep.count_nonzero()) if kept is None else int(kept)) < 1:
        raise RbaHipError("the panoptic merge needs at least one kept query (the reference returns before the merge, maskformer_model.py:414-416)")


def _merge_outputs(shape, Q, device):
    return torch.empty(shape, dtype=torch.uint8, device=device), torch.zeros((3, Q), dtype=torch.int32, device=device)


@_hip_op
def panoptic_merge(mask, score, keep, kept=None):
    """K16a.  mask [Q,H,W] mask logits at the output resolution, score fp32 [Q], keep uint8 [Q] (non-zero: the query competes) ->
    (winner uint8 [H,W], counts int32 [3,Q]).  Per pixel, over the kept q in ascending order: s = sigmoid(mask[q,p]), v = score[q] * s; best = the first q
    with the largest v; winner = best where its s >= 0.5, else 0xFF; counts[0][q] = the pixels q won, counts[1][q] = its own s >= 0.5 area,
    counts[2][q] = their intersection (maskformer_model.py:420-427 for every kept query in one pass).  1 <= Q <= 255, 1 <= H * W < 2^31."""
    _chk(mask, "mask", dim=3)
    Q, H, W = mask.shape
    _queries(score, keep, Q, kept)
    if not 1 <= H * W < 1 << 31:
        raise RbaHipError(f"panoptic_merge needs 1 <= H * W < 2^31 pixels, got {H} x {W}")
    winner, counts = _merge_outputs((H, W), Q, mask.device)
    _launch("rba_panoptic_merge_f32", _p(mask), _p(score), _p(keep), _p(winner), _p(counts), Q, H * W)
    return winner, counts


@_hip_op
def panoptic_merge_up4(mask_lowres, score, keep, crop, kept=None):
    """K16a fused with the x4 upsample (maskformer_model.py:294-299) and the crop (:330-332), ops.rba_reduce_up4's contract: mask_lowres [Q,h,w];
    the rule of `panoptic_merge` on the [crop_h, crop_w] window of the virtual [Q,4h,4w] map -> (winner uint8 [crop_h,crop_w], counts int32 [3,Q])."""
    _chk(mask_lowres, "mask_lowres", dim=3)
    Q, h, w = mask_lowres.shape
    _queries(score, keep, Q, kept)
    ch, cw = int(crop[0]), int(crop[1])
    if h < 1 or w < 1 or not (1 <= ch <= 4 * h and 1 <= cw <= 4 * w):
        raise RbaHipError(f"crop {(ch, cw)} must lie inside the x4 map {(4 * h, 4 * w)} and hold at least one pixel")
    winner, counts = _merge_outputs((ch, cw), Q, mask_lowres.device)
    _launch("rba_panoptic_merge_up4_f32", _p(mask_lowres), _p(score), _p(keep), _p(winner), _p(counts), Q, h, w, ch, cw)
    return winner, counts


@_hip_op
def panoptic_assign(winner, seg_of_query):
    """K16b.  winner uint8 (K16a's), seg_of_query int32 [Q] (the segment id of each query, 0 = dropped) -> panoptic int32 of winner's shape:
    seg_of_query[winner], 0 where winner is 0xFF.  The reference's `panoptic_seg[mask] = id` writes (:437-445) touch disjoint pixels: one gather."""
    _chk(winner, "winner", dtype=torch.uint8)
    _chk(seg_of_query, "seg_of_query", dtype=torch.int32, dim=1)
    Q = seg_of_query.numel()
    if not 1 <= Q <= MAX_QUERIES:
        raise RbaHipError(f"seg_of_query must have 1 <= Q <= {MAX_QUERIES} entries, got {Q}")
    if not 1 <= winner.numel() < 1 << 31:
        raise RbaHipError(f"panoptic_assign needs 1 <= pixels < 2^31, got {winner.numel()}")
    panoptic = torch.empty(winner.shape, dtype=torch.int32, device=winner.device)
    _launch("rba_panoptic_assign_i32", _p(winner), _p(seg_of_query), _p(panoptic), Q, winner.numel())
    return panoptic


@_hip_op
def segment_pairs(gt, pred, G, P, counts, bad):
    """K16c.  gt, pred int32 maps of one shape holding dense segment ids, counts int64 [G,P], bad int64 [1]: counts[gt, pred] += 1 per pixel with
    0 <= gt < G and 0 <= pred < P, bad[0] += 1 for every other pixel (evaluation.py:152-159's np.unique(pan_gt * OFFSET + pan_pred) on dense ids).
    counts and bad are accumulated into -- zero them per image or per evaluation; nothing is read back and nothing synchronises."""
    G, P = int(G), int(P)
    if G < 1 or P < 1 or G * P > MAX_PAIRS:
        raise RbaHipError(f"segment_pairs needs 1 <= G, P and G * P <= 2^24, got G = {G}, P = {P}")
    _chk(gt, "gt", dtype=torch.int32)
    _chk(pred, "pred", dtype=torch.int32)
    if gt.shape != pred.shape:
        raise RbaHipError(f"gt {tuple(gt.shape)} and pred {tuple(pred.shape)} must have the same shape")
    if gt.numel() < 1:
        raise RbaHipError("segment_pairs: empty maps")
    _chk(counts, "counts", dtype=torch.int64, dim=2)
    if tuple(counts.shape) != (G, P):
        raise RbaHipError(f"counts must have shape {(G, P)}, got {tuple(counts.shape)}")
    _chk(bad, "bad", dtype=torch.int64, dim=1)
    if bad.numel() != 1:
        raise RbaHipError(f"bad must have 1 element, got {bad.numel()}")
    _launch("rba_segment_pairs_accum", _p(gt), _p(pred), gt.numel(), G, P, _p(counts), _p(bad))


def merge_segments(counts, classes, thing_classes, overlap_threshold):
    """The reference's loop over the kept queries (maskformer_model.py:418-452) on the host, over Python ints: counts = K16a's [3][Q] as lists, classes[q] =
    the class of query q or a negative number where it is not kept -> (seg_of_query list [Q], segments_info, the number of segments)."""
    won, own, inter = counts
    seg_of_query = [0] * len(classes)
    segments_info, stuff_ids, current = [], {}, 0
    for q, cls in enumerate(classes):
        if cls < 0:
            continue
        mask_area, original_area = won[q], own[q]
        if mask_area == 0 or original_area == 0 or inter[q] == 0 or mask_area / original_area < overlap_threshold:
            continue
        isthing = cls in thing_classes
        if not isthing:
            if cls in stuff_ids:
                seg_of_query[q] = stuff_ids[cls]
                continue
            stuff_ids[cls] = current + 1
        current += 1
        seg_of_query[q] = current
        segments_info.append({"id": current, "isthing": bool(isthing), "category_id": cls})
    return seg_of_query, segments_info, current


@_hip_op
def panoptic_segments(mask, score, keep, classes, thing_classes, overlap_threshold, crop=None):
    """The closed-set merge end to end: K16a (``crop`` given: the up4 form on mask = the quarter-resolution logits), ONE read-back of its counts,
    `merge_segments` on the host, the upload of its table, K16b -> (panoptic int32 [H,W], segments_info, the number of segments).
    classes: a host list, classes[q] = the class of query q, negative where keep[q] is 0 (the caller has read it with `keep`)."""
    classes = [int(c) for c in classes]
    kept = sum(1 for c in classes if c >= 0)
    if crop is None:
        winner, counts = panoptic_merge(mask, score, keep, kept=kept)
    else:
        winner, counts = panoptic_merge_up4(mask, score, keep, crop, kept=kept)
    seg_of_query, segments_info, current = merge_segments(counts.tolist(), classes, thing_classes, overlap_threshold)
    return panoptic_assign(winner, torch.tensor(seg_of_query, dtype=torch.int32, device=mask.device)), segments_info, current


__all__ = ["panoptic_merge", "panoptic_merge_up4", "panoptic_assign", "segment_pairs", "merge_segments", "panoptic_segments", "MAX_QUERIES", "NOBODY",
           "MAX_PAIRS"]
