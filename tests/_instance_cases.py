"""Fixtures and restatements for the K17 tests (docs/kernels/K17.md), all on the CPU so that every seed is checked without a device.

* `stats_reference`: K17a's per-query sums in numpy, fp64 (the sum of the sigmoids as a float, the kernel's is a 2^-32 fixed-point integer).
* `instance_reference`: MaskFormer.instance_inference (mask2former/maskformer_model.py:488-527) restated in numpy fp64, with Detectron2's
  BitMasks.get_bounding_boxes rule for the boxes the reference leaves commented out (:520): (xmin, ymin, xmax + 1, ymax + 1), zeros for an empty mask.
* `reference_lines_fp32`: the reference's own lines typed as fp32 torch ops, for the CPU comparison and the distance quoted in docs/kernels/K17.md.
* the decision margins, asserted in fp64 before a GPU is asked anything:
  (a) logits sit on a 1/8 grid; the x4 taps are multiples of 1/8, so interpolated values are multiples of 1/512 and exact in fp32: every full-resolution
      or interpolated logit is exactly 0 or at least LOGIT = 1/512 from 0, and `> 0` is the same decision in every arithmetic;
  (b) every two neighbours among the descending top-k scores, and rank topk and rank topk + 1, are a relative GAP = 1e-5 apart, so the set of detections
      AND their descending order are the same in fp32 and fp64: position i of a result is one (query, class) pair on both sides.
  With both held no pixel and no detection is left out of any comparison.
* SCORE_BAR: |scores - fp64| <= 1e-6.  Derived, not chosen: the sum of the sigmoids is exact; what remains is rba_sigmoid's absolute error (<~ 1e-7,
  csrc/common.h) and three fp32 roundings (the int64 -> fp32 conversion, the division, the product with the class score), each <= 6e-8 relative on
  values in [0, 1]: ~2.8e-7, held at about four times that.
* SIGMOID_ERR = 1e-7: rba_sigmoid's bound, for |ssum - fp64 sum * 2^32| <= count * 2^32 * SIGMOID_ERR.
"""
import numpy as np
import torch
import torch.nn.functional as F

from tests._panoptic_cases import grid_logits, upsample4_fp64

GAP = 1e-5
LOGIT = 1.0 / 512
SCORE_BAR = 1e-6
SIGMOID_ERR = 1e-7
SSUM_ONE = 1 << 32


# ---------------------------------------------------------------------------------------------------------------- restatements
def _sigmoid64(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64)))


def boxes_of(masks):
    """Detectron2's BitMasks.get_bounding_boxes on bool masks [N,H,W] -> float64 [N,4]"""
    masks = np.asarray(masks).astype(bool)
    boxes = np.zeros((masks.shape[0], 4), dtype=np.float64)
    x_any, y_any = masks.any(axis=1), masks.any(axis=2)
    for i in range(masks.shape[0]):
        x, y = np.where(x_any[i])[0], np.where(y_any[i])[0]
        if len(x) > 0 and len(y) > 0:
            boxes[i] = (x[0], y[0], x[-1] + 1, y[-1] + 1)
    return boxes


def stats_reference(mask, keep):
    """mask [Q,H,W] logits, keep [Q] bool -> (count int64 [Q], sigmoid sum float64 [Q], box int64 [Q,4] = (min x, min y, max x, max y), (W, H, -1, -1)
    where the query has no positive pixel or is not kept)"""
    mask = np.asarray(mask, dtype=np.float64)
    Q, H, W = mask.shape
    keep = np.asarray(keep).astype(bool)
    pos = (mask > 0) & keep[:, None, None]                                # NaN > 0 is False
    count = pos.reshape(Q, -1).sum(1).astype(np.int64)
    ssum = np.where(pos, _sigmoid64(mask), 0.0).reshape(Q, -1).sum(1)
    box = np.tile(np.array([W, H, -1, -1], dtype=np.int64), (Q, 1))
    b = boxes_of(pos)
    for q in range(Q):
        if count[q]:
            box[q] = (b[q, 0], b[q, 1], b[q, 2] - 1, b[q, 3] - 1)
    return count, ssum, box


def instance_reference(mask_cls, mask_pred, topk, thing_classes=None):
    """:488-527 in fp64 -> {"qidx", "classes" int64 [N], "scores" float64 [N], "masks" bool [N,H,W], "boxes" float64 [N,4]} in descending class score"""
    mask_cls = np.asarray(mask_cls, dtype=np.float64)
    mask_pred = np.asarray(mask_pred, dtype=np.float64)
    K = mask_cls.shape[1] - 1
    e = np.exp(mask_cls - mask_cls.max(1, keepdims=True))
    scores = (e / e.sum(1, keepdims=True))[:, :-1].reshape(-1)            # :493
    order = np.argsort(-scores, kind="stable")[:topk]                     # :497-498
    cls_score, labels, qidx = scores[order], order % K, order // K        # :499-501
    if thing_classes is not None:                                         # :506-513
        sel = np.isin(labels, sorted(thing_classes))
        cls_score, labels, qidx = cls_score[sel], labels[sel], qidx[sel]
    planes = mask_pred[qidx]                                              # :503
    masks = planes > 0                                                    # :517
    flat = masks.reshape(len(qidx), planes[0].size if len(qidx) else 0)
    mask_score = np.where(flat, _sigmoid64(planes).reshape(flat.shape), 0.0).sum(1) / (flat.sum(1) + 1e-6)   # :523-524
    return {"qidx": qidx.astype(np.int64), "classes": labels.astype(np.int64), "scores": cls_score * mask_score, "masks": masks, "boxes": boxes_of(masks)}


def reference_lines_fp32(mask_cls, mask_pred, topk, thing_classes=None):
    """the reference's lines :488-527 as it types them, fp32 torch ops on the tensors' device -> the same dictionary (torch tensors)"""
    num_classes, num_queries = mask_cls.shape[1] - 1, mask_cls.shape[0]
    scores = F.softmax(mask_cls, dim=-1)[:, :-1]
    labels = torch.arange(num_classes, device=mask_cls.device).unsqueeze(0).repeat(num_queries, 1).flatten(0, 1)
    scores_per_image, topk_indices = scores.flatten(0, 1).topk(topk, sorted=False)
    labels_per_image = labels[topk_indices]
    topk_indices = topk_indices // num_classes
    mask_pred = mask_pred[topk_indices]
    if thing_classes is not None:
        keep = torch.zeros_like(scores_per_image).bool()
        for i, lab in enumerate(labels_per_image):
            keep[i] = int(lab) in thing_classes
        scores_per_image, labels_per_image, mask_pred, topk_indices = scores_per_image[keep], labels_per_image[keep], mask_pred[keep], topk_indices[keep]
    pred_masks = (mask_pred > 0).float()
    mask_scores_per_image = (mask_pred.sigmoid().flatten(1) * pred_masks.flatten(1)).sum(1) / (pred_masks.flatten(1).sum(1) + 1e-6)
    return {"qidx": topk_indices, "classes": labels_per_image, "scores": scores_per_image * mask_scores_per_image, "masks": pred_masks}


def by_pair(qidx, classes):
    """{(query, class): position} -- the detections' identity; asserts that no pair appears twice"""
    pairs = [(int(q), int(c)) for q, c in zip(np.asarray(qidx).tolist(), np.asarray(classes).tolist())]
    assert len(set(pairs)) == len(pairs)
    return {p: i for i, p in enumerate(pairs)}


# ---------------------------------------------------------------------------------------------------------------- margins
def assert_logit_margin(x):
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    assert np.all((x == 0) | (np.abs(x) >= LOGIT)), "a logit closer to 0 than the margin"


def assert_topk_margin(mask_cls, topk):
    """-> the smallest relative gap between neighbours among the first topk + 1 descending scores"""
    s = np.sort(F.softmax(torch.as_tensor(mask_cls).double(), -1)[:, :-1].reshape(-1).numpy())[::-1]
    head = s[:topk + 1]
    gap = ((head[:-1] - head[1:]) / head[:-1]).min() if len(head) > 1 else float("inf")
    assert gap >= GAP, f"two neighbouring scores among the first {len(head)} are {gap:.3g} apart (relative), the margin is {GAP}"
    return gap


# ---------------------------------------------------------------------------------------------------------------- K17a / K17b fixtures
STATS_SHAPES = [(7, 9), (8, 12), (61, 93), (128, 256)]      # HW % 4 != 0: element loads / one tile / several tiles into one counter / several workgroups
STATS_QUERIES = [1, 5, 100]
KEEP_MODES = ["all", "three", "one"]
PLACED_SHAPE = (5, 36, 52)                                   # HW % 4 == 0: the 16-byte form with a head and a tail
UP4_CASES = [(5, 7, (18, 26)), (16, 24, (61, 93))]
UP4_Q = 12


def keep_of(mode, Q):
    keep = torch.zeros(Q, dtype=torch.bool)
    if mode == "all":
        keep[:] = True
    elif mode == "one":
        keep[Q // 2] = True
    else:                                                    # three of them, spread (fewer where Q has fewer)
        keep[[0, Q // 2, Q - 1]] = True
    return keep


def stats_case(Q, H, W, mode):
    """-> (mask [Q,H,W] on the 1/8 grid with a few exact zeros, keep bool [Q]), margin asserted"""
    g = torch.Generator().manual_seed(Q * 1000 + H)
    mask = grid_logits(g, (Q, H, W))
    mask[torch.rand((Q, H, W), generator=g) < 0.02] = 0.0    # exactly 0 is not > 0
    assert_logit_margin(mask.numpy())
    return mask, keep_of(mode, Q)


def special_case():
    """five kept planes at 13 x 22: 0 = nowhere positive, 1 = positive everywhere, 2 = NaN sprinkled over a grid plane, 3 = one positive pixel in the last
    row and column, 4 = large logits (sigmoid = 1 exactly)"""
    g = torch.Generator().manual_seed(17)
    mask = grid_logits(g, (5, 13, 22))
    mask[0] = -mask[0].abs()
    mask[1] = mask[1].abs()
    mask[2][torch.rand((13, 22), generator=g) < 0.2] = float("nan")
    mask[3] = -mask[3].abs()
    mask[3, 12, 21] = 0.125
    mask[4] = mask[4].sign() * 40.0
    assert_logit_margin(mask.numpy())
    return mask, torch.ones(5, dtype=torch.bool)


def up4_case(h, w, crop):
    """-> (mask_lowres [Q,h,w] on the 1/8 grid, keep, the fp64 x4 window [Q,crop_h,crop_w]); the window's margin asserted"""
    g = torch.Generator().manual_seed(h * 100 + w)
    low = grid_logits(g, (UP4_Q, h, w))
    up = upsample4_fp64(low)[:, :crop[0], :crop[1]]
    assert_logit_margin(up.numpy())
    assert torch.equal(up.float().double(), up), "the interpolated logits are exact in fp32"
    return low, keep_of("three", UP4_Q), up


# ---------------------------------------------------------------------------------------------------------------- instance_inference scenarios
SCENARIOS = {"cityscapes": dict(Q=100, K=19, topk=100, H=61, W=93, seed=4, things=frozenset(range(11, 19))),
             "small": dict(Q=16, K=8, topk=20, H=32, W=48, seed=2, things=frozenset({1, 4, 6}))}


def scenario(name):
    """-> (mask_cls [Q,K+1], mask_pred [Q,H,W], topk): class logits spread so that several classes of one query reach the top-k, masks on the 1/8 grid with
    some planes nowhere positive; both margins asserted"""
    s = SCENARIOS[name]
    g = torch.Generator().manual_seed(s["seed"])
    mask_cls = torch.randn(s["Q"], s["K"] + 1, generator=g) * 3
    mask_cls[::7, s["K"]] += 6.0                             # some queries predict void
    mask_pred = grid_logits(g, (s["Q"], s["H"], s["W"]))
    blob = torch.rand((s["Q"], 1, 1), generator=g)
    yy, xx = torch.meshgrid(torch.arange(s["H"]), torch.arange(s["W"]), indexing="ij")
    inside = ((yy[None] % 23) < 23 * blob) & ((xx[None] % 31) < 31 * blob)
    mask_pred = torch.where(inside, mask_pred.abs(), -mask_pred.abs())
    mask_pred[3::11] = -mask_pred[3::11].abs()               # empty masks: score 0, box zeros
    assert_logit_margin(mask_pred.numpy())
    assert_topk_margin(mask_cls, s["topk"])
    return mask_cls, mask_pred, s["topk"]
