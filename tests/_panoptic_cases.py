"""Fixtures and restatements for the K16 tests (docs/kernels/K16.md), all on the CPU so that every seed is checked without a device.

* `merge_reference`: K16a's per-pixel rule in numpy, fp64.
* `assert_margins`: the winner and `solid` are discrete decisions on fp32 values whose last bit differs between `exp` implementations, so every parity
  fixture proves in fp64, before a GPU is asked anything, that (a) the relative gap between each pixel's best and second-best product exceeds
  GAP = 1e-5 and (b) every kept logit is 0 exactly or at least LOGIT = 1e-3 away from 0.  With both held, equality is exact and no pixel is left out.
* the merge, up4 and model scenarios, built to satisfy the margins (logits on a 1/8 grid or block-valued, well-separated scores).
* `pq_reference`: the reference's PQ computation (mask2former/evaluation/evaluation.py:130-213, 252-280, 72-109) restated on sparse ids with
  dictionaries, independent of rba_amd.panoptic_evaluation, and the hand fixtures whose PQ is written down by hand.
"""
import numpy as np
import torch
import torch.nn.functional as F

GAP = 1e-5
LOGIT = 1e-3
NOBODY = 0xFF


# ---------------------------------------------------------------------------------------------------------------- K16a
def merge_reference(mask, score, keep):
    """mask [Q,...] logits, score [Q], keep [Q] bool -> (winner uint8 [...], counts int64 [3,Q]) in fp64"""
    mask = np.asarray(mask, dtype=np.float64)
    Q = mask.shape[0]
    flat = mask.reshape(Q, -1)
    keep = np.asarray(keep).astype(bool)
    s = 1.0 / (1.0 + np.exp(-flat))
    v = np.asarray(score, dtype=np.float64)[:, None] * s
    v[~keep] = -np.inf
    best = v.argmax(0)                                                   # the first maximum
    solid = s >= 0.5
    solid_best = solid[best, np.arange(flat.shape[1])]
    counts = np.zeros((3, Q), dtype=np.int64)
    counts[0] = np.bincount(best, minlength=Q)
    counts[1] = np.where(keep, solid.sum(1), 0)
    counts[2] = np.bincount(best[solid_best], minlength=Q)
    winner = np.where(solid_best, best, NOBODY).astype(np.uint8)
    return winner.reshape(mask.shape[1:]), counts


def assert_margins(mask, score, keep, twins=()):
    """the two decision margins, in fp64; `twins`: queries that duplicate a lower query on purpose (the tie case) and are left out of the gap"""
    mask = np.asarray(mask, dtype=np.float64)
    Q = mask.shape[0]
    flat = mask.reshape(Q, -1)
    keep = np.asarray(keep).astype(bool)
    x = flat[keep]
    assert np.all((x == 0) | (np.abs(x) >= LOGIT)), "a kept logit closer to 0 than the margin"
    compete = keep.copy()
    compete[list(twins)] = False
    v = np.asarray(score, dtype=np.float64)[compete, None] / (1.0 + np.exp(-flat[compete]))
    if v.shape[0] >= 2:
        top = np.sort(v, axis=0)[-2:]
        gap = (top[1] - top[0]) / top[1]
        assert gap.min() > GAP, f"best and second-best product {gap.min():.3g} apart (relative), the margin is {GAP}"


def grid_logits(g, shape):
    """non-zero multiples of 1/8 in [-5, 5]"""
    k = torch.randint(1, 41, shape, generator=g)
    sign = torch.randint(0, 2, shape, generator=g) * 2 - 1
    return (k * sign).float() / 8


def keep_of(mode, Q):
    keep = torch.zeros(Q, dtype=torch.bool)
    if mode == "all":
        keep[:] = True
    elif mode == "one":
        keep[Q // 2] = True
    else:                                                                # alternating
        keep[(1 if Q > 1 else 0)::2] = True
    return keep


MERGE_SHAPES = [(1, 1, 1), (3, 5, 7), (16, 37, 53), (100, 64, 96), (255, 33, 65)]
KEEP_MODES = ["all", "one", "alternating"]
PLACED_SHAPE = (7, 36, 52)                                              # HW % 4 == 0: the 16-byte form with a head and a tail, two workgroups
MERGE_SEEDS = {(100, 64, 96, "all"): 3}                               # where the default seed Q * 1000 + H fails the margins (checked on the CPU)


def merge_case(Q, H, W, mode):
    """-> (mask [Q,H,W], score [Q], keep bool [Q]) fp32 on the CPU, margins asserted"""
    g = torch.Generator().manual_seed(MERGE_SEEDS.get((Q, H, W, mode), Q * 1000 + H))
    mask = grid_logits(g, (Q, H, W))
    score = 0.3 + 0.7 * torch.rand(Q, generator=g)
    keep = keep_of(mode, Q)
    assert_margins(mask.numpy(), score.numpy(), keep.numpy())
    return mask, score, keep


def never_solid_case():
    """the one kept query is below 0.5 everywhere: it wins every pixel and owns none"""
    g = torch.Generator().manual_seed(5)
    mask = grid_logits(g, (4, 9, 11))
    mask[2] = -mask[2].abs()
    score = torch.tensor([0.9, 0.8, 0.7, 0.6])
    keep = torch.tensor([False, False, True, False])
    assert_margins(mask.numpy(), score.numpy(), keep.numpy())
    return mask, score, keep


def tie_case():
    """queries 1 and 3 have the same score and the same plane, which is the best wherever it is positive: the lower q must win"""
    g = torch.Generator().manual_seed(6)
    mask = grid_logits(g, (5, 12, 10))
    mask[1] = mask[1].abs() + 5.0
    mask[1, :, :3] = -4.0
    mask[3] = mask[1]
    score = torch.tensor([0.5, 0.95, 0.6, 0.95, 0.4])
    keep = torch.ones(5, dtype=torch.bool)
    assert_margins(mask.numpy(), score.numpy(), keep.numpy(), twins=(3,))
    return mask, score, keep


def upsample4_fp64(low):
    return F.interpolate(low.double()[None], scale_factor=4, mode="bilinear", align_corners=False)[0]


UP4_CASES = [(9, 13, (35, 50)), (24, 40, (96, 160)), (2, 3, (8, 12))]
UP4_Q = 12


def up4_case(h, w, crop):
    """-> (mask_lowres [Q,h,w] on the 1/8 grid -- its x4 interpolation is exact in fp32 --, score, keep); margins asserted on the fp64 up-sampled window"""
    g = torch.Generator().manual_seed(h * 100 + w)
    low = grid_logits(g, (UP4_Q, h, w))
    score = 0.3 + 0.7 * torch.rand(UP4_Q, generator=g)
    keep = keep_of("alternating", UP4_Q)
    up = upsample4_fp64(low)[:, :crop[0], :crop[1]]
    assert_margins(up.numpy(), score.numpy(), keep.numpy())
    return low, score, keep


# ---------------------------------------------------------------------------------------------------------------- MaskFormer.panoptic_inference scenarios
THING_CLASSES = frozenset(range(11, 19))                                 # Cityscapes: 0..10 stuff, 11..18 things
OBJECT_MASK_THRESHOLD, OVERLAP_THRESHOLD = 0.5, 0.6


def _class_logits(Q, K, classes, g):
    """[Q,K+1] logits: query q < len(classes) prefers classes[q] with a score of its own (well separated), the rest predict void"""
    mask_cls = torch.randn(Q, K + 1, generator=g)
    mask_cls[:, K] -= 2.0
    for q, c in enumerate(classes):
        mask_cls[q, c] += 6.0 + 0.45 * (q % 9) + 0.04 * q
    mask_cls[len(classes):, K] += 9.0
    return mask_cls


def _model_margins(mask_cls, mask_pred):
    K = mask_cls.shape[-1] - 1
    prob = F.softmax(mask_cls.double(), -1)
    scores, labels = prob.max(-1)
    keep = labels.ne(K) & (scores > OBJECT_MASK_THRESHOLD)
    assert_margins(mask_pred.numpy(), scores.numpy(), keep.numpy())
    return int(keep.sum())


def box_scenario(H=61, W=93):
    """the scenario of tests/test_model_gpu.py::test_open_panoptic_inference_vs_oracle at 61 x 93: eight overlapping boxes, two "stuff" queries of class 3,
    a band on the right that stays unclaimed.  Block-valued logits (5 - 0.3 q inside, -6 - 0.25 q outside, +- 1/8 steps) instead of Gaussian noise, so
    that the margins hold on every pixel.  Query 5 loses most of its box to query 6, whose score is higher (dropped by the overlap threshold); query 7 is >= 0.5
    only where a stronger query wins, and wins (below 0.5) a strip nobody else wants: won area > 0, intersection 0."""
    g = torch.Generator().manual_seed(13)
    Q, K = 16, 19
    classes = [3, 3, 11, 12, 0, 13, 8, 11]
    mask_cls = _class_logits(Q, K, classes, g)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    q_ = torch.arange(Q).float().view(Q, 1, 1)
    mask_pred = (-6.0 - 0.25 * q_).expand(Q, H, W).clone()
    for q in range(6):
        y0, x0 = 7 * q, 12 * q
        inside = (yy >= y0) & (yy < y0 + 22) & (xx >= x0) & (xx < x0 + 20)
        mask_pred[q][inside] = 5.0 - 0.3 * q
    inside6 = (yy >= 37) & (yy < 57) & (xx >= 62) & (xx < 84)             # over most of query 5 (rows 35..56, columns 60..79)
    mask_pred[6][inside6] = 5.0 - 0.3 * 6
    mask_pred[7][(yy >= 40) & (yy < 50) & (xx >= 62) & (xx < 75)] = 2.0  # >= 0.5 only where query 6 is stronger
    mask_pred[7][(yy >= 58) & (xx < 40)] = -1.0                          # wins a strip below the boxes without being >= 0.5
    mask_pred += torch.randint(-1, 2, (Q, H, W), generator=g).float() / 8
    kept = _model_margins(mask_cls, mask_pred)
    assert kept == len(classes)
    return mask_cls, mask_pred


def many_query_scenario(H=48, W=80, Q=100, kept=40):
    """Q = 100 queries of which 40 are kept: a 5 x 8 grid of cells, one kept query each, every cell overlapped by its right neighbour"""
    g = torch.Generator().manual_seed(101)
    K = 19
    classes = [(3 * q) % 19 for q in range(kept)]
    mask_cls = _class_logits(Q, K, classes, g)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    q_ = torch.arange(Q).float().view(Q, 1, 1)
    mask_pred = (-6.0 - 0.125 * q_).expand(Q, H, W).clone()
    ch, cw = H // 5, W // 8
    for q in range(kept):
        cy, cx = divmod(q, 8)
        inside = (yy >= cy * ch) & (yy < (cy + 1) * ch) & (xx >= cx * cw) & (xx < (cx + 1) * cw + 4)
        mask_pred[q][inside] = 6.0 - 0.1 * q
    mask_pred += torch.randint(-1, 2, (Q, H, W), generator=g).float() / 16
    assert _model_margins(mask_cls, mask_pred) == kept
    return mask_cls, mask_pred


# ---------------------------------------------------------------------------------------------------------------- K16c
def pair_counts_reference(gt, pred, G, P):
    """np.unique pair counts on dense ids -> (counts int64 [G,P], pixels with an id out of range)"""
    gt, pred = np.asarray(gt).reshape(-1).astype(np.int64), np.asarray(pred).reshape(-1).astype(np.int64)
    ok = (gt >= 0) & (gt < G) & (pred >= 0) & (pred < P)
    keys, cnt = np.unique(gt[ok] * P + pred[ok], return_counts=True)
    out = np.zeros(G * P, dtype=np.int64)
    out[keys] = cnt
    return out.reshape(G, P), int((~ok).sum())


def pair_maps(kind, n, G, P, seed):
    """-> (gt, pred) int32 numpy of n pixels"""
    rng = np.random.default_rng(seed)
    if kind == "single":
        return np.full(n, G - 1, np.int32), np.full(n, P - 1, np.int32)
    gt, pred = rng.integers(0, G, n).astype(np.int32), rng.integers(0, P, n).astype(np.int32)
    if kind == "out_of_range":
        where = rng.random(n) < 0.1
        gt[where & (rng.random(n) < 0.5)] = G
        pred[where & (rng.random(n) < 0.3)] = -1
        pred[where & (rng.random(n) < 0.3)] = P + 5
        gt[where & (rng.random(n) < 0.1)] = -7
    return gt, pred


# ---------------------------------------------------------------------------------------------------------------- PQ
OFFSET = 256 * 256 * 256
CATEGORIES = [{"id": 1, "name": "car", "isthing": 1, "supercategory": "vehicle"}, {"id": 2, "name": "road", "isthing": 0, "supercategory": "flat"},
              {"id": 3, "name": "dog", "isthing": 1, "supercategory": "animal"}, {"id": 4, "name": "sky", "isthing": 0, "supercategory": "sky"}]
UNKNOWN_NAMES = ["dog"]


def pq_reference(images, categories=CATEGORIES, unknown_names=UNKNOWN_NAMES):
    """images: [(pan_pred, segments_info, pan_gt, gt_segments_info)] -> (results in pq_compute's layout, {label: [iou, tp, fp, fn]})"""
    cats = {}
    unknown_ids = []
    for c in categories:
        c = dict(c)
        if unknown_names is not None and c["name"] in unknown_names:
            unknown_ids.append(c["id"])
            c.update(id=-c["id"] - 1, name="unknown_" + c["name"], supercategory="unknown_" + c["supercategory"])
        cats[c["id"]] = c
    if unknown_names is not None:
        cats[255] = {"supercategory": "unknown", "isthing": 1, "id": 255, "name": "unknown"}
    stat = {}

    def st(label):
        return stat.setdefault(label, [0.0, 0, 0, 0])

    for pan_pred, segments_info, pan_gt, gt_segments_info in images:
        pan_pred, pan_gt = np.asarray(pan_pred).astype(np.uint64), np.asarray(pan_gt).astype(np.uint64)
        gts = {}
        for s in gt_segments_info:
            s = dict(s)
            if s["category_id"] in unknown_ids:
                s["original_category_id"] = -s["category_id"] - 1
                s["category_id"] = 255
            gts[s["id"]] = s
        preds = {s["id"]: dict(s) for s in segments_info}
        for label, cnt in zip(*np.unique(pan_pred, return_counts=True)):
            if int(label) in preds:
                preds[int(label)]["area"] = int(cnt)
        for label, cnt in zip(*np.unique(pan_gt, return_counts=True)):
            if int(label) in gts:
                gts[int(label)]["area"] = int(cnt)
        pairs = {(int(k) // OFFSET, int(k) % OFFSET): int(c) for k, c in zip(*np.unique(pan_gt * np.uint64(OFFSET) + pan_pred, return_counts=True))}
        gt_done, pred_done = set(), set()
        for (gl, pl), inter in pairs.items():
            if gl not in gts or pl not in preds or gts[gl].get("iscrowd", 0) == 1 or gts[gl]["category_id"] != preds[pl]["category_id"]:
                continue
            iou = inter / (preds[pl]["area"] + gts[gl]["area"] - inter - pairs.get((0, pl), 0))
            if iou > 0.5:
                for label in [gts[gl]["category_id"]] + ([gts[gl]["original_category_id"]] if "original_category_id" in gts[gl] else []):
                    st(label)[1] += 1
                    st(label)[0] += iou
                gt_done.add(gl)
                pred_done.add(pl)
        crowd = {}
        for gl, s in gts.items():
            if gl in gt_done:
                continue
            if s.get("iscrowd", 0) == 1:
                crowd[s["category_id"]] = gl
                continue
            st(s["category_id"])[3] += 1
            if "original_category_id" in s:
                st(s["original_category_id"])[3] += 1
        for pl, s in preds.items():
            if pl in pred_done:
                continue
            ignored = pairs.get((0, pl), 0) + (pairs.get((crowd[s["category_id"]], pl), 0) if s["category_id"] in crowd else 0)
            if ignored / s["area"] > 0.5:
                continue
            st(s["category_id"])[2] += 1

    def average(select):
        rows, per_class = [], {}
        for label, c in cats.items():
            if not select(c):
                continue
            iou, tp, fp, fn = st(label)
            if tp + fp + fn == 0:
                per_class[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
                continue
            per_class[label] = {"pq": iou / (tp + 0.5 * fp + 0.5 * fn), "sq": iou / tp if tp else 0, "rq": tp / (tp + 0.5 * fp + 0.5 * fn)}
            rows.append(per_class[label])
        n = len(rows)
        if n == 0:
            return {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}, per_class
        return {k: sum(r[k] for r in rows) / n for k in ("pq", "sq", "rq")} | {"n": n}, per_class

    results = {}
    results["All"], results["per_class"] = average(lambda c: c["id"] >= 0 and c["id"] != 255)
    results["Known Things"], _ = average(lambda c: c["isthing"] == 1 and c["id"] > -1 and c["id"] != 255)
    results["Unknown Things"], _ = average(lambda c: c["isthing"] == 1 and c["id"] == 255)
    results["Stuff"], _ = average(lambda c: c["isthing"] != 1 and c["id"] >= -1)
    return results, stat


def _img(rows):
    return np.array(rows, dtype=np.int32)


ZERO = {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}

# Hand fixtures on 4 x 4 images: name -> (images, the rows of evaluate() written down by hand, {label: (tp, fp, fn)}).
HAND = {
    # both segments match exactly: IoU 1 for car (1) and road (2); sky (4) is untouched: tp + fp + fn = 0, listed with zeros and not averaged
    "perfect": ([(_img([[1, 1, 2, 2]] * 4), [{"id": 1, "category_id": 1}, {"id": 2, "category_id": 2}],
                  _img([[1000, 1000, 2000, 2000]] * 4), [{"id": 1000, "category_id": 1, "iscrowd": 0}, {"id": 2000, "category_id": 2, "iscrowd": 0}])],
                {"All": {"pq": 1.0, "sq": 1.0, "rq": 1.0, "n": 2}, "Known Things": {"pq": 1.0, "sq": 1.0, "rq": 1.0, "n": 1}, "Unknown Things": ZERO,
                 "Stuff": {"pq": 1.0, "sq": 1.0, "rq": 1.0, "n": 1},
                 "per_class": {1: {"pq": 1.0, "sq": 1.0, "rq": 1.0}, 2: {"pq": 1.0, "sq": 1.0, "rq": 1.0}, 4: {"pq": 0.0, "sq": 0.0, "rq": 0.0}}},
                {1: (1, 0, 0), 2: (1, 0, 0)}),
    # a car of 4 pixels, a prediction on 2 of them: IoU = 2 / (2 + 4 - 2) = 0.5 exactly, which is NOT a match: one fn and one fp
    "iou_half": ([(_img([[1, 1, 0, 0], [0] * 4, [0] * 4, [0] * 4]), [{"id": 1, "category_id": 1}],
                   _img([[7, 7, 7, 7], [0] * 4, [0] * 4, [0] * 4]), [{"id": 7, "category_id": 1, "iscrowd": 0}])],
                 {"All": {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 1}, "Known Things": {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 1}, "Unknown Things": ZERO, "Stuff": ZERO,
                  "per_class": {1: {"pq": 0.0, "sq": 0, "rq": 0.0}, 2: {"pq": 0.0, "sq": 0.0, "rq": 0.0}, 4: {"pq": 0.0, "sq": 0.0, "rq": 0.0}}},
                 {1: (0, 1, 1)}),
    # row 0: a CROWD car region; prediction 1 (car) lies 3/4 in it: ignored.  Row 1: road, prediction 2 covers 3 of its 4 pixels: IoU 3 / 4, a match.
    # Row 2: unlabelled; prediction 3 (car) lies wholly in VOID: ignored.  Cars end with tp + fp + fn = 0.
    "void_and_crowd": ([(_img([[1, 1, 1, 0], [1, 2, 2, 2], [3, 3, 3, 3], [0] * 4]),
                         [{"id": 1, "category_id": 1}, {"id": 2, "category_id": 2}, {"id": 3, "category_id": 1}],
                         _img([[5] * 4, [6] * 4, [0] * 4, [0] * 4]), [{"id": 5, "category_id": 1, "iscrowd": 1}, {"id": 6, "category_id": 2, "iscrowd": 0}])],
                       {"All": {"pq": 0.75, "sq": 0.75, "rq": 1.0, "n": 1}, "Known Things": ZERO, "Unknown Things": ZERO,
                        "Stuff": {"pq": 0.75, "sq": 0.75, "rq": 1.0, "n": 1},
                        "per_class": {1: {"pq": 0.0, "sq": 0.0, "rq": 0.0}, 2: {"pq": 0.75, "sq": 0.75, "rq": 1.0}, 4: {"pq": 0.0, "sq": 0.0, "rq": 0.0}}},
                       {2: (1, 0, 0)}),
    # two dogs (a held-out category: 255 with original_category_id -4).  The open-set prediction covers 6 of the first dog's 8 pixels: IoU 6 / 8, counted
    # for 255 AND for -4; the second dog is missed: fn for both.  Unknown Things: pq = 0.75 / (1 + 0.5) = 0.5, sq = 0.75, rq = 1 / 1.5.
    "unknown": ([(_img([[1, 1, 1, 0], [1, 1, 1, 0], [0] * 4, [0] * 4]), [{"id": 1, "category_id": 255}],
                  _img([[9] * 4, [9] * 4, [0] * 4, [10] * 4]), [{"id": 9, "category_id": 3, "iscrowd": 0}, {"id": 10, "category_id": 3, "iscrowd": 0}])],
                {"All": ZERO, "Known Things": ZERO, "Unknown Things": {"pq": 0.5, "sq": 0.75, "rq": 1 / 1.5, "n": 1}, "Stuff": ZERO,
                 "per_class": {1: {"pq": 0.0, "sq": 0.0, "rq": 0.0}, 2: {"pq": 0.0, "sq": 0.0, "rq": 0.0}, 4: {"pq": 0.0, "sq": 0.0, "rq": 0.0}}},
                {255: (1, 0, 1), -4: (1, 0, 1)}),
}


def synthetic_ground_truth(shape, seed):
    """a 3 x 3 grid of ground-truth cells with RGB-coded (sparse) ids over `shape` -> (pan_gt int64 [H,W], gt_segments_info); cell 4 is unlabelled, cell 8
    a crowd region, two cells are dogs (held out)"""
    H, W = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    cell = (yy * 3 // H) * 3 + xx * 3 // W
    cats = [1, 2, 3, 4, None, 1, 3, 2, 1]
    ids = rng.choice(np.arange(1000, OFFSET - 1), size=9, replace=False)
    pan_gt = np.zeros(shape, dtype=np.int64)
    info = []
    for c in range(9):
        if cats[c] is None:
            continue
        pan_gt[cell == c] = ids[c]
        info.append({"id": int(ids[c]), "category_id": cats[c], "iscrowd": int(c == 8)})
    return pan_gt, info
