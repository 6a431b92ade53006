"""Open-set panoptic quality: PQ / SQ / RQ over "All", "Known Things", "Unknown Things" and "Stuff" -- the rows the reference publishes.

Restates, on arrays instead of PNG / JSON files, mask2former/evaluation/evaluation.py: the category rewrite of ``pq_compute`` (:252-280), the per-image
matching of ``pq_compute_single_core`` (:130-213) and ``PQStat.pq_average`` (:72-109), which coco_panoptic_open_evaluator.py drives.  The one heavy
step, the segment-pair counts ``np.unique(pan_gt * OFFSET + pan_pred, return_counts=True)`` (:152-159), runs on the device (K16c,
docs/kernels/K16.md) on dense ids: one launch and one read-back of a [G,P] matrix per image; without a device the same class counts the pairs with
np.unique on the host.  Everything behind the matrix -- matching, TP / FP / FN, IoU sums -- is host arithmetic on Python numbers in the reference's
order, so both paths give the same statistics bit for bit.

File formats (COCO JSON, panopticapi PNGs), dataset readers and a command line are not part of this module."""
import numpy as np
import torch

from . import panoptic_ops

VOID = 0                      # panopticapi's id of unlabelled pixels
UNKNOWN_ID = 255              # the category every unknown ground-truth segment and every open-set prediction carries
METRICS = (("All", None, None), ("Known Things", True, False), ("Unknown Things", True, True), ("Stuff", False, None))      # evaluation.py:309-310


class PQStatCat:
    """evaluation.py:41-53"""
    __slots__ = ("iou", "tp", "fp", "fn")

    def __init__(self):
        self.iou, self.tp, self.fp, self.fn = 0.0, 0, 0, 0

    def __iadd__(self, other):
        self.iou += other.iou
        self.tp += other.tp
        self.fp += other.fp
        self.fn += other.fn
        return self


class PQStat:
    """evaluation.py:56-109"""

    def __init__(self):
        self.pq_per_cat = {}

    def __getitem__(self, label):
        if label not in self.pq_per_cat:
            self.pq_per_cat[label] = PQStatCat()
        return self.pq_per_cat[label]

    def __iadd__(self, other):
        for label, cat in other.pq_per_cat.items():
            mine = self[label]
            mine += cat
        return self

    def as_ints(self):
        """{label: (tp, fp, fn)} of the categories that were touched"""
        return {label: (c.tp, c.fp, c.fn) for label, c in self.pq_per_cat.items()}

    def pq_average(self, categories, isthing, isunknown):
        """:72-109.  categories: the rewritten {label: info}; (isthing, isunknown) selects a row of METRICS."""
        pq = sq = rq = 0
        n = 0
        per_class = {}
        for label, info in categories.items():
            cid = info["id"]
            if isthing is None:                                  # "All": the known categories
                if cid < 0 or cid == UNKNOWN_ID:
                    continue
            else:
                if isthing != (info["isthing"] == 1):
                    continue
                if isunknown is None:
                    if cid < -1:
                        continue
                elif isunknown:
                    if cid != UNKNOWN_ID:
                        continue
                elif cid <= -1 or cid == UNKNOWN_ID:
                    continue
            c = self[label]
            if c.tp + c.fp + c.fn == 0:
                per_class[label] = {"pq": 0.0, "sq": 0.0, "rq": 0.0}
                continue
            denominator = c.tp + 0.5 * c.fp + 0.5 * c.fn
            pq_c = c.iou / denominator
            sq_c = c.iou / c.tp if c.tp != 0 else 0
            rq_c = c.tp / denominator
            per_class[label] = {"pq": pq_c, "sq": sq_c, "rq": rq_c}
            n += 1
            pq += pq_c
            sq += sq_c
            rq += rq_c
        if n == 0:
            return {"pq": 0.0, "sq": 0.0, "rq": 0.0, "n": 0}, per_class
        return {"pq": pq / n, "sq": sq / n, "rq": rq / n, "n": n}, per_class


def rewrite_categories(categories, unknown_label_list):
    """:252-274 -> ({label: info}, the ids of the categories named in unknown_label_list).  A category named there moves to label -id - 1 as
    "unknown_<name>", and the one open-set category 255 ("unknown", a thing) is appended; None leaves the categories as they are."""
    by_id = {c["id"]: dict(c) for c in categories}
    if unknown_label_list is None:
        return by_id, ()
    out, unknown_ids = {}, []
    for cid, c in by_id.items():
        if c["name"] not in unknown_label_list:
            out[cid] = c
            continue
        unknown_ids.append(cid)
        c["supercategory"] = "unknown_" + str(c.get("supercategory", ""))
        c["id"] = -cid - 1
        c["name"] = "unknown_" + c["name"]
        out[-cid - 1] = c
    out[UNKNOWN_ID] = {"supercategory": "unknown", "isthing": 1, "id": UNKNOWN_ID, "name": "unknown"}
    return out, tuple(unknown_ids)


def _host_array(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def dense_ground_truth(pan_gt):
    """The sparse (RGB-coded) ground-truth ids -> (ids, dense int32 map): one np.unique(return_inverse=True); ids[0] is VOID whether or not the image
    has unlabelled pixels, so row 0 of the pair matrix is always the VOID row."""
    gt = _host_array(pan_gt)
    ids, dense = np.unique(gt.reshape(-1), return_inverse=True)
    if ids[0] < VOID:
        raise ValueError(f"ground-truth segment ids must be non-negative, got {int(ids[0])}")
    dense = dense.astype(np.int32).reshape(gt.shape)
    if ids[0] != VOID:
        ids = np.concatenate([np.array([VOID], dtype=ids.dtype), ids])
        dense += 1
    return ids, dense


def pair_matrix_host(dense_gt, pan_pred, G, P):
    """The [G,P] pair counts with np.unique on the host (:152-159) -> (matrix int64, the number of pixels whose prediction id is outside 0..P-1)."""
    pred = _host_array(pan_pred).astype(np.int64).reshape(-1)
    inside = (pred >= 0) & (pred < P)
    keys, cnt = np.unique(dense_gt.reshape(-1).astype(np.int64)[inside] * P + pred[inside], return_counts=True)
    matrix = np.zeros(G * P, dtype=np.int64)
    matrix[keys] = cnt
    return matrix.reshape(G, P), int(pred.size - int(inside.sum()))


def pair_matrix_device(dense_gt, pan_pred, G, P, device):
    """The same through K16c: one launch, one read-back of the matrix with its bad counter behind it."""
    gt = torch.from_numpy(np.ascontiguousarray(dense_gt)).to(device)
    pred = pan_pred if isinstance(pan_pred, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(_host_array(pan_pred)))
    pred = pred.to(device=device, dtype=torch.int32).contiguous()
    buf = torch.zeros(G * P + 1, dtype=torch.int64, device=device)
    panoptic_ops.segment_pairs(gt, pred, G, P, buf[:G * P].view(G, P), buf[G * P:])
    host = buf.cpu().numpy()
    return host[:G * P].reshape(G, P), int(host[G * P])


class PanopticOpenEvaluator:
    """categories: [{"id", "name", "isthing"[, "supercategory"]}] as in a panoptic ground-truth file; unknown_label_list: the names of the categories held
    out as unknown (None: closed-set PQ); device: where K16c runs (None: the pair counts are made on the host)."""

    def __init__(self, categories, unknown_label_list=None, device=None):
        self.categories, self.unknown_category_ids = rewrite_categories(categories, unknown_label_list)
        self.device = None if device is None else torch.device(device)
        self.pq_stat = PQStat()
        self.images = 0

    def reset(self):
        self.pq_stat = PQStat()
        self.images = 0

    def __iadd__(self, other):
        """pool another evaluator's statistics (another rank's share of the images)"""
        self.pq_stat += other.pq_stat
        self.images += other.images
        return self

    def _gt_segments(self, gt_segments_info):
        """:275-280: a segment of a held-out category becomes category 255 and remembers where it came from"""
        out = {}
        for seg in gt_segments_info:
            seg = dict(seg)
            if seg["category_id"] in self.unknown_category_ids:
                seg["original_category_id"] = -seg["category_id"] - 1
                seg["category_id"] = UNKNOWN_ID
            out[int(seg["id"])] = seg
        return out

    def process(self, pan_pred, segments_info, pan_gt, gt_segments_info):
        """One image.  pan_pred [H,W]: dense segment ids (0 = VOID) as MaskFormer.panoptic_inference gives them, with its segments_info; pan_gt [H,W]: the
        ground truth's ids (sparse, 0 = VOID) with gt_segments_info = [{"id", "category_id"[, "iscrowd"]}].  Arrays or tensors."""
        if tuple(pan_pred.shape) != tuple(pan_gt.shape):
            raise ValueError(f"pan_pred {tuple(pan_pred.shape)} and pan_gt {tuple(pan_gt.shape)} must have the same shape")
        gt_ids, dense_gt = dense_ground_truth(pan_gt)
        pred_segms = {int(s["id"]): dict(s) for s in segments_info}
        if any(i <= VOID for i in pred_segms):
            raise KeyError(f"predicted segment ids must be positive, got {sorted(pred_segms)}")
        G, P = len(gt_ids), max(pred_segms, default=VOID) + 1
        if self.device is None:
            matrix, bad = pair_matrix_host(dense_gt, pan_pred, G, P)
        else:
            matrix, bad = pair_matrix_device(dense_gt, pan_pred, G, P, self.device)
        if bad:
            raise KeyError(f"{bad} pixels of pan_pred carry an id outside 0..{P - 1}: a segment that is in the map and not in segments_info (:137-141)")
        self._match(matrix.tolist(), [int(i) for i in gt_ids], self._gt_segments(gt_segments_info), pred_segms)
        self.images += 1

    def _match(self, matrix, gt_ids, gt_segms, pred_segms):
        """:133-213 on the pair counts: matrix[g][p] = pixels with ground-truth id gt_ids[g] and predicted id p; row 0 is VOID."""
        pq_stat = self.pq_stat
        P = len(matrix[0])
        gt_area = [sum(row) for row in matrix]
        pred_area = [sum(row[p] for row in matrix) for p in range(P)]
        # predicted segments: area and sanity checks (:133-149)
        for p in range(1, P):
            if pred_area[p] and p not in pred_segms:
                raise KeyError(f"segment {p} is in the predicted map and not in segments_info")
        for p, seg in pred_segms.items():
            if pred_area[p] == 0:
                raise KeyError(f"segment {p} is in segments_info and not in the predicted map")
            if seg["category_id"] not in self.categories:
                raise KeyError(f"segment {p} has unknown category_id {seg['category_id']}")
        # matched pairs (:161-186), in ascending (ground-truth id, predicted id) order as np.unique gives them
        gt_matched, pred_matched = set(), set()
        for g, row in enumerate(matrix):
            gt_seg = gt_segms.get(gt_ids[g])
            if gt_seg is None or gt_seg.get("iscrowd", 0) == 1:
                continue
            for p, intersection in enumerate(row):
                if intersection == 0 or p not in pred_segms or gt_seg["category_id"] != pred_segms[p]["category_id"]:
                    continue
                union = pred_area[p] + gt_area[g] - intersection - matrix[0][p]
                iou = intersection / union
                if iou > 0.5:
                    pq_stat[gt_seg["category_id"]].tp += 1
                    pq_stat[gt_seg["category_id"]].iou += iou
                    if "original_category_id" in gt_seg:
                        pq_stat[gt_seg["original_category_id"]].tp += 1
                        pq_stat[gt_seg["original_category_id"]].iou += iou
                    gt_matched.add(gt_ids[g])
                    pred_matched.add(p)
        # false negatives (:187-198); crowd segments are ignored and remembered per category
        row_of = {label: g for g, label in enumerate(gt_ids)}
        crowd_row = {}
        for label, gt_seg in gt_segms.items():
            if label in gt_matched:
                continue
            if gt_seg.get("iscrowd", 0) == 1:
                crowd_row[gt_seg["category_id"]] = row_of.get(label)
                continue
            pq_stat[gt_seg["category_id"]].fn += 1
            if "original_category_id" in gt_seg:
                pq_stat[gt_seg["original_category_id"]].fn += 1
        # false positives (:200-213): a prediction more than half inside VOID and its category's crowd region is ignored
        for p, seg in pred_segms.items():
            if p in pred_matched:
                continue
            intersection = matrix[0][p]
            g = crowd_row.get(seg["category_id"])
            if g is not None:
                intersection += matrix[g][p]
            if intersection / pred_area[p] > 0.5:
                continue
            pq_stat[seg["category_id"]].fp += 1

    def evaluate(self):
        """{"All", "Known Things", "Unknown Things", "Stuff": {"pq", "sq", "rq", "n"}, "per_class": {label: {"pq", "sq", "rq"}} of the "All" row} (:309-317)"""
        results = {}
        for name, isthing, isunknown in METRICS:
            results[name], per_class = self.pq_stat.pq_average(self.categories, isthing, isunknown)
            if name == "All":
                results["per_class"] = per_class
        return results
