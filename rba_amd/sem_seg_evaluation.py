"""Closed-set semantic-segmentation evaluation: Detectron2's ``SemSegEvaluator`` (detectron2/evaluation/sem_seg_evaluation.py, v0.6; the reference builds
it at train_net.py:96-121) with the confusion matrix kept on the device.

Detectron2 copies every argmax map to the host and runs ``np.bincount((K + 1) * pred + gt)`` there.  Here each (prediction, label) pair is ONE launch of
K13 (ops.confusion_accumulate) into an int64 [(K+1), (K+1)] matrix on the device; nothing is read back per image.  ``evaluate()`` sums the matrix
over the ranks with one all_reduce (distributed.pooled_confusion), reads it back once and computes the four metrics on the host in float64.

Detectron2 is not installed beside this library, so parity with its evaluator is by restating its definitions, not by running it (unpinned).
Cityscapes' own ``CityscapesSemSegEvaluator`` is cityscapesscripts' pixel-level evaluation: TP / (TP + FP + FN) over the non-ignored pixels, averaged
over the 19 classes -- the same number from the same matrix (IoU-<class> and mIoU below)."""
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .h2d import to_device

__all__ = ["SemSegEvaluator", "sem_seg_metrics"]


def sem_seg_metrics(conf, class_names=None) -> dict:
    """The summed confusion matrix C [(K+1), (K+1)] (rows = predictions, columns = ground truth, last column = ignored pixels) -> {"mIoU", "fwIoU",
    "mACC", "pACC", "IoU-<name>", "ACC-<name>"} in percent, float64, on the host.  Detectron2 v0.6's definitions, with M = C[:-1, :-1]:

        tp = diag(M), pos_gt = M.sum(axis=0), pos_pred = M.sum(axis=1), union = pos_gt + pos_pred - tp
        acc_valid = pos_gt > 0, iou_valid = (pos_gt + pos_pred) > 0
        acc = tp / pos_gt and iou = tp / union where acc_valid, NaN elsewhere
        mACC = sum(acc[acc_valid]) / #acc_valid          mIoU = sum(iou[acc_valid]) / #iou_valid
        fwIoU = sum(iou[acc_valid] * (pos_gt / sum(pos_gt))[acc_valid])          pACC = sum(tp) / sum(pos_gt)

    The v0.6 quirk is kept: a class that is predicted but never labelled counts in mIoU's denominator (iou_valid) and not in its numerator
    (acc_valid).  Whenever every class occurs in the labels -- Cityscapes val -- the two sets are equal and mIoU is the plain mean of the per-class
    IoUs, as in later versions."""
    C = conf.detach().cpu().numpy() if isinstance(conf, torch.Tensor) else np.asarray(conf)
    if C.ndim != 2 or C.shape[0] != C.shape[1] or C.shape[0] < 2:
        raise ValueError(f"conf must be a square [(K+1), (K+1)] matrix, got shape {C.shape}")
    K = C.shape[0] - 1
    names = list(class_names) if class_names is not None else [str(k) for k in range(K)]
    if len(names) != K:
        raise ValueError(f"{len(names)} class names for {K} classes")
    M = C[:-1, :-1].astype(np.float64)
    acc = np.full(K, np.nan, dtype=np.float64)
    iou = np.full(K, np.nan, dtype=np.float64)
    tp = M.diagonal().astype(np.float64)
    pos_gt = M.sum(axis=0)
    pos_pred = M.sum(axis=1)
    class_weights = pos_gt / np.sum(pos_gt)
    acc_valid = pos_gt > 0
    acc[acc_valid] = tp[acc_valid] / pos_gt[acc_valid]
    iou_valid = (pos_gt + pos_pred) > 0
    union = pos_gt + pos_pred - tp
    iou[acc_valid] = tp[acc_valid] / union[acc_valid]
    res = {"mIoU": 100 * np.sum(iou[acc_valid]) / np.sum(iou_valid),
           "fwIoU": 100 * np.sum(iou[acc_valid] * class_weights[acc_valid]),
           "mACC": 100 * np.sum(acc[acc_valid]) / np.sum(acc_valid),
           "pACC": 100 * np.sum(tp) / np.sum(pos_gt)}
    for i, name in enumerate(names):
        res[f"IoU-{name}"] = 100 * iou[i]
    for i, name in enumerate(names):
        res[f"ACC-{name}"] = 100 * acc[i]
    return {k: float(v) for k, v in res.items()}


class SemSegEvaluator:
    """Detectron2's SemSegEvaluator surface: ``reset()``, ``process(inputs, outputs)``, ``evaluate()``.

    ``lut``: a uint8 [256] table the labels are read through (Cityscapes raw ids -> trainIds: sem_seg_datasets.cityscapes_lut()).  ``device``: where
    the matrix lives (default: the current HIP device); there is no CPU path."""

    def __init__(self, num_classes, ignore_label=255, class_names=None, lut=None, device=None):
        self.num_classes = int(num_classes)
        if not 1 <= self.num_classes <= 255:
            raise ValueError(f"num_classes must be in 1..255, got {num_classes}")
        self.ignore_label = ignore_label
        self.class_names = list(class_names) if class_names is not None else [str(k) for k in range(self.num_classes)]
        if len(self.class_names) != self.num_classes:
            raise ValueError(f"{len(self.class_names)} class names for {self.num_classes} classes")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.lut = None if lut is None else torch.as_tensor(lut, dtype=torch.uint8).to(self.device).contiguous()
        n = self.num_classes + 1
        self._conf = torch.zeros((n, n), dtype=torch.int64, device=self.device)
        self._bad = torch.zeros(2, dtype=torch.int64, device=self.device)
        self.images = 0

    def reset(self):
        self._conf.zero_()
        self._bad.zero_()
        self.images = 0

    @property
    def confusion(self):
        """this rank's matrix so far, on the device (int64 [(K+1), (K+1)])"""
        return self._conf

    def process(self, inputs, outputs):
        """One output per input.  input: {"sem_seg": label map [H,W], uint8 or int64, host or device}; output: {"argmax": int32 [H,W]} (what
        MaskFormer.rba_scores(..., return_argmax=True) and the TTA wrapper give) or {"sem_seg": [K,H,W]} (argmax over dim 0, first maximum, as
        torch.argmax).  Evaluated at the label's size; nothing is read back."""
        if len(inputs) != len(outputs):
            raise ValueError(f"{len(inputs)} inputs but {len(outputs)} outputs")
        for inp, out in zip(inputs, outputs):
            if out.get("argmax") is not None:
                pred = out["argmax"]
            else:
                pred = out["sem_seg"].argmax(dim=0).to(torch.int32)
            gt = inp["sem_seg"]
            if not gt.is_cuda:
                gt = to_device(gt, self.device)
            ops.confusion_accumulate(pred.contiguous(), gt.contiguous(), self.num_classes, self._conf, self._bad, self.ignore_label, self.lut)
            self.images += 1

    def evaluate(self):
        """-> OrderedDict({"sem_seg": {...}}) with sem_seg_metrics' keys; every rank returns the same.  ``self.matrix`` is the summed matrix (numpy
        int64) afterwards.  Raises when a label or a prediction was out of range: the matrix would silently miss those pixels."""
        from . import distributed as D
        host = D.pooled_confusion_flat(self._conf, self._bad).cpu().numpy()         # the one all_reduce, the one read-back
        n = self.num_classes + 1
        self.matrix = host[:n * n].reshape(n, n).copy()
        bad_label, bad_pred = int(host[n * n]), int(host[n * n + 1])
        if bad_label or bad_pred:
            raise ValueError(f"SemSegEvaluator: {bad_label} pixel(s) with a label outside 0..{self.num_classes - 1} that is not the ignore label "
                             f"({self.ignore_label}), {bad_pred} pixel(s) with a prediction outside 0..{self.num_classes - 1}")
        return OrderedDict({"sem_seg": sem_seg_metrics(self.matrix, self.class_names)})
