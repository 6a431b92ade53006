"""Closed-set segmentation datasets: the Cityscapes reader behind ``python -m rba_amd.evaluate_semseg`` (layout of the reference's
datasets/cityscapes.py:76-106):

    <root>/leftImg8bit/<split>/<city>/<stem>_leftImg8bit.png
    <root>/gtFine/<split>/<city>/<stem>_gtFine_labelTrainIds.png      (made by cityscapesscripts' createTrainIdLabelImgs), or
    <root>/gtFine/<split>/<city>/<stem>_gtFine_labelIds.png           (the raw ids the dataset ships with)

With the raw-id PNGs the reader hands out the ids as they are together with ``dataset.lut``, the 256-entry id -> trainId table: the evaluator gives
it to K13 (ops.confusion_accumulate), so the labels need no preprocessing pass.  Cities and files are sorted.

This reader is NOT one of ``rba_amd.datasets``' OoD benchmarks: ``datasets.get_dataset("cityscapes", ...)`` keeps raising KeyError and the OoD
command line does not list it.  Items have the OoD readers' two forms, so ``datasets.prefetch(..., raw=True)`` drives it."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from .datasets import _to_item, _to_raw_item, read_image, read_label

__all__ = ["CITYSCAPES_CLASSES", "CITYSCAPES_ID_TO_TRAINID", "CityscapesSemSeg", "cityscapes_lut"]

# the 19 train classes, trainId order (cityscapesscripts' labels.py)
CITYSCAPES_CLASSES = ["road", "sidewalk", "building", "wall", "fence", "pole", "traffic light", "traffic sign", "vegetation", "terrain", "sky",
                      "person", "rider", "car", "truck", "bus", "train", "motorcycle", "bicycle"]

# id 0..33 -> trainId (cityscapesscripts' labels.py); 255 = ignored in evaluation
CITYSCAPES_ID_TO_TRAINID = [255, 255, 255, 255, 255, 255, 255, 0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15,
                            255, 255, 16, 17, 18]
IGNORE_LABEL = 255


def cityscapes_lut():
    """uint8 [256]: id -> trainId for ids 0..33, 255 (ignore) for every other byte"""
    lut = np.full(256, IGNORE_LABEL, dtype=np.uint8)
    lut[:len(CITYSCAPES_ID_TO_TRAINID)] = CITYSCAPES_ID_TO_TRAINID
    return torch.from_numpy(lut)


class CityscapesSemSeg(Dataset):
    """``labels``: "trainIds" | "labelIds" | "auto" (trainIds when every image has its labelTrainIds PNG, else labelIds).  ``lut`` is None for trainId
    labels and the id -> trainId table for raw ids.  ``__getitem__`` -> (uint8 [3,H,W], int64 [H,W]); ``raw_item`` -> (uint8 [H,W,3], uint8 [H,W]);
    the label values are the file's own (trainIds, or raw ids to be read through ``lut``)."""
    num_classes = len(CITYSCAPES_CLASSES)
    ignore_label = IGNORE_LABEL
    class_names = CITYSCAPES_CLASSES

    def __init__(self, root, split="val", labels="auto"):
        if labels not in ("auto", "trainIds", "labelIds"):
            raise ValueError(f"labels must be 'auto', 'trainIds' or 'labelIds', got {labels!r}")
        images_dir, targets_dir = os.path.join(root, "leftImg8bit", split), os.path.join(root, "gtFine", split)
        if not os.path.isdir(images_dir) or not os.path.isdir(targets_dir):
            raise RuntimeError(f"Cityscapes split {split!r} not found under {root}: need leftImg8bit/{split} and gtFine/{split}")
        self.images, stems = [], []
        for city in sorted(os.listdir(images_dir)):
            for f in sorted(os.listdir(os.path.join(images_dir, city))):
                if f.endswith("_leftImg8bit.png"):
                    self.images.append(os.path.join(images_dir, city, f))
                    stems.append(os.path.join(targets_dir, city, f[:-len("_leftImg8bit.png")]))
        train = [s + "_gtFine_labelTrainIds.png" for s in stems]
        if labels == "auto":
            labels = "trainIds" if train and all(os.path.exists(p) for p in train) else "labelIds"
        self.label_source = labels
        self.labels = train if labels == "trainIds" else [s + "_gtFine_labelIds.png" for s in stems]
        self.lut = None if labels == "trainIds" else cityscapes_lut()

    def __len__(self):
        return len(self.images)

    def _decode(self, index):
        return read_image(self.images[index]), read_label(self.labels[index])

    def __getitem__(self, index):
        return _to_item(*self._decode(index))

    def raw_item(self, index):
        return _to_raw_item(*self._decode(index))
