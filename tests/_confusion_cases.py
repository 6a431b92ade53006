"""Shared by the K13 / SemSegEvaluator tests: the numpy oracle of rba_confusion_accum's per-pixel rule (include/rba_hip.h) and the map generators.

The oracle restates the rule, not the kernel: labels through the table (outside 0..255 = bad label), ignore_label -> K, then np.bincount((K+1) * pred + gt)
on the pixels whose label is in 0..K and whose prediction is in 0..K-1 -- Detectron2's SemSegEvaluator.process line on the valid pixels."""
import numpy as np

# launch-rule sizes that break vector heads, tails and the grid-stride loop; confusion_sizes() adds two full sweeps of the capped grid plus 17 pixels
SMALL_SIZES = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4097)

# cityscapesscripts' id -> trainId for ids 0..33 (the test of rba_amd.sem_seg_datasets compares the product's own list with the reference file's)
CITYSCAPES_ID_TO_TRAINID = [255, 255, 255, 255, 255, 255, 255, 0, 1, 255, 255, 2, 3, 4, 255, 255, 255, 5, 255, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 255, 255,
                            16, 17, 18]


def cityscapes_lut():
    lut = np.full(256, 255, dtype=np.uint8)
    lut[:34] = CITYSCAPES_ID_TO_TRAINID
    return lut


def oracle(pred, gt, K, ignore_label=255, lut=None):
    """-> (conf int64 [(K+1), (K+1)], bad int64 [2]) of one call on zeroed outputs"""
    p = np.asarray(pred).reshape(-1).astype(np.int64)
    g = np.asarray(gt).reshape(-1).astype(np.int64)
    assert p.shape == g.shape
    bad_label = np.zeros(p.shape, dtype=bool)
    if lut is not None:
        in_table = (g >= 0) & (g <= 255)
        bad_label |= ~in_table
        g = np.where(in_table, np.asarray(lut, dtype=np.int64)[np.clip(g, 0, 255)], g)
    if ignore_label is not None and ignore_label >= 0:
        g = np.where(g == ignore_label, K, g)
    bad_label |= (g < 0) | (g > K)
    bad_pred = ~bad_label & ((p < 0) | (p >= K))
    ok = ~bad_label & ~bad_pred
    conf = np.bincount((K + 1) * p[ok] + g[ok], minlength=(K + 1) ** 2).astype(np.int64).reshape(K + 1, K + 1)
    return conf, np.array([bad_label.sum(), bad_pred.sum()], dtype=np.int64)


def confusion_sizes():
    """SMALL_SIZES and one size of two full sweeps of K13's launch rule plus 17 pixels, from the rule's constants"""
    from rba_amd import ops
    return SMALL_SIZES + (2 * ops.CONFUSION_GRID_CAP * ops.CONFUSION_THREADS * ops.CONFUSION_TILE + 17,)


def make_cityscapes(root, cities=("aachen", "bonn"), per_city=(3, 2), h=24, w=40, split="val", train_ids=True, label_ids=True, seed=0):
    """A synthetic Cityscapes tree (leftImg8bit/<split>/<city>/..., gtFine/<split>/<city>/...) written in an order that is NOT the sorted one.
    Raw ids are drawn from 0..33 in blocks; the trainId PNGs hold the table's image of them (0..18 and 255).  -> [(image path, image HWC, raw ids, trainIds)]
    in sorted (city, file) order"""
    import os
    from PIL import Image
    rng = np.random.RandomState(seed)
    lut = cityscapes_lut()
    items = []
    for city, n in reversed(list(zip(cities, per_city))):
        os.makedirs(os.path.join(root, "leftImg8bit", split, city))
        os.makedirs(os.path.join(root, "gtFine", split, city))
        for i in reversed(range(n)):
            stem = f"{city}_{i:06d}_000019"
            img = rng.randint(0, 256, (h, w, 3), dtype=np.uint8)
            ids = np.kron(rng.randint(0, 34, ((h + 5) // 6, (w + 7) // 8)), np.ones((6, 8), dtype=np.int64))[:h, :w].astype(np.uint8)
            ip = os.path.join(root, "leftImg8bit", split, city, stem + "_leftImg8bit.png")
            Image.fromarray(img).save(ip)
            if label_ids:
                Image.fromarray(ids).save(os.path.join(root, "gtFine", split, city, stem + "_gtFine_labelIds.png"))
            if train_ids:
                Image.fromarray(lut[ids]).save(os.path.join(root, "gtFine", split, city, stem + "_gtFine_labelTrainIds.png"))
            items.append((ip, img, ids, lut[ids]))
    return sorted(items, key=lambda t: t[0])


CONTENTS = ("constant", "alternating", "uniform", "blocks", "boundary16")


def make_maps(content, n, K, seed=0):
    """-> (pred int32 [n], gt uint8 [n]) with every prediction in 0..K-1 and every label in 0..K-1"""
    rng = np.random.default_rng(seed * 1000003 + K * 101 + CONTENTS.index(content))
    if content == "constant":                                # one counter takes everything
        return np.full(n, K - 1, dtype=np.int32), np.full(n, (K - 1) // 2, dtype=np.uint8)
    if content == "alternating":                             # two pairs, pixel by pixel: no run is longer than one
        odd = (np.arange(n) & 1).astype(bool)
        return np.where(odd, K - 1, 0).astype(np.int32), np.where(odd, 0, K - 1).astype(np.uint8)
    if content == "uniform":
        return rng.integers(0, K, n, dtype=np.int32), rng.integers(0, K, n).astype(np.uint8)
    if content == "blocks":                                  # block-constant: runs of 1..5000 pixels
        runs = rng.integers(1, 5001, n // 2500 + 2)
        while runs.sum() < n:
            runs = np.concatenate([runs, rng.integers(1, 5001, 16)])
        return (np.repeat(rng.integers(0, K, runs.size, dtype=np.int32), runs)[:n].copy(),
                np.repeat(rng.integers(0, K, runs.size).astype(np.uint8), runs)[:n].copy())
    if content == "boundary16":                              # a run boundary at every multiple of 16 - 1 and + 1
        i = np.arange(n)
        seg = 2 * ((i + 1) // 16) + ((i % 16 >= 1) & (i % 16 < 15))
        return (seg % K).astype(np.int32), ((seg * 7 + 3) % K).astype(np.uint8)
    raise KeyError(content)
