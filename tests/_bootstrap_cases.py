"""Generators and truths of the bootstrap tests (K18, docs/kernels/K18.md).  No device: tests/test_bootstrap_cpu.py checks this file on the CPU,
tests/test_bootstrap_curve_gpu.py holds the kernels to it.

A case is 6 - 9 images of 24 x 40 with a border labelled 255 and 3 - 10 % positives: a few thousand labelled pixels.  The truth of every trial is
rba_amd.metrics.ood_metrics on the trial's pixels on the CPU (held to scikit-learn by tests/test_metrics.py); the integers K18 returns (P, N, auroc2,
fp95, tp95) are derived here from metrics.binary_clf_curve with ood_metrics' own rules, and `truth` asserts that they reproduce ood_metrics' floats."""
import functools

import numpy as np
import torch

from rba_amd import metrics

H, W, BORDER = 24, 40, 2


def _label_maps(rng, n_images, share, without_positives=()):
    """uint8 [n, H, W]: 255 on the border, `share` of the interior pixels 1, the rest 0"""
    lab = np.full((n_images, H, W), 255, dtype=np.uint8)
    for i in range(n_images):
        inner = (rng.rand(H - 2 * BORDER, W - 2 * BORDER) < (0.0 if i in without_positives else share)).astype(np.uint8)
        if i not in without_positives:
            inner[0, 0] = 1
        lab[i, BORDER:-BORDER, BORDER:-BORDER] = inner
    return lab


def draws(seed, n_images, trials, ratio, full_last=False):
    """bool [T, n]: np.random.choice(np.arange(n), int(n * ratio), replace=False) per trial, evaluate_ood_bootstrapped's call"""
    rng = np.random.RandomState(seed)
    m = np.zeros((trials, n_images), dtype=bool)
    for t in range(trials):
        m[t, rng.choice(np.arange(n_images), int(n_images * ratio), replace=False)] = True
    if full_last:
        m[-1] = True
    return m


def _scored(rng, lab, ties=None):
    s = (rng.randn(*lab.shape) + 1.5 * (lab == 1)).astype(np.float32)
    return s if ties is None else (np.round(s * ties) / ties).astype(np.float32)


def _collinear():
    """(d) every image holds, by descending score: 47 positives + 5 negatives at 5.0, then three runs of 1 positive + 3 negatives (4.0, 3.0, 2.0), then
    the remaining negatives at 1.0.  For any k images the ROC points are (tp, fp) = (47k, 5k), (48k, 8k), (49k, 11k), (50k, 14k), (50k, all): the first
    point above 0.95 * 50k is (48k, 8k), which lies on the collinear stretch of step (k, 3k) and is dropped, as is (49k, 11k); the answer is (50k, 14k)."""
    n = 8
    lab = np.full((n, H, W), 255, dtype=np.uint8)
    score = np.zeros((n, H, W), dtype=np.float32)
    inner = (H - 2 * BORDER) * (W - 2 * BORDER)
    for i in range(n):
        rng = np.random.RandomState(100 + i)
        l = np.zeros(inner, dtype=np.uint8)
        s = np.full(inner, 1.0, dtype=np.float32)
        order = rng.permutation(inner)
        at = 0
        for value, pos, neg in ((5.0, 47, 5), (4.0, 1, 3), (3.0, 1, 3), (2.0, 1, 3)):
            l[order[at:at + pos]] = 1
            s[order[at:at + pos + neg]] = value
            at += pos + neg
        lab[i, BORDER:-BORDER, BORDER:-BORDER] = l.reshape(H - 2 * BORDER, W - 2 * BORDER)
        score[i, BORDER:-BORDER, BORDER:-BORDER] = s.reshape(H - 2 * BORDER, W - 2 * BORDER)
    return score, lab, draws(4, n, 7, 0.5, full_last=True)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (score fp32 [n,H,W], labels uint8 [n,H,W], members bool [T,n]) as numpy arrays; treat them as read-only"""
    if name == "continuous":                                      # (a)
        rng = np.random.RandomState(1)
        lab = _label_maps(rng, 7, 0.06)
        return _scored(rng, lab), lab, draws(1, 7, 7, 0.5)
    if name == "ties":                                            # (b) scores rounded to 1/8: ties are the rule
        rng = np.random.RandomState(2)
        lab = _label_maps(rng, 8, 0.05)
        return _scored(rng, lab, ties=8), lab, draws(2, 8, 7, 0.5)
    if name == "constant":                                        # (c) one run across all chunks
        rng = np.random.RandomState(3)
        lab = _label_maps(rng, 6, 0.08)
        return np.full(lab.shape, 0.25, dtype=np.float32), lab, draws(3, 6, 7, 0.5, full_last=True)
    if name == "collinear":                                       # (d)
        return _collinear()
    if name.startswith("trials"):                                 # (e) trials_<T>_<ratio in percent>; the last trial is the full set
        T, ratio = int(name.split("_")[1]), int(name.split("_")[2]) / 100.0
        rng = np.random.RandomState(5)
        lab = _label_maps(rng, 9, 0.04)
        return _scored(rng, lab, ties=16), lab, draws(50 + T, 9, T, ratio, full_last=True)
    if name == "no_positive":                                     # (f) the only case with a trial that holds no positive: trial 2 = images {1, 4}
        rng = np.random.RandomState(6)
        lab = _label_maps(rng, 6, 0.10, without_positives=(1, 4))
        m = draws(6, 6, 5, 0.5)
        m[2] = [False, True, False, False, True, False]
        for t in (0, 1, 3, 4):                                    # every other trial holds an image with positives
            m[t, 0] = True
        return _scored(rng, lab, ties=8), lab, m
    raise KeyError(name)


TRIAL_CASES = [f"trials_{T}_{r}" for T in (1, 7, 64) for r in (50, 100)]
CASES = ["continuous", "ties", "constant", "collinear"] + TRIAL_CASES + ["no_positive"]


@functools.lru_cache(maxsize=None)
def pooled(name):
    """-> (scores fp32 [n], labels int64 [n], image_ids int64 [n]) torch CPU tensors: the labelled pixels of every image, image by image"""
    score, lab, _ = case(name)
    s, y, ids = [], [], []
    for i in range(score.shape[0]):
        si, yi = metrics.select_labelled(torch.from_numpy(score[i]), torch.from_numpy(lab[i]))
        s.append(si)
        y.append(yi.to(torch.int64))
        ids.append(torch.full((si.numel(),), i, dtype=torch.int64))
    return torch.cat(s), torch.cat(y), torch.cat(ids)


@functools.lru_cache(maxsize=None)
def sorted_list(name):
    """-> (score fp32 [n] sorted descending, tag int32 [n]) torch CPU tensors: K18's input"""
    s, y, ids = pooled(name)
    s, order = torch.sort(s, descending=True, stable=True)
    return s.contiguous(), ((ids[order] << 1) | y[order]).to(torch.int32).contiguous()


def integer_curve(scores, labels):
    """-> dict of Python ints and the float ap from metrics.binary_clf_curve, by ood_metrics' rules: P, N, auroc2 = sum dfp * (tp_prev + tp), fp95 / tp95 =
    the first point kept by drop_intermediate with tp / P > 0.95 (0, 0 if there is none), and fp95_all / tp95_all = the same WITHOUT the rule"""
    fps, tps = metrics.binary_clf_curve(scores, labels)
    fps, tps = fps.tolist(), tps.tolist()
    P, N = tps[-1], fps[-1]
    auroc2 = sum((f - pf) * (pt + t) for f, t, pf, pt in zip(fps, tps, [0] + fps[:-1], [0] + tps[:-1]))
    keep = [True] * len(fps)
    for i in range(1, len(fps) - 1):
        keep[i] = (fps[i + 1] - fps[i], tps[i + 1] - tps[i]) != (fps[i] - fps[i - 1], tps[i] - tps[i - 1])
    above = [i for i in range(len(fps)) if P > 0 and float(np.float64(tps[i]) / np.float64(P)) > 0.95]
    kept = [i for i in above if keep[i]]
    return {"P": P, "N": N, "auroc2": auroc2, "fp95": fps[kept[0]] if kept else 0, "tp95": tps[kept[0]] if kept else 0,
            "fp95_all": fps[above[0]] if above else 0, "tp95_all": tps[above[0]] if above else 0}


@functools.lru_cache(maxsize=None)
def truth(name):
    """-> dict of numpy arrays [T]: auroc, aupr, fpr95 (float64, ood_metrics on the trial's pixels) and P, N, auroc2, fp95, tp95, fp95_all (int64, computed
    in Python integers: auroc2 stays far below 2^63 at these sizes).  Asserts that the integers reproduce the floats."""
    s, y, ids = pooled(name)
    _, _, members = case(name)
    out = {k: [] for k in ("auroc", "aupr", "fpr95", "P", "N", "auroc2", "fp95", "tp95", "fp95_all")}
    for row in members:
        sel = torch.from_numpy(row)[ids]
        r = metrics.ood_metrics(s[sel], y[sel])
        c = integer_curve(s[sel], y[sel])
        with np.errstate(divide="ignore", invalid="ignore"):
            fpr95 = np.float64(c["fp95"]) / np.float64(c["N"])
            auroc = np.float64(c["auroc2"]) / (2.0 * np.float64(c["P"]) * np.float64(c["N"]))
        assert np.array_equal(np.float64(r["fpr95"]), fpr95, equal_nan=True), (name, r, c)          # the same quotient of the same two integers
        assert (np.isnan(r["auroc"]) and np.isnan(auroc)) or abs(r["auroc"] - auroc) < 1e-12, (name, r, c)
        for k in ("auroc", "aupr", "fpr95"):
            out[k].append(r[k])
        for k in ("P", "N", "auroc2", "fp95", "tp95", "fp95_all"):
            out[k].append(c[k])
    return {k: np.asarray(v, dtype=np.float64 if k in ("auroc", "aupr", "fpr95") else np.int64) for k, v in out.items()}
