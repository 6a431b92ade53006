"""Shared by tests/golden/make_golden.py (``--only g9_criterion``), tests/test_criterion_reference_cpu.py and tests/test_criterion_reference_gpu.py:
the layout of ``tests/golden/g9_criterion.npz``, the mapping of the case modules' seeded draws into the reference's domain, the seeded inputs of
the fixture's cases and the two derived bounds.

The fixture is written by the reference's own ``mask2former/modeling/criterion.py`` and ``matcher.py`` (imported behind stand-ins, see the
generator's docstring); nothing here restates a loss.  Keys are ``<case>/<item>``: ``l64`` / ``l32`` = the reference's loss on .double() / .float()
of the stored inputs, ``g_<leaf>`` = float64 autograd's gradient for that leaf, ``b_<leaf>`` = err(float32 gradient, float64 gradient) in the metric
of tests/_rba_bwd_cases.py.  The "crop" cases store ``s_<leaf>_<axis>`` sums of the gradient instead, and a crc32 of each regenerated input.
"""
import functools
import os
import zlib

import numpy as np
import torch
import torch.nn.functional as F

from tests import _dense_hybrid_cases as D
from tests import _pebal_cases as P
from tests import _point_loss_cases as C
from tests import _rba_bwd_cases as R

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g9_criterion.npz")

# Both sides of a CPU comparison are the same torch operations in double: one rounding of 2^-53 per operation, reductions of at most 1e5 terms
# (the crop's 2 x 128 x 256 pixel means) -> 1e5 x 2^-53 = 1.1e-11 in the worst case of errors that all add, 1e-12 taken.  Where the reference
# itself computes in float32 whatever it is given (``pred_logits.float()`` of loss_labels, ``ood_mask.float()`` as the BCE target,
# ``out_mask.float()`` of the matcher) the restatement runs under the same cast and is held to one float32 rounding.
REL64 = 1e-12
REL32 = 2.0 ** -23

SMALL = (1, 20, 5, 7, 9, 25, 33)                    # (B, Q, K, h, w, H, W)
K19 = (2, 12, 19, 7, 9, 25, 33)
CROP = (2, 100, 19, 32, 64, 128, 256)
THR_IN, THR_OUT, BETA, OOD_REG, EOS = -1.0, -0.1, D.BETA, P.OOD_REG, 0.1
MATCHER_WEIGHTS = {"cost_class": 2.0, "cost_mask": 5.0, "cost_dice": 5.0}          # the recipes' CLASS_WEIGHT / MASK_WEIGHT / DICE_WEIGHT
MATCHER_SHAPES = ((20, 4, 64, 8, 16), (100, 7, 333, 8, 16))                         # (Q, T, P, h, w); targets at 4 h x 4 w
SET_T, SET_SIZES, SET_P, SET_NUM_MASKS = (3, 0, 2), ((25, 33), (25, 33), (20, 28)), 50, 4.0
FWD_T, FWD_PM, FWD_PL, FWD_AUX = (3, 2), 64, 48, 2
FORWARDS = {
    "mix": dict(losses=["labels", "masks", "outlier"], weights={"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "outlier_loss": 1.0},
                settings=dict(outlier_loss_target="nls", score_norm="tanh", outlier_loss_func="squared_hinge", smoothness_score="none")),
    "densehybrid": dict(losses=["densehybrid"], weights={"densehybrid_loss": 1.0},
                        settings=dict(outlier_loss_target="none", score_norm="none", outlier_loss_func="squared_hinge", smoothness_score="none")),
    "pebal": dict(losses=["gambler", "smoothness", "sparsity", "outlier"], weights=dict(P.RECIPE_WEIGHTS),
                  settings=dict(outlier_loss_target="energy", score_norm="none", outlier_loss_func="squared_hinge", smoothness_score="energy")),
}


@functools.lru_cache(maxsize=None)
def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def t(a):
    """a fixture array as a torch tensor (integer planes as int64)"""
    x = torch.from_numpy(np.ascontiguousarray(a))
    return x.to(torch.int64) if x.dtype in (torch.uint8, torch.int32, torch.int16) else x


# ---------------------------------------------------------------------------------------------------------------- the reference's domain
def domain_sem_seg(labels, K):
    """The DenseHybrid label plane inside the reference's domain: a class, 254 or 255.  Every other value (the seeded draws hold 200) -> 255."""
    keep = ((labels >= 0) & (labels < K)) | (labels == D.OUTLIER) | (labels == 255)
    return torch.where(keep, labels, torch.full_like(labels, 255))


def domain_pebal(outlier_masks, sem_seg, K):
    """The gambler loss's two planes inside the reference's domain: value 200 -> 255 in ``sem_seg``, and ``outlier_masks`` set to 255 wherever
    ``sem_seg`` is not a class and the pixel is not an outlier (an inlier pixel without a class is an IndexError there)."""
    is_class = (sem_seg >= 0) & (sem_seg < K)
    sem_seg = torch.where(is_class | (sem_seg == 255), sem_seg, torch.full_like(sem_seg, 255))
    outlier_masks = torch.where(~is_class & (outlier_masks != 1), torch.full_like(outlier_masks, 255), outlier_masks)
    return outlier_masks, sem_seg


def planes_of(labels):
    """one label plane (classes, 254 = outlier, 255 = void) -> (outlier_masks 0 / 1 / 255, sem_seg = the plane itself): what the COCO-mix mapper
    hands every recipe"""
    om = torch.zeros_like(labels)
    om[labels == D.OUTLIER] = 1
    om[labels == 255] = 255
    return om, labels.clone()


def without_outliers(outlier_masks):
    """the no-outlier variant: every outlier pixel becomes void (it has no class, so it cannot become an inlier)"""
    return torch.where(outlier_masks == 1, torch.full_like(outlier_masks, 255), outlier_masks)


# ---------------------------------------------------------------------------------------------------------------- seeded inputs
def dense_inputs(shape, seed):
    """(pred_logits, pred_masks, ood_pred, labels): labels = K10's draw inside the domain"""
    B, Q, K, h, w, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    logits = 2.0 * torch.randn(B, Q, K + 1, generator=gen)
    masks = 3.0 * torch.randn(B, Q, h, w, generator=gen)
    ood = 1.5 * torch.randn(B, 2, h, w, generator=gen)
    return logits, masks, ood, domain_sem_seg(D.draw_labels(gen, B, K, H, W), K)


def set_inputs():
    """the "small" case of loss_labels / loss_masks: three images with 3, 0 and 2 targets, target masks of two sizes (so that the reference pads)
    that differ from the prediction's, fixed indices -> (pred_logits [3,Q,K+1], pred_masks [3,Q,h,w], targets, indices, coords [5,P,2])"""
    _, Q, K, h, w, _, _ = SMALL
    gen = torch.Generator().manual_seed(12100)
    logits = 2.0 * torch.randn(3, Q, K + 1, generator=gen)
    masks = 3.0 * torch.randn(3, Q, h, w, generator=gen)
    targets = [{"labels": torch.randint(0, K, (n,), generator=gen), "masks": (C.smooth(gen, n, H, W, 1.0) > 0).float() if n else torch.zeros(0, H, W)}
               for n, (H, W) in zip(SET_T, SET_SIZES)]
    indices = [(torch.tensor([4, 11, 17]), torch.tensor([2, 0, 1])), (torch.tensor([], dtype=torch.int64), torch.tensor([], dtype=torch.int64)),
               (torch.tensor([0, 19]), torch.tensor([1, 0]))]
    return logits, masks, targets, indices, torch.rand(5, SET_P, 2, generator=gen)


def matcher_inputs(shape, seed):
    """tests/_point_loss_cases.planted at this size: (pred_logits [1,Q,K+1], pred_masks [1,Q,h,w], target, coords [P,2] uniform,
    centres [P,2]).  ``centres`` are P pixel centres of the prediction's grid, whose sizes are powers of two: there a sampled logit is the
    pixel's own bits and a sampled target a multiple of 1/4, whatever the order of the sampler's arithmetic.  The float32 comparison with the
    reference's captured C is made at ``centres``: only there are both sides the same operations under the same cast.  At uniform coordinates
    ``grid_sample`` and ``ref_point_sample`` round a sampled logit differently (1 ulp, 9.5e-7 at |x| = 8), which the cost's P-term means pass
    on: measured 1.36e-7 of max|C| at P = 333 (0.90e-7 at P = 64) against the 2^-23 = 1.19e-7 that assumes one rounding of the result -- that
    assumption, not the restatement, is what fails there, and the uniform coordinates are held in float64 (2.6e-16) instead."""
    Q, T, P_, h, w = shape
    logits, pred, targets, coords = C.planted(Q=Q, T=T, P=P_, B=1, K=19, pred_hw=(h, w), seed=seed)
    pix = torch.randint(0, h * w, (P_,), generator=torch.Generator().manual_seed(seed + 50))
    centres = torch.stack([((pix % w).float() + 0.5) / w, (torch.div(pix, w, rounding_mode="floor").float() + 0.5) / h], dim=-1)
    return logits, pred, targets[0], coords, centres


def forward_inputs():
    """"k19"-sized outputs with FWD_AUX aux_outputs entries (the final outputs plus noise, so that every entry's matching is far from a tie),
    planted targets, one label plane for all three recipes -> (leaves = {name: tensor}, targets, matcher coords [P,2], loss coords [N,P,2])"""
    B, Q, K, h, w, H, W = K19
    logits, masks, ood, labels = dense_inputs(K19, 12300)
    gen = torch.Generator().manual_seed(12301)
    leaves = {"pred_logits": logits, "pred_masks": masks, "ood_pred": ood}
    targets = []
    for b, n in enumerate(FWD_T):
        rows = torch.randperm(Q, generator=gen)[:n]
        up = F.interpolate(masks[b, rows][None], size=(H, W), mode="bilinear", align_corners=False)[0]
        cls = torch.randint(0, K, (n,), generator=gen)
        leaves["pred_logits"][b, rows, cls] += 4.0
        om, ss = planes_of(labels[b])
        targets.append({"labels": cls, "masks": (up > 0).float(), "outlier_masks": om, "sem_seg": ss})
    for i in range(FWD_AUX):
        leaves[f"aux{i}_pred_logits"] = leaves["pred_logits"] + 0.3 * torch.randn(logits.shape, generator=gen)
        leaves[f"aux{i}_pred_masks"] = masks + 0.5 * torch.randn(masks.shape, generator=gen)
    return leaves, targets, torch.rand(FWD_PM, 2, generator=gen), torch.rand(sum(FWD_T), FWD_PL, 2, generator=gen)


def outputs_of(leaves, ood=False):
    out = {"pred_logits": leaves["pred_logits"], "pred_masks": leaves["pred_masks"],
           "aux_outputs": [{"pred_logits": leaves[f"aux{i}_pred_logits"], "pred_masks": leaves[f"aux{i}_pred_masks"]} for i in range(FWD_AUX)]}
    if ood:
        out["ood_pred"] = leaves["ood_pred"]
    return out


def forward_leaves(name):
    return [k for k in ("pred_logits", "pred_masks") + (("ood_pred",) if name == "densehybrid" else ())] + \
           [f"aux{i}_{k}" for i in range(FWD_AUX) for k in ("pred_logits", "pred_masks")]


def weight_of(name, key):
    base = key.rsplit("_", 1)[0] if key.rsplit("_", 1)[-1].isdigit() else key
    return FORWARDS[name]["weights"][base]


# ---------------------------------------------------------------------------------------------------------------- the crop: sums and checksums
def crc(x):
    return np.uint32(zlib.crc32(np.ascontiguousarray(x.detach().cpu().numpy()).tobytes()))


def grad_sums(g):
    """what the crop stores of a gradient.  pred_masks [B,Q,h,w]: row sums [B,h], column sums [B,w], per-query sums [B,Q].  pred_logits
    [B,Q,K+1]: per-class sums [B,K+1] and per-query sums over the K classes [B,Q] (over all K + 1 columns a softmax gradient sums to 0).
    ood_pred [B,2,h,w]: row, column and per-channel sums."""
    g = g.detach().double()
    if g.dim() == 4:
        return {"row": g.sum((1, 3)), "col": g.sum((1, 2)), "qry": g.sum((2, 3))}
    return {"cls": g.sum(1), "qry": g[..., :-1].sum(-1)}


@functools.lru_cache(maxsize=None)
def crop_cases():
    """{case: (leaves, targets)} of the recipe crop: the case modules' seeded draws mapped into the domain"""
    K = CROP[2]
    out = {}
    for combo in R.COMBOS:
        lg, mk, lab = R.loss_inputs("crop", combo, True)
        out["outlier/" + "_".join(combo)] = ({"pred_logits": lg, "pred_masks": mk}, [{"outlier_masks": x} for x in lab])
    lg, mk, ood, lab = D.loss_inputs("crop")
    out["densehybrid"] = ({"pred_logits": lg, "pred_masks": mk, "ood_pred": ood}, [{"sem_seg": x, "outlier_masks": x} for x in domain_sem_seg(lab, K)])
    lg, mk, om, ss = P.loss_inputs("crop")
    om, ss = domain_pebal(om, ss, K)
    out["pebal"] = ({"pred_logits": lg, "pred_masks": mk}, [{"outlier_masks": a, "sem_seg": b} for a, b in zip(om, ss)])
    return out


def rel(a, a64):
    """max|a - a64| / max|a64| (tests/_rba_bwd_cases.err) for arrays and scalars alike; 0 / 0 = 0"""
    a, a64 = torch.as_tensor(a).detach().double(), torch.as_tensor(a64).detach().double()
    d, m = float((a - a64).abs().max()), float(a64.abs().max())
    return 0.0 if d == 0.0 else d / m
