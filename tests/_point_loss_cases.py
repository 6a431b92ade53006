"""Shared by tests/test_point_loss_cpu.py, tests/test_point_loss_gpu.py and tests/test_finetune_criterion_gpu.py: seeded inputs and the torch
restatement of what K8 computes -- detectron2's point_sample, the two losses of SetCriterion.loss_masks (criterion.py:23-68, 194-243), the
matcher's cost in its ORIGINAL pos / neg form (matcher.py:15-62, 105-149; the kernel uses softplus(x) - x t) and the uncertainty selection
(criterion.py:76-90 + detectron2's get_uncertain_point_coords_with_randomness).  Everything is dtype-generic: the same function in double is the
truth and in float is b, the fp32-CPU error of the same case.  Error metric, bar and check are those of tests/_rba_bwd_cases.py.

Parity: ``ref_mask_losses``, ``ref_match_cost``, ``ref_loss_labels`` and ``ref_criterion`` are PINNED BY REFERENCE CODE -- tests/golden/g9_criterion.npz
holds what the reference's own ``loss_masks``, ``loss_labels``, ``dice_loss``, ``sigmoid_ce_loss``, ``batch_dice_loss``, ``batch_sigmoid_ce_loss``,
``HungarianMatcher`` (cost matrix and assignment) and ``SetCriterion.forward`` compute, and tests/test_criterion_reference_cpu.py holds these
restatements to it at relative 1e-12 (2^-23 where the reference computes in float32).  ``ref_point_sample`` is held there against the generator's
stand-in for Detectron2's ``point_sample`` (``grid_sample(input, 2 coords - 1)``, restated: unpinned), and ``ref_select`` -- the uncertainty
importance sampling -- remains unpinned: the fixture hands the reference's loss its stored coordinates.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from tests._rba_bwd_cases import FLOOR, bar, check, err, ref_outlier_loss  # noqa: F401  (re-exported: one metric, one bar)


# ---------------------------------------------------------------------------------------------------------------- the restatement
def ref_point_sample(planes, coords, index=None):
    """F.grid_sample(planes[:, None], 2 c - 1, align_corners=False) with zero padding, written out: planes [M,h,w], coords [N,P,2] or [1,P,2]
    as (x, y), index [N] (None: row n reads plane n) -> [N,P] in planes' dtype"""
    M, h, w = planes.shape
    src = planes if index is None else planes[index]
    N = src.shape[0]
    c = coords.to(planes.dtype).expand(N, -1, -1)
    px, py = c[..., 0] * w - 0.5, c[..., 1] * h - 0.5
    x0, y0 = torch.floor(px), torch.floor(py)
    ax, ay = px - x0, py - y0
    flat = src.reshape(N, h * w)
    out = torch.zeros_like(px)
    for dy, dx, wt in ((0, 0, (1 - ax) * (1 - ay)), (0, 1, ax * (1 - ay)), (1, 0, (1 - ax) * ay), (1, 1, ax * ay)):
        xi, yi = x0 + dx, y0 + dy
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        off = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).long()
        out = out + torch.where(inside, flat.gather(1, off), torch.zeros_like(px)) * wt
    return out


def ref_mask_losses(pred_masks, plane_index, coords, labels, num_masks):
    """criterion.py:230-239 with sigmoid_ce_loss (:50-68) and dice_loss (:23-42): pred_masks [B,Q,h,w] -> (loss_mask, loss_dice)"""
    x = ref_point_sample(pred_masks.flatten(0, 1), coords, plane_index)
    labels = labels.to(x.dtype)
    loss_mask = F.binary_cross_entropy_with_logits(x, labels, reduction="none").mean(1).sum() / num_masks
    s = x.sigmoid()
    loss_dice = (1 - (2 * (s * labels).sum(-1) + 1) / (s.sum(-1) + labels.sum(-1) + 1)).sum() / num_masks
    return loss_mask, loss_dice


def ref_match_cost(pred_masks, tgt_masks, coords, pred_logits, tgt_ids, w_mask, w_class, w_dice):
    """matcher.py:105-149: pred_masks [Q,h,w], tgt_masks [T,H,W], coords [P,2], pred_logits [Q,K+1] -> C [Q,T]"""
    cost_class = -pred_logits.softmax(-1)[:, tgt_ids]
    x = ref_point_sample(pred_masks, coords[None])
    t = ref_point_sample(tgt_masks.to(x.dtype), coords[None])
    pos = F.binary_cross_entropy_with_logits(x, torch.ones_like(x), reduction="none")
    neg = F.binary_cross_entropy_with_logits(x, torch.zeros_like(x), reduction="none")
    cost_mask = (torch.einsum("nc,mc->nm", pos, t) + torch.einsum("nc,mc->nm", neg, 1 - t)) / x.shape[1]
    s = x.sigmoid()
    cost_dice = 1 - (2 * torch.einsum("nc,mc->nm", s, t) + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None, :] + 1)
    return w_mask * cost_mask + w_class * cost_class + w_dice * cost_dice


def ref_select(pred_masks, plane_index, candidates, k):
    """-> (indices [N,k] of the k candidates of smallest |logit|, |logit| of every candidate [N,R])"""
    x = ref_point_sample(pred_masks.flatten(0, 1), candidates, plane_index).abs()
    return torch.topk(-x, k=k, dim=1)[1], x


def ref_loss_labels(pred_logits, targets, indices, num_classes, eos_coef):
    classes = torch.full(pred_logits.shape[:2], num_classes, dtype=torch.int64)
    for b, (t, (i, j)) in enumerate(zip(targets, indices)):
        classes[b, i] = t["labels"][j]
    weight = torch.ones(num_classes + 1, dtype=pred_logits.dtype)
    weight[-1] = eos_coef
    return F.cross_entropy(pred_logits.transpose(1, 2), classes, weight)


def ref_criterion(pred_logits, pred_masks, targets, indices, num_masks, loss_coords, num_classes, eos_coef):
    """the reference's three losses of the fine-tune recipe for one outputs entry -> {"loss_ce", "loss_mask", "loss_dice", "outlier_loss"}.
    targets[i]: "labels" [T], "masks" [T,H,W] (one size), "outlier_masks" [H,W]; loss_coords [N,P,2] in the order of the images' pairs"""
    Q = pred_logits.shape[1]
    plane_index = torch.cat([b * Q + i for b, (i, _) in enumerate(indices)])
    tgt = torch.cat([t["masks"][j] for t, (_, j) in zip(targets, indices)]).to(pred_masks.dtype)
    with torch.no_grad():
        labels = ref_point_sample(tgt, loss_coords)
    lm, ld = ref_mask_losses(pred_masks, plane_index, loss_coords, labels, num_masks)
    return {"loss_ce": ref_loss_labels(pred_logits, targets, indices, num_classes, eos_coef), "loss_mask": lm, "loss_dice": ld,
            "outlier_loss": ref_outlier_loss(pred_logits, pred_masks, torch.stack([t["outlier_masks"] for t in targets]))}


def _num(v):
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def scalar_bar(l32, l64):
    """|l - l64| <= 4 max(|l32 - l64|, 2^-20 |l64|)"""
    return 4.0 * max(abs(_num(l32) - _num(l64)), FLOOR * abs(_num(l64)))


def check_scalar(what, l, l32, l64):
    l, l64 = _num(l), _num(l64)
    d, lim = abs(l - l64), scalar_bar(l32, l64)
    print(f"{what}: {l:.9g} truth {l64:.9g}  |d| = {d:.3e}  bar = {lim:.3e}")
    assert np.isfinite(l) and d <= lim, f"{what}: |{l:.9g} - {l64:.9g}| = {d:.3e} > {lim:.3e}"


# ---------------------------------------------------------------------------------------------------------------- inputs
def smooth(gen, M, h, w, amp):
    """M smooth random planes [M,h,w]: coarse noise, bilinearly enlarged"""
    coarse = torch.randn(M, 1, max(2, h // 8 + 1), max(2, w // 8 + 1), generator=gen)
    return amp * F.interpolate(coarse, size=(h, w), mode="bilinear", align_corners=True)[:, 0].contiguous()


def exact_centres(size):
    """the pixels j of an axis of `size` whose centre coordinate c = fp32((j + 0.5) / size) gives the pixel coordinate c size - 0.5 == j exactly in
    fp32, with the product rounded or fused -- there a sampled value must be the pixel's bits"""
    out = []
    for j in range(size):
        c = np.float32((j + 0.5) / size)
        if np.float32(c * np.float32(size)) - np.float32(0.5) == j and np.float32(np.float64(c) * size - 0.5) == j:
            out.append(j)
    return out


BELOW_ONE = float(np.nextafter(np.float32(1.0), np.float32(0.0)))
SAMPLE_SHAPES = ((3, 1, 1, 5), (2, 1, 7, 64), (2, 5, 1, 65), (4, 32, 64, 333), (1, 128, 256, 12544))       # (N, h, w, P)


@functools.lru_cache(maxsize=None)
def sample_inputs(shape, shared):
    """(planes [N + 2, h, w], coords [N | 1, P, 2], centres = [(p, y, x)] the points placed on exact pixel centres): uniform points with exactly 0, the
    largest float below 1, values slightly outside [0, 1] and pixel centres written over the first ones"""
    N, h, w, P = shape
    gen = torch.Generator().manual_seed(8100 + 7 * SAMPLE_SHAPES.index(shape) + int(shared))
    planes = smooth(gen, N + 2, h, w, 3.0) if h * w > 1 else torch.randn(N + 2, h, w, generator=gen)
    coords = torch.rand(1 if shared else N, P, 2, generator=gen)
    xs, ys = exact_centres(w), exact_centres(h)
    assert xs and ys
    special = [(0.0, 0.0), (BELOW_ONE, BELOW_ONE), (-0.01, 1.02)]
    centres = []
    for k in range(min(4, len(xs) * len(ys))):
        x, y = xs[(k * 3) % len(xs)], ys[(k * 5) % len(ys)]
        centres.append((len(special), y, x))
        special.append((float(np.float32((x + 0.5) / w)), float(np.float32((y + 0.5) / h))))
    special += [(1.0, 0.5), (0.5, -1e-7), (1e30, -1e30)]
    keep = [(p, y, x) for p, y, x in centres if p < P]
    for p, (cx, cy) in enumerate(special[:P]):
        coords[:, p, 0], coords[:, p, 1] = cx, cy
    return planes, coords, keep


LOSS_SHAPES = ((1, 1, 1, 1), (9, 32, 64, 448), (3, 5, 7, 63), (5, 128, 256, 12544))                        # (N, h, w, P)
W_MASK, W_DICE = 5.0, 2.0           # the upstream gradients of the two losses in the tests


@functools.lru_cache(maxsize=None)
def loss_inputs(shape, variant="plain"):
    """(pred_masks [2, Q, h, w] with 2 Q > N, plane_index [N] distinct, coords [N,P,2], labels [N,P], num_masks).  Labels: binary masks at 4x the
    resolution, point-sampled -- fractional.  variant "contend": all P points of a mask identical; "wide": logits 40 randn clipped to +-120."""
    N, h, w, P = shape
    gen = torch.Generator().manual_seed(8200 + LOSS_SHAPES.index(shape))
    Q = (N + 3) // 2 + 1
    pred = smooth(gen, 2 * Q, h, w, 4.0) if h * w > 1 else torch.randn(2 * Q, h, w, generator=gen)
    if variant == "wide":
        pred = (40.0 * torch.randn(2 * Q, h, w, generator=gen)).clamp(-120.0, 120.0)
    index = torch.randperm(2 * Q, generator=gen)[:N]
    coords = torch.rand(N, P, 2, generator=gen)
    if variant == "contend":
        coords = coords[:, :1].expand(N, P, 2).contiguous()
    tgt = (smooth(gen, N, 4 * h, 4 * w, 1.0) > 0).float()
    labels = ref_point_sample(tgt, coords)
    return pred.view(2, Q, h, w), index, coords, labels, float(max(N - 1, 1))


def _loss_autograd(pred, index, coords, labels, num_masks, dtype):
    p = pred.to(dtype).clone().requires_grad_(True)
    lm, ld = ref_mask_losses(p, index, coords.to(dtype), labels.to(dtype), num_masks)
    (W_MASK * lm + W_DICE * ld).backward()
    return lm.detach(), ld.detach(), p.grad


@functools.lru_cache(maxsize=None)
def loss_truth(shape, variant="plain"):
    """{"l64": (loss_mask, loss_dice), "l32": ..., "g64": d (W_MASK loss_mask + W_DICE loss_dice) / d pred_masks, "b": fp32 CPU autograd's error}"""
    args = loss_inputs(shape, variant)
    lm64, ld64, g64 = _loss_autograd(*args, torch.float64)
    lm32, ld32, g32 = _loss_autograd(*args, torch.float32)
    return {"l64": (lm64, ld64), "l32": (lm32, ld32), "g64": g64, "b": err(g32, g64) if float(g64.abs().max()) > 0 else 0.0}


COST_SHAPES = ((1, 1, 1), (100, 7, 333), (100, 37, 12544), (200, 19, 448), (3, 1, 64))                      # (Q, T, P)
COST_K, COST_PRED, COST_TGT, COST_WEIGHTS = 19, (32, 64), (128, 256), (5.0, 2.0, 5.0)                      # weights: mask, class, dice


@functools.lru_cache(maxsize=None)
def cost_inputs(shape):
    """(pred_masks [Q,32,64], tgt_masks [T,128,256] binary, coords [P,2], pred_logits [Q,K+1], tgt_ids [T])"""
    Q, T, P = shape
    gen = torch.Generator().manual_seed(8300 + COST_SHAPES.index(shape))
    pred = smooth(gen, Q, *COST_PRED, 4.0)
    tgt = (smooth(gen, T, *COST_TGT, 1.0) > 0.3).float()
    return pred, tgt, torch.rand(P, 2, generator=gen), 2.0 * torch.randn(Q, COST_K + 1, generator=gen), torch.randint(0, COST_K + 1, (T,), generator=gen)


@functools.lru_cache(maxsize=None)
def cost_truth(shape):
    """(C64 [Q,T], b)"""
    pred, tgt, coords, logits, ids = cost_inputs(shape)
    c64 = ref_match_cost(pred.double(), tgt.double(), coords.double(), logits.double(), ids, *COST_WEIGHTS)
    return c64, err(ref_match_cost(pred, tgt, coords, logits, ids, *COST_WEIGHTS), c64)


@functools.lru_cache(maxsize=None)
def planted(Q=100, T=7, P=333, B=1, K=COST_K, pred_hw=COST_PRED, seed=8400):
    """The row-dominant fixture: per image, T targets that are thresholded, noised 4x enlargements of T distinct predicted masks ->
    (pred_logits [B,Q,K+1], pred_masks [B,Q,h,w], targets = [{"labels", "masks" [T,4h,4w], "rows" = the planted queries}], coords [P,2]).
    The planted query's class logit is raised, so all three cost terms agree."""
    gen = torch.Generator().manual_seed(seed)
    h, w = pred_hw
    pred = smooth(gen, B * Q, h, w, 4.0).view(B, Q, h, w)
    logits = torch.randn(B, Q, K + 1, generator=gen)
    targets = []
    for b in range(B):
        rows = torch.randperm(Q, generator=gen)[:T]
        up = F.interpolate(pred[b, rows][None], scale_factor=4, mode="bilinear", align_corners=False)[0]
        masks = ((up + 0.5 * torch.randn(up.shape, generator=gen)) > 0).float()
        labels = torch.randint(0, K, (T,), generator=gen)
        logits[b, rows, labels] += 4.0
        targets.append({"labels": labels, "masks": masks, "rows": rows})
    return logits, pred, targets, torch.rand(P, 2, generator=gen)


def planted_assignment(logits, pred, target, coords, weights=COST_WEIGHTS):
    """fp64 cost of one image, the asserted margin -- every column's minimum sits in its own row and beats the column's runner-up by more than
    8 * 2^-20 * max|C|, twice the bar, so the optimum is the column-wise argmin and cannot move within the bar -> (C64, rows [T], margin, bound)"""
    c64 = ref_match_cost(pred.double(), target["masks"].double(), coords.double(), logits.double(), target["labels"], *weights)
    two = torch.topk(c64, k=min(2, c64.shape[0]), dim=0, largest=False)
    rows = two.indices[0]
    bound = 8.0 * FLOOR * float(c64.abs().max())
    margin = float((two.values[1] - two.values[0]).min()) if c64.shape[0] > 1 else float("inf")
    assert len(set(rows.tolist())) == c64.shape[1], "fixture: two columns share their best row"
    assert margin > bound, f"fixture: margin {margin:.3e} <= {bound:.3e}"
    return c64, rows, margin, bound
