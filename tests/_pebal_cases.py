"""Shared by tests/test_gambler_loss_gpu.py, tests/test_gaussian_blur_planes_gpu.py, tests/test_score_reg_gpu.py, tests/test_pebal_criterion_gpu.py
and tools/pebal_loss_probe.py: the torch restatements of the reference's gambler, smoothness and sparsity losses, seeded inputs and the fp64 /
fp32 CPU autograd truths.

The restatements are written from mask2former/modeling/criterion.py:245-388 of the reference.  Their parity is PINNED BY REFERENCE CODE inside the
reference's domain: tests/golden/g9_criterion.npz holds what the reference's own ``gambler_loss`` (both branches, K = 19 -- it hard-codes 19
channels), ``smoothness_loss`` and ``sparsity_loss`` compute, losses and float64 gradients, and tests/test_criterion_reference_cpu.py holds these
restatements and ``ref_pebal_entry`` (through the recipe's ``SetCriterion.forward``) to it at relative 1e-12.  What stays restated and unpinned:
``ref_blur``, torchvision's ``GaussianBlur(7, sigma=1)`` (torchvision is absent; the generator's stand-in is the same definition): the 1-D kernel
exp(-0.5 (x / sigma)^2) on linspace(-(k-1)/2, (k-1)/2, k) normalised to 1, the 2-D kernel their outer product, reflect padding, a per-plane
correlation.  One departure, of the kernel's contract and outside the reference's domain (so against these restatements only): an inlier pixel
whose ``sem_seg`` value is not a class is void (an index error in the reference).  The targets are not written, here or in the reference: its
``labels[...] = 0`` lines act on a ``torch.cat`` copy.  ``self.pebal_reward`` of the reference is dead code (``reward.nelement() > 0`` always holds) and is not
restated.  Error metric, bar and checks are those of tests/_rba_bwd_cases.py and tests/_point_loss_cases.py.
"""
import functools
import os
import shutil

import torch
import torch.nn.functional as F

from tests._dense_hybrid_cases import OUTLIER, draw_labels
from tests._rba_bwd_cases import err, ref_outlier_loss, ref_score

OOD_REG = 0.1
BLUR_K, BLUR_SIGMA = 7, 1.0


def ref_blur(planes, kernel_size=BLUR_K, sigma=BLUR_SIGMA):
    """transforms.GaussianBlur(kernel_size, sigma) of [B,H,W] planes (criterion.py:350-353: the B planes are the channels of one image there)"""
    half = (kernel_size - 1) * 0.5
    x = torch.linspace(-half, half, steps=kernel_size, dtype=planes.dtype, device=planes.device)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = pdf / pdf.sum()
    k2 = torch.mm(k1[:, None], k1[None, :])
    r = kernel_size // 2
    padded = F.pad(planes[:, None], (r, r, r, r), mode="reflect")
    return F.conv2d(padded, k2[None, None])[:, 0]


def ref_gambler_tail(sem, labels, ood_reg=OOD_REG):
    """criterion.py:337-388 behind the class map.  sem [B,K+1,h,w], labels [B,H,W] int64 in the kernel's convention (< K: an inlier pixel of that
    class, 254: outlier, anything else void) -> (loss, parts), parts = the kernel's losses[1:3], stats and R"""
    K = sem.shape[1] - 1
    logits = F.interpolate(sem, size=labels.shape[-2:], mode="bilinear", align_corners=True)              # :337
    probs = logits.softmax(dim=1)                                                                         # :339
    ood_mask, id_mask = labels == OUTLIER, (labels >= 0) & (labels < K)                                   # :342-343, :371, :378
    true_pred, reservation = probs[:, :-1], probs[:, -1]                                                  # :345
    reward = ref_blur(torch.logsumexp(logits[:, :-1], dim=1).pow(2))                                      # :347-353
    reservation = torch.div(reservation, reward)                                                          # :359 / :383
    index = torch.where(id_mask, labels, torch.zeros_like(labels))                                        # :372-373 / :382
    t_in = torch.add(torch.gather(true_pred, index=index.unsqueeze(1), dim=1).squeeze(1), reservation)[id_mask].log()      # :374-378 / :384-386
    n_ood = int(ood_mask.sum())
    if n_ood > 0:                                                                                         # :357
        boosted = torch.add(true_pred, reservation.unsqueeze(1))[ood_mask.unsqueeze(1).repeat(1, K, 1, 1)]      # :362-363 (the 19 there is K)
        t_out = torch.clamp(boosted, min=1e-7).log()                                                      # :367
        loss = -(t_in.mean() + (ood_reg * t_out).mean())                                                  # :368, :379
        s_out, out_mean = t_out.sum(), t_out.mean()
    else:
        loss = -t_in.mean()                                                                               # :388
        s_out = out_mean = torch.zeros((), dtype=sem.dtype)
    parts = {"in_mean": t_in.mean(), "out_mean": out_mean, "S_in": t_in.sum(), "S_out": s_out, "n_in": int(id_mask.sum()), "n_ood": n_ood,
             "R": reward.detach()}
    return loss, parts


def ref_sem_full(pred_logits, pred_masks):
    """criterion.py:325-336: the class map with the no-object column.  pred_logits [B,Q,K+1], pred_masks [B,Q,h,w] -> [B,K+1,h,w]"""
    return torch.einsum("bqc,bqhw->bchw", F.softmax(pred_logits, dim=-1), pred_masks.sigmoid())


def gambler_labels(outlier_masks, sem_seg, K):
    """the one label plane of criterion.py:342-343, 371-378: outlier 1 -> 254, 255 -> void, otherwise the class (not a class: void)"""
    sem_seg = sem_seg.to(torch.int64)
    labels = torch.where((sem_seg >= 0) & (sem_seg < K), sem_seg, torch.full_like(sem_seg, 255))
    labels[outlier_masks == 255] = 255
    labels[outlier_masks == 1] = OUTLIER
    return labels


def ref_gambler_loss(pred_logits, pred_masks, outlier_masks, sem_seg, ood_reg=OOD_REG):
    """criterion.py:323-388 -> scalar"""
    return ref_gambler_tail(ref_sem_full(pred_logits, pred_masks), gambler_labels(outlier_masks, sem_seg, pred_logits.shape[-1] - 1), ood_reg)[0]


SMOOTHNESS_MODES = {"nls": "neg_logit_sum", "energy": "energy"}


def ref_smoothness(score):
    """criterion.py:270-279.  score [B,h,w] -> scalar"""
    h_shifted = torch.zeros_like(score)
    h_shifted[:, :-1, :] = score[:, 1:, :]
    h_shifted[:, -1, :] = score[:, -1, :]
    w_shifted = torch.zeros_like(score)
    w_shifted[:, :, :-1] = score[:, :, 1:]
    w_shifted[:, :, -1] = score[:, :, -1]
    return (torch.sum((h_shifted - score) ** 2) + torch.sum((w_shifted - score) ** 2)) / 2


def ref_sparsity(score, outlier_masks):
    """criterion.py:311-319.  score [B,h,w], outlier_masks [B,H,W] or None -> scalar"""
    if outlier_masks is None:
        return torch.zeros((), dtype=score.dtype)
    up = F.interpolate(score.unsqueeze(1), size=outlier_masks.shape[-2:], mode="bilinear", align_corners=True).squeeze(1)
    return torch.mean(torch.norm(up[outlier_masks == 1], dim=0))


def ref_smoothness_score(pred_logits, pred_masks, smoothness_score="energy"):
    """criterion.py:254-263"""
    return ref_score(pred_masks, F.softmax(pred_logits, dim=-1)[..., :-1], SMOOTHNESS_MODES[smoothness_score])


# ---------------------------------------------------------------------------------------------------------------- the recipe
RECIPE_YAML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pebal",
                           "maskformer2_swin_base_IN21k_384_bs16_90k_1dl_pebal_finetune.yaml")       # the reference's file, settings only


def recipe_cfg(tmp_path):
    """``load_cfg`` of the recipe with its _BASE_ chain stood in for by the criterion keys that chain sets (as tests/test_point_loss_cpu.py does
    for the outlier recipe)"""
    from rba_amd.config import load_cfg
    d = tmp_path / "pebal"
    d.mkdir(parents=True)
    shutil.copy(RECIPE_YAML, d / os.path.basename(RECIPE_YAML))
    (tmp_path / "maskformer2_R50_bs16_90k.yaml").write_text(
        "MODEL:\n  SEM_SEG_HEAD:\n    NUM_CLASSES: 19\n  MASK_FORMER:\n    DEEP_SUPERVISION: True\n    NO_OBJECT_WEIGHT: 0.1\n    CLASS_WEIGHT: 2.0\n"
        "    MASK_WEIGHT: 5.0\n    DICE_WEIGHT: 5.0\n    TRAIN_NUM_POINTS: 12544\n    OVERSAMPLE_RATIO: 3.0\n    IMPORTANCE_SAMPLE_RATIO: 0.75\n")
    return load_cfg(str(d / os.path.basename(RECIPE_YAML)))


def ref_pebal_entry(pred_logits, pred_masks, outlier_masks, sem_seg):
    """the recipe's four losses of one outputs entry (maskformer_model.py:164-175 with its settings: energy scores, squared hinge, ood_reg 0.1)"""
    score = ref_smoothness_score(pred_logits, pred_masks, "energy")
    return {"gambler_loss": ref_gambler_loss(pred_logits, pred_masks, outlier_masks, sem_seg, OOD_REG), "smoothness_loss": ref_smoothness(score),
            "sparsity_loss": ref_sparsity(score, outlier_masks),
            "outlier_loss": ref_outlier_loss(pred_logits, pred_masks, outlier_masks, "energy", "none", "squared_hinge")}


RECIPE_WEIGHTS = {"gambler_loss": 1.0, "smoothness_loss": 3e-6, "sparsity_loss": 5e-4, "outlier_loss": 1.0}


@functools.lru_cache(maxsize=None)
def criterion_inputs():
    """the "crop" fixture's final outputs and targets, and one aux_outputs entry drawn beside them: (logits, masks, aux_logits, aux_masks,
    outlier_masks, sem_seg) on the CPU"""
    logits, masks, om, ss = loss_inputs("crop")
    gen = torch.Generator().manual_seed(11250)
    return logits, masks, 2.0 * torch.randn(logits.shape, generator=gen), 3.0 * torch.randn(masks.shape, generator=gen), om, ss


def _criterion_autograd(dtype):
    logits, masks, aux_logits, aux_masks, om, ss = criterion_inputs()
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (logits, masks, aux_logits, aux_masks)]
    losses = dict(ref_pebal_entry(leaves[0], leaves[1], om, ss))
    losses.update({k + "_0": v for k, v in ref_pebal_entry(leaves[2], leaves[3], om, ss).items()})
    total = sum(v * RECIPE_WEIGHTS[k[:-2] if k.endswith("_0") else k] for k, v in losses.items())
    total.backward()
    return {k: v.detach() for k, v in losses.items()}, total.detach(), [t.grad for t in leaves]


@functools.lru_cache(maxsize=None)
def criterion_truth():
    """{"l64", "l32" = every key, "t64", "t32" = the weighted total, "g64" = its gradients for the four leaves, "b"}"""
    l64, t64, g64 = _criterion_autograd(torch.float64)
    l32, t32, g32 = _criterion_autograd(torch.float32)
    return {"l64": l64, "l32": l32, "t64": t64, "t32": t32, "g64": g64, "b": [err(a, b) for a, b in zip(g32, g64)]}


# ---------------------------------------------------------------------------------------------------------------- K11a: the tail
# (B, K, h, w, H, W): a non-integer ratio; the recipe's K, x4, two images, W across a blur tile; the smallest size the blur admits (every pixel
# sees both reflections); down-sampling (entries that are exactly 0 stay 0); a single source pixel; H not a multiple of the blur tile and W
# across one; the template edges K + 1 = 20 | 21 and K + 1 = 32
TAIL_SHAPES = ((1, 3, 7, 9, 25, 33), (2, 19, 16, 32, 64, 128), (1, 2, 2, 3, 4, 4), (1, 2, 9, 7, 5, 6), (1, 2, 1, 1, 5, 6), (1, 3, 5, 20, 7, 70),
               (1, 19, 8, 8, 32, 32), (1, 20, 8, 8, 32, 32), (1, 31, 4, 4, 9, 9))
# two laps of the partial / finish reduction (tests/_dense_hybrid_cases.py LAP_SHAPES): 263 workgroups, and the 2048 cap
LAP_SHAPES = ((1, 3, 16, 16, 261, 257), (1, 3, 16, 16, 725, 727))
# found by the size-pair sweep (tests/test_training_kernel_fuzz_gpu.py; tests/_dense_hybrid_cases.py FOUND_SHAPES): down-sampling pairs whose
# destinations land on source pixels exactly -- the second tap's weight is 0 in torch and was -2^-22 in the backward's fused product.  (Listed
# after LAP_SHAPES: the seeds are indices into the concatenation.)
FOUND_SHAPES = ((2, 2, 28, 33, 13, 11),)
MIN_R = 0.25


@functools.lru_cache(maxsize=None)
def tail_inputs(shape):
    """(sem [B,K+1,h,w] = 1.2 rand -- the class map's own range --, labels [B,H,W] int64: K10's draw) on the CPU, seeded by the shape"""
    B, K, h, w, H, W = shape
    gen = torch.Generator().manual_seed(11100 + (TAIL_SHAPES + LAP_SHAPES + FOUND_SHAPES).index(shape))
    sem = 1.2 * torch.rand(B, K + 1, h, w, generator=gen)
    return sem, draw_labels(gen, B, K, H, W)


def _tail_autograd(sem, labels, dtype):
    s = sem.to(dtype).clone().requires_grad_(True)
    loss, parts = ref_gambler_tail(s, labels)
    loss.backward()
    return loss.detach(), {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in parts.items()}, s.grad


@functools.lru_cache(maxsize=None)
def tail_truth(shape):
    """fp64 and fp32 CPU autograd: {"l64", "l32", "parts64", "parts32", "g64" = d loss / d sem, "b" = fp32 autograd's error}.  A fixture whose
    blurred reward comes near 0 would make the division by R ill-conditioned: it fails here, as a fixture, not as the kernel."""
    sem, labels = tail_inputs(shape)
    l64, p64, g64 = _tail_autograd(sem, labels, torch.float64)
    l32, p32, g32 = _tail_autograd(sem, labels, torch.float32)
    assert float(p64["R"].min()) >= MIN_R, f"fixture {shape}: min R64 = {float(p64['R'].min()):.3g} < {MIN_R}"
    return {"l64": l64, "l32": l32, "parts64": p64, "parts32": p32, "g64": g64, "b": err(g32, g64)}


# ---------------------------------------------------------------------------------------------------------------- the blur and its adjoint
BLUR_SHAPES = ((1, 4, 4), (2, 5, 9), (1, 7, 70), (1, 64, 128))


@functools.lru_cache(maxsize=None)
def blur_inputs(shape):
    """(planes u [B,H,W], cotangent v [B,H,W]) on the CPU"""
    gen = torch.Generator().manual_seed(11300 + BLUR_SHAPES.index(shape))
    return 1.0 + torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen)


@functools.lru_cache(maxsize=None)
def blur_truth(shape):
    """{"y64" = A u, "g64" = A^T v by fp64 autograd, "b_y", "b_g" = the fp32 restatement's errors}"""
    u, v = blur_inputs(shape)
    out = {}
    for dtype in (torch.float64, torch.float32):
        x = u.to(dtype).clone().requires_grad_(True)
        y = ref_blur(x)
        (y * v.to(dtype)).sum().backward()
        out[dtype] = (y.detach(), x.grad)
    (y64, g64), (y32, g32) = out[torch.float64], out[torch.float32]
    return {"y64": y64, "g64": g64, "b_y": err(y32, y64), "b_g": err(g32, g64)}


# ---------------------------------------------------------------------------------------------------------------- K11b
# (B, h, w, H, W): K9's shapes -- a non-integer ratio; x4, two images; down-sampling; a single source pixel; axes that do not resample
REG_SHAPES = ((1, 7, 9, 25, 33), (2, 32, 64, 128, 256), (1, 9, 7, 4, 3), (1, 1, 1, 5, 6), (1, 3, 1, 3, 8), (1, 1, 5, 1, 5))
REG_LAP_SHAPES = ((1, 16, 16, 261, 257), (1, 16, 16, 725, 727))     # the same two laps for K11b
REG_UPSTREAM = ((1.0, 0.0), (0.0, 1.0), (0.5, 2.0))                 # (d / d smoothness, d / d sparsity): each alone, both together


@functools.lru_cache(maxsize=None)
def reg_inputs(shape):
    """(score [B,h,w] = -(3 + randn), the energy score's range; labels [B,H,W] int64: 60 % inlier (0), 25 % outlier (1), 15 % void (255); a map of at
    most 32 pixels gets one outlier pixel whatever the draw) on the CPU"""
    B, h, w, H, W = shape
    gen = torch.Generator().manual_seed(11400 + (REG_SHAPES + REG_LAP_SHAPES).index(shape))
    score = -(3.0 + torch.randn(B, h, w, generator=gen))
    r = torch.rand(B, H, W, generator=gen)
    labels = torch.full((B, H, W), 255, dtype=torch.int64)
    labels[r < 0.6] = 0
    labels[r < 0.25] = 1
    if B * H * W <= 32:
        labels.view(-1)[-1] = 1
    assert (labels == 1).any()
    return score, labels


def _reg_autograd(score, labels, dtype, up):
    s = score.to(dtype).clone().requires_grad_(True)
    smooth, sparse = ref_smoothness(s), ref_sparsity(s, labels)
    (up[0] * smooth + up[1] * sparse).backward()
    return smooth.detach(), sparse.detach(), s.grad


@functools.lru_cache(maxsize=None)
def reg_truth(shape, labelled=True):
    """{"sm64", "sm32", "sp64", "sp32", "g64"[upstream], "b"[upstream]}; labelled=False: no labels at all (sparsity 0)"""
    score, labels = reg_inputs(shape)
    labels = labels if labelled else None
    t = {"g64": {}, "b": {}}
    for up in REG_UPSTREAM:
        sm64, sp64, g64 = _reg_autograd(score, labels, torch.float64, up)
        sm32, sp32, g32 = _reg_autograd(score, labels, torch.float32, up)
        g64 = torch.zeros_like(score, dtype=torch.float64) if g64 is None else g64
        g32 = torch.zeros_like(score) if g32 is None else g32
        t["g64"][up], t["b"][up] = g64, (err(g32, g64) if float(g64.abs().max()) > 0 else 0.0)
        t.update(sm64=sm64, sm32=sm32, sp64=sp64, sp32=sp32)
    return t


# ---------------------------------------------------------------------------------------------------------------- the losses end to end
# (B, Q, K, h, w, H, W)
LOSS_SHAPES = {"small": (1, 20, 5, 7, 9, 25, 33), "crop": (2, 100, 19, 32, 64, 128, 256)}


@functools.lru_cache(maxsize=None)
def loss_inputs(shape):
    """(pred_logits [B,Q,K+1], pred_masks [B,Q,h,w], outlier_masks [B,H,W] int64: 0 / 1 / 255, sem_seg [B,H,W] int64: classes, 255 where the pixel
    is an outlier or void, about 2 % 200 -- a value that is no class: void) on the CPU, from K10's label draw"""
    B, Q, K, h, w, H, W = LOSS_SHAPES[shape]
    gen = torch.Generator().manual_seed(11200 + sorted(LOSS_SHAPES).index(shape))
    logits = 2.0 * torch.randn(B, Q, K + 1, generator=gen)
    masks = 3.0 * torch.randn(B, Q, h, w, generator=gen)
    labels = draw_labels(gen, B, K, H, W)
    outlier_masks = torch.zeros_like(labels)
    outlier_masks[labels == OUTLIER] = 1
    outlier_masks[labels == 255] = 255
    sem_seg = labels.clone()
    sem_seg[labels == OUTLIER] = 255
    return logits, masks, outlier_masks, sem_seg


def _leaves_autograd(fn, logits, masks, dtype):
    lg, mk = logits.to(dtype).clone().requires_grad_(True), masks.to(dtype).clone().requires_grad_(True)
    loss = fn(lg, mk)
    loss.backward()
    return loss.detach(), lg.grad, mk.grad


def leaves_truth(fn, logits, masks):
    """fp64 / fp32 CPU autograd of a scalar fn(pred_logits, pred_masks): {"l64", "l32", "g64" = (d / d pred_logits, d / d pred_masks), "b"}"""
    l64, *g64 = _leaves_autograd(fn, logits, masks, torch.float64)
    l32, *g32 = _leaves_autograd(fn, logits, masks, torch.float32)
    return {"l64": l64, "l32": l32, "g64": tuple(g64), "b": tuple(err(a, b) for a, b in zip(g32, g64))}


@functools.lru_cache(maxsize=None)
def loss_truth(shape):
    logits, masks, om, ss = loss_inputs(shape)
    sem64 = ref_sem_full(logits.double(), masks.double())
    r64 = ref_gambler_tail(sem64, gambler_labels(om, ss, logits.shape[-1] - 1))[1]["R"]
    assert float(r64.min()) >= MIN_R, f"fixture {shape}: min R64 = {float(r64.min()):.3g} < {MIN_R}"
    return leaves_truth(lambda lg, mk: ref_gambler_loss(lg, mk, om, ss), logits, masks)
