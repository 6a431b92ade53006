"""Shared by tests/test_dense_hybrid_loss_gpu.py, tests/test_densehybrid_finetune_gpu.py and tools/dense_hybrid_loss_probe.py: the torch
restatement of the reference's DenseHybrid loss, seeded inputs and the fp64 / fp32 CPU autograd truths.

The restatement (``ref_tail``, ``ref_densehybrid_loss``) is written from mask2former/modeling/criterion.py:93-97 and :390-433 of the reference.
Its parity is PINNED BY REFERENCE CODE inside the reference's domain (labels that are a class, 254 or 255): tests/golden/g9_criterion.npz holds what
the reference's own ``densehybrid_loss`` computes (loss and float64 gradients at "small", at K = 19 and at the "crop"), and
tests/test_criterion_reference_cpu.py holds this restatement to it at relative 1e-12.  One departure, of the kernel's contract and outside that
domain (so against this restatement only): a label that is neither a class nor 254 is ignored by the segmentation term whatever its value (the
reference maps 254 and 255 to ``ignore_index``; any other value is an index error there).  The targets are not written, here or in the reference:
its relabelling acts on a ``torch.cat`` copy.  Error metric, bar and checks are those of tests/_rba_bwd_cases.py and tests/_point_loss_cases.py.
"""
import functools

import torch
import torch.nn.functional as F

from tests._rba_bwd_cases import err

OUTLIER = 254


def ref_tail(sem, ood, labels, beta):
    """criterion.py:406-431 behind the class map.  sem [B,K,h,w], ood [B,2,h,w], labels [B,H,W] int64 -> (loss, parts), parts = the kernel's
    losses[1:4] and stats as a dict of scalars"""
    K = sem.shape[1]
    logits = F.interpolate(sem, size=labels.shape[-2:], mode="bilinear", align_corners=True)              # :406
    logits_ood = F.interpolate(ood, size=labels.shape[-2:], mode="bilinear", align_corners=True)          # :407
    cls_out, ood_out = F.log_softmax(logits, dim=1), F.log_softmax(logits_ood, dim=1)                     # :410-411
    label_ood = (labels == OUTLIER).to(labels.dtype)                                                      # :413-414
    lse = torch.logsumexp(logits, dim=1) * label_ood                                                      # :415
    m = logits.mean(1).mean()                                                                             # get_batch_avg, :93-97
    reg = -m.view(1, 1, 1).repeat(*labels.shape) * label_ood
    n_ood = label_ood[label_ood == 1].numel()
    loss_ood = (lse + reg.detach()).sum() / n_ood                                                         # :423 (0 / 0 = NaN without an outlier pixel)
    seg_labels = torch.where((labels >= 0) & (labels < K), labels, torch.full_like(labels, K))            # :424-425, every other value too
    loss_seg = F.nll_loss(cls_out, seg_labels, ignore_index=K)                                            # :427
    loss_th = F.nll_loss(ood_out, label_ood, ignore_index=2)                                              # :429
    loss = loss_seg + beta * loss_ood + beta * 10 * loss_th                                               # :431
    parts = {"loss_seg": loss_seg, "loss_ood": loss_ood, "loss_th": loss_th,
             "S_seg": F.nll_loss(cls_out, seg_labels, ignore_index=K, reduction="sum"), "S_ood": lse.sum(),
             "S_th": F.nll_loss(ood_out, label_ood, ignore_index=2, reduction="sum"), "S_x": logits.sum(),
             "n_seg": int((seg_labels < K).sum()), "n_ood": n_ood, "n_all": labels.numel(), "m": m}
    return loss, parts


def ref_sem(pred_logits, pred_masks):
    """criterion.py:392-405: the class map.  pred_logits [B,Q,K+1], pred_masks [B,Q,h,w] -> [B,K,h,w]"""
    return torch.einsum("bqc,bqhw->bchw", F.softmax(pred_logits, dim=-1)[..., :-1], pred_masks.sigmoid())


def ref_densehybrid_loss(pred_logits, pred_masks, ood_pred, labels, beta=0.03):
    """criterion.py:390-433 -> scalar"""
    return ref_tail(ref_sem(pred_logits, pred_masks), ood_pred, labels, beta)[0]


def draw_labels(gen, B, K, H, W):
    """classes uniform in [0, K); 15 % -> 254; 10 % -> 255; about 2 % -> 200 (a value the reference does not know: ignored); a map of at most 32
    pixels gets one class pixel and one outlier pixel whatever the draw"""
    labels = torch.randint(0, K, (B, H, W), generator=gen)
    r = torch.rand(B, H, W, generator=gen)
    labels[r < 0.15] = OUTLIER
    labels[(r >= 0.15) & (r < 0.25)] = 255
    labels[(r >= 0.25) & (r < 0.27)] = 200
    if B * H * W <= 32:
        labels.view(-1)[0], labels.view(-1)[-1] = K - 1, OUTLIER
    assert ((labels >= 0) & (labels < K)).any() and (labels == OUTLIER).any(), "fixture: n_seg > 0 and n_ood > 0"
    return labels


# (B, K, h, w, H, W): a non-integer ratio; the recipe's K, x4, two images; down-sampling (some pixels get no gradient); a single source pixel; an
# axis that does not resample; the template edges K = 20 | 21 and K = 32
TAIL_SHAPES = ((1, 3, 7, 9, 25, 33), (2, 19, 16, 32, 64, 128), (1, 2, 9, 7, 4, 3), (1, 2, 1, 1, 5, 6), (1, 3, 3, 1, 3, 8),
               (1, 20, 8, 8, 32, 32), (1, 21, 8, 8, 32, 32), (1, 32, 4, 4, 9, 9))
# two laps of the partial / finish reduction, a 16 x 16 class map under one large label map: 263 workgroups (the finishing workgroup's threads 0 .. 6
# take a second record; a ragged last workgroup), and the 2048 cap (every partial thread walks a second pixel; the finish's eighth lap)
LAP_SHAPES = ((1, 3, 16, 16, 261, 257), (1, 3, 16, 16, 725, 727))
# found by the size-pair sweep (tests/test_training_kernel_fuzz_gpu.py): 19 -> 11 columns put label column 5 on source column 9 exactly, and the
# backward's fused product gave its second tap, column 10, a weight of -2^-22 where torch gives 0 -- a source pixel of column 10 whose other label
# pixel is void must be exactly 0.  (Listed after LAP_SHAPES: the seeds are indices into the concatenation.)
FOUND_SHAPES = ((2, 2, 35, 19, 18, 11),)
BETA = 0.03
PART_NAMES = ("loss_seg", "loss_ood", "loss_th", "S_seg", "S_ood", "S_th", "S_x", "n_seg", "n_ood", "n_all", "m")


@functools.lru_cache(maxsize=None)
def tail_inputs(shape):
    """(sem [B,K,h,w] = 1.5 + 2 randn -- a positive mean, like the class map's, so that S_x and m are not sums that cancel to nothing --, ood
    [B,2,h,w] = 1.5 randn, labels [B,H,W] int64) on the CPU, seeded by the shape"""
    B, K, h, w, H, W = shape
    gen = torch.Generator().manual_seed(10100 + (TAIL_SHAPES + LAP_SHAPES + FOUND_SHAPES).index(shape))
    sem = 1.5 + 2.0 * torch.randn(B, K, h, w, generator=gen)
    ood = 1.5 * torch.randn(B, 2, h, w, generator=gen)
    return sem, ood, draw_labels(gen, B, K, H, W)


def _tail_autograd(sem, ood, labels, dtype):
    s, o = sem.to(dtype).clone().requires_grad_(True), ood.to(dtype).clone().requires_grad_(True)
    loss, parts = ref_tail(s, o, labels, BETA)
    loss.backward()
    return loss.detach(), {k: (float(v.detach()) if isinstance(v, torch.Tensor) else v) for k, v in parts.items()}, s.grad, o.grad


@functools.lru_cache(maxsize=None)
def tail_truth(shape):
    """fp64 and fp32 CPU autograd: {"l64", "l32", "parts64", "parts32", "gs64" = d loss / d sem, "go64" = d loss / d ood, "b_sem", "b_ood"}"""
    sem, ood, labels = tail_inputs(shape)
    l64, p64, gs64, go64 = _tail_autograd(sem, ood, labels, torch.float64)
    l32, p32, gs32, go32 = _tail_autograd(sem, ood, labels, torch.float32)
    return {"l64": l64, "l32": l32, "parts64": p64, "parts32": p32, "gs64": gs64, "go64": go64, "b_sem": err(gs32, gs64), "b_ood": err(go32, go64)}


# (B, Q, K, h, w, H, W)
LOSS_SHAPES = {"small": (1, 20, 5, 7, 9, 25, 33), "crop": (2, 100, 19, 32, 64, 128, 256)}


@functools.lru_cache(maxsize=None)
def loss_inputs(shape):
    """(pred_logits [B,Q,K+1], pred_masks [B,Q,h,w], ood_pred [B,2,h,w], labels [B,H,W] int64) on the CPU"""
    B, Q, K, h, w, H, W = LOSS_SHAPES[shape]
    gen = torch.Generator().manual_seed(10200 + sorted(LOSS_SHAPES).index(shape))
    logits = 2.0 * torch.randn(B, Q, K + 1, generator=gen)
    masks = 3.0 * torch.randn(B, Q, h, w, generator=gen)
    ood = 1.5 * torch.randn(B, 2, h, w, generator=gen)
    return logits, masks, ood, draw_labels(gen, B, K, H, W)


def _loss_autograd(logits, masks, ood, labels, dtype):
    leaves = [t.to(dtype).clone().requires_grad_(True) for t in (logits, masks, ood)]
    loss = ref_densehybrid_loss(*leaves, labels, BETA)
    loss.backward()
    return (loss.detach(),) + tuple(t.grad for t in leaves)


@functools.lru_cache(maxsize=None)
def loss_truth(shape):
    """{"l64", "l32", "g64" = (d / d pred_logits, d / d pred_masks, d / d ood_pred), "b" = fp32 CPU autograd's error of each}"""
    args = loss_inputs(shape)
    l64, *g64 = _loss_autograd(*args, torch.float64)
    l32, *g32 = _loss_autograd(*args, torch.float32)
    return {"l64": l64, "l32": l32, "g64": tuple(g64), "b": tuple(err(a, b) for a, b in zip(g32, g64))}
