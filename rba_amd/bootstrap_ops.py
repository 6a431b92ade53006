"""Python entry points of K18 (csrc/bootstrap_curve.hip, docs/kernels/K18.md): the ROC and precision-recall curves of up to 64 image subsets -- the trials
of OODEvaluator.evaluate_ood_bootstrapped (support.py:305-351) -- from one globally sorted pixel list, and the producer of that list's (score, tag) pairs.

Written in rba_amd.ops' style with its decorator, validators and launch line (as rba_amd.panoptic_ops and rba_amd.instance_ops): a wrapper reads top to
bottom as its checks, its output allocation, its `_launch` lines; a bad argument raises RbaHipError before anything is allocated or enqueued; there is no
fallback path."""
import torch

from ._lib import RbaHipError
from .ops import _chk, _hip_op, _launch, _p

MAX_TRIALS = 64               # one lane of a wave per trial
MAX_IMAGES = 1 << 30          # K18_MAX_IMAGES: the tag is (image_index << 1) | label in an int32
MAX_PIXELS = (1 << 31) - 1    # counts are 32-bit in registers
FILL_WAVES = 8192             # 256 CUs x 4 SIMDs x 8 waves: the chunk passes run one wave per chunk


def default_chunk(n):
    """The pixels per wave of the two chunk passes for a list of n pixels: enough chunks to fill the device (FILL_WAVES), between 2048 and 8192 -- fewer
    pixels per wave only multiply the per-chunk integers and the serial sum of the chunks' ap partials (docs/kernels/K18.md, docs/measurements.md)."""
    return min(8192, max(2048, -(-n // FILL_WAVES) + 63 & ~63))


# ---------------------------------------------------------------------------------------------------------------- argument contracts, each written once
def _sorted_list(score, tag):
    """score fp32 [n] (sorted descending by the caller) and tag int32 [n] = (image_index << 1) | label in the same order, 1 <= n < 2^31 -> n"""
    _chk(score, "score", dim=1)
    _chk(tag, "tag", dtype=torch.int32, dim=1)
    if score.numel() != tag.numel():
        raise RbaHipError(f"score and tag must have the same length, got {score.numel()} and {tag.numel()}")
    if not 1 <= score.numel() <= MAX_PIXELS:
        raise RbaHipError(f"the sorted list holds 1 <= n < 2^31 pixels, got {score.numel()}")
    return score.numel()


def _trials(member, T):
    """member int64 [n_images]: the 64 bits of an image's membership word (bit t set = the image belongs to trial t; torch has no arithmetic on uint64, the
    kernels read the same eight bytes as uint64), 1 <= n_images <= 2^30, and 1 <= T <= 64 trials -> (n_images, T)"""
    if isinstance(T, bool) or not isinstance(T, int) or not 1 <= T <= MAX_TRIALS:
        raise RbaHipError(f"T must be an int with 1 <= T <= {MAX_TRIALS} trials, got {T!r}")
    _chk(member, "member", dtype=torch.int64, dim=1)
    if not 1 <= member.numel() <= MAX_IMAGES:
        raise RbaHipError(f"member must hold 1 <= n_images <= 2^30 words, got {member.numel()}")
    return member.numel(), T


def _chunk(chunk):
    if isinstance(chunk, bool) or not isinstance(chunk, int) or not 64 <= chunk <= 1 << 20 or chunk % 64:
        raise RbaHipError(f"chunk must be a multiple of 64 in [64, 2^20], got {chunk!r}")
    return chunk


def _image_index(image_index):
    if isinstance(image_index, bool) or not isinstance(image_index, int) or not 0 <= image_index < MAX_IMAGES:
        raise RbaHipError(f"image_index must be an int with 0 <= image_index < 2^30, got {image_index!r}")
    return image_index


@_hip_op
def subset_curves(score, tag, member, T, chunk=None):
    """K18.  score fp32 [n] sorted descending, tag int32 [n], member int64 [n_images] (`_sorted_list`, `_trials`) -> dict of device tensors [T]:
    P, N (int64: the subset's positive and negative pixels), auroc2 (int64, exact: sum of dfp * (tp_prev + tp) over the subset's thresholds = twice the
    trapezoid area times P * N), ap (float64: sum of dtp * tp / (tp + fp), bitwise reproducible), fp95, tp95 (int64: the counts at the first ROC point
    kept by scikit-learn's drop_intermediate with tp / P > 0.95; both 0 when P = 0).  `chunk` (tests and tools): the pixels per wave, `default_chunk(n)` when None.

    Three launches and, between the first two, the prefix of the per-chunk totals as torch ops on [T, 2, chunks] integers; nothing is read back."""
    n = _sorted_list(score, tag)
    n_images, T = _trials(member, T)
    chunk = _chunk(default_chunk(n) if chunk is None else chunk)
    dev, chunks = score.device, -(-n // chunk)
    totals = torch.empty((T, 2, chunks), dtype=torch.int32, device=dev)             # (tp, cnt) planes, the chunk index innermost: the scan's dimension
    upto_end = torch.empty((T, 2, chunks), dtype=torch.int32, device=dev)
    has_end = torch.empty(chunks, dtype=torch.int32, device=dev)
    _launch("rba_subset_curves_totals", _p(score), _p(tag), _p(member), n, n_images, T, chunk, _p(totals), _p(upto_end), _p(has_end))
    # the prefix over chunks: counts in front of each chunk, and at the last run end in front of it (a run may span any number of chunks)
    ends = torch.cumsum(totals, -1, dtype=torch.int64)
    base = ends - totals
    at_end = base + upto_end                                                        # at the last run end INSIDE chunk c (where it has one)
    index = torch.where(has_end > 0, torch.arange(chunks, device=dev), torch.full((chunks,), -1, device=dev))
    before = torch.cat([index.new_full((1,), -1), torch.cummax(index, 0).values[:-1]])      # the last chunk in front of c that has a run end
    prev = torch.where(before >= 0, at_end.index_select(-1, before.clamp(min=0)), torch.zeros_like(at_end)).contiguous()
    auroc2 = torch.zeros(T, dtype=torch.int64, device=dev)
    ap_part = torch.empty((T, chunks), dtype=torch.float64, device=dev)
    _launch("rba_subset_curves_walk", _p(score), _p(tag), _p(member), n, n_images, T, chunk, _p(base), _p(prev), _p(auroc2), _p(ap_part))
    ap = torch.empty(T, dtype=torch.float64, device=dev)
    at95 = torch.empty((T, 2), dtype=torch.int64, device=dev)
    _launch("rba_subset_curves_finish", _p(score), _p(tag), _p(member), n, n_images, T, chunk, _p(base), _p(prev), _p(ends), _p(ap_part), _p(ap),
            _p(at95))
    P = ends[:, 0, -1]
    return {"P": P, "N": ends[:, 1, -1] - P, "auroc2": auroc2, "ap": ap, "fp95": at95[:, 0], "tp95": at95[:, 1]}


@_hip_op
def labelled_tags(score, labels, image_index, out_score, out_tag, cursor):
    """K18's input.  score fp32 (any shape) and labels uint8 or int64 of the same number of pixels, one image; appends (score, (image_index << 1) | label)
    of every pixel labelled 0 or 1 to out_score fp32 [capacity] / out_tag int32 [capacity] at the device-side cursor (int64 [2], zeroed by the caller
    before the first image: [0] = pairs asked for so far, [1] = 1 once a pair did not fit).  No host synchronisation; the caller reads `cursor` once after
    the last image.  Order within the buffer is unspecified."""
    _chk(score, "score")
    _chk(labels, "labels", dtype=torch.uint8 if isinstance(labels, torch.Tensor) and labels.dtype == torch.uint8 else torch.int64)
    if labels.numel() != score.numel() or not 1 <= score.numel() <= MAX_PIXELS:
        raise RbaHipError(f"score and labels must hold the same 1 <= n < 2^31 pixels, got {score.numel()} and {labels.numel()}")
    image_index = _image_index(image_index)
    _chk(out_score, "out_score", dim=1)
    _chk(out_tag, "out_tag", dtype=torch.int32, dim=1)
    if out_score.numel() != out_tag.numel():
        raise RbaHipError(f"out_score and out_tag must have the same capacity, got {out_score.numel()} and {out_tag.numel()}")
    _chk(cursor, "cursor", dtype=torch.int64, dim=1)
    if cursor.numel() != 2:
        raise RbaHipError(f"cursor must have 2 elements, got {cursor.numel()}")
    _launch("rba_labelled_tags_i32", _p(score), _p(labels), labels.element_size(), score.numel(), image_index, _p(out_score), _p(out_tag),
            out_score.numel(), _p(cursor))


def member_words(members, device):
    """members: bool [T, n_images] (numpy or torch), T <= 64 -> int64 [n_images] on `device`, bit t of word i = members[t, i]"""
    m = torch.as_tensor(members).to(torch.bool)
    if m.dim() != 2 or not 1 <= m.shape[0] <= MAX_TRIALS:
        raise RbaHipError(f"members must be [T, n_images] with 1 <= T <= {MAX_TRIALS}, got shape {tuple(m.shape)}")
    bits = [1 << t if t < 63 else -(1 << 63) for t in range(m.shape[0])]                   # bit 63 is the sign of the int64 that carries the word
    weights = torch.tensor(bits, dtype=torch.int64)
    return (m.to(torch.int64) * weights[:, None]).sum(0).to(device).contiguous()


__all__ = ["subset_curves", "labelled_tags", "member_words", "default_chunk", "MAX_TRIALS", "MAX_IMAGES"]
