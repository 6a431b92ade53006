"""Python entry points of the HIP kernels: validate (device / dtype / contiguity / shape), allocate the
output with torch (device memory + stream plumbing only) and enqueue the kernel on torch's current stream.

A wrapper reads top to bottom as: its checks (calls of the validators below, one per argument contract), its output allocation, one `_launch` line.

Error behaviour mirrors the reference's native op (pixel_decoder/ops/src/cuda/ms_deform_attn_cuda.cu:33-43:
AT_ASSERTM on contiguity and device -> RuntimeError): a bad argument raises RuntimeError (RbaHipError); there is
no fallback path.
"""
import contextlib
import ctypes
import threading
import functools
import math
import os

import torch

from . import _lib
from ._lib import RbaHipError
from .lru import derived


def _stream():
    """The HIP stream a kernel is enqueued on: torch's current stream of the CURRENT device -- which `_hip_op` has made the
    device of the call's tensors."""
    return torch.cuda.current_stream().cuda_stream


def _launch(name, *args, stream=None):
    """THE launch line: entry point `name` of the current kernel library (read at call time, so `_lib.use_library` holds) with `args` and the current
    stream (`stream`: one read by the caller for several launches); a hipError_t other than 0 raises RbaHipError naming the entry point."""
    code = getattr(_lib.load(), name)(*args, torch.cuda.current_stream().cuda_stream if stream is None else stream)
    if code:
        _lib.check(code, name)


def _query(name, *args):
    """A host-side question to the current library (`*_bytes`, `*_elems`, `*_supported`, ...): no stream, the answer is returned as it is."""
    return getattr(_lib.load(), name)(*args)


def _cuda_tensors(args):
    for a in args:
        if isinstance(a, torch.Tensor):
            if a.is_cuda:
                yield a
        elif isinstance(a, (list, tuple)):
            yield from _cuda_tensors(a)
        elif isinstance(a, SplitActivations):
            if a.data.is_cuda:
                yield a.data
        elif isinstance(a, torch.nn.Module):
            yield from (p_ for p_ in a.parameters(recurse=False) if p_.is_cuda)


def _hip_op(fn):
    """Every launch wrapper: all device tensors of a call must live on ONE HIP device (RbaHipError otherwise), and the call
    runs with that device current, so outputs, workspaces, `_stream()` and the kernel all refer to the tensors' device and its
    current stream -- also when the caller never called torch.cuda.set_device (get_model(device="cuda:1"))."""
    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = None
        for t in _cuda_tensors(args + tuple(kwargs.values())):
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise RbaHipError(f"{fn.__name__}: tensors on different devices ({dev} and {t.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


# ---------------------------------------------------------------------------------------------------------------- argument contracts, each written once
def _chk(t, name, dtype=torch.float32, dim=None):
    if not isinstance(t, torch.Tensor):
        raise RbaHipError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RbaHipError(f"{name} must be a HIP (cuda) tensor; rba_amd kernels have no CPU path")
    if t.dtype != dtype:
        raise RbaHipError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RbaHipError(f"{name} tensor has to be contiguous")
    if dim is not None and t.dim() != dim:
        raise RbaHipError(f"{name} must have {dim} dims, got shape {tuple(t.shape)}")
    return t


def _vec(t, name, n, optional=False):
    """A bias, a norm's weight or bias: an fp32 vector of exactly n elements (the kernels take a bare pointer and read n); None only where `optional`."""
    if t is None and optional:
        return None
    _chk(t, name, dim=1)
    if t.numel() != n:
        raise RbaHipError(f"{name} must have {n} elements, got {t.numel()}")
    return t


def _shaped(t, name, shape, optional=False):
    """An fp32 tensor of exactly `shape` (a residual, an addend, a gradient); None only where `optional`."""
    if t is None and optional:
        return None
    _chk(t, name)
    if tuple(t.shape) != tuple(shape):
        raise RbaHipError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _one_element(t, name):
    """An upstream gradient of a scalar loss: a one-element fp32 device tensor (the kernels read it on the device)."""
    if _chk(t, name).numel() != 1:
        raise RbaHipError(f"{name} must have one element, got shape {tuple(t.shape)}")
    return t


def _labels(labels, name="labels"):
    """The label map of the loss kernels K9 - K11: int64 or uint8, contiguous, [B,H,W] -> bytes per label (what the entry points' `label_bytes` takes)."""
    _chk(labels, name, dtype=torch.uint8 if isinstance(labels, torch.Tensor) and labels.dtype == torch.uint8 else torch.int64, dim=3)
    return labels.element_size()


def _packed(planes, K, out_features=None, bf16x6=True):
    """The layout contract of split_weight's output for a weight [N, K]: [ceil(N / 128), K / 16, P, 128, 2, 8] with P = 2 float16 planes (the f16x3 form) or,
    where the wrapper has a bf16x6 kernel, P = 3 bfloat16 planes -- the dtype says which.  N = ``out_features``, or all packed rows.  -> (N, f16)."""
    f16 = planes.dtype == torch.float16 or not bf16x6
    _chk(planes, "planes", dtype=torch.float16 if f16 else torch.bfloat16, dim=6)
    N = planes.shape[0] * 128 if out_features is None else int(out_features)
    if tuple(planes.shape[2:]) != ((2, 128, 2, 8) if f16 else (3, 128, 2, 8)) or planes.shape[1] * 16 != K or (N + 127) // 128 != planes.shape[0]:
        raise RbaHipError(f"planes must be split_weight(W [N, K]) for N = {N}, K = {K}: [ceil(N/128), K/16, 2 | 3, 128, 2, 8] float16 | bfloat16, "
                          f"got {tuple(planes.shape)} {planes.dtype}")
    return N, f16


def _split_x(x, who, dim=None):
    """An activation operand that is fp32 rows or SplitActivations (of logical rank `dim`) -> (pointer, is_split)."""
    if not isinstance(x, SplitActivations):
        return _chk(x, "x", dim=dim).data_ptr(), False
    _chk(x.data, "x.data", dtype=torch.int32, dim=1)
    if dim is not None and len(x.shape) != dim:
        raise RbaHipError(f"{who} needs SplitActivations of logical rank {dim}, got shape {x.shape}")
    return x.data.data_ptr(), True


def _split_into_ok(split_into, image, H, W, C):
    """``split_into`` of the channels-last resamplers: SplitActivations of logical shape [B, H, W, C] whose image `image` the launch fills."""
    if (not isinstance(split_into, SplitActivations) or len(split_into.shape) != 4 or tuple(split_into.shape[1:]) != (H, W, C) or C % 32
            or not 0 <= image < split_into.shape[0]):
        raise RbaHipError("split_into must be SplitActivations of shape [B, H, W, C] (C % 32 == 0) with 0 <= image < B")


def _gn_nhwc_ok(C, num_groups):
    return C % num_groups == 0 and (C // num_groups) % 4 == 0 and C <= 1024 and 256 % (C // 4) == 0


def _tiles128(M, N):
    """Number of 128 x 128 output tiles of an [M, N] GEMM (csrc: tiles128) -- what the dispatch predicates below count."""
    return ((M + 127) // 128) * ((N + 127) // 128)


def _scratch(nbytes, device, min_words=1):
    """Per-call scratch of at least `nbytes` for a kernel that writes every word it later reads."""
    return torch.empty(max(nbytes // 4, min_words), dtype=torch.float32, device=device)


def _p(t):
    return 0 if t is None else t.data_ptr()


SCORE_MODES = {"rba": 0, "energy": 1, "neg_logit_sum": 2}


def _mode(score):
    if score not in SCORE_MODES:
        raise RbaHipError(f"unknown score {score!r}; choose from {sorted(SCORE_MODES)}")
    return SCORE_MODES[score]


_STREAM_WORKSPACES = {}   # (device, stream, kind) -> buffer: "tiles" (K1's counter) and one kind per kernel with partial sums


def _stream_workspace(kind, device, words, alloc, dtype):
    """The per-(device, stream) buffers: one of each kind per stream that launches, replaced by a larger one when a call needs more.  Launches that
    share a buffer are ordered by their stream, and torch's allocator keeps a replaced buffer's memory on that stream."""
    key = (device.index, _stream(), kind)                # called under _hip_op: the current device IS `device`
    ws = _STREAM_WORKSPACES.get(key)
    if ws is None or ws.numel() < words:
        ws = _STREAM_WORKSPACES[key] = alloc(words, dtype=dtype, device=device)
    return ws


def _k1_workspace(device):
    """8 zeroed bytes per (device, stream) for K1's dynamic tile counter (the kernel leaves them zero)."""
    return _stream_workspace("tiles", device, 2, torch.zeros, torch.int32)


def _workspace(query_name, kind, device, *dims):
    """A kernel's partial sums (K1 / K4 backward, match_cost, the loss kernels K9 - K11): the library's `query_name(*dims, &bytes)` says how many bytes
    this call needs -> (the stream's `kind` buffer of at least that size, the bytes).  Grow-only (a run over varying sizes keeps the largest, not one
    per size); every such kernel writes each word it later reads."""
    n = ctypes.c_int64(0)
    _lib.check(_query(query_name, *dims, ctypes.addressof(n)), query_name)
    return _stream_workspace(kind, device, max(int(n.value) // 4, 1), torch.empty, torch.float32), int(n.value)


@_hip_op
def rba_reduce(mask_pred, cls_prob, want_sem_seg=False, want_argmax=False, score="rba"):
    """K1.  mask_pred [Q,H,W] full-resolution mask logits, cls_prob [Q,K] -> (rba [H,W], sem_seg [K,H,W] | None,
    argmax int32 [H,W] | None).  maskformer_model.py:381-386 + evaluate_ood.py:150 + support.py:385-388."""
    _chk(mask_pred, "mask_pred", dim=3)
    _chk(cls_prob, "cls_prob", dim=2)
    Q, H, W = mask_pred.shape
    if cls_prob.shape[0] != Q:
        raise RbaHipError(f"cls_prob has {cls_prob.shape[0]} queries, mask_pred {Q}")
    K = cls_prob.shape[1]
    mode = _mode(score)
    dev = mask_pred.device
    rba = torch.empty((H, W), dtype=torch.float32, device=dev)
    sem = torch.empty((K, H, W), dtype=torch.float32, device=dev) if want_sem_seg else None
    arg = torch.empty((H, W), dtype=torch.int32, device=dev) if want_argmax else None
    _launch("rba_reduce_ws_f32", _p(mask_pred), _p(cls_prob), _p(rba), _p(sem), _p(arg), Q, K, H * W, mode, _p(_k1_workspace(dev)))
    return rba, sem, arg


@_hip_op
def rba_reduce_up4(mask_lowres, cls_prob, crop_hw, want_sem_seg=False, want_argmax=False, score="rba"):
    """K1 fused with the x4 upsample (maskformer_model.py:294-299) and the crop (:330-332).
    mask_lowres [Q,h,w]; outputs are [crop_h, crop_w] of the virtual [4h,4w] map."""
    _chk(mask_lowres, "mask_lowres", dim=3)
    _chk(cls_prob, "cls_prob", dim=2)
    Q, h, w = mask_lowres.shape
    if cls_prob.shape[0] != Q:
        raise RbaHipError(f"cls_prob has {cls_prob.shape[0]} queries, mask_lowres {Q}")
    K = cls_prob.shape[1]
    ch, cw = int(crop_hw[0]), int(crop_hw[1])
    mode = _mode(score)
    dev = mask_lowres.device
    rba = torch.empty((ch, cw), dtype=torch.float32, device=dev)
    sem = torch.empty((K, ch, cw), dtype=torch.float32, device=dev) if want_sem_seg else None
    arg = torch.empty((ch, cw), dtype=torch.int32, device=dev) if want_argmax else None
    _launch("rba_reduce_up4_f32", _p(mask_lowres), _p(cls_prob), _p(rba), _p(sem), _p(arg), Q, K, h, w, ch, cw, mode)
    return rba, sem, arg


def _k1_backward_args(who, mask_pred, cls_prob, grad, grad_name, grad_shape, need_mask, need_prob):
    """The argument block both backward forms of K1 share: mask_pred [Q,h,w], cls_prob [Q,K], the upstream gradient `grad` of shape
    `grad_shape(K, h, w)`, at least one output -> (Q, K, h * w, workspace | None, its bytes, grad_mask | None, grad_prob | None)."""
    _chk(mask_pred, "mask_pred", dim=3)
    _chk(cls_prob, "cls_prob", dim=2)
    Q, H, W = mask_pred.shape
    if cls_prob.shape[0] != Q:
        raise RbaHipError(f"cls_prob has {cls_prob.shape[0]} queries, mask_pred {Q}")
    K = cls_prob.shape[1]
    _chk(grad, grad_name, dim=len(grad_shape(K, H, W)))
    if tuple(grad.shape) != grad_shape(K, H, W):
        raise RbaHipError(f"{grad_name} must have shape {grad_shape(K, H, W)}, got {tuple(grad.shape)}")
    if not (need_mask or need_prob):
        raise RbaHipError(f"{who}: at least one of need_mask / need_prob")
    dev = mask_pred.device
    ws, ws_bytes = _workspace("rba_reduce_bwd_workspace_f32", "grad_prob", dev, Q, K, H * W) if need_prob else (None, 0)
    grad_mask = torch.empty((Q, H, W), dtype=torch.float32, device=dev) if need_mask else None
    grad_prob = torch.empty((Q, K), dtype=torch.float32, device=dev) if need_prob else None
    return Q, K, H * W, ws, ws_bytes, grad_mask, grad_prob


@_hip_op
def rba_reduce_backward(mask_pred, cls_prob, grad_score, score="rba", need_mask=True, need_prob=True):
    """K1 backward.  mask_pred [Q,h,w], cls_prob [Q,K] (rba_reduce's inputs), grad_score [h,w] = dL/d score ->
    (grad_mask [Q,h,w] | None, grad_prob [Q,K] | None), the gradients of rba_reduce's score (criterion.py:449-463 under autograd).
    Both are bitwise reproducible from launch to launch."""
    mode = _mode(score)
    Q, K, HW, ws, ws_bytes, grad_mask, grad_prob = _k1_backward_args("rba_reduce_backward", mask_pred, cls_prob, grad_score, "grad_score",
                                                                     lambda K, H, W: (H, W), need_mask, need_prob)
    _launch("rba_reduce_bwd_f32", _p(mask_pred), _p(cls_prob), _p(grad_score), _p(grad_mask), _p(grad_prob), Q, K, HW, mode, _p(ws), ws_bytes)
    return grad_mask, grad_prob


@_hip_op
def sem_seg_backward(mask_pred, cls_prob, grad_sem, need_mask=True, need_prob=True):
    """The per-class adjoint of K1.  mask_pred [Q,h,w], cls_prob [Q,K] (rba_reduce's inputs), grad_sem [K,h,w] = dL/d sem_seg (rba_reduce's
    ``want_sem_seg`` output, the class map einsum("qc,qhw->chw", cls_prob, sigmoid(mask_pred))) -> (grad_mask [Q,h,w] | None, grad_prob [Q,K] | None).
    K1 backward's kernel with the per-class gradient loaded instead of derived from a score's; both are bitwise reproducible from launch to launch."""
    Q, K, HW, ws, ws_bytes, grad_mask, grad_prob = _k1_backward_args("sem_seg_backward", mask_pred, cls_prob, grad_sem, "grad_sem",
                                                                     lambda K, H, W: (K, H, W), need_mask, need_prob)
    _launch("rba_sem_seg_bwd_f32", _p(mask_pred), _p(cls_prob), _p(grad_sem), _p(grad_mask), _p(grad_prob), Q, K, HW, _p(ws), ws_bytes)
    return grad_mask, grad_prob


@_hip_op
def resample_bilinear(x, size, add=None):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) for x [C,h,w] or [B,C,h,w]; optional fused
    `+ add` (the FPN top-down sum of msdeformattn.py:358)."""
    _chk(x, "x")
    if x.dim() not in (3, 4):
        raise RbaHipError("x must be [C,h,w] or [B,C,h,w]")
    H, W = int(size[0]), int(size[1])
    lead = tuple(x.shape[:-2])
    h, w = x.shape[-2:]
    _shaped(add, "add", lead + (H, W), optional=True)
    out = torch.empty(lead + (H, W), dtype=torch.float32, device=x.device)
    _launch("rba_resample_bilinear_f32", _p(x), _p(add), _p(out), math.prod(lead), h, w, H, W)
    return out


@_hip_op
def tta_merge(views, flips, size, want_sem_seg=False, want_argmax=False, score="rba"):
    """K12a, the multi-view merge of test-time augmentation (test_time_augmentation.py:83-97).  views: 1..16 class maps [K,h_a,w_a] (what
    rba_reduce_up4(..., want_sem_seg=True) gives for each view), flips: one bool per view, size: the output (H, W) -> (score [H,W],
    sem_seg [K,H,W] | None, argmax int32 [H,W] | None): every view resampled to (H, W) (align_corners=False), a flipped view read at column
    W - 1 - x, the views added in order and divided once by their number; the score of that mean as K1 computes it.  No resized map exists."""
    views, flips = list(views), [bool(f) for f in flips]
    if not 1 <= len(views) <= _lib.TTA_MAX_VIEWS:
        raise RbaHipError(f"tta_merge takes 1..{_lib.TTA_MAX_VIEWS} views, got {len(views)}")
    if len(flips) != len(views):
        raise RbaHipError(f"tta_merge: {len(views)} views but {len(flips)} flip flags")
    for a, v in enumerate(views):
        _chk(v, f"views[{a}]", dim=3)
    K = views[0].shape[0]
    if any(v.shape[0] != K for v in views):
        raise RbaHipError(f"tta_merge: every view must have the same K, got {[v.shape[0] for v in views]}")
    if not 1 <= K <= 32:
        raise RbaHipError(f"tta_merge needs 1 <= K <= 32, got {K}")
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1 or any(v.shape[1] < 1 or v.shape[2] < 1 for v in views):
        raise RbaHipError("tta_merge: empty view or output")
    if K * H * W >= 1 << 31 or any(v.numel() >= 1 << 31 for v in views):
        raise RbaHipError("tta_merge: K H W and every K h w must be below 2^31")
    mode = _mode(score)
    arg_ = _lib.TtaViews()
    for a, v in enumerate(views):
        arg_.sem[a], arg_.h[a], arg_.w[a], arg_.flip[a] = v.data_ptr(), v.shape[1], v.shape[2], int(flips[a])
    dev = views[0].device
    rba = torch.empty((H, W), dtype=torch.float32, device=dev)
    sem = torch.empty((K, H, W), dtype=torch.float32, device=dev) if want_sem_seg else None
    arg = torch.empty((H, W), dtype=torch.int32, device=dev) if want_argmax else None
    _launch("rba_tta_merge_f32", ctypes.addressof(arg_), len(views), K, H, W, mode, _p(rba), _p(sem), _p(arg))
    return rba, sem, arg


def pil_bilinear_coeffs(n_in, n_out):
    """Pillow's coefficient table of Image.resize(BILINEAR) for one axis of n_in -> n_out pixels (src/libImaging/Resample.c precompute_coeffs +
    normalize_coeffs_8bpc), built in double as Pillow builds it -> (kk int32 [n_out, ksize], bounds int32 [n_out, 2] = (first pixel, count), ksize).
    The triangle filter's support is max(n_in / n_out, 1): it widens when down-scaling.  Weights are summed left to right, as Pillow sums them."""
    import numpy as np
    n_in, n_out = int(n_in), int(n_out)
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)                 # (int) truncates; the operands are >= 0 after the clamp ...
    xmin = np.where(center - support + 0.5 < 0, 0, xmin)                            # ... and a negative one clamps to 0 either way
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    j = np.arange(ksize, dtype=np.float64)[None, :]
    x = (j + xmin[:, None] - center[:, None] + 0.5) * (1.0 / fs)
    w = np.where(np.abs(x) < 1.0, 1.0 - np.abs(x), 0.0)
    w = np.where(j < xmax[:, None], w, 0.0)
    ww = np.zeros(n_out, dtype=np.float64)
    for c in range(ksize):                                                          # Pillow's running sum, left to right
        ww = ww + w[:, c]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    s = w * float(1 << 22)
    kk = np.where(s < 0, (s - 0.5).astype(np.int64), (s + 0.5).astype(np.int64)).astype(np.int32)      # (int) truncates toward zero
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return np.ascontiguousarray(kk), np.ascontiguousarray(bounds), ksize


_PIL_TABLES = {}          # (device index, n_in, n_out) -> (kk, bounds, ksize) on the device


def _pil_tables(device, n_in, n_out):
    """The device copy of one axis' table, uploaded once per (device, n_in, n_out): a TTA recipe has a dozen of them, a few hundred KB together"""
    key = (device.index, int(n_in), int(n_out))
    t = _PIL_TABLES.get(key)
    if t is None:
        if len(_PIL_TABLES) >= 256:
            _PIL_TABLES.clear()
        kk, bounds, ksize = pil_bilinear_coeffs(n_in, n_out)
        t = _PIL_TABLES[key] = (torch.from_numpy(kk).to(device), torch.from_numpy(bounds).to(device), ksize)
    return t


@_hip_op
def resize_u8_pil_bilinear(image, size, flip=False):
    """K12b.  image uint8 [C,h,w] -> uint8 [C,H,W]: Pillow's Image.resize((W, H), BILINEAR) of the image, equal to Pillow in every byte (what
    Detectron2's ResizeTransform gives a uint8 image), with ``flip`` the result flipped horizontally (HFlipTransform) in the same pass."""
    _chk(image, "image", dtype=torch.uint8, dim=3)
    C, h, w = (int(v) for v in image.shape)
    H, W = int(size[0]), int(size[1])
    if min(C, h, w, H, W) < 1 or max(C * h * w, C * h * W, C * H * W) >= 1 << 31:
        raise RbaHipError("resize_u8_pil_bilinear needs a non-empty [C,h,w] image and size, each of C h w, C h W, C H W below 2^31")
    dev = image.device
    kx, bx, ksx = _pil_tables(dev, w, W) if w != W else (None, None, 0)
    ky, by, ksy = _pil_tables(dev, h, H) if h != H else (None, None, 0)
    out = torch.empty((C, H, W), dtype=torch.uint8, device=dev)
    tmp = torch.empty((C, h, W), dtype=torch.uint8, device=dev) if w != W and h != H else None
    _launch("rba_resize_u8_pil_bilinear", _p(image), _p(out), _p(tmp), C, h, w, H, W, _p(kx), _p(bx), ksx, _p(ky), _p(by), ksy, int(bool(flip)))
    return out


@_hip_op
def confusion_accumulate(pred, gt, num_classes, conf, bad, ignore_label=255, lut=None):
    """K13.  pred int32 (an argmax map: rba_reduce / tta_merge ``want_argmax``), gt uint8 | int64 of the same shape, conf int64 [K+1, K+1], bad int64 [2]:
    conf[pred, label] += 1 per pixel (Detectron2's SemSegEvaluator layout: rows = predictions, columns = ground truth, column K = ignored), where
    label = gt, through ``lut`` (uint8 [256]; a gt outside 0..255 is a bad label) when given, ``ignore_label`` (None or < 0: none) -> K.  A label outside
    0..K adds to bad[0], a prediction outside 0..K-1 (its label in range) to bad[1], neither to conf.  conf and bad are accumulated into -- zero them once
    per evaluation; nothing is read back and nothing synchronises.  Pixels are evaluated at the label's size: a shape mismatch is the caller's error."""
    K = int(num_classes)
    if not 1 <= K <= 255:
        raise RbaHipError(f"confusion_accumulate needs 1 <= num_classes <= 255, got {K}")
    _chk(pred, "pred", dtype=torch.int32)
    if not isinstance(gt, torch.Tensor) or gt.dtype not in (torch.uint8, torch.int64):
        raise RbaHipError(f"gt must be a uint8 or int64 tensor, got {gt.dtype if isinstance(gt, torch.Tensor) else type(gt).__name__}")
    _chk(gt, "gt", dtype=gt.dtype)
    if pred.shape != gt.shape:
        raise RbaHipError(f"pred {tuple(pred.shape)} and gt {tuple(gt.shape)} must have the same shape (evaluate at the label's size)")
    if pred.numel() < 1:
        raise RbaHipError("confusion_accumulate: empty maps")
    _chk(conf, "conf", dtype=torch.int64, dim=2)
    if tuple(conf.shape) != (K + 1, K + 1):
        raise RbaHipError(f"conf must have shape {(K + 1, K + 1)}, got {tuple(conf.shape)}")
    _chk(bad, "bad", dtype=torch.int64, dim=1)
    if bad.numel() != 2:
        raise RbaHipError(f"bad must have 2 elements, got {bad.numel()}")
    if lut is not None:
        _chk(lut, "lut", dtype=torch.uint8, dim=1)
        if lut.numel() != 256:
            raise RbaHipError(f"lut must have 256 entries, got {lut.numel()}")
    ignore = -1 if ignore_label is None or int(ignore_label) < 0 else int(ignore_label)
    _launch("rba_confusion_accum", _p(pred), _p(gt), gt.element_size(), pred.numel(), K, ignore, _p(lut), _p(conf), _p(bad))


def nearest_index_tables(h, w, new_h, new_w):
    """(ny int32 [new_h] | None, nx int32 [new_w] | None) on the CPU: the source row and column F.interpolate(size=(new_h, new_w), mode="nearest")
    reads for every output row and column of a float64 [1,1,h,w] map -- what Detectron2's ResizeTransform gives the reference's float64 labels; None
    for an axis whose size does not change (the index itself).  Asked of ATen itself, on a map of the very shape, once per shape: the CPU kernel's
    index arithmetic depends on the data type (fp64 here; the fp32 rule of ATen's nearest_idx differs from it in two columns at 1024 -> 1228) and, at
    small sizes, on the shape of the other axis too, so no closed form is restated (docs/kernels/K14.md).  The result is checked to be separable."""
    h, w, new_h, new_w = int(h), int(w), int(new_h), int(new_w)
    src = torch.arange(h * w, dtype=torch.float64).view(h, w)                        # the value names its pixel; exact below 2^53
    out = torch.nn.functional.interpolate(src[None, None], size=(new_h, new_w), mode="nearest")[0, 0]
    ny = torch.div(out[:, 0], w, rounding_mode="floor").to(torch.int64)
    nx = (out[0, :] - ny[0] * w).to(torch.int64)
    if int(ny.min()) < 0 or int(ny.max()) >= h or int(nx.min()) < 0 or int(nx.max()) >= w or not torch.equal(out, src[ny][:, nx]):
        raise RbaHipError(f"F.interpolate(mode='nearest') of a {h} x {w} map to {new_h} x {new_w} is not a row table times a column table")
    if (new_h == h and not torch.equal(ny, torch.arange(h))) or (new_w == w and not torch.equal(nx, torch.arange(w))):
        raise RbaHipError(f"F.interpolate(mode='nearest') of a {h} x {w} map to {new_h} x {new_w} moves an axis whose size does not change")
    return (None if new_h == h else ny.to(torch.int32)), (None if new_w == w else nx.to(torch.int32))


_NEAREST_TABLES = {}      # (device index, h, w, new_h, new_w) -> (ny, nx) on the device


def _nearest_tables(device, h, w, new_h, new_w):
    key = (device.index, int(h), int(w), int(new_h), int(new_w))
    t = _NEAREST_TABLES.get(key)
    if t is None:
        if len(_NEAREST_TABLES) >= 256:
            _NEAREST_TABLES.clear()
        t = _NEAREST_TABLES[key] = tuple(None if v is None else v.to(device) for v in nearest_index_tables(h, w, new_h, new_w))
    return t


@_hip_op
def train_view(img, lab, params, obj=None, objmask=None, lut=None, ignore_label=255, ood_label=254, pad_size=None):
    """K14.  img uint8 [3,h,w], lab uint8 [h,w] (through ``lut`` uint8 [256] when given), ``params`` a dataset_mappers.TrainViewParams (every sampled
    decision: paste position, resize target, crop, colour legs, flip) and, where ``params.paste`` is set, the object ``obj`` uint8 [3,bh,bw] with its mask
    ``objmask`` uint8 [bh,bw] -> (image uint8 [3,pad_h,pad_w], sem_seg int64 [pad_h,pad_w], outlier_mask int64 [ch,cw], hist int32 [256]): the training
    view of MaskFormerSemanticCocoMixDatasetMapper in one launch, equal to the host composition in every element (docs/kernels/K14.md).  ``pad_size``
    (pad_h, pad_w): the output canvas, the crop's size when None.  Nothing is read back.  The shape contract (crop inside the resized frame, box inside
    the source, canvas no smaller than the crop) is the entry point's: a violation raises RbaHipError, nothing is clamped."""
    _chk(img, "img", dtype=torch.uint8, dim=3)
    _chk(lab, "lab", dtype=torch.uint8, dim=2)
    h, w = int(img.shape[1]), int(img.shape[2])
    if img.shape[0] != 3 or tuple(lab.shape) != (h, w):
        raise RbaHipError(f"train_view needs img [3,h,w] and lab [h,w], got {tuple(img.shape)} and {tuple(lab.shape)}")
    v = _lib.TrainView()
    v.img, v.lab, v.h, v.w = img.data_ptr(), lab.data_ptr(), h, w
    if lut is not None:
        _chk(lut, "lut", dtype=torch.uint8, dim=1)
        if lut.numel() != 256:
            raise RbaHipError(f"lut must have 256 entries, got {lut.numel()}")
        v.lut = lut.data_ptr()
    if params.paste is not None:
        _chk(obj, "obj", dtype=torch.uint8, dim=3)
        _chk(objmask, "objmask", dtype=torch.uint8, dim=2)
        if obj.shape[0] != 3 or tuple(obj.shape[1:]) != tuple(objmask.shape) or objmask.numel() < 1:
            raise RbaHipError(f"train_view needs obj [3,bh,bw] and objmask [bh,bw], got {tuple(obj.shape)} and {tuple(objmask.shape)}")
        v.obj, v.objmask, v.bh, v.bw = obj.data_ptr(), objmask.data_ptr(), int(objmask.shape[0]), int(objmask.shape[1])
        v.py, v.px = int(params.paste[0]), int(params.paste[1])
    dev = img.device
    v.new_h, v.new_w = int(params.new_h), int(params.new_w)
    if min(v.new_h, v.new_w) < 1:
        raise RbaHipError(f"train_view: empty resize target {(v.new_h, v.new_w)}")
    v.y0, v.x0, v.ch, v.cw = (int(c) for c in params.crop)
    v.pad_h, v.pad_w = (v.ch, v.cw) if pad_size is None else (int(pad_size[0]), int(pad_size[1]))
    if min(v.ch, v.cw) < 1 or v.pad_h < v.ch or v.pad_w < v.cw:
        raise RbaHipError(f"train_view: crop {(v.ch, v.cw)} and canvas {(v.pad_h, v.pad_w)}: the crop is non-empty and the canvas no smaller")
    tables = []                                                  # kept alive until the launch is enqueued
    if v.new_w != w:
        kx, bx, v.ksize_x = _pil_tables(dev, w, v.new_w)
        v.kx, v.bx = kx.data_ptr(), bx.data_ptr()
        tables += [kx, bx]
    if v.new_h != h:
        ky, by, v.ksize_y = _pil_tables(dev, h, v.new_h)
        v.ky, v.by = ky.data_ptr(), by.data_ptr()
        tables += [ky, by]
    if v.new_w != w or v.new_h != h:
        ny, nx = _nearest_tables(dev, h, w, v.new_h, v.new_w)
        v.ny, v.nx = _p(ny), _p(nx)
        tables += [ny, nx]
    v.flip, v.ignore_label, v.ood_label = int(bool(params.flip)), int(ignore_label), int(ood_label)
    c = params.color
    if c is not None:
        k = v.color
        k.enabled, k.brightness, k.beta, k.order = 1, int(bool(c.brightness)), float(c.beta), int(bool(c.order))
        k.contrast, k.contrast_alpha, k.saturation, k.saturation_alpha = int(bool(c.contrast)), float(c.contrast_alpha), int(bool(c.saturation)), float(c.saturation_alpha)
        k.hue, k.hue_delta = int(bool(c.hue)), int(c.hue_delta)
    image = torch.empty((3, v.pad_h, v.pad_w), dtype=torch.uint8, device=dev)
    sem_seg = torch.empty((v.pad_h, v.pad_w), dtype=torch.int64, device=dev)
    outlier_mask = torch.empty((v.ch, v.cw), dtype=torch.int64, device=dev)
    hist = torch.empty(256, dtype=torch.int32, device=dev)
    v.image, v.sem_seg, v.outlier_mask, v.hist = image.data_ptr(), sem_seg.data_ptr(), outlier_mask.data_ptr(), hist.data_ptr()
    _launch("rba_train_view_u8", ctypes.addressof(v))
    return image, sem_seg, outlier_mask, hist


# K15's launch rule (csrc/adamw_step.hip): 256 threads; K15a gives one workgroup ADAMW_SHARE flat elements until ADAMW_MAX_PARTIALS workgroups are reached,
# then equal larger shares; K15b's workgroup steps one chunk of one tensor: ADAMW_CHUNK elements (one 16-byte access per thread and array) while the
# whole state has at most ADAMW_SMALL elements -- the step is launch-bound there and many short workgroups finish soonest -- else ADAMW_CHUNK_LARGE
# (every workgroup re-sums the partials: up to 4 KiB, amortised over 448 KiB of state traffic)
ADAMW_THREADS, ADAMW_SHARE, ADAMW_MAX_PARTIALS, ADAMW_CHUNK, ADAMW_CHUNK_LARGE, ADAMW_SMALL = 256, 4096, _lib.ADAMW_MAX_PARTIALS, 1024, 16384, 1 << 20


class AdamWPlan:
    """What K15 needs besides the three flat buffers, built once per optimizer by `adamw_plan`: the parameters (kept alive: the device table holds
    their raw pointers), each one's slice [offset, offset + n) of the flat layout, the two device tables, the partials and the one-float stats."""
    __slots__ = ("params", "ptrs", "offsets", "sizes", "total", "chunk", "n_blocks", "n_partials", "tensors", "blocks", "partials", "stats", "device")


def adamw_flat(plan_or_total, device=None):
    """A zeroed flat fp32 buffer of K15's layout (grad, exp_avg or exp_avg_sq): the gaps between the slices must hold zeros, and stay zero."""
    total, device = (plan_or_total.total, plan_or_total.device) if isinstance(plan_or_total, AdamWPlan) else (int(plan_or_total), device)
    return torch.zeros(total, dtype=torch.float32, device=device)


@_hip_op
def adamw_plan(params, lr_mults, weight_decays, chunk=None):
    """K15's tables for `params` (fp32 HIP tensors, contiguous, at least one element each; views of larger tensors are fine), with the per-tensor
    learning-rate multiplier and weight decay -> AdamWPlan.  Slices are laid out in the order given, each starting on a multiple of four elements.
    ``chunk``: elements per workgroup of K15b (a multiple of 4), by the launch rule above when None.  Built and uploaded here, once."""
    params = list(params)
    if not params or len(lr_mults) != len(params) or len(weight_decays) != len(params):
        raise RbaHipError("adamw_plan needs at least one parameter and one lr multiplier and one weight decay per parameter")
    for i, p_ in enumerate(params):
        _chk(p_, f"params[{i}]")
        if p_.numel() < 1:
            raise RbaHipError(f"params[{i}] is empty")
    if len({p_.data_ptr() for p_ in params}) != len(params):
        raise RbaHipError("adamw_plan: a parameter is listed twice")
    plan = AdamWPlan()
    plan.params, plan.device = params, params[0].device
    plan.ptrs = [p_.data_ptr() for p_ in params]
    plan.sizes = [p_.numel() for p_ in params]
    plan.offsets, at = [], 0
    for n in plan.sizes:
        plan.offsets.append(at)
        at += (n + 3) // 4 * 4
    plan.total = at
    plan.chunk = int(chunk) if chunk is not None else (ADAMW_CHUNK if at <= ADAMW_SMALL else ADAMW_CHUNK_LARGE)
    if plan.chunk < 4 or plan.chunk % 4:
        raise RbaHipError(f"adamw_plan: chunk must be a positive multiple of 4, got {plan.chunk}")
    pairs = [(t, c) for t, n in enumerate(plan.sizes) for c in range((n + plan.chunk - 1) // plan.chunk)]
    plan.n_blocks = len(pairs)
    if plan.n_blocks >= 1 << 31:
        raise RbaHipError(f"adamw_plan: {plan.n_blocks} chunks of {plan.chunk} elements exceed one launch's grid; pass a larger chunk")
    plan.n_partials = max(1, min(ADAMW_MAX_PARTIALS, (at + ADAMW_SHARE - 1) // ADAMW_SHARE))
    table = (_lib.AdamWTensor * len(params))()
    for d, ptr, off, n, m, wd in zip(table, plan.ptrs, plan.offsets, plan.sizes, lr_mults, weight_decays):
        d.param, d.offset, d.n, d.lr_mult, d.weight_decay = ptr, off, n, float(m), float(wd)
    host = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8)
    plan.tensors = torch.empty(host.numel(), dtype=torch.uint8, device=plan.device)
    plan.tensors.copy_(host)
    plan.blocks = torch.empty((plan.n_blocks, 2), dtype=torch.int32, device=plan.device)
    plan.blocks.copy_(torch.tensor(pairs, dtype=torch.int32))
    plan.partials = torch.empty(plan.n_partials, dtype=torch.float32, device=plan.device)
    plan.stats = torch.zeros(1, dtype=torch.float32, device=plan.device)
    return plan


def _adamw_flat_ok(plan, t, name):
    """A flat buffer of `plan`'s layout: fp32, exactly plan.total elements, on the plan's device, 16-byte aligned."""
    if not isinstance(plan, AdamWPlan):
        raise RbaHipError("plan must be an AdamWPlan (ops.adamw_plan)")
    _vec(t, name, plan.total)
    if t.device != plan.device or t.data_ptr() % 16:
        raise RbaHipError(f"{name} must be on {plan.device} and 16-byte aligned")
    return t


@_hip_op
def grad_sqnorm(plan, grad, grad_scale=1.0):
    """K15a.  plan.partials[b] = the sum of (grad * grad_scale)^2 over workgroup b's share of the flat gradient buffer, every slot written, in a fixed
    order (bitwise reproducible) -> plan.partials.  Nothing is read back."""
    _adamw_flat_ok(plan, grad, "grad")
    _launch("rba_grad_sqnorm_f32", grad.data_ptr(), plan.total, float(grad_scale), plan.partials.data_ptr(), plan.n_partials)
    return plan.partials


@_hip_op
def clip_adamw_step(plan, grad, exp_avg, exp_avg_sq, step, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=0.0, grad_scale=1.0):
    """K15b, after `grad_sqnorm` with the same grad and grad_scale.  Step number ``step`` (1 for the first) of torch.optim.AdamW(amsgrad=False) on every
    parameter of the plan, in place, behind clip_grad_norm_(params, max_norm) (max_norm <= 0: no clipping) of grad * grad_scale; ``lr`` is the learning
    rate of a group with multiplier 1.  exp_avg and exp_avg_sq are updated in place, grad is left as it is, plan.stats[0] receives the gradient norm.
    The bias corrections are formed here in double, as torch forms them.  The parameters are written through raw pointers: every one's version counter
    is raised here, so that the caches keyed on it see the step.  A parameter whose storage moved since the plan was built raises.  Nothing is read
    back and nothing synchronises."""
    _adamw_flat_ok(plan, grad, "grad")
    _adamw_flat_ok(plan, exp_avg, "exp_avg")
    _adamw_flat_ok(plan, exp_avg_sq, "exp_avg_sq")
    step, (beta1, beta2) = int(step), (float(b) for b in betas)
    if step < 1 or not (0.0 <= beta1 < 1.0 and 0.0 <= beta2 < 1.0) or eps < 0.0:
        raise RbaHipError(f"clip_adamw_step needs step >= 1, betas in [0, 1) and eps >= 0, got step {step}, betas {(beta1, beta2)}, eps {eps}")
    for i, (p_, ptr, n) in enumerate(zip(plan.params, plan.ptrs, plan.sizes)):
        if p_.data_ptr() != ptr or p_.numel() != n:
            raise RbaHipError(f"clip_adamw_step: parameter {i} of the plan was moved or resized since adamw_plan; build a new plan")
    h = _lib.AdamWHyper(lr=float(lr), beta1=beta1, beta2=beta2, eps=float(eps), bias_correction1=1.0 - beta1 ** step,
                        bias_correction2_sqrt=(1.0 - beta2 ** step) ** 0.5, grad_scale=float(grad_scale), max_norm=float(max_norm))
    _launch("rba_clip_adamw_step_f32", plan.tensors.data_ptr(), plan.blocks.data_ptr(), plan.n_blocks, plan.chunk, grad.data_ptr(), exp_avg.data_ptr(),
            exp_avg_sq.data_ptr(), plan.partials.data_ptr(), plan.n_partials, ctypes.addressof(h), plan.stats.data_ptr())
    torch.autograd.graph.increment_version(plan.params)


# K13's launch rule (csrc/confusion.hip), for tests that size a map to a number of sweeps of the capped grid
CONFUSION_THREADS, CONFUSION_TILE, CONFUSION_GRID_CAP, CONFUSION_LDS_MAX_K = 256, 16, 512, 126


def _level_shapes(spatial_shapes, L):
    """spatial_shapes of multi-scale deformable attention: int64 [L, 2] = (h, w) per level (the kernels take a bare pointer and read 2 L values)."""
    _chk(spatial_shapes, "spatial_shapes", torch.int64, 2)
    if tuple(spatial_shapes.shape) != (L, 2):
        raise RbaHipError(f"spatial_shapes must have shape {(L, 2)}, got {tuple(spatial_shapes.shape)}")
    return spatial_shapes


def _msda_args(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step, grad_output=None, backward=False):
    """The argument block of multi-scale deformable attention, forward and (``backward``: with grad_output) backward -> (dtype, N, S, M, D, L, Lq, P)."""
    # float or double, like the reference op (AT_DISPATCH_FLOATING_TYPES, ms_deform_attn_cuda.cu:69); all tensors of one type
    dt = value.dtype if isinstance(value, torch.Tensor) and value.dtype == torch.float64 else torch.float32
    _chk(value, "value", dt, dim=4)
    _chk(level_start_index, "level_start_index", torch.int64, 1)
    _chk(sampling_locations, "sampling_loc", dt, dim=6)
    _chk(attention_weights, "attn_weight", dt, dim=5)
    if backward:
        _chk(grad_output, "grad_output", dt, dim=3)
    N, S, M, D = value.shape
    _, Lq, M2, L, P, two = sampling_locations.shape
    if M2 != M or two != 2 or sampling_locations.shape[0] != N:
        raise RbaHipError("sampling_loc shape does not match value")
    if tuple(attention_weights.shape) != (N, Lq, M, L, P):
        raise RbaHipError("attn_weight shape does not match sampling_loc")
    _level_shapes(spatial_shapes, L)
    if level_start_index.shape[0] != L:
        raise RbaHipError("level_start_index must have L elements")
    if backward and tuple(grad_output.shape) != (N, Lq, M * D):
        raise RbaHipError(f"grad_output must have shape {(N, Lq, M * D)}, got {tuple(grad_output.shape)}")
    step = min(N, int(im2col_step))
    if N > 0 and N % step != 0:
        raise RbaHipError(f"batch({N}) must divide im2col_step({step})")
    return dt, N, S, M, D, L, Lq, P


@_hip_op
def ms_deform_attn_forward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights,
                           im2col_step=128):
    """K2.  Same signature and checks as MultiScaleDeformableAttention.ms_deform_attn_forward
    (pixel_decoder/ops/functions/ms_deform_attn_func.py:36-37, ops/src/cuda/ms_deform_attn_cuda.cu:25-85):
    value [N,S,M,D], spatial_shapes [L,2] int64, level_start_index [L] int64, sampling_locations
    [N,Lq,M,L,P,2], attention_weights [N,Lq,M,L,P] -> [N,Lq,M*D].  `im2col_step` is accepted for signature
    compatibility and only validated (the kernel needs no batch chunking)."""
    dt, N, S, M, D, L, Lq, P = _msda_args(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step)
    out = torch.empty((N, Lq, M * D), dtype=dt, device=value.device)
    _launch("rba_ms_deform_attn_fwd_f64" if dt == torch.float64 else "rba_ms_deform_attn_fwd_f32",
            _p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_locations), _p(attention_weights), _p(out), N, S, M, D, L, Lq, P)
    return out


@_hip_op
def ms_deform_attn_backward(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, grad_output,
                            im2col_step=128):
    """K2 backward.  Same signature and checks as MultiScaleDeformableAttention.ms_deform_attn_backward
    (pixel_decoder/ops/functions/ms_deform_attn_func.py:43-49, ops/src/cuda/ms_deform_attn_cuda.cu:88-158): the forward's five
    tensors and grad_output [N,Lq,M*D] -> (grad_value [N,S,M,D], grad_sampling_loc [N,Lq,M,L,P,2], grad_attn_weight [N,Lq,M,L,P]).
    grad_value is summed with float atomics (last bits may differ between launches); the other two are bitwise reproducible.
    `im2col_step` is only validated."""
    dt, N, S, M, D, L, Lq, P = _msda_args(value, spatial_shapes, level_start_index, sampling_locations, attention_weights, im2col_step, grad_output, backward=True)
    dev = value.device
    grad_value = torch.empty((N, S, M, D), dtype=dt, device=dev)
    grad_loc = torch.empty((N, Lq, M, L, P, 2), dtype=dt, device=dev)
    grad_attn = torch.empty((N, Lq, M, L, P), dtype=dt, device=dev)
    _launch("rba_ms_deform_attn_bwd_f64" if dt == torch.float64 else "rba_ms_deform_attn_bwd_f32",
            _p(value), _p(spatial_shapes), _p(level_start_index), _p(sampling_locations), _p(attention_weights), _p(grad_output),
            _p(grad_value), _p(grad_loc), _p(grad_attn), N, S, M, D, L, Lq, P)
    return grad_value, grad_loc, grad_attn


@_hip_op
def masked_xattn(q, k, v, mask_logits=None, split_keys=None):
    """K3.  q [B,Q,nH,hd] (unscaled), k, v [B,S,nH,hd], mask_logits [B,Q,S] | None -> [B,Q,nH*hd].
    split_keys: use the split-key matrix-pipe path (needs a scratch buffer, allocated here); None = automatic
    (it wins from about a thousand keys; below that its three launches cost more than they save)."""
    _chk(q, "q", dim=4)
    _chk(k, "k", dim=4)
    _chk(v, "v", dim=4)
    B, Q, nH, hd = q.shape
    S = k.shape[1]
    if tuple(k.shape) != (B, S, nH, hd) or tuple(v.shape) != (B, S, nH, hd):
        raise RbaHipError("k / v shape mismatch")
    _shaped(mask_logits, "mask_logits", (B, Q, S), optional=True)
    out = torch.empty((B, Q, nH * hd), dtype=torch.float32, device=q.device)
    if split_keys is None:
        split_keys = S >= 1024
    ws = _scratch(_query("rba_masked_xattn_workspace_bytes", B, Q, S, nH), q.device, 4) if split_keys else None
    _launch("rba_masked_xattn_f32", _p(q), _p(k), _p(v), _p(mask_logits), _p(out), _p(ws), B, Q, S, nH, hd)
    return out


@_hip_op
def masked_xattn_backward(q, k, v, mask_logits, grad_out, need_q=True, need_k=True, need_v=True):
    """K3 backward.  masked_xattn's inputs (q [B,Q,nH,hd] unscaled, k, v [B,S,nH,hd], mask_logits [B,Q,S] | None) and grad_out [B,Q,nH*hd] =
    dL/d out -> (grad_q | None, grad_k | None, grad_v | None), the gradients of the attention core in exact fp32 (the mask gets none: the
    reference detaches it).  A gradient that is not needed is not computed.  All three are bitwise reproducible from launch to launch."""
    if not (need_q or need_k or need_v):
        raise RbaHipError("masked_xattn_backward: at least one of need_q / need_k / need_v")
    _chk(q, "q", dim=4)
    _chk(k, "k", dim=4)
    _chk(v, "v", dim=4)
    B, Q, nH, hd = q.shape
    S = k.shape[1]
    if tuple(k.shape) != (B, S, nH, hd) or tuple(v.shape) != (B, S, nH, hd):
        raise RbaHipError("k / v shape mismatch")
    _shaped(mask_logits, "mask_logits", (B, Q, S), optional=True)
    _shaped(grad_out, "grad_out", (B, Q, nH * hd))
    dev = q.device
    alloc = torch.empty if B and Q else torch.zeros             # no query: an empty sum, decided here
    grad_q = torch.empty((B, Q, nH, hd), dtype=torch.float32, device=dev) if need_q else None
    grad_k = alloc((B, S, nH, hd), dtype=torch.float32, device=dev) if need_k else None
    grad_v = alloc((B, S, nH, hd), dtype=torch.float32, device=dev) if need_v else None
    if B and Q:
        ws = _scratch(_query("rba_masked_xattn_bwd_workspace_bytes", B, Q, S, nH), dev, 4)
        _launch("rba_masked_xattn_bwd_f32", _p(q), _p(k), _p(v), _p(mask_logits), _p(grad_out), _p(grad_q), _p(grad_k), _p(grad_v), _p(ws),
                B, Q, S, nH, hd)
    return grad_q, grad_k, grad_v


@_hip_op
def mask_logits(embed, feat, mode=None):
    """K4.  einsum("bqc,bchw->bqhw") (mask2former_transformer_decoder.py:479): embed [B,Q,C], feat [B,C,h,w].  `mode` (default: _split_mode())
    "f16x3" = three f16 matrix-pipe products per fp32 product (|x| < 65504), anything else = the exact-fp32 MFMA kernel."""
    _chk(embed, "embed", dim=3)
    _chk(feat, "feat")
    if feat.dim() not in (3, 4):
        raise RbaHipError("feat must be [B,C,N] or [B,C,h,w]")
    B, Q, C = embed.shape
    if feat.shape[0] != B or feat.shape[1] != C:
        raise RbaHipError("feat shape does not match embed")
    sp = tuple(feat.shape[2:])
    out = torch.empty((B, Q) + sp, dtype=torch.float32, device=embed.device)
    _launch("rba_mask_logits_f16x3_f32" if (_split_mode() if mode is None else mode) == "f16x3" else "rba_mask_logits_f32",
            _p(embed), _p(feat), _p(out), B, Q, C, math.prod(sp))
    return out


@_hip_op
def mask_logits_backward(embed, feat, grad_out, need_embed=True, need_feat=True):
    """K4 backward.  embed [B,Q,C], feat [B,C,N] or [B,C,h,w] (mask_logits' inputs), grad_out [B,Q] + feat.shape[2:] = dL/d out ->
    (grad_embed [B,Q,C] | None, grad_feat like feat | None), the gradients of the einsum (mask2former_transformer_decoder.py:479 under autograd)
    in exact fp32 whatever mode the forward ran in.  Both are bitwise reproducible from launch to launch.  The operand a call does not read
    (embed without need_feat, feat without need_embed) may be None."""
    if not (need_embed or need_feat):
        raise RbaHipError("mask_logits_backward: at least one of need_embed / need_feat")
    if need_feat or embed is not None:
        _chk(embed, "embed", dim=3)
    if need_embed or feat is not None:
        _chk(feat, "feat")
    _chk(grad_out, "grad_out")
    if grad_out.dim() not in (3, 4):
        raise RbaHipError("grad_out must be [B,Q,N] or [B,Q,h,w]")
    B, Q = grad_out.shape[:2]
    sp = tuple(grad_out.shape[2:])
    C = embed.shape[2] if embed is not None else feat.shape[1]
    _shaped(embed, "embed", (B, Q, C), optional=True)
    _shaped(feat, "feat", (B, C) + sp, optional=True)
    N = math.prod(sp)
    dev = grad_out.device
    ws, ws_bytes = _workspace("rba_mask_logits_bwd_workspace_f32", "grad_embed", dev, B, Q, C, N) if need_embed else (None, 0)
    alloc = torch.empty if B and Q and N else torch.zeros          # an empty reduction: the entry point is a no-op, the gradient is 0
    grad_embed = alloc((B, Q, C), dtype=torch.float32, device=dev) if need_embed else None
    grad_feat = alloc((B, C) + sp, dtype=torch.float32, device=dev) if need_feat else None
    _launch("rba_mask_logits_bwd_f32", _p(embed), _p(feat), _p(grad_out), _p(grad_embed), _p(grad_feat), B, Q, C, N, _p(ws), ws_bytes)
    return grad_embed, grad_feat


def _planes(t, name):
    """Mask planes [..., h, w] (at least one leading axis) -> (number of planes, h, w)."""
    _chk(t, name)
    if t.dim() < 3 or t.shape[-1] < 1 or t.shape[-2] < 1:
        raise RbaHipError(f"{name} must be [..., h, w] with h, w >= 1, got shape {tuple(t.shape)}")
    return math.prod(t.shape[:-2]), t.shape[-2], t.shape[-1]


def _point_coords(coords, name, N):
    """Normalised (x, y) points: [N,P,2], or [1,P,2] / [P,2] shared by all N rows -> (P, shared)."""
    _chk(coords, name)
    if coords.dim() == 2:
        coords = coords[None]
    if coords.dim() != 3 or coords.shape[2] != 2 or coords.shape[0] not in (1, N):
        raise RbaHipError(f"{name} must be [{N},P,2], [1,P,2] or [P,2], got shape {tuple(coords.shape)}")
    return coords.shape[1], int(coords.shape[0] != N)


def _plane_index(index, N=None):
    _chk(index, "plane_index", dtype=torch.int64, dim=1)
    if N is not None and index.numel() != N:
        raise RbaHipError(f"plane_index must have {N} elements, got {index.numel()}")
    return index.numel()


def _grid_rows_ok(who, N):
    if N > 65535:
        raise RbaHipError(f"{who}: at most 65535 rows per call, got {N}")


@_hip_op
def point_sample(planes, coords, plane_index=None):
    """K8.  detectron2's point_sample (F.grid_sample(x, 2 c - 1, align_corners=False), bilinear, zero padding): planes [..., h, w] fp32, coords
    [N,P,2] (x, y) or shared [1,P,2] / [P,2], plane_index int64 [N] choosing each row's plane (repeats allowed; None: row n reads plane n)
    -> [N,P].  A row whose index names no plane is NaN."""
    M, h, w = _planes(planes, "planes")
    N = M if plane_index is None else _plane_index(plane_index)
    _grid_rows_ok("point_sample", N)
    P, shared = _point_coords(coords, "coords", N)
    out = torch.empty((N, P), dtype=torch.float32, device=planes.device)
    _launch("rba_point_sample_f32", _p(planes), _p(plane_index), _p(coords), _p(out), M, N, h, w, P, shared)
    return out


def _mask_point_loss_args(pred_masks, plane_index, point_coords, point_labels, num_masks):
    M, h, w = _planes(pred_masks, "pred_masks")
    N = _plane_index(plane_index)
    _grid_rows_ok("mask_point_loss", N)
    _chk(point_coords, "point_coords", dim=3)
    P = point_coords.shape[1]
    _shaped(point_coords, "point_coords", (N, P, 2))
    _shaped(point_labels, "point_labels", (N, P))
    if N < 1 or P < 1 or not float(num_masks) > 0:
        raise RbaHipError(f"mask_point_loss: needs N >= 1 masks, P >= 1 points and num_masks > 0, got N = {N}, P = {P}, num_masks = {num_masks}")
    return M, N, h, w, P


@_hip_op
def mask_point_loss(pred_masks, plane_index, point_coords, point_labels, num_masks):
    """K8.  The reference's two mask losses (criterion.py:230-239: point_sample + sigmoid_ce_loss + dice_loss) of N matched masks in one call.
    pred_masks [..., h, w] (e.g. [B,Q,h,w]); mask n is plane plane_index[n] (int64 [N]) of its flattened leading axes, sampled at
    point_coords[n] [N,P,2] against point_labels [N,P] -> (losses [2] = (loss_mask, loss_dice), sums [N,4] = per-mask (bce, sigma t, sigma, t)
    sums for the backward).  Both are bitwise reproducible from launch to launch."""
    M, N, h, w, P = _mask_point_loss_args(pred_masks, plane_index, point_coords, point_labels, num_masks)
    dev = pred_masks.device
    sums = torch.empty((N, 4), dtype=torch.float32, device=dev)
    losses = torch.empty((2,), dtype=torch.float32, device=dev)
    _launch("rba_mask_point_loss_fwd_f32", _p(pred_masks), _p(plane_index), _p(point_coords), _p(point_labels), _p(sums), _p(losses),
            M, N, h, w, P, float(num_masks))
    return losses, sums


@_hip_op
def mask_point_loss_backward(pred_masks, plane_index, point_coords, point_labels, sums, num_masks, grad_loss_mask=None, grad_loss_dice=None):
    """K8.  mask_point_loss's inputs and `sums`, and the two upstream gradients as one-element fp32 device tensors (one may be None = 0; they are
    read on the device) -> the gradient like pred_masks: planes no mask names are exactly 0, the others are summed with float atomics and may
    differ in the last bits from launch to launch."""
    M, N, h, w, P = _mask_point_loss_args(pred_masks, plane_index, point_coords, point_labels, num_masks)
    _shaped(sums, "sums", (N, 4))
    if grad_loss_mask is None and grad_loss_dice is None:
        raise RbaHipError("mask_point_loss_backward: at least one of grad_loss_mask / grad_loss_dice")
    for g, name in ((grad_loss_mask, "grad_loss_mask"), (grad_loss_dice, "grad_loss_dice")):
        if g is not None:
            _one_element(g, name)
    grad = torch.empty(pred_masks.shape, dtype=torch.float32, device=pred_masks.device)
    _launch("rba_mask_point_loss_bwd_f32", _p(pred_masks), _p(plane_index), _p(point_coords), _p(point_labels), _p(sums), _p(grad_loss_mask),
            _p(grad_loss_dice), _p(grad), M, N, h, w, P, float(num_masks))
    return grad


@_hip_op
def match_cost(pred_masks, tgt_masks, coords, cls_prob, tgt_ids, cost_mask=1.0, cost_class=1.0, cost_dice=1.0):
    """K8.  The matcher's cost matrix of one image (matcher.py:105-149): pred_masks [Q,h,w], tgt_masks [T,H,W] fp32, the shared points coords
    [P,2] or [1,P,2], cls_prob [Q,K+1] = softmax of the class logits, tgt_ids int64 [T] -> [Q,T] =
    cost_mask * batch_sigmoid_ce + cost_class * (-cls_prob[:, tgt_ids]) + cost_dice * batch_dice.  Bitwise reproducible from launch to launch.
    tgt_ids outside [0, K] are refused: that check reads one flag back from the device (the matcher needs the matrix on the host anyway)."""
    _chk(pred_masks, "pred_masks", dim=3)
    _chk(tgt_masks, "tgt_masks", dim=3)
    _chk(cls_prob, "cls_prob", dim=2)
    _chk(tgt_ids, "tgt_ids", dtype=torch.int64, dim=1)
    Q, h, w = pred_masks.shape
    T, H, W = tgt_masks.shape
    P, _ = _point_coords(coords, "coords", 1)
    K1 = cls_prob.shape[1]
    if coords.numel() != 2 * P or cls_prob.shape[0] != Q or tgt_ids.numel() != T or min(Q, T, P, K1, h, w, H, W) < 1:
        raise RbaHipError(f"match_cost: pred_masks [Q,h,w], tgt_masks [T,H,W], coords [P,2], cls_prob [Q,K+1], tgt_ids [T], all sizes >= 1; got "
                          f"{tuple(pred_masks.shape)}, {tuple(tgt_masks.shape)}, {tuple(coords.shape)}, {tuple(cls_prob.shape)}, {tuple(tgt_ids.shape)}")
    if bool(((tgt_ids < 0) | (tgt_ids >= K1)).any()):
        raise RbaHipError(f"match_cost: tgt_ids must lie in [0, {K1 - 1}]")
    dev = pred_masks.device
    ws, ws_bytes = _workspace("rba_match_cost_workspace_f32", "match_cost", dev, Q, T, P)
    cost = torch.empty((Q, T), dtype=torch.float32, device=dev)
    _launch("rba_match_cost_f32", _p(pred_masks), _p(tgt_masks), _p(coords), _p(cls_prob), _p(tgt_ids), _p(cost), Q, T, P, h, w, H, W, K1,
            float(cost_mask), float(cost_class), float(cost_dice), _p(ws), ws_bytes)
    return cost


TAIL_FUNCS = {"squared_hinge": 0, "binary_cross_entropy": 1, "mse": 2, "l1": 3}


def _outlier_tail_args(score, labels, func):
    """The argument block of K9: score fp32 contiguous [B,h,w], labels int64 or uint8 contiguous [B,H,W], every size >= 1 and B H W, B h w < 2^31,
    func one of TAIL_FUNCS -> (B, h, w, H, W, bytes per label, func number)."""
    _chk(score, "score", dim=3)
    nb = _labels(labels)
    if func not in TAIL_FUNCS:
        raise RbaHipError(f"unknown func {func!r}; choose from {sorted(TAIL_FUNCS)}")
    (B, h, w), (H, W) = score.shape, labels.shape[1:]
    if labels.shape[0] != B or min(B, h, w, H, W) < 1 or max(B * H * W, B * h * w) >= 1 << 31:
        raise RbaHipError(f"outlier_tail: score [B,h,w] and labels [B,H,W] of one B, all sizes >= 1, B H W and B h w < 2^31; got "
                          f"{tuple(score.shape)} and {tuple(labels.shape)}")
    return B, h, w, H, W, nb, TAIL_FUNCS[func]


@_hip_op
def outlier_tail(score, labels, func, thr_in, thr_out):
    """K9.  The reference's outlier loss behind its score map (criterion.py:474-518): score [B,h,w] upsampled to labels [B,H,W] (int64 or uint8;
    0 = inlier, 1 = outlier, anything else ignored) as F.interpolate(align_corners=True) does, the terms of `func` (TAIL_FUNCS) against the two
    thresholds, the masked means and the halving rule -> (loss [1], stats [4] = (sum_in, n_in, sum_out, n_out) for the backward;
    "binary_cross_entropy": (sum, B H W, 0, 0)).  No outlier pixel: the inlier mean is not halved; no inlier pixel: NaN.  Nothing is read back
    to the host; both results are bitwise reproducible from launch to launch."""
    B, h, w, H, W, nb, f = _outlier_tail_args(score, labels, func)
    dev = score.device
    ws, _ = _workspace("rba_outlier_tail_workspace_f32", "outlier_tail", dev, B, H, W)
    loss = torch.empty((1,), dtype=torch.float32, device=dev)
    stats = torch.empty((4,), dtype=torch.float32, device=dev)
    _launch("rba_outlier_tail_fwd_f32", _p(score), _p(labels), nb, B, h, w, H, W, f, float(thr_in), float(thr_out), _p(ws), _p(loss), _p(stats))
    return loss, stats


@_hip_op
def outlier_tail_backward(score, labels, stats, grad_loss, func, thr_in, thr_out):
    """K9.  outlier_tail's inputs and `stats`, and the upstream gradient as a one-element fp32 device tensor (read on the device) -> grad_score
    [B,h,w], bitwise reproducible from launch to launch; a score pixel no label pixel samples gets 0."""
    B, h, w, H, W, nb, f = _outlier_tail_args(score, labels, func)
    _shaped(stats, "stats", (4,))
    _one_element(grad_loss, "grad_loss")
    grad = torch.empty((B, h, w), dtype=torch.float32, device=score.device)
    _launch("rba_outlier_tail_bwd_f32", _p(score), _p(labels), nb, B, h, w, H, W, f, float(thr_in), float(thr_out), _p(stats), _p(grad_loss),
            _p(grad))
    return grad


def _dense_hybrid_loss_args(sem, ood, labels):
    """The argument block of K10: sem fp32 contiguous [B,K,h,w] with 1 <= K <= 32, ood fp32 contiguous [B,2,h,w], labels int64 or uint8 contiguous
    [B,H,W], every size >= 1 and B H W, B K h w < 2^31 -> (B, K, h, w, H, W, bytes per label)."""
    _chk(sem, "sem", dim=4)
    _chk(ood, "ood", dim=4)
    nb = _labels(labels)
    (B, K, h, w), (H, W) = sem.shape, labels.shape[1:]
    if tuple(ood.shape) != (B, 2, h, w):
        raise RbaHipError(f"ood must have shape {(B, 2, h, w)} (sem is {tuple(sem.shape)}), got {tuple(ood.shape)}")
    if not 1 <= K <= 32:
        raise RbaHipError(f"dense_hybrid_loss: 1 <= K <= 32 classes, got {K}")
    if labels.shape[0] != B or min(B, h, w, H, W) < 1 or max(B * H * W, B * K * h * w) >= 1 << 31:
        raise RbaHipError(f"dense_hybrid_loss: sem [B,K,h,w] and labels [B,H,W] of one B, all sizes >= 1, B H W and B K h w < 2^31; got "
                          f"{tuple(sem.shape)} and {tuple(labels.shape)}")
    return B, K, h, w, H, W, nb


@_hip_op
def dense_hybrid_loss(sem, ood, labels, beta):
    """K10.  The reference's DenseHybrid loss behind its class map (criterion.py:406-431): sem [B,K,h,w] (the class map at mask resolution) and ood
    [B,2,h,w] (``ood_pred``) sampled at every pixel of labels [B,H,W] (int64 or uint8; < K: that class, 254: outlier, anything else ignored by the
    segmentation term) as F.interpolate(align_corners=True) does, log_softmax / logsumexp, get_batch_avg's mean and the two nll_loss means ->
    (losses [4] = (loss, loss_seg, loss_ood, loss_th), stats [8] = (S_seg, S_ood, S_th, S_x, n_seg, n_ood, B H W, m), lse [B,H,W] = logsumexp_k of
    the sampled class map, for the backward).  No class pixel or no outlier pixel: NaN.  Nothing is read back to the host; every result is bitwise
    reproducible from launch to launch."""
    B, K, h, w, H, W, nb = _dense_hybrid_loss_args(sem, ood, labels)
    dev = sem.device
    ws, _ = _workspace("rba_dense_hybrid_loss_workspace_f32", "dense_hybrid_loss", dev, B, H, W)
    losses = torch.empty((4,), dtype=torch.float32, device=dev)
    stats = torch.empty((8,), dtype=torch.float32, device=dev)
    lse = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _launch("rba_dense_hybrid_loss_fwd_f32", _p(sem), _p(ood), _p(labels), nb, B, K, h, w, H, W, float(beta), _p(ws), _p(losses), _p(stats), _p(lse))
    return losses, stats, lse


@_hip_op
def dense_hybrid_loss_backward(sem, ood, labels, stats, lse, grad_loss, beta):
    """K10.  dense_hybrid_loss's inputs, its ``stats`` and ``lse``, and the upstream gradient of losses[0] as a one-element fp32 device tensor (read
    on the device) -> (grad_sem [B,K,h,w], grad_ood [B,2,h,w]), bitwise reproducible from launch to launch; a pixel no label pixel samples gets 0."""
    B, K, h, w, H, W, nb = _dense_hybrid_loss_args(sem, ood, labels)
    _shaped(stats, "stats", (8,))
    _shaped(lse, "lse", (B, H, W))
    _one_element(grad_loss, "grad_loss")
    grad_sem = torch.empty((B, K, h, w), dtype=torch.float32, device=sem.device)
    grad_ood = torch.empty((B, 2, h, w), dtype=torch.float32, device=sem.device)
    _launch("rba_dense_hybrid_loss_bwd_f32", _p(sem), _p(ood), _p(labels), nb, _p(lse), B, K, h, w, H, W, float(beta), _p(stats), _p(grad_loss),
            _p(grad_sem), _p(grad_ood))
    return grad_sem, grad_ood


def _gambler_loss_args(sem, labels):
    """The argument block of K11a: sem fp32 contiguous [B,K+1,h,w] with 2 <= K + 1 <= 32, labels int64 or uint8 contiguous [B,H,W] with H, W >= 4
    (the blur's reflect padding), every other size >= 1, B <= 65535 and B H W, B (K+1) h w < 2^31 -> (B, K, h, w, H, W, bytes per label)."""
    _chk(sem, "sem", dim=4)
    nb = _labels(labels)
    (B, K1, h, w), (H, W) = sem.shape, labels.shape[1:]
    if not 2 <= K1 <= 32:
        raise RbaHipError(f"gambler_loss: 2 <= K + 1 <= 32 channels (the classes and the reservation channel), got {K1}")
    if labels.shape[0] != B or min(B, h, w) < 1 or min(H, W) < 4 or B > 65535 or max(B * H * W, B * K1 * h * w) >= 1 << 31:
        raise RbaHipError(f"gambler_loss: sem [B,K+1,h,w] and labels [B,H,W] of one B <= 65535, H and W >= 4, all other sizes >= 1, B H W and "
                          f"B (K+1) h w < 2^31; got {tuple(sem.shape)} and {tuple(labels.shape)}")
    return B, K1 - 1, h, w, H, W, nb


@_hip_op
def gambler_loss(sem, labels, ood_reg=0.1):
    """K11a.  The reference's gambler loss behind its class map (criterion.py:337-388): sem [B,K+1,h,w] (the class map at mask resolution WITH the
    no-object column: channel K is the reservation channel) sampled at every pixel of labels [B,H,W] (int64 or uint8; < K: an inlier pixel of
    that class, 254: outlier, anything else void) as F.interpolate(align_corners=True) does, softmax, the squared logsumexp reward blurred by
    GaussianBlur(7, sigma=1), the log terms and their means -> (losses [3] = (loss, inlier mean, outlier mean), stats [4] = (S_in, S_out, n_in,
    n_ood), R [B,H,W] = the blurred reward, for the backward).  No inlier pixel: NaN; no outlier pixel: the outlier mean is 0.  Nothing is read
    back to the host; every result is bitwise reproducible from launch to launch."""
    B, K, h, w, H, W, nb = _gambler_loss_args(sem, labels)
    dev = sem.device
    ws, _ = _workspace("rba_gambler_loss_workspace_f32", "gambler_loss", dev, B, H, W)
    losses = torch.empty((3,), dtype=torch.float32, device=dev)
    stats = torch.empty((4,), dtype=torch.float32, device=dev)
    reward = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    R = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    _launch("rba_gambler_loss_fwd_f32", _p(sem), _p(labels), nb, B, K, h, w, H, W, float(ood_reg), _p(ws), _p(reward), _p(losses), _p(stats), _p(R))
    return losses, stats, R


@_hip_op
def gambler_loss_backward(sem, labels, stats, R, grad_loss, ood_reg=0.1):
    """K11a.  gambler_loss's inputs, its ``stats`` and ``R``, and the upstream gradient of losses[0] as a one-element fp32 device tensor (read on
    the device) -> grad_sem [B,K+1,h,w], the gradient through the blurred reward included; bitwise reproducible from launch to launch; a pixel no
    label pixel samples gets 0."""
    B, K, h, w, H, W, nb = _gambler_loss_args(sem, labels)
    _shaped(stats, "stats", (4,))
    _shaped(R, "R", (B, H, W))
    _one_element(grad_loss, "grad_loss")
    dev = sem.device
    grad_R = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    grad_reward = torch.empty((B, H, W), dtype=torch.float32, device=dev)
    grad_sem = torch.empty((B, K + 1, h, w), dtype=torch.float32, device=dev)
    _launch("rba_gambler_loss_bwd_f32", _p(sem), _p(labels), nb, _p(R), B, K, h, w, H, W, float(ood_reg), _p(stats), _p(grad_loss), _p(grad_R),
            _p(grad_reward), _p(grad_sem))
    return grad_sem


def _blur_planes_args(x, name, kernel_size, sigma):
    """x fp32 contiguous [B,H,W], 1 <= B <= 65535, an odd kernel_size <= 15, sigma > 0, H and W > kernel_size // 2 -> (B, H, W)"""
    _chk(x, name, dim=3)
    B, H, W = x.shape
    if (kernel_size % 2 == 0 or not 1 <= kernel_size <= 15 or sigma <= 0 or not 1 <= B <= 65535 or min(H, W) <= kernel_size // 2
            or B * H * W >= 1 << 31):
        raise RbaHipError(f"gaussian_blur_planes needs [B,H,W] planes with 1 <= B <= 65535, an odd kernel_size <= 15, sigma > 0 and planes larger "
                          f"than the padding; got {tuple(x.shape)}, kernel_size {kernel_size}, sigma {sigma}")
    return B, H, W


@_hip_op
def gaussian_blur_planes(planes, kernel_size=7, sigma=1.0):
    """transforms.GaussianBlur(kernel_size, sigma) of each of the B planes [B,H,W] (reflect padding) in one launch; for B = 1 the bits of
    ``gaussian_blur``."""
    B, H, W = _blur_planes_args(planes, "planes", kernel_size, sigma)
    out = torch.empty_like(planes)
    _launch("rba_gaussian_blur_planes_f32", _p(planes), _p(out), B, H, W, int(kernel_size), float(sigma))
    return out


@_hip_op
def gaussian_blur_planes_adjoint(grad_out, kernel_size=7, sigma=1.0):
    """The adjoint of ``gaussian_blur_planes`` (autograd's backward of it): grad_out [B,H,W] -> grad_in [B,H,W].  Not the blur itself: near a
    border the taps the reflect padding folds back add.  Bitwise reproducible."""
    B, H, W = _blur_planes_args(grad_out, "grad_out", kernel_size, sigma)
    grad_in = torch.empty_like(grad_out)
    _launch("rba_gaussian_blur_planes_adjoint_f32", _p(grad_out), _p(grad_in), B, H, W, int(kernel_size), float(sigma))
    return grad_in


def _score_reg_args(score, labels):
    """The argument block of K11b: score fp32 contiguous [B,h,w]; labels None, or int64 / uint8 contiguous [B,H,W]; every size >= 1 and B H W,
    B h w < 2^31 -> (B, h, w, H, W, bytes per label); without labels H = W = 1."""
    _chk(score, "score", dim=3)
    B, h, w = score.shape
    H, W, nb = 1, 1, 8
    if labels is not None:
        nb = _labels(labels)
        H, W = labels.shape[1:]
        if labels.shape[0] != B:
            raise RbaHipError(f"score_reg: score [B,h,w] and labels [B,H,W] of one B; got {tuple(score.shape)} and {tuple(labels.shape)}")
    if min(B, h, w, H, W) < 1 or max(B * H * W, B * h * w) >= 1 << 31:
        raise RbaHipError(f"score_reg: all sizes >= 1, B H W and B h w < 2^31; got {tuple(score.shape)} and {(B, H, W)}")
    return B, h, w, H, W, nb


@_hip_op
def score_reg(score, labels=None):
    """K11b.  The reference's smoothness and sparsity losses behind their score map (criterion.py:270-279, 311-319): score [B,h,w]; labels
    [B,H,W] (int64 or uint8; 1 = outlier) or None -> (losses [2] = (smoothness = half the sum of the squared forward differences along both axes,
    sparsity = the 2-norm of the align_corners=True upsampled score over the outlier pixels; 0 without labels or without an outlier pixel),
    stats [2] = the two sums, for the backward).  Nothing is read back; bitwise reproducible from launch to launch."""
    B, h, w, H, W, nb = _score_reg_args(score, labels)
    dev = score.device
    ws, _ = _workspace("rba_score_reg_workspace_f32", "score_reg", dev, B, h, w, H, W)
    losses = torch.empty((2,), dtype=torch.float32, device=dev)
    stats = torch.empty((2,), dtype=torch.float32, device=dev)
    _launch("rba_score_reg_fwd_f32", _p(score), _p(labels), nb, B, h, w, H, W, _p(ws), _p(losses), _p(stats))
    return losses, stats


@_hip_op
def score_reg_backward(score, labels, stats, grad_smoothness=None, grad_sparsity=None):
    """K11b.  score_reg's inputs and ``stats``, and the two upstream gradients as one-element fp32 device tensors (one may be None = 0; they are
    read on the device) -> grad_score [B,h,w], bitwise reproducible; the sparsity part is 0 where the norm is 0."""
    B, h, w, H, W, nb = _score_reg_args(score, labels)
    _shaped(stats, "stats", (2,))
    if grad_smoothness is None and grad_sparsity is None:
        raise RbaHipError("score_reg_backward: at least one of grad_smoothness / grad_sparsity")
    for g, name in ((grad_smoothness, "grad_smoothness"), (grad_sparsity, "grad_sparsity")):
        if g is not None:
            _one_element(g, name)
    grad = torch.empty((B, h, w), dtype=torch.float32, device=score.device)
    _launch("rba_score_reg_bwd_f32", _p(score), _p(labels), nb, B, h, w, H, W, _p(stats), _p(grad_smoothness), _p(grad_sparsity), _p(grad))
    return grad


@_hip_op
def swin_bias_fragments(rel_bias, window_size):
    """[nH,N,N] gathered relative-position bias -> the MFMA-fragment-ordered copy K5 reads with coalesced loads."""
    _chk(rel_bias, "rel_bias", dim=3)
    nH = rel_bias.shape[0]
    N = int(window_size) * int(window_size)
    if window_size < 1 or tuple(rel_bias.shape) != (nH, N, N):
        raise RbaHipError(f"rel_bias must be [nH, ws*ws, ws*ws] for window_size {window_size}, got {tuple(rel_bias.shape)}")
    frag = torch.empty(_query("rba_swin_bias_fragments_elems", nH, window_size), dtype=torch.float32, device=rel_bias.device)
    _launch("rba_swin_bias_fragments_f32", _p(rel_bias), _p(frag), nH, window_size)
    return frag


def swin_window_attn_split_ok(head_dim, window_size):
    """Geometries whose window-attention kernel can write SplitActivations (the f16x3 matrix-pipe form)."""
    return head_dim == 32 and window_size == 12


@_hip_op
def swin_window_attn(qkv, qkv_bias, rel_bias, H, W, num_heads, window_size, shift, bias_frag=None, split_out=False):
    """K5.  qkv [B,H*W,3*C] = Linear(norm1(x)) on un-padded tokens, qkv_bias [3*C], rel_bias [nH,N,N] ->
    attention output [B,H*W,C] (before proj).  swin.py:131-171 + :251-284 + :413-440."""
    _chk(qkv, "qkv", dim=3)
    _chk(rel_bias, "rel_bias", dim=3)
    B, L, C3 = qkv.shape
    C = C3 // 3
    if L != H * W or C3 != 3 * C or C % num_heads:
        raise RbaHipError("qkv shape does not match H, W, num_heads")
    hd = C // num_heads
    N = window_size * window_size
    if tuple(rel_bias.shape) != (num_heads, N, N):
        raise RbaHipError("rel_bias must be [nH, ws*ws, ws*ws]")
    _vec(qkv_bias, "qkv_bias", C3)
    if bias_frag is not None:
        _vec(bias_frag, "bias_frag", _query("rba_swin_bias_fragments_elems", num_heads, window_size))
    if split_out:                                   # the proj Linear's split A operand (see swin_window_attn_split_ok)
        if not swin_window_attn_split_ok(hd, window_size) or bias_frag is None:
            raise RbaHipError("split_out needs head_dim 32, 12 x 12 windows and bias_frag")
        out = SplitActivations.empty((B, L, C), qkv.device)
        _launch("rba_swin_window_attn_split_out_f32", _p(qkv), _p(qkv_bias), _p(bias_frag), _p(out.data), B, H, W, num_heads, hd, window_size, shift)
        return out
    out = torch.empty((B, L, C), dtype=torch.float32, device=qkv.device)
    _launch("rba_swin_window_attn_f32", _p(qkv), _p(qkv_bias), _p(rel_bias), _p(bias_frag), _p(out), B, H, W, num_heads, hd, window_size, shift)
    return out


SWIN_ATTN_FUSED = os.environ.get("RBA_SWIN_ATTN_FUSED", "1") != "0"      # A/B switch (tools): 0 keeps the unfused LN -> qkv -> K5 -> proj sequence


def _k7_ok(supported, C, num_heads, window_size):
    return SWIN_ATTN_FUSED and _split_mode() == "f16x3" and num_heads * 32 == C and bool(_query(supported, int(C), int(window_size)))


def swin_attn_block_ok(C, num_heads, window_size):
    """True when swin_attn_block() has a kernel for this geometry (K7: head_dim 32, 12 x 12 windows, f16x3 mode)."""
    return _k7_ok("rba_swin_attn_block_supported", C, num_heads, window_size)


def swin_attn_qkv_ok(C, num_heads, window_size):
    """True when swin_attn_qkv() has a kernel for this geometry (K7 without proj: C = 128 / 256, head_dim 32, 12 x 12 windows, f16x3 mode)."""
    return _k7_ok("rba_swin_attn_qkv_supported", C, num_heads, window_size)


def _k7_args(who, supported, x, norm1, image, qkv_bias, bias_frag, H, W, window_size, more=()):
    """K7's argument block (`who` = the wrapper, `supported` = its geometry query; `more`: further (vector [C], name) pairs): x [B, H*W, C] of a geometry that form has a kernel for, norm1 = (weight [C], bias [C],
    eps), qkv_bias [3C], image / bias_frag of the sizes the library states -> (B, L, C, norm1.weight, norm1.bias, eps)."""
    _chk(x, "x", dim=3)
    B, L, C = x.shape
    if L != H * W or not _query(supported, int(C), int(window_size)):
        raise RbaHipError(f"{who}: check {who}_ok(C, num_heads, window_size) first; x must be [B, H*W, C]")
    g1, b1, eps1 = norm1
    _vec(g1, "norm1.weight", C)
    _vec(b1, "norm1.bias", C)
    for t, name in more:
        _vec(t, name, C)
    _vec(qkv_bias, "qkv_bias", 3 * C)
    _chk(image, "image", dtype=torch.uint8, dim=1)
    if image.numel() != _query("rba_swin_attn_block_weight_bytes", int(C)):
        raise RbaHipError("image must come from swin_attn_block_weights of this block's qkv / proj weights")
    _vec(bias_frag, "bias_frag", _query("rba_swin_bias_fragments_elems", C // 32, int(window_size)))      # = swin_bias_fragments(...)
    return B, L, C, g1, b1, float(eps1)


@_hip_op
def swin_attn_qkv(x, norm1, image, qkv_bias, bias_frag, H, W, window_size, shift):
    """K7 without proj: window_attention(qkv(norm1(x))) before the output projection (swin.py:235-168), returned as SplitActivations -- the proj Linear's A
    operand: ``x = ops.linear(y, attn.proj, residual=x)`` finishes the half block.  x [B, H*W, C] is only read.  Check swin_attn_qkv_ok first."""
    B, L, C, g1, b1, eps1 = _k7_args("swin_attn_qkv", "rba_swin_attn_qkv_supported", x, norm1, image, qkv_bias, bias_frag, H, W, window_size)
    out = SplitActivations.empty((B, L, C), x.device)
    _launch("rba_swin_attn_qkv_split_out_f32", _p(x), _p(out.data), _p(g1), _p(b1), eps1, _p(image), _p(qkv_bias), _p(bias_frag), B, H, W, C,
            int(window_size), int(shift))
    return out


@_hip_op
def swin_attn_block_weights(qkv_weight, proj_weight):
    """qkv.weight [3C, C] + proj.weight [C, C] -> K7's per-head image of MFMA operand fragments (uint8; once per weight load)."""
    _chk(qkv_weight, "qkv_weight", dim=2)
    _chk(proj_weight, "proj_weight", dim=2)
    C = proj_weight.shape[0]
    if tuple(qkv_weight.shape) != (3 * C, C) or tuple(proj_weight.shape) != (C, C) or C % 32:
        raise RbaHipError("swin_attn_block_weights needs qkv.weight [3C, C] and proj.weight [C, C], C % 32 == 0")
    img = torch.empty(int(_query("rba_swin_attn_block_weight_bytes", C)), dtype=torch.uint8, device=qkv_weight.device)
    _launch("rba_swin_attn_block_pack_f32", _p(qkv_weight), _p(proj_weight), _p(img), C)
    return img


@_hip_op
def swin_attn_block(x, norm1, image, qkv_bias, bias_frag, proj_bias, H, W, window_size, shift, norm2=None):
    """K7: x [B, H*W, C] <- x + proj(window_attention(qkv(norm1(x)))) IN PLACE (swin.py:235-284); with ``norm2`` also returns
    y2 = norm2(x) (:284-293).  norm1 / norm2 = (weight, bias, eps); image = swin_attn_block_weights(...); bias_frag = swin_bias_fragments(...).
    Returns (x, y2 | None).  Check swin_attn_block_ok first."""
    B, L, C, g1, b1, eps1 = _k7_args("swin_attn_block", "rba_swin_attn_block_supported", x, norm1, image, qkv_bias, bias_frag, H, W, window_size,
                                      more=((proj_bias, "proj_bias"),))
    y2, g2, b2, eps2 = None, None, None, 0.0
    if norm2 is not None:
        g2, b2, eps2 = norm2
        _vec(g2, "norm2.weight", C)
        _vec(b2, "norm2.bias", C)
        y2 = torch.empty_like(x)
    _launch("rba_swin_attn_block_f32", _p(x), _p(y2), _p(g1), _p(b1), eps1, _p(image), _p(qkv_bias), _p(bias_frag), _p(proj_bias), _p(g2), _p(b2),
            float(eps2), B, H, W, C, int(window_size), int(shift))
    return x, y2


@_hip_op
def group_norm(x, num_groups, weight, bias, eps=1e-5, relu=False):
    """GroupNorm (+ReLU) of x [B,C,h,w] -- the norm/activation of Detectron2's Conv2d wrapper
    (msdeformattn.py:222-235, 278-297)."""
    _chk(x, "x", dim=4)
    B, C, h, w = x.shape
    _vec(weight, "weight", C)
    _vec(bias, "bias", C)
    if C % num_groups:
        raise RbaHipError("channels must be divisible by num_groups")
    ws = _scratch(_query("rba_group_norm_workspace_bytes", B, C, h * w, num_groups), x.device)
    y = torch.empty_like(x)
    _launch("rba_group_norm_f32", _p(x), _p(weight), _p(bias), _p(y), _p(ws), B, C, h * w, num_groups, float(eps), int(bool(relu)))
    return y


@_hip_op
def add_layer_norm(x, weight, bias, eps=1e-5, residual=None, residual_bias=None, inplace_sum=False, frag=False):
    """y = LayerNorm(x + residual + residual_bias) over the last dim.  Returns (s, y) where s = the summed tensor
    (x itself when there is nothing to add; written in place over x when inplace_sum, else a new tensor).
    ``frag``: y is returned as SplitActivations (the f16x3 GEMM's A operand, already split and fragment-ordered) for linear()."""
    _chk(x, "x")
    C = x.shape[-1]
    _vec(weight, "weight", C)
    _vec(bias, "bias", C)
    rows = x.numel() // C if C else 0
    _shaped(residual, "residual", x.shape, optional=True)
    _vec(residual_bias, "residual_bias", C, optional=True)
    if frag and C % 32:
        raise RbaHipError("add_layer_norm(frag=True) needs C % 32 == 0")
    has_sum = residual is not None or residual_bias is not None
    s = x if (not has_sum or inplace_sum) else torch.empty_like(x)
    y = SplitActivations.empty(tuple(x.shape), x.device) if frag else torch.empty_like(x)
    _launch("rba_add_layer_norm_frag_f32" if frag else "rba_add_layer_norm_f32", _p(x), _p(residual), _p(residual_bias), _p(weight), _p(bias),
            _p(s) if has_sum else 0, _p(y.data) if frag else _p(y), rows, C, float(eps))
    return s, y


@_hip_op
def msda_prepare(raw, reference_points, spatial_shapes, M, L, P):
    """raw [N, Lq, M*L*P*3] (offsets | logits of the fused sampling Linear), reference_points [N, Lq, L, 2], spatial_shapes [L,2] int64
    -> (sampling_locations [N,Lq,M,L,P,2], attention_weights [N,Lq,M,L,P]) as MSDeformAttn.forward computes them."""
    _chk(raw, "raw", dim=3)
    _chk(reference_points, "reference_points", dim=4)
    _level_shapes(spatial_shapes, L)
    N, Lq, W3 = raw.shape
    if W3 != 3 * M * L * P or tuple(reference_points.shape) != (N, Lq, L, 2):
        raise RbaHipError("msda_prepare: shapes do not match")
    loc = torch.empty((N, Lq, M, L, P, 2), dtype=torch.float32, device=raw.device)
    attw = torch.empty((N, Lq, M, L, P), dtype=torch.float32, device=raw.device)
    _launch("rba_msda_prepare_f32", _p(raw), _p(reference_points), _p(spatial_shapes), _p(loc), _p(attw), N * Lq, M, L, P)
    return loc, attw


def msda_fused_ok(D, L, P, S=None, M=None):
    """Geometries of the one-launch deformable attention core (head_dim 32, 4 points, 1 or 3 levels: every released configuration); with
    S positions and M heads given, also that one image's value [S, M, 32] fp32 stays below 4 GiB (the kernel's 32-bit tap offsets)."""
    return D == 32 and P == 4 and L in (1, 3) and (S is None or M is None or S * M * 128 < (1 << 32))


@_hip_op
def msda_fused(value, spatial_shapes, level_start_index, raw, reference_points, M, L, P):
    """MSDeformAttn.forward's core in one launch: value [N,S,M,32], raw [N,Lq,M*L*P*3] (offsets | logits of the fused sampling Linear),
    reference_points [N,Lq,L,2] -> [N,Lq,M*32]; sampling locations and the softmax over the L*P logits are computed inside the gather
    kernel (bit-identical to msda_prepare + ms_deform_attn_forward)."""
    _chk(value, "value", dim=4)
    _level_shapes(spatial_shapes, L)
    _chk(level_start_index, "level_start_index", torch.int64, 1)
    _chk(raw, "raw", dim=3)
    _chk(reference_points, "reference_points", dim=4)
    N, S, M2, D = value.shape
    _, Lq, W3 = raw.shape
    if (M2 != M or not msda_fused_ok(D, L, P, S, M) or W3 != 3 * M * L * P or raw.shape[0] != N or tuple(reference_points.shape) != (N, Lq, L, 2)
            or level_start_index.shape[0] != L):
        raise RbaHipError("msda_fused: shapes do not match (head_dim 32, P = 4, L in {1, 3})")
    out = torch.empty((N, Lq, M * D), dtype=torch.float32, device=value.device)
    _launch("rba_msda_fused_f32", _p(value), _p(spatial_shapes), _p(level_start_index), _p(raw), _p(reference_points), _p(out), N, S, M, D, L, Lq, P)
    return out


@_hip_op
def merge_layer_norm(x, H, W, weight, bias, eps=1e-5):
    """PatchMerging's gather + LayerNorm: x [B, H*W, C] -> [B, ceil(H/2)*ceil(W/2), 4C] = LN over the 2x2 neighbourhoods in the order
    (ee, oe, eo, oo), odd maps zero-padded -- the concatenated tensor is never materialised."""
    _chk(x, "x", dim=3)
    B, L, C = x.shape
    _vec(weight, "weight", 4 * C)
    _vec(bias, "bias", 4 * C)
    if L != H * W or C % 4:
        raise RbaHipError("merge_layer_norm needs x [B, H*W, C] (C % 4 == 0) and a LayerNorm over 4C channels")
    y = torch.empty((B, ((H + 1) // 2) * ((W + 1) // 2), 4 * C), dtype=torch.float32, device=x.device)
    _launch("rba_merge_layer_norm_f32", _p(x), _p(weight), _p(bias), _p(y), B, H, W, C, float(eps))
    return y


@_hip_op
def skinny_linear(x, weight, bias=None, relu=False, x_add=None, add_cols=None, segments=1, out=None):
    """F.linear(x, weight, bias) [+ ReLU] for x with at most 128 rows (the decoder's 100 queries): [..., K] -> [..., N].
    x_add: output columns n < add_cols (default: all; a multiple of 16) are computed from ``x + x_add`` -- the query position embedding of
    mask2former_transformer_decoder.py:48-58, 106-118 added inside the projection.  segments = s > 1: the N outputs are returned as s
    separately contiguous tensors [..., N / s] (q, k, v of a stacked in_proj weight) written by the one launch.
    out (segments = 1 only): a caller-owned contiguous fp32 [..., N] tensor (e.g. a row slice of a larger one) the launch writes instead of a new tensor."""
    _chk(x, "x")
    _chk(weight, "weight", dim=2)
    K = x.shape[-1]
    N = weight.shape[0]
    M = x.numel() // K if K else 0
    lead = tuple(x.shape[:-1])
    if weight.shape[1] != K or K % 32 or M > 128:
        raise RbaHipError("skinny_linear needs weight [N,K], K % 32 == 0 and at most 128 rows")
    _vec(bias, "bias", N, optional=True)
    segments = int(segments)
    if segments < 1 or N % segments:
        raise RbaHipError("segments must divide N")
    if out is not None:
        _chk(out, "out")
        if segments != 1 or tuple(out.shape) != lead + (N,):
            raise RbaHipError("out must be a contiguous fp32 [..., N] tensor with x's leading shape (segments = 1)")
    if x_add is None and segments == 1:
        if out is None:
            out = torch.empty(lead + (N,), dtype=torch.float32, device=x.device)
        _launch("rba_skinny_linear_f32", _p(x), _p(weight), _p(bias), _p(out), M, N, K, int(bool(relu)))
        return out
    _shaped(x_add, "x_add", x.shape, optional=True)
    add_cols = N if add_cols is None else int(add_cols)
    if add_cols % 16 or not 0 <= add_cols <= N:
        raise RbaHipError("add_cols must be a multiple of 16 in [0, N]")
    seg_n = N // segments
    segs = None
    if out is None:
        out = segs = torch.empty((segments,) + lead + (seg_n,), dtype=torch.float32, device=x.device)
    _launch("rba_skinny_linear_add_f32", _p(x), _p(x_add), add_cols, _p(weight), _p(bias), _p(out), M, N, K, int(bool(relu)), seg_n if segments > 1 else 0)
    if segs is None:
        return out
    return segs[0] if segments == 1 else tuple(segs[i] for i in range(segments))


class SplitActivations:
    """A [..., K] fp32 activation tensor held ONLY as the f16x3 GEMM's A operand: h = f16(x), l = f16((x - h) 2^11), stored per
    (32-row group, 32-wide block of K) as four 1 KiB pieces [h g0 | l g0 | h g1 | l g1], each [k-half][row & 31][8 f16] with
    k = 32 b + 16 half + 8 g + i (csrc/split_linear_h3.h, "PRE").  Same bytes as the fp32 tensor (rows padded to a multiple of 32,
    padding never written); produced by add_layer_norm(frag=True), consumed by linear().  ``shape`` = the logical fp32 shape."""
    __slots__ = ("data", "shape")

    def __init__(self, data, shape):
        self.data, self.shape = data, tuple(shape)

    @staticmethod
    def empty(shape, device):
        M, K = math.prod(shape[:-1]), shape[-1]
        return SplitActivations(torch.empty((((M + 31) // 32) * 32 * K,), dtype=torch.int32, device=device), shape)

    @property
    def device(self):
        return self.data.device

    def numel(self):
        return math.prod(self.shape)

    @staticmethod
    def pack(x):
        """Reference packer (torch ops; tests and tools): the image the kernels write for x."""
        K = x.shape[-1]
        x2 = x.reshape(-1, K).float()
        M = x2.shape[0]
        Mp = (M + 31) // 32 * 32
        xp = torch.zeros((Mp, K), dtype=torch.float32, device=x.device)
        xp[:M] = x2
        h = xp.half()
        l = ((xp - h.float()) * 2048.0).half()
        hl = torch.stack([h, l], 0).reshape(2, Mp // 32, 32, K // 32, 2, 2, 8)          # [hl, rg, l31, b, half, g, i]
        img = hl.permute(1, 3, 5, 0, 4, 2, 6).contiguous()                              # [rg, b, g, hl, half, l31, i]
        return SplitActivations(img.reshape(-1).view(torch.int32), x.shape)

    def unpack(self):
        """fp32 values h + l 2^-11 of the image (rows beyond M dropped)."""
        K = self.shape[-1]
        M = self.numel() // K
        Mp = (M + 31) // 32 * 32
        img = self.data.view(torch.float16).reshape(Mp // 32, K // 32, 2, 2, 2, 32, 8)  # [rg, b, g, hl, half, l31, i]
        hl = img.permute(3, 0, 5, 1, 4, 2, 6).reshape(2, Mp, K).float()
        return (hl[0] + hl[1] / 2048.0)[:M].reshape(self.shape)


_SPLIT = threading.local()
_SPLIT_DEFAULT = "f16x3"
"""ops.SPLIT_MODE: arithmetic of the token Linear (K6), PER THREAD (round 5: it was a process global; a re-score on another thread, or a tool
flipping it, changed the kernels of every forward in flight).  Read it as `ops.SPLIT_MODE`, set it for a block with `ops.split_mode(mode)`.  "f16x3": two f16 pieces per operand, three f16 MFMAs per product -- as accurate as an
fp32 GEMM for |x|, |w| < 65504 (beyond f16's range the output is NaN, never silently wrong), twice the speed of "bf16x6": three
bf16 pieces, six MFMAs, fp32's full range."""


def _split_mode():
    return getattr(_SPLIT, "mode", _SPLIT_DEFAULT)


def __getattr__(name):                     # module attribute: ops.SPLIT_MODE = the calling thread's mode
    if name == "SPLIT_MODE":
        return _split_mode()
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


class _OpsModule(type(os)):
    """`ops.SPLIT_MODE = "bf16x6"` was the supported switch until round 4.  Since the mode became per thread an assignment only created a module attribute that
    SHADOWED the getter above: ops.SPLIT_MODE then read "bf16x6" (graph keys, cache names) while every kernel kept dispatching on the thread's real mode -- a NaN
    re-score written the old way was a silent no-op.  Assignment now fails loudly."""

    def __setattr__(self, name, value):
        if name == "SPLIT_MODE":
            raise AttributeError('ops.SPLIT_MODE is read-only (the arithmetic mode is per thread): run the block inside `with ops.split_mode("bf16x6"):`')
        super().__setattr__(name, value)


import sys as _sys  # noqa: E402
_sys.modules[__name__].__class__ = _OpsModule


@_hip_op
def split_weight(weight, mode=None):
    """fp32 weight [N,K] -> the packed operand planes of the token Linear, tiled as the kernel's LDS image (once per weight load):
    mode "bf16x6": three bf16 planes hi, mid, lo (sum exactly `weight`), [N/128, K/16, 3, 128, 2, 8] bf16, the 8-element half h of
    row r in slot h ^ ((r >> 3) & 1);  mode "f16x3": h = f16(w), l = f16((w - h) 2^11), [N/128, K/16, 2, 128, 2, 8] float16 with
    the k order of csrc/split_linear_h3.h.  Default: ops.SPLIT_MODE."""
    _chk(weight, "weight", dim=2)
    N, K = weight.shape
    if not split_linear_supported(N, K):
        raise RbaHipError("split_weight needs weight [N,K] with K % 32 == 0")
    mode = _split_mode() if mode is None else mode
    if mode not in ("f16x3", "bf16x6"):
        raise RbaHipError(f"unknown split mode {mode!r}")
    f16 = mode == "f16x3"
    packed = torch.empty(((N + 127) // 128, K // 16, 2 if f16 else 3, 128, 2, 8), dtype=torch.float16 if f16 else torch.bfloat16, device=weight.device)
    _launch("rba_split_weight_f16x2" if f16 else "rba_split_weight_bf16x3", _p(weight), _p(packed), N, K)
    return packed


@_hip_op
def unpack_split_weight(packed):
    """Inverse of split_weight's tiling: -> planes [3, Np, K] bf16 or [2, Np, K] float16, Np = N rounded up to 128 (for inspection
    and tests)."""
    nt, S, P = packed.shape[:3]
    r = torch.arange(128, device=packed.device)
    flip = ((r >> 3) & 1).bool()
    un = torch.where(flip.view(1, 1, 1, 128, 1, 1), packed.flip(4), packed)          # slot -> half
    if P == 2:        # f16x3: sub-stage 2 b + g, half h holds k = 32 b + 16 h + 8 g + (0..7)
        un = un.reshape(nt, S // 2, 2, P, 128, 2, 8).permute(3, 0, 4, 1, 5, 2, 6)     # [P, nt, row, b, h, g, 8]
        return un.reshape(P, nt * 128, S * 16)
    return un.permute(2, 0, 3, 1, 4, 5).reshape(3, nt * 128, S * 16)


def split_linear_supported(N, K):
    return K % 32 == 0 and N >= 1 and K >= 32


TILES_MIN = 64


def split_linear_pays(M, N, K, gelu=False):
    """Where the bf16x6 kernel beats hipBLASLt's fp32 GEMM on MI355X (tools/gemm_v4_sweep.py, profiles/r02_split_linear.txt):
    1.3-1.7x whenever there are at least 64 tiles of 128 x 128 (below 256 tiles the library switches to 128 x 64 tiles so that
    every CU still gets work) and K >= 64.  Since round 5 this is a statement about speed only: linear() runs the library's own kernels for every shape."""
    if not split_linear_supported(N, K) or K < 64:
        return False
    return _tiles128(M, N) >= TILES_MIN


@_hip_op
def linear(x, lin, use_bias=True, gelu=False, relu=False, residual=None, split_out=False):
    """``F.linear(x, lin.weight, lin.bias)`` [+ exact GELU | ReLU] for an ``nn.Linear`` on a token tensor, through the split
    kernel of the current ops.SPLIT_MODE (weight planes are split once per weight load and cached on the module) -- no library GEMM for any shape.
    ``residual`` (f16x3 form only, see linear_residual_fused): returns ``(residual + x W^T) + bias`` written IN PLACE over `residual`.
    ``split_out`` (f16x3, with gelu): the result is returned as SplitActivations for the next linear() (fc1 -> fc2)."""
    w = lin.weight
    N, K = w.shape
    M = x.numel() // K if K else 0
    bias = lin.bias if use_bias else None
    if isinstance(x, SplitActivations):
        if _split_mode() != "f16x3" or x.shape[-1] != K:
            raise RbaHipError("SplitActivations feed the f16x3 Linear only (check linear_takes_split(M, N, K) before producing them)")
        return split_linear(x, _cached_planes(lin, w), bias, gelu=gelu, out_features=N, relu=relu, residual=residual, split_out=split_out)
    _chk(x, "x") if x.is_contiguous() else _chk(x.contiguous(), "x")          # HIP fp32 tensors only: no CPU path here either
    if split_out:
        if _split_mode() != "f16x3" or not split_linear_supported(N, K):
            raise RbaHipError("linear(split_out=True) needs the f16x3 mode and K % 32 == 0")
        return split_linear(x.contiguous(), _cached_planes(lin, w), bias, gelu=gelu, out_features=N, split_out=True)
    if residual is not None and not linear_residual_fused(M, N, K):
        raise RbaHipError("linear(residual=...) needs the fused f16x3 path: check linear_residual_fused(M, N, K) first")
    if split_linear_supported(N, K):
        # round 5: every shape runs the library's own GEMM (the f16x3 / bf16x6 kernels take any M and N); `split_linear_pays` only says where they beat
        # hipBLASLt, and the small launches it used to send there (tiny test nets, the bf16x6 re-score of the encoder / decoder Linears) are latency-bound anyway
        return split_linear(x.contiguous(), _cached_planes(lin, w), bias, gelu=gelu, out_features=N, relu=relu, residual=residual)
    # K not a multiple of 32 (no layer of the released architectures): zero-pad K once per weight load and per call -- still no library GEMM
    Kp = (K + 31) // 32 * 32
    xp = torch.zeros(tuple(x.shape[:-1]) + (Kp,), dtype=torch.float32, device=x.device)
    xp[..., :K] = x
    return split_linear(xp, _cached_planes(lin, w, pad_k=Kp), bias, gelu=gelu, out_features=N, relu=relu)


def _cached_planes(lin, w, pad_k=None):
    """split_weight(w) of the current split mode, cached on the module per mode (the bf16x6 planes of the non-finite fallback stay
    beside the f16x3 ones: switching modes does not re-split).  pad_k: w zero-padded to that many columns first."""
    def build():
        w2 = w.detach().contiguous()
        if pad_k is not None:
            w2 = torch.nn.functional.pad(w2, (0, pad_k - w2.shape[1]))
        return split_weight(w2)

    return derived(lin, ("planes", _split_mode()), (w,), build, pad_k)


@contextlib.contextmanager
def split_mode(mode):
    """Run a block with ops.SPLIT_MODE = mode ("f16x3" | "bf16x6") ON THE CALLING THREAD, e.g. to re-score an image whose f16x3 result is NaN
    (an activation or weight beyond f16's range) on the full-range kernels.  Other threads of the process keep their own mode; launches already
    enqueued on any stream are not affected (the mode selects kernels at launch time)."""
    if mode not in ("f16x3", "bf16x6"):
        raise RbaHipError(f"unknown split mode {mode!r}")
    prev = _split_mode()
    _SPLIT.mode = mode
    try:
        yield
    finally:
        _SPLIT.mode = prev


SPLIT_ACTIVATIONS = os.environ.get("RBA_SPLIT_ACTIVATIONS", "1") != "0"      # A/B switch (tools): producers keep writing fp32 rows


# smallest K whose Linear takes its A operand as a split image.  Round 2 stopped at K > 256 (the LDS-staged fp32-row kernel served Swin stages
# 1-2); round 3 hands the operand over from K = 128 on: those launches are HBM-bound either way (+0.8 % images/s, tools: RBA_SPLIT_MIN_K)
SPLIT_MIN_K = int(os.environ.get("RBA_SPLIT_MIN_K", "128"))


def linear_takes_split(M, N, K):
    """True when linear() on this shape runs a kernel whose A operand a producer can hand over as SplitActivations: the pipelined
    128-column f16x3 kernel (K >= SPLIT_MIN_K, at least 160 tiles of 128 x 128) or, for smaller launches, the sub-tile kernel of
    csrc/split_linear_h3q.h (K % 64 == 0, K >= 256, N % 32 == 0, at least 32 tiles: Swin stage 4's proj / fc2 with 128 tiles)."""
    if not (SPLIT_ACTIVATIONS and _split_mode() == "f16x3" and K >= SPLIT_MIN_K and K % 32 == 0):
        return False
    tiles = _tiles128(M, N)
    return tiles >= 160 or (tiles >= 32 and K % 64 == 0 and K >= 256 and N % 32 == 0)


MLP_FUSED_MIN_ROWS = 32768          # 256 workgroups of 128 rows: below that the unfused pair's 128 x 128 tiles fill the chip better


def mlp_fused_ok(M, C, hidden):
    """True when mlp_fused() applies: the one-kernel Swin MLP exists for C = 128 (Swin-B stage 1), f16x3 mode."""
    return SPLIT_ACTIVATIONS and _split_mode() == "f16x3" and C == 128 and hidden % 32 == 0 and hidden >= 64 and M >= MLP_FUSED_MIN_ROWS


@_hip_op
def mlp_fused(x, fc1, fc2, residual):
    """residual + fc2(GELU(fc1(x))) in one kernel, in place over `residual` (Mlp + residual add of a Swin block, swin.py:35-41, 293): the
    hidden tensor stays in registers.  Bit-identical to linear(split_out=True) + linear(residual=...)."""
    _chk(x, "x")
    _chk(residual, "residual")
    C, hidden = fc1.weight.shape[1], fc1.weight.shape[0]
    M = x.numel() // C
    if (x.shape[-1] != C or tuple(fc2.weight.shape) != (C, hidden) or tuple(residual.shape) != tuple(x.shape) or C != 128 or hidden % 32
            or _split_mode() != "f16x3"):
        raise RbaHipError("mlp_fused needs C == 128, hidden % 32 == 0, matching fc1 / fc2 and the f16x3 mode")
    _vec(fc1.bias, "fc1.bias", hidden)
    _vec(fc2.bias, "fc2.bias", C, optional=True)
    _launch("rba_swin_mlp_fused_f16x3_f32", _p(x), _p(_cached_planes(fc1, fc1.weight)), _p(fc1.bias), _p(_cached_planes(fc2, fc2.weight)), _p(fc2.bias),
            _p(residual), _p(residual), M, C, hidden)
    return residual


@_hip_op
def mlp_fused_ln(x, norm, fc1, fc2):
    """x <- x + fc2(GELU(fc1(LayerNorm(x)))) IN PLACE in one kernel (swin.py:293): mlp_fused with norm2 computed in the kernel's prologue from the rows it
    loads anyway.  norm = (weight, bias, eps).  Same conditions as mlp_fused (check mlp_fused_ok)."""
    _chk(x, "x")
    g, b, eps = norm
    C, hidden = fc1.weight.shape[1], fc1.weight.shape[0]
    _vec(g, "norm.weight", C)
    _vec(b, "norm.bias", C)
    M = x.numel() // C
    if x.shape[-1] != C or tuple(fc2.weight.shape) != (C, hidden) or C != 128 or hidden % 32 or _split_mode() != "f16x3":
        raise RbaHipError("mlp_fused_ln needs C == 128, hidden % 32 == 0, matching fc1 / fc2 and the f16x3 mode")
    _vec(fc1.bias, "fc1.bias", hidden)
    _vec(fc2.bias, "fc2.bias", C, optional=True)
    _launch("rba_swin_mlp_fused_ln_f16x3_f32", _p(x), _p(g), _p(b), float(eps), _p(_cached_planes(fc1, fc1.weight)), _p(fc1.bias),
            _p(_cached_planes(fc2, fc2.weight)), _p(fc2.bias), M, C, hidden)
    return x


def linear_residual_fused(M, N, K):
    """True when linear(..., residual=r) runs as ONE kernel (the f16x3 GEMM with the residual add in its epilogue)."""
    return _split_mode() == "f16x3" and split_linear_pays(M, N, K)


@_hip_op
def split_linear(x, planes, bias=None, gelu=False, out_features=None, relu=False, residual=None, split_out=False):
    """F.linear(x, W, bias) [+ exact GELU] with W given as split_weight(W): fp32-accurate on the bf16 / f16 matrix pipe (the planes'
    dtype says which form they were packed for).
    ``out_features`` = N when it is not a multiple of 128 (the packed planes are padded)."""
    xp, pre = _split_x(x, "split_linear")
    K = x.shape[-1]
    N, f16 = _packed(planes, K, out_features)
    M = x.numel() // K if K else 0
    lead = tuple(x.shape[:-1])
    if not split_linear_supported(N, K):
        raise RbaHipError("split_linear needs x [..., K] and split_weight(W) of a weight [N,K] with K % 32 == 0")
    _vec(bias, "bias", N, optional=True)
    act = 1 if gelu else (2 if relu else 0)
    if split_out:                            # GELU(x W^T + bias) handed to the next Linear as its split A operand
        if not f16 or act != 1 or residual is not None or N % 32:
            raise RbaHipError("split_out needs f16x3 planes, gelu=True, no residual and N % 32 == 0")
        out = SplitActivations.empty(lead + (N,), x.device)
        _launch("rba_split_linear_f16x3_gelu_split_out", xp, 1 if pre else 0, _p(planes), _p(bias), _p(out.data), M, N, K)
        return out
    if residual is not None:                 # out = (residual + x W^T) + bias, in place over `residual` (f16x3 planes, no activation)
        _chk(residual, "residual")
        if not f16 or act or tuple(residual.shape) != lead + (N,):
            raise RbaHipError("residual needs f16x3 planes, no activation and a [..., N] tensor")
        if pre:
            _launch("rba_split_linear_f16x3_frag_f32", xp, _p(planes), _p(bias), _p(residual), _p(residual), M, N, K, 0)
        else:
            _launch("rba_split_linear_f16x3_res_f32", xp, _p(planes), _p(bias), _p(residual), _p(residual), M, N, K)
        return residual
    if pre and not f16:
        raise RbaHipError("SplitActivations need f16x3 planes")
    out = torch.empty(lead + (N,), dtype=torch.float32, device=x.device)
    if pre:
        _launch("rba_split_linear_f16x3_frag_f32", xp, _p(planes), _p(bias), 0, _p(out), M, N, K, act)
    else:
        _launch("rba_split_linear_f16x3_f32" if f16 else "rba_split_linear_f32", xp, _p(planes), _p(bias), _p(out), M, N, K, act)
    return out


@_hip_op
def split_linear_nchw_out(x, planes, bias, rows_per_image, out_features=None):
    """x [B*P, K] (NHWC rows) -> [B, N, P]: the Linear of split_linear written channel-major (NHWC in, NCHW out); the planes' dtype says
    for which arithmetic form they were packed (float16: f16x3, bfloat16: bf16x6)."""
    _chk(x, "x", dim=2)
    M, K = x.shape
    N, f16 = _packed(planes, K, out_features)
    if rows_per_image < 1 or M % rows_per_image:
        raise RbaHipError("split_linear_nchw_out needs x [B*P, K] with M % rows_per_image == 0")
    _vec(bias, "bias", N, optional=True)
    out = torch.empty((M // rows_per_image, N, rows_per_image), dtype=torch.float32, device=x.device)
    _launch("rba_split_linear_nchw_out_f16x3_f32" if f16 else "rba_split_linear_nchw_out_f32", _p(x), _p(planes), _p(bias), _p(out), M, N, K, rows_per_image)
    return out


GN_MOMENTS = os.environ.get("RBA_GN_MOMENTS", "1") != "0"      # A/B switch (tools): 0 keeps the separate statistics passes of the FPN's GroupNorms


def _gn_moments_ok(rows_per_image, N, num_groups):
    return (GN_MOMENTS and _split_mode() == "f16x3" and rows_per_image % 128 == 0 and N % 128 == 0 and N % num_groups == 0
            and (N // num_groups) in (4, 8, 16, 32))


def linear_emits_gn_moments(M, N, K, rows_per_image, num_groups):
    """True when linear_gn_stats runs as ONE GEMM whose epilogue leaves the GroupNorm moments of its output (the LDS-staged f16x3 kernel: K <= 256, 128-column tiles)."""
    return _gn_moments_ok(rows_per_image, N, num_groups) and K <= 256 and K % 32 == 0 and _tiles128(M, N) >= 160 and M % rows_per_image == 0


def conv3x3_emits_gn_moments(B, H, W, N, num_groups):
    """True when conv3x3_nhwc_gn_stats runs the split-image convolution with the moment epilogue."""
    return _gn_moments_ok(H * W, N, num_groups) and conv3x3_takes_split(B * H * W, N)


def _merge_gn_moments(moments, B, G, splits, eps):
    mr = torch.empty((B, G, 2), dtype=torch.float32, device=moments.device)
    _launch("rba_group_norm_nhwc_merge_f32", _p(moments), _p(mr), B, G, splits, float(eps))
    return mr


@_hip_op
def linear_gn_stats(x, lin, num_groups, eps, rows_per_image, use_bias=True):
    """(y, mr): y = F.linear(x, lin.weight[, lin.bias]) on tokens x [B, P, K] and mr [B, G, 2] = group_norm_nhwc_stats(y) -- the statistics come out of the
    GEMM's epilogue (per-tile moments, merged in double) instead of a second pass over y.  y is bit-identical to linear(x, lin); mr equals the stats pass up
    to the summation order.  Check linear_emits_gn_moments first."""
    _chk(x, "x")
    w = lin.weight
    N, K = w.shape
    M = x.numel() // K
    if not linear_emits_gn_moments(M, N, K, rows_per_image, num_groups) or x.shape[-1] != K:
        raise RbaHipError("linear_gn_stats: check linear_emits_gn_moments(M, N, K, rows_per_image, G) first")
    bias = _vec(lin.bias if use_bias else None, "bias", N, optional=True)
    planes = _cached_planes(lin, w)
    B, splits = M // rows_per_image, rows_per_image // 128
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    mom = torch.empty((B, num_groups, splits, 3), dtype=torch.float32, device=x.device)
    _launch("rba_split_linear_f16x3_gn_moments_f32", _p(x), _p(planes), _p(bias), _p(out), M, N, K, rows_per_image, int(num_groups), _p(mom))
    return out, _merge_gn_moments(mom, B, int(num_groups), splits, eps)


@_hip_op
def conv3x3_nhwc_gn_stats(x, planes, num_groups, eps, bias=None, out_features=None):
    """(y, mr): conv3x3_nhwc(x) of SplitActivations x [B,H,W,C] and the GroupNorm statistics of y [B, G, 2] from the convolution's own epilogue.
    Check conv3x3_emits_gn_moments first."""
    if not isinstance(x, SplitActivations):
        raise RbaHipError("conv3x3_nhwc_gn_stats needs SplitActivations of logical shape [B,H,W,C]")
    xp, _ = _split_x(x, "conv3x3_nhwc_gn_stats", dim=4)
    B, H, W, C = x.shape
    N, _ = _packed(planes, 9 * C, out_features, bf16x6=False)
    if C % 32 or not conv3x3_emits_gn_moments(B, H, W, N, num_groups):
        raise RbaHipError("conv3x3_nhwc_gn_stats: check conv3x3_emits_gn_moments(B, H, W, N, G) first")
    _vec(bias, "bias", N, optional=True)
    splits = H * W // 128
    out = torch.empty((B, H, W, N), dtype=torch.float32, device=x.device)
    mom = torch.empty((B, num_groups, splits, 3), dtype=torch.float32, device=x.device)
    _launch("rba_conv3x3_nhwc_f16x3_split_in_gn_moments_f32", xp, _p(planes), _p(bias), _p(out), B, H, W, C, N, int(num_groups), _p(mom))
    return out, _merge_gn_moments(mom, B, int(num_groups), splits, eps)


def split_linear_nchw_out_takes_gn(planes, rows_per_image, K, num_groups):
    """True when split_linear_nchw_out_gn applies: f16x3 planes, whole 128-row tiles per image, four-channel chunks inside one group."""
    return planes.dtype == torch.float16 and rows_per_image % 128 == 0 and K % num_groups == 0 and (K // num_groups) % 4 == 0 and K % 32 == 0


@_hip_op
def split_linear_nchw_out_gn(x, mr, weight, bias_gn, num_groups, relu, planes, bias, rows_per_image, out_features=None):
    """split_linear_nchw_out(group_norm_nhwc(x) [+ ReLU]) with the normalisation applied while the rows are loaded (f16x3 planes only): x [B*P, K] is the
    RAW convolution output, mr [B, G, 2] its statistics (group_norm_nhwc_stats), weight / bias_gn the GroupNorm's affine.  Bit-identical to the two-call form."""
    _chk(x, "x", dim=2)
    _chk(mr, "mr", dim=3)
    M, K = x.shape
    N, _ = _packed(planes, K, out_features, bf16x6=False)
    if rows_per_image < 1 or M % rows_per_image or not split_linear_nchw_out_takes_gn(planes, rows_per_image, K, num_groups):
        raise RbaHipError("split_linear_nchw_out_gn needs x [B*P, K], P % 128 == 0 and (K / G) % 4 == 0")
    B = M // rows_per_image
    if tuple(mr.shape) != (B, num_groups, 2):
        raise RbaHipError("mr must be [B, G, 2]")
    _vec(weight, "weight", K)
    _vec(bias_gn, "bias_gn", K)
    _vec(bias, "bias", N, optional=True)
    out = torch.empty((B, N, rows_per_image), dtype=torch.float32, device=x.device)
    _launch("rba_split_linear_nchw_out_gn_f16x3_f32", _p(x), _p(mr), _p(weight), _p(bias_gn), int(num_groups), int(bool(relu)), _p(planes), _p(bias), _p(out),
            M, N, K, rows_per_image)
    return out


COMPOSED_MASK_HEAD = os.environ.get("RBA_COMPOSED_MASK_HEAD", "1") != "0"    # A/B switch (tools): 0 = the masked decoder always materialises the mask-feature map


class RowIndex:
    """A validated row index of split_linear_nchw_out_gn_rows: ``data`` int32 [B, R] with every value inside [0, rows_per_image).  Built by ``row_index`` (which
    reads the values back once: build it where plans are cached, never inside a graph capture); the launch wrapper takes nothing else, so it never has to look."""
    __slots__ = ("data", "rows_per_image")

    def __init__(self, data, rows_per_image):
        self.data, self.rows_per_image = data, rows_per_image


def row_index(idx, rows_per_image):
    """idx: integer tensor [B, R] of row numbers inside an image of `rows_per_image` rows -> RowIndex (int32, contiguous).  Refuses any other dtype or shape and
    any value outside [0, rows_per_image)."""
    if not isinstance(idx, torch.Tensor) or not idx.is_cuda or idx.dtype not in (torch.int32, torch.int64) or idx.dim() != 2 or idx.numel() == 0:
        raise RbaHipError("row_index needs a HIP int32 / int64 tensor [B, R]")
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= rows_per_image:
        raise RbaHipError(f"row_index: values must lie in [0, {rows_per_image}), got [{lo}, {hi}]")
    return RowIndex(idx.to(torch.int32).contiguous(), int(rows_per_image))


def _image_planes(planes, K, out_features, B):
    """f16x3 planes shared by every image ([nt, K/16, 2, 128, 2, 8], `_packed`'s contract) or one image each ([B, nt, K/16, 2, 128, 2, 8]) -> (N, byte stride)."""
    if planes.dim() != 7:
        return _packed(planes, K, out_features, bf16x6=False)[0], 0
    _chk(planes, "planes", dtype=torch.float16, dim=7)
    if planes.shape[0] != B:
        raise RbaHipError(f"per-image planes must be [B = {B}, ...], got {tuple(planes.shape)}")
    return _packed(planes[0], K, out_features, bf16x6=False)[0], planes.stride(0) * 2


@_hip_op
def split_linear_nchw_out_gn_rows(x, mr, weight, bias_gn, num_groups, relu, planes, bias, rows_per_image, out_features=None, rows=None):
    """split_linear_nchw_out_gn on selected rows and / or with per-image operands (the mask heads on the deferred mask-feature operand, docs/kernels/K4.md):
    rows = RowIndex [B, R] -> out [B, N, R], bit-identical to split_linear_nchw_out_gn(...)[:, :, rows] (None: every row, R = P); planes [B, nt, ...] and bias [B, N]
    give image b its own weight image and bias (compose_query_operand).  P % 128 == 0 and R % 128 == 0."""
    _chk(x, "x", dim=2)
    _chk(mr, "mr", dim=3)
    M, K = x.shape
    P = int(rows_per_image)
    if P < 1 or M % P or planes.dtype != torch.float16 or not split_linear_nchw_out_takes_gn(planes, P, K, num_groups) or P * K >= 1 << 30:
        raise RbaHipError("split_linear_nchw_out_gn_rows needs x [B*P, K], float16 planes, P % 128 == 0, (K / G) % 4 == 0 and P * K < 2^30")
    B = M // P
    N, wstride = _image_planes(planes, K, out_features, B)
    if tuple(mr.shape) != (B, num_groups, 2):
        raise RbaHipError("mr must be [B, G, 2]")
    _vec(weight, "weight", K)
    _vec(bias_gn, "bias_gn", K)
    bstride = 0
    if bias is not None and bias.dim() == 2:
        _shaped(bias, "bias", (B, N))
        bstride = N
    else:
        _vec(bias, "bias", N, optional=True)
    R = P
    if rows is not None:
        if not isinstance(rows, RowIndex) or rows.rows_per_image != P or rows.data.shape[0] != B or rows.data.shape[1] % 128 or rows.data.device != x.device:
            raise RbaHipError("rows must be ops.row_index(idx [B, R], rows_per_image) for this x, with R % 128 == 0")
        R = rows.data.shape[1]
    out = torch.empty((B, N, R), dtype=torch.float32, device=x.device)
    _launch("rba_split_linear_nchw_out_gn_rows_f16x3_f32", _p(x), _p(mr), _p(weight), _p(bias_gn), int(num_groups), int(bool(relu)), _p(planes), wstride, _p(bias),
            bstride, _p(None if rows is None else rows.data), _p(out), B, P, R, N, K)
    return out


@_hip_op
def compose_query_operand(embed, weight, bias):
    """embed [B, Q, C] (the mask embeddings), weight [C, K] and bias [C] | None of the mask-feature 1 x 1 convolution -> (planes [B, 1, K/16, 2, 128, 2, 8] float16:
    split_weight(embed[b] @ weight) per image, bias_q [B, Q] = embed[b] @ bias) in one launch; fp32 FMAs in a fixed order.  Q <= 128, C <= 256, C % 4 == 0, K % 32 == 0."""
    _chk(embed, "embed", dim=3)
    _chk(weight, "weight", dim=2)
    B, Q, C = embed.shape
    K = weight.shape[1]
    if weight.shape[0] != C or not (1 <= Q <= 128 and 4 <= C <= 256 and C % 4 == 0 and K >= 32 and K % 32 == 0):
        raise RbaHipError("compose_query_operand needs embed [B, Q <= 128, C <= 256] (C % 4 == 0) and weight [C, K] with K % 32 == 0")
    _vec(bias, "bias", C, optional=True)
    planes = torch.empty((B, 1, K // 16, 2, 128, 2, 8), dtype=torch.float16, device=embed.device)
    bias_q = torch.empty((B, Q), dtype=torch.float32, device=embed.device)
    _launch("rba_compose_query_operand_f16x2", _p(embed), _p(weight), _p(bias), _p(planes), _p(bias_q), B, Q, C, K)
    return planes, bias_q


def composed_mask_head_pays(rows_per_image, sparse_rows):
    """The shape half of the masked decoder's selection rule (docs/kernels/K4.md): projecting the attention masks' gathered rows (`sparse_rows`: summed over the
    levels the layers use) instead of the whole map pays while they are at most half the map's rows."""
    return 2 * sparse_rows <= rows_per_image


@_hip_op
def conv3x3_weight(weight, mode=None):
    """conv weight [N, C, 3, 3] -> split_weight (form `mode`, default ops.SPLIT_MODE) of the implicit-GEMM matrix [N, 9 C],
    k = (3 ky + kx) C + c."""
    _chk(weight, "weight", dim=4)
    N, C, kh, kw = weight.shape
    if (kh, kw) != (3, 3) or C % 32:
        raise RbaHipError("conv3x3_weight needs a [N, C, 3, 3] weight with C % 32 == 0")
    return split_weight(weight.permute(0, 2, 3, 1).reshape(N, 9 * C).contiguous(), mode=mode)


def conv3x3_takes_split(M, N):
    """True when conv3x3_nhwc can read its input as SplitActivations (the pipelined f16x3 kernel: at least 256 tiles of 128 x 128)."""
    return SPLIT_ACTIVATIONS and _split_mode() == "f16x3" and _tiles128(M, N) >= 256


@_hip_op
def conv3x3_nhwc(x, planes, bias=None, out_features=None):
    """3x3, stride 1, pad 1 convolution of NHWC x [B,H,W,C] with conv3x3_weight(W) -> [B,H,W,N] (implicit GEMM on K6; the planes'
    dtype says for which form they were packed)."""
    xp, pre = _split_x(x, "conv3x3_nhwc", dim=4)
    B, H, W, C = x.shape
    N, f16 = _packed(planes, 9 * C, out_features)
    if C % 32:
        raise RbaHipError("conv3x3_nhwc needs x [B,H,W,C] with C % 32 == 0")
    _vec(bias, "bias", N, optional=True)
    if pre and not (f16 and conv3x3_takes_split(B * H * W, N)):
        raise RbaHipError("conv3x3_nhwc: SplitActivations need f16x3 planes and conv3x3_takes_split(B*H*W, N)")
    out = torch.empty((B, H, W, N), dtype=torch.float32, device=x.device)
    _launch("rba_conv3x3_nhwc_f16x3_split_in_f32" if pre else "rba_conv3x3_nhwc_f16x3_f32" if f16 else "rba_conv3x3_nhwc_f32",
            xp, _p(planes), _p(bias), _p(out), B, H, W, C, N)
    return out


_CONCURRENT_STREAMS = {}        # library handle -> last value set (the hint is per loaded library)


def set_concurrent_streams(n):
    """Tell the kernel library how many HIP streams of this process run forwards at the same time (default 1): with two or more, the K6 launches
    that would fill only half the chip use whole-CU workgroups and leave the other CUs to the other streams (include/rba_hip.h).  Speed only --
    results are bit-identical.  Returns the previous setting.  Call it before the streams start launching (and before capturing hipGraphs: a
    graph replays the launch forms it was captured with; MaskFormer keys its graphs on concurrent_streams()).  Restore it in a `finally`."""
    n = max(1, int(n))
    prev = int(_query("rba_set_concurrent_streams", n))
    _CONCURRENT_STREAMS[id(_lib.load())] = n
    return prev


def concurrent_streams():
    """The hint last given to set_concurrent_streams for the current library (1 if never set)."""
    return _CONCURRENT_STREAMS.get(id(_lib.load()), 1)


# ---------------------------------------------------------------------------------------------------------------- small token Linears
# A/B switch (tools): 0 sends the small Linears back to linear() -- the K6 split kernel -- and to separate add / LayerNorm launches
TOKEN_LINEAR = os.environ.get("RBA_TOKEN_LINEAR", "1") != "0"


def token_linear_ok(N, K):
    """Shapes the row-complete token Linear serves (csrc/token_linear.hip): N <= 256 outputs, K a multiple of 32; f16x3 arithmetic only
    (under ops.split_mode("bf16x6"), the full-range fallback, these Linears run the bf16x6 K6 kernel instead -- no library GEMM on any path since round 5)."""
    return TOKEN_LINEAR and _split_mode() == "f16x3" and 1 <= N <= 256 and K >= 32 and K % 32 == 0


TOKEN_MAX_ROWS = 8192      # beyond that a 128 x 128-tiled GEMM re-reads the weight far less often than one workgroup per 16 rows does


def token_linear_pays(M, N, K):
    """True when the row-complete kernel is the launch to use for an [M, K] x [N, K]^T Linear: the encoder / decoder-memory token counts of one
    image (2 048 at C2, 4 830 at C5) -- its callers then also fold `+ pos`, sibling Linears and the post-norm residual step into the launch."""
    return token_linear_ok(N, K) and N % 4 == 0 and 1 <= M <= TOKEN_MAX_ROWS


def _token_planes(lin):
    """fragment-ordered f16 (h, l) image of lin.weight, packed once per weight load and cached on the module"""
    w = lin.weight

    def build():
        w2 = w.detach().contiguous()
        _chk(w2, "weight", dim=2)
        N, K = w2.shape
        packed = torch.empty((((N + 15) // 16) * (K // 32) * 128, 4), dtype=torch.int32, device=w.device)
        _launch("rba_token_linear_pack_f16x2", _p(w2), _p(packed), N, K)
        return packed

    return derived(lin, "token_planes", (w,), build)


@_hip_op
def token_linear(x, lin, x_add=None, use_bias=True, relu=False, residual=None, norm=None):
    """``F.linear(x + x_add, lin.weight, lin.bias)`` [+ ReLU] on a token tensor [..., K] with N <= 256 outputs, as one launch of the
    row-complete kernel; with ``residual`` and ``norm`` (an nn.LayerNorm over N): ``norm(residual + F.linear(x, W, b))`` -- the post-norm
    residual step of an encoder layer (msdeformattn.py:134-138) in the GEMM's epilogue.  Check token_linear_ok(N, K) first."""
    _chk(x, "x")
    N, K = lin.weight.shape
    if x.shape[-1] != K or not token_linear_ok(N, K):
        raise RbaHipError("token_linear: x [..., K] with K % 32 == 0, N <= 256 and the f16x3 mode (see token_linear_ok)")
    M = x.numel() // K
    _shaped(x_add, "x_add", x.shape, optional=True)
    bias = _vec(lin.bias if use_bias else None, "bias", N, optional=True)
    if (residual is None) != (norm is None):
        raise RbaHipError("token_linear: residual and norm come together")
    ln_w, ln_b, ln_eps, act = 0, 0, 0.0, 2 if relu else 0
    if norm is not None:
        _chk(residual, "residual")
        if tuple(residual.shape) != tuple(x.shape[:-1]) + (N,) or N % 16 or relu or norm.weight.numel() != N:
            raise RbaHipError("token_linear(norm=...): residual [..., N], N % 16 == 0, no activation")
        ln_w, ln_b, ln_eps = _p(norm.weight), _p(norm.bias), float(norm.eps)
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=torch.float32, device=x.device)
    _launch("rba_token_linear_f32", _p(x), _p(x_add), _p(_token_planes(lin)), _p(bias), _p(residual), ln_w, ln_b, ln_eps, _p(out), M, N, K, act)
    return out


@_hip_op
def token_linear_multi(x, specs):
    """Up to three Linears over the same rows in ONE launch.  specs: [(lin, x_add | None, out | None, col0, relu), ...]; problem i computes
    F.linear(x + x_add_i, W_i, b_i) [ReLU] and writes it into out_i[..., col0 : col0 + N_i] (out_i = a fresh [..., N_i] tensor when None; several
    problems may fill column slices of one wider tensor).  Returns the list of output tensors.  Check token_linear_ok(N_i, K) first."""
    _chk(x, "x")
    K = x.shape[-1]
    M = x.numel() // K if K else 0
    lead = tuple(x.shape[:-1])
    if not 1 <= len(specs) <= 3:
        raise RbaHipError("token_linear_multi: one to three problems")
    arr = (_lib.TokenLinearProblem * len(specs))()
    outs, keep = [], []
    for i, (lin, x_add, out, col0, relu) in enumerate(specs):
        N, K_ = lin.weight.shape
        if K_ != K or not token_linear_ok(N, K) or N % 4:
            raise RbaHipError("token_linear_multi: weights [N <= 256, N % 4 == 0, K] with x's K % 32 == 0 (see token_linear_ok)")
        _shaped(x_add, "x_add", x.shape, optional=True)
        _vec(lin.bias, "bias", N, optional=True)
        if out is None:
            out, col0 = torch.empty(lead + (N,), dtype=torch.float32, device=x.device), 0
        else:
            _chk(out, "out")
            if tuple(out.shape[:-1]) != lead or col0 % 4 or col0 + N > out.shape[-1] or out.shape[-1] % 4:
                raise RbaHipError("token_linear_multi: out [..., ld] with ld % 4 == 0 and a column slice col0 % 4 == 0 inside it")
        planes = _token_planes(lin)
        keep.append(planes)
        arr[i] = _lib.TokenLinearProblem(_p(x_add) or None, _p(planes), _p(lin.bias) or None, out.data_ptr() + 4 * col0, N, out.shape[-1], 2 if relu else 0)
        outs.append(out)
    _launch("rba_token_linear_multi_f32", _p(x), ctypes.byref(arr), len(specs), M, K)
    return outs


@_hip_op
def patch_im2col(image, mean, std, Hp, Wp):
    """image [3,h,w] (uint8 or fp32) -> [(Hp/4)*(Wp/4), 64] fp32: (image - mean) / std, zero padding to Hp x Wp (ImageList semantics:
    the padding is zero AFTER normalisation) and the im2col of the 4x4 / stride-4 patch convolution in one pass; column
    c*16 + ky*4 + kx, columns 48..63 zero.  `mean`, `std`: three python floats each."""
    if image.dtype not in (torch.uint8, torch.float32):
        raise RbaHipError("image must be uint8 or float32")
    _chk(image, "image", dtype=image.dtype, dim=3)
    if image.shape[0] != 3 or Hp % 4 or Wp % 4 or Hp < image.shape[1] or Wp < image.shape[2] or len(mean) != 3 or len(std) != 3:
        raise RbaHipError("patch_im2col needs a [3,h,w] image and Hp >= h, Wp >= w multiples of 4")
    h, w = int(image.shape[1]), int(image.shape[2])
    out = torch.empty(((Hp // 4) * (Wp // 4), 64), dtype=torch.float32, device=image.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in std])
    _launch("rba_patch_im2col_u8" if image.dtype == torch.uint8 else "rba_patch_im2col_f32", _p(image), _p(out), h, w, int(Hp), int(Wp),
            ctypes.addressof(m), ctypes.addressof(sd))
    return out


def _nhwc_rows(x):
    """channels-last x [B, P, C] or [B, H, W, C] -> (B, P, C)"""
    _chk(x, "x")
    if x.dim() not in (3, 4):
        raise RbaHipError("x must be [B,P,C] or [B,H,W,C]")
    B, C = x.shape[0], x.shape[-1]
    return B, (x.numel() // (B * C) if B * C else 0), C


@_hip_op
def group_norm_nhwc(x, num_groups, weight, bias, eps=1e-5, relu=False):
    """GroupNorm (+ReLU) of channels-last x [B, P, C] (or [B, H, W, C]): the same operator as group_norm on the token layout."""
    B, P, C = _nhwc_rows(x)
    _vec(weight, "weight", C)
    _vec(bias, "bias", C)
    if not _gn_nhwc_ok(C, num_groups):
        raise RbaHipError("group_norm_nhwc needs C % G == 0, (C/G) % 4 == 0, C <= 1024 and 256 % (C/4) == 0")
    ws = _scratch(_query("rba_group_norm_nhwc_workspace_bytes", B, P, C, num_groups), x.device)
    y = torch.empty_like(x)
    _launch("rba_group_norm_nhwc_f32", _p(x), _p(weight), _p(bias), _p(y), _p(ws), B, P, C, num_groups, float(eps), int(bool(relu)))
    return y


@_hip_op
def resample_bilinear_nhwc(x, size, add=None, split_into=None, image=0):
    """F.interpolate(mode="bilinear", align_corners=False) of channels-last x [h, w, C] -> [H, W, C], optional fused `+ add`.
    ``split_into``: a SplitActivations of logical shape [B, H, W, C] (SplitActivations.empty): the result becomes image `image` of it
    (the 3x3 convolution's split operand, conv3x3_takes_split) and nothing else is written; returns split_into."""
    _chk(x, "x", dim=3)
    h, w, C = x.shape
    H, W = int(size[0]), int(size[1])
    if C % 4:
        raise RbaHipError("resample_bilinear_nhwc needs C % 4 == 0")
    _shaped(add, "add", (H, W, C), optional=True)
    if split_into is not None:
        _split_into_ok(split_into, image, H, W, C)
        _launch("rba_resample_bilinear_nhwc_split_out_f32", _p(x), _p(add), _p(split_into.data), C, h, w, H, W, image * H * W)
        return split_into
    out = torch.empty((H, W, C), dtype=torch.float32, device=x.device)
    _launch("rba_resample_bilinear_nhwc_f32", _p(x), _p(add), _p(out), C, h, w, H, W)
    return out


@_hip_op
def group_norm_nhwc_stats(x, num_groups, eps=1e-5):
    """(mean, rstd) per image and group of channels-last x [B, P, C] (or [B, H, W, C]) -> [B, G, 2]: the statistics half of group_norm_nhwc, for a
    consumer that folds the normalisation into its own loads (resample_bilinear_nhwc_gn)."""
    B, P, C = _nhwc_rows(x)
    if not _gn_nhwc_ok(C, num_groups):
        raise RbaHipError("group_norm_nhwc_stats needs C % G == 0, (C/G) % 4 == 0, C <= 1024 and 256 % (C/4) == 0")
    ws = _scratch(_query("rba_group_norm_nhwc_workspace_bytes", B, P, C, num_groups), x.device)
    mr = torch.empty((B, num_groups, 2), dtype=torch.float32, device=x.device)
    _launch("rba_group_norm_nhwc_stats_f32", _p(x), _p(mr), _p(ws), B, P, C, num_groups, float(eps))
    return mr


@_hip_op
def resample_bilinear_nhwc_gn(x, size, add, num_groups, x_norm=None, add_norm=None, split_into=None, image=0):
    """The FPN top-down step `GroupNorm(add) + F.interpolate(ReLU(GroupNorm(x)))` with the normalisations folded into the loads: x [h, w, C] and
    add [H, W, C] are the RAW convolution outputs; ``x_norm`` = (mr [G, 2], weight, bias, relu) or None (x is used as it is), ``add_norm`` =
    (mr, weight, bias) or None.  The arithmetic of group_norm_nhwc + resample_bilinear_nhwc(add=...) (equal up to fma contraction: one ulp).  ``split_into`` / ``image`` as there."""
    _chk(x, "x", dim=3)
    _chk(add, "add", dim=3)
    h, w, C = x.shape
    H, W = int(size[0]), int(size[1])
    if tuple(add.shape) != (H, W, C) or not _gn_nhwc_ok(C, num_groups):
        raise RbaHipError("resample_bilinear_nhwc_gn: add must be [H, W, C]; C % G == 0, (C/G) % 4 == 0")

    def unpack(n, with_relu):
        if n is None:
            return 0, 0, 0, 0
        mr, wgt, b = n[0], n[1], n[2]
        _chk(mr, "mr")
        if mr.numel() != 2 * num_groups:
            raise RbaHipError("norm = (mr [G, 2], weight [C], bias [C])")
        return _p(mr), _p(_vec(wgt, "weight", C)), _p(_vec(b, "bias", C)), (int(bool(n[3])) if with_relu and len(n) > 3 else 0)
    xm, xg, xb, xr = unpack(x_norm, True)
    am, ag, ab, _ = unpack(add_norm, False)
    into = split_into is not None
    if into:
        _split_into_ok(split_into, image, H, W, C)
    out = split_into if into else torch.empty((H, W, C), dtype=torch.float32, device=x.device)
    _launch("rba_resample_bilinear_nhwc_gn_f32", _p(x), xm, xg, xb, xr, _p(add), am, ag, ab, _p(out.data) if into else _p(out), int(into), C, num_groups,
            h, w, H, W, image * H * W if into else 0)
    return out


@_hip_op
def bn_relu_conv1x1(x, scale, shift, weight, bias=None):
    """conv1x1(relu(x * scale[c] + shift[c])) for x [B,C,...] -> [B,O,...] (O = weight.shape[0] in {1,2,4}): the DenseHybrid
    `ood_pred` head BNReluConv(hidden_dim, 2, k=1) in eval mode (mask2former_transformer_decoder.py:216-230, 467-468)."""
    _chk(x, "x")
    if x.dim() < 3:
        raise RbaHipError("x must be [B,C,...]")
    B, C = x.shape[:2]
    _chk(weight, "weight", dim=2)
    O = weight.shape[0]
    P = x.numel() // (B * C) if B * C else 0
    if weight.shape[1] != C or O not in (1, 2, 4):
        raise RbaHipError("bn_relu_conv1x1 needs weight [O,C] with O in {1,2,4}")
    _vec(scale, "scale", C)
    _vec(shift, "shift", C)
    _vec(bias, "bias", O, optional=True)
    out = torch.empty((B, O) + tuple(x.shape[2:]), dtype=torch.float32, device=x.device)
    _launch("rba_bn_relu_conv1x1_f32", _p(x), _p(scale), _p(shift), _p(weight), _p(bias), _p(out), B, C, O, P)
    return out


@_hip_op
def resample_bilinear_ac(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=True) for x [C,h,w] or [B,C,h,w] (maskformer_model.py:305)."""
    _chk(x, "x")
    if x.dim() not in (3, 4):
        raise RbaHipError("x must be [C,h,w] or [B,C,h,w]")
    H, W = int(size[0]), int(size[1])
    lead = tuple(x.shape[:-2])
    h, w = x.shape[-2:]
    out = torch.empty(lead + (H, W), dtype=torch.float32, device=x.device)
    _launch("rba_resample_bilinear_ac_f32", _p(x), _p(out), math.prod(lead), h, w, H, W)
    return out


@_hip_op
def gaussian_blur(score, kernel_size=7, sigma=1.0):
    """transforms.GaussianBlur(kernel_size, sigma) of a score map [H,W] (reflect padding): the evaluator's optional smoothing."""
    _chk(score, "score", dim=2)
    H, W = score.shape
    if kernel_size % 2 == 0 or not (1 <= kernel_size <= 15) or sigma <= 0 or (H and W and (H <= kernel_size // 2 or W <= kernel_size // 2)):
        raise RbaHipError("gaussian_blur needs an odd kernel_size <= 15, sigma > 0 and a map larger than the padding")
    out = torch.empty_like(score)
    _launch("rba_gaussian_blur_f32", _p(score), _p(out), H, W, int(kernel_size), float(sigma))
    return out


@_hip_op
def quad_mean(v):
    """v [..., 4, S] -> ((v0 + v1) + (v2 + v3)) * 0.25 [..., S]: the bilinear sample at the centre of each 2 x 2 cell (rba_quad_mean_f32)"""
    _chk(v, "v")
    if v.dim() < 2 or v.shape[-2] != 4:
        raise RbaHipError(f"quad_mean expects [..., 4, S], got {tuple(v.shape)}")
    S = v.shape[-1]
    out = torch.empty(v.shape[:-2] + (S,), dtype=torch.float32, device=v.device)
    _launch("rba_quad_mean_f32", _p(v), _p(out), v.numel() // (4 * S) if S else 0, S)
    return out


@_hip_op
def softmax_drop_last(logits):
    """F.softmax(logits, -1)[..., :-1] as one launch (rba_softmax_drop_last_f32): [..., K + 1] -> [..., K] contiguous, K + 1 <= 64"""
    _chk(logits, "logits")
    K1 = logits.shape[-1]
    if not 2 <= K1 <= 64:
        raise RbaHipError(f"softmax_drop_last supports 2..64 classes, got {K1}")
    out = torch.empty(logits.shape[:-1] + (K1 - 1,), dtype=torch.float32, device=logits.device)
    _launch("rba_softmax_drop_last_f32", _p(logits), _p(out), logits.numel() // K1, K1)
    return out


@_hip_op
def ood_components(score, threshold, min_dummy=None):
    """Open-set panoptic epilogue of a score map [H,W] (maskformer_model.py:454-474): binary = score > threshold, 3x3 opening
    then closing, 4-connected components.  Returns (labels int32 [H,W] with 0 = background and components numbered 1..n in
    raster order of their first pixel, n) like cv2.connectedComponents(connectivity=4) minus the background count."""
    _chk(score, "score", dim=2)
    H, W = score.shape
    a = torch.empty((H, W), dtype=torch.uint8, device=score.device)
    b = torch.empty_like(a)
    st = _stream()                                                                          # read once for the six launches
    _launch("rba_threshold_u8", _p(score), _p(a), H * W, float(threshold), stream=st)
    for dilate, (src, dst) in ((0, (a, b)), (1, (b, a)), (1, (a, b)), (0, (b, a))):          # open, then close
        _launch("rba_morph3x3_u8", _p(src), _p(dst), H, W, dilate, stream=st)
    roots = torch.empty((H, W), dtype=torch.int32, device=score.device)
    _launch("rba_ccl4_roots_i32", _p(a), _p(roots), H, W, stream=st)
    flat = roots.view(-1)
    is_root = flat == torch.arange(H * W, dtype=torch.int32, device=score.device)
    rank = torch.cumsum(is_root.to(torch.int32), 0, dtype=torch.int32)                    # raster-order number of every root
    labels = torch.where(flat >= 0, rank[flat.clamp_min(0).long()], torch.zeros_like(flat))
    n = int(rank[-1].item()) if H * W else 0
    return labels.view(H, W), n
