"""Python entry points of K19 (csrc/mit_attn.hip, csrc/mit_conv.hip, docs/kernels/K19.md): the three pieces of the MiT (SegFormer) backbone
(mask2former/modeling/backbone/mix_transformer.py) that are neither a Linear nor a LayerNorm -- the spatial-reduction attention core, the depthwise
3x3 convolution + GELU of the MLP, and the gather of the strided / overlapping convolutions -- plus the two weight repacks they need.

Written in rba_amd.ops' style with its decorator, validators and launch line (as rba_amd.instance_ops): a wrapper reads top to bottom as its checks, its
output allocation, one `_launch` line; a bad argument raises RbaHipError before anything is allocated or enqueued; there is no fallback path."""
import torch

from ._lib import RbaHipError
from .ops import _chk, _hip_op, _launch, _p, _vec

HEAD_DIMS = (32, 64)          # K19a's two instantiations
COLUMN_MULTIPLE = 32          # cols' row length: k * k * C rounded up to what ops.linear takes without padding (147 -> 160 for the stem)


# ---------------------------------------------------------------------------------------------------------------- argument contracts, each written once
def _heads(C, num_heads, who):
    """C = num_heads * head_dim with head_dim in {32, 64} -> head_dim"""
    num_heads = int(num_heads)
    if num_heads < 1 or C % num_heads or C // num_heads not in HEAD_DIMS:
        raise RbaHipError(f"{who} needs head_dim in {HEAD_DIMS}, got {C} channels over {num_heads} heads")
    return C // num_heads


def _channels4(C, who):
    """a lane owns four channels: C % 4 == 0"""
    if C < 4 or C % 4:
        raise RbaHipError(f"{who} needs C % 4 == 0 channels, got C = {C}")
    return C


def _map(H, W, rows, who):
    """an H x W token map of `rows` tokens per image"""
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W != rows or H * W >= 1 << 31:
        raise RbaHipError(f"{who} needs tokens of an H x W map with 1 <= H * W < 2^31, got H = {H}, W = {W} for {rows} tokens per image")
    return H, W


def padded_columns(k, C):
    """Kp of `im2col_nhwc` and `conv_linear_weight`: k * k * C rounded up to a multiple of 32"""
    return (k * k * C + COLUMN_MULTIPLE - 1) // COLUMN_MULTIPLE * COLUMN_MULTIPLE


def conv_out_size(n, k, stride, pad):
    """floor((n + 2 pad - k) / stride) + 1 windows along an axis of n, 0 where none fits"""
    return 0 if n + 2 * pad < k else (n + 2 * pad - k) // stride + 1


def _window(k, stride, pad):
    k, stride, pad = int(k), int(stride), int(pad)
    if not (1 <= k <= 64 and stride >= 1 and 0 <= pad < k):
        raise RbaHipError(f"im2col_nhwc needs 1 <= k <= 64, stride >= 1 and 0 <= pad < k, got k = {k}, stride = {stride}, pad = {pad}")
    return k, stride, pad


# ---------------------------------------------------------------------------------------------------------------- weight repacks (once per weight load)
def dwconv_taps(weight):
    """[C,1,3,3] depthwise weight -> w9 [9,C] tap-major (w9[3 ky + kx][c]), K19b's weight operand"""
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (1, 3, 3):
        raise RbaHipError(f"dwconv_taps takes a depthwise [C,1,3,3] weight, got {tuple(weight.shape)}")
    return weight.detach().reshape(weight.shape[0], 9).t().contiguous()


def conv_linear_weight(weight):
    """[Co,Ci,k,k] convolution weight -> [Co,Kp] in K19c's column order (ky, kx, c), zero in columns k * k * Ci .. Kp - 1: the convolution as a Linear
    over `im2col_nhwc`'s rows"""
    if weight.dim() != 4 or weight.shape[2] != weight.shape[3]:
        raise RbaHipError(f"conv_linear_weight takes a [Co,Ci,k,k] weight, got {tuple(weight.shape)}")
    Co, Ci, k, _ = weight.shape
    out = weight.new_zeros((Co, padded_columns(k, Ci)))
    out[:, : k * k * Ci] = weight.detach().permute(0, 2, 3, 1).reshape(Co, k * k * Ci)
    return out


# ---------------------------------------------------------------------------------------------------------------- launches
@_hip_op
def sr_attention(q, kv, num_heads, scale=None):
    """K19a.  q [B,N,C] (the q Linear's output, unscaled), kv [B,S,2C] (the kv Linear's output as it lies: k | v, head-major) ->
    out [B,N,C] = softmax(q k^T * scale) v per head, head-major (mix_transformer.py:113-117).  scale defaults to head_dim^-0.5.  head_dim = C /
    num_heads in {32, 64}; N >= 1, S >= 1.  Exact fp32 products, online softmax: no [B*nH,N,S] tensor exists; the same kernel in both ops.SPLIT_MODEs."""
    _chk(q, "q", dim=3)
    _chk(kv, "kv", dim=3)
    B, N, C = q.shape
    hd = _heads(C, num_heads, "sr_attention")
    S = kv.shape[1]
    if kv.shape[0] != B or kv.shape[2] != 2 * C:
        raise RbaHipError(f"kv must be [B,S,2C] = [{B},S,{2 * C}] for q {tuple(q.shape)}, got {tuple(kv.shape)}")
    if N < 1 or S < 1 or S > 1 << 30 or B > 65535:
        raise RbaHipError(f"sr_attention needs N >= 1, 1 <= S <= 2^30 and B <= 65535, got B = {B}, N = {N}, S = {S}")
    out = torch.empty((B, N, C), dtype=torch.float32, device=q.device)
    _launch("rba_sr_attn_f32", _p(q), _p(kv), _p(out), B, N, S, int(num_heads), hd, float(hd ** -0.5 if scale is None else scale))
    return out


@_hip_op
def dwconv3x3_gelu(x, w9, bias, H, W):
    """K19b.  x [B,H*W,C] channels-last tokens, w9 [9,C] (`dwconv_taps`), bias [C] -> GELU(depthwise3x3(x) + bias) [B,H*W,C]: erf GELU, stride 1, zero
    padding 1, every image on its own (Mlp.forward, mix_transformer.py:53-55).  C % 4 == 0."""
    _chk(x, "x", dim=3)
    B, rows, C = x.shape
    _channels4(C, "dwconv3x3_gelu")
    H, W = _map(H, W, rows, "dwconv3x3_gelu")
    _chk(w9, "w9", dim=2)
    if tuple(w9.shape) != (9, C):
        raise RbaHipError(f"w9 must be dwconv_taps(weight) [9,{C}], got {tuple(w9.shape)}")
    _vec(bias, "bias", C)
    y = torch.empty((B, rows, C), dtype=torch.float32, device=x.device)
    _launch("rba_dwconv3x3_gelu_nhwc_f32", _p(x), _p(w9), _p(bias), _p(y), B, H, W, C)
    return y


@_hip_op
def im2col_nhwc(x, H, W, k, stride, pad, nchw_in=False):
    """K19c.  x [B,H*W,C] channels-last tokens (or, ``nchw_in``, the image batch [B,C,H,W]) -> (cols [B,Ho*Wo,Kp], Ho, Wo): the windows of a k x k
    convolution of stride `stride` and zero padding `pad` as rows, column order (ky, kx, c), Kp = `padded_columns(k, C)`, zeros outside the image
    and in the padded columns; Ho = `conv_out_size(H, k, stride, pad)`.  `ops.linear(cols, view of conv_linear_weight)` is the convolution."""
    k, stride, pad = _window(k, stride, pad)
    if nchw_in:
        _chk(x, "x", dim=4)
        B, C = x.shape[:2]
        if (int(H), int(W)) != tuple(x.shape[2:]):
            raise RbaHipError(f"im2col_nhwc(nchw_in=True): x is {tuple(x.shape)}, not [B,C,{H},{W}]")
        H, W = _map(H, W, x.shape[2] * x.shape[3], "im2col_nhwc")
    else:
        _chk(x, "x", dim=3)
        B, rows, C = x.shape
        H, W = _map(H, W, rows, "im2col_nhwc")
    if C < 1 or k * k * C > 1 << 24:
        raise RbaHipError(f"im2col_nhwc needs 1 <= k * k * C <= 2^24 columns, got k = {k}, C = {C}")
    Kp, Ho, Wo = padded_columns(k, C), conv_out_size(H, k, stride, pad), conv_out_size(W, k, stride, pad)
    cols = torch.empty((B, Ho * Wo, Kp), dtype=torch.float32, device=x.device)
    _launch("rba_im2col_nhwc_f32", _p(x), _p(cols), B, H, W, C, k, stride, pad, Kp, 1 if nchw_in else 0)
    return cols, Ho, Wo


__all__ = ["sr_attention", "dwconv3x3_gelu", "im2col_nhwc", "dwconv_taps", "conv_linear_weight", "padded_columns", "conv_out_size", "HEAD_DIMS"]
