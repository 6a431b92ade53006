"""Mix Transformer (SegFormer's MiT) backbone, inference only, for MI355X.

Same parameter tree (hence state-dict keys) as the reference's ``MixVisionTransformer`` and its six registered variants ``mit_b0`` .. ``mit_b5``
(mask2former/modeling/backbone/mix_transformer.py:207-493), but a different dataflow: the token map stays [B, H*W, C] channels-last for the whole
network and never visits NCHW.  Every Linear is the repository's split GEMM (``ops.linear``), every LayerNorm ``ops.add_layer_norm`` (which also
makes the residual adds, as in the Swin block); the three convolutions with a stride -- the overlapping patch embeddings and the attention's
spatial reduction -- are one gather (K19c, ``mit_ops.im2col_nhwc``) in front of the same GEMM; the attention core is K19a (``mit_ops.sr_attention``)
and the MLP's depthwise convolution + GELU is K19b (``mit_ops.dwconv3x3_gelu``).  No library GEMM, convolution or attention call is on the path.

Three LayerNorm eps values as the reference constructs them: the block norms and the stage norms are ``partial(nn.LayerNorm, eps=1e-6)`` (:399),
``patch_embed*.norm`` (:179) and ``attn.norm`` (:81) are plain ``nn.LayerNorm`` (1e-5).  Dropout and DropPath are identities at inference.
"""
from types import SimpleNamespace

import torch.nn as nn

from ... import mit_ops, ops
from ..._lib import RbaHipError
from ...arch import MIT_VARIANTS
from ...lru import derived
from ...registry import BACKBONE_REGISTRY

BLOCK_EPS = 1e-6


def _conv_as_linear(owner, conv):
    """`conv` as an nn.Linear over K19c's rows (weight [Co, Kp] view, bias), cached per weight load"""
    w, b = conv.weight, conv.bias               # the view holds the bias OBJECT: a replaced bias is a new key
    return derived(owner, "linear_view", (w, b), lambda: SimpleNamespace(weight=mit_ops.conv_linear_weight(w), bias=b))


class OverlapPatchEmbed(nn.Module):
    """k x k convolution of stride `stride` and padding k // 2, then LayerNorm (:164-204)"""

    def __init__(self, patch_size, stride, in_chans, embed_dim):
        super().__init__()
        self.patch_size, self.stride = patch_size, stride
        self.proj = nn.Conv2d(in_chans, embed_dim, kernel_size=patch_size, stride=stride, padding=patch_size // 2)
        self.norm = nn.LayerNorm(embed_dim)

    def forward(self, x, H, W, nchw_in=False):
        """x: tokens [B, H*W, Cin] (``nchw_in``: the image batch [B,3,H,W]) -> tokens [B, Ho*Wo, C], Ho, Wo"""
        cols, Ho, Wo = mit_ops.im2col_nhwc(x, H, W, self.patch_size, self.stride, self.patch_size // 2, nchw_in=nchw_in)
        x = ops.linear(cols, _conv_as_linear(self, self.proj))
        return ops.add_layer_norm(x, self.norm.weight, self.norm.bias, self.norm.eps)[1], Ho, Wo


class Attention(nn.Module):
    def __init__(self, dim, num_heads, sr_ratio):
        super().__init__()
        self.dim, self.num_heads, self.sr_ratio = dim, num_heads, sr_ratio
        self.scale = (dim // num_heads) ** -0.5
        self.q = nn.Linear(dim, dim)
        self.kv = nn.Linear(dim, dim * 2)
        self.proj = nn.Linear(dim, dim)
        if sr_ratio > 1:
            self.sr = nn.Conv2d(dim, dim, kernel_size=sr_ratio, stride=sr_ratio)
            self.norm = nn.LayerNorm(dim)

    def forward(self, y, H, W):
        """y = norm1(x) [B, H*W, C] -> the heads' outputs [B, H*W, C] in front of `proj` (:100-117)"""
        q = ops.linear(y, self.q)
        if self.sr_ratio > 1:
            cols, _, _ = mit_ops.im2col_nhwc(y, H, W, self.sr_ratio, self.sr_ratio, 0)
            y = ops.linear(cols, _conv_as_linear(self, self.sr))
            y = ops.add_layer_norm(y, self.norm.weight, self.norm.bias, self.norm.eps)[1]
        return mit_ops.sr_attention(q, ops.linear(y, self.kv), self.num_heads, self.scale)


class DWConv(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dwconv = nn.Conv2d(dim, dim, 3, 1, 1, bias=True, groups=dim)

    def taps(self):
        """K19b's tap-major weight, once per weight load"""
        w = self.dwconv.weight
        return derived(self, "taps", (w,), lambda: mit_ops.dwconv_taps(w))


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.dwconv = DWConv(hidden)
        self.fc2 = nn.Linear(hidden, dim)


class Block(nn.Module):
    def __init__(self, dim, num_heads, mlp_ratio, sr_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=BLOCK_EPS)
        self.attn = Attention(dim, num_heads, sr_ratio)
        self.norm2 = nn.LayerNorm(dim, eps=BLOCK_EPS)
        self.mlp = Mlp(dim, int(dim * mlp_ratio))

    def forward(self, x, H, W, pending=None):
        """x [B, H*W, C] residual stream; ``pending`` = (t, bias) not yet added to it (the previous block's fc2 output).  Returns (x, pending) as the
        Swin block does: a projection's output rides into x in the GEMM's epilogue where that form exists (ops.linear_residual_fused), else it is
        added by the next add+LayerNorm (:157-161)."""
        M, C, hidden = x.numel() // x.shape[-1], x.shape[-1], self.mlp.fc2.in_features
        a, m, n1, n2 = self.attn, self.mlp, self.norm1, self.norm2
        t, tb = pending if pending is not None else (None, None)
        x, y = ops.add_layer_norm(x, n1.weight, n1.bias, n1.eps, t, tb, inplace_sum=True)
        y = a(y, H, W)
        if ops.linear_residual_fused(M, C, C):
            x = ops.linear(y, a.proj, residual=x)
            y = ops.add_layer_norm(x, n2.weight, n2.bias, n2.eps)[1]
        else:
            x, y = ops.add_layer_norm(x, n2.weight, n2.bias, n2.eps, ops.linear(y, a.proj, use_bias=False), a.proj.bias, inplace_sum=True)
        y = ops.linear(y, m.fc1)
        y = mit_ops.dwconv3x3_gelu(y, m.dwconv.taps(), m.dwconv.dwconv.bias, H, W)
        if ops.linear_residual_fused(M, C, hidden):
            return ops.linear(y, m.fc2, residual=x), None
        return x, (ops.linear(y, m.fc2, use_bias=False), m.fc2.bias)


class MixVisionTransformer(nn.Module):
    """forward(x [B,3,H,W]) -> {"res2".."res5": [B,C_s,H/4..H/32,W/4..W/32]} -- the reference's "stage1".."stage4" (:334-370) under the names the
    pixel decoder here uses, as channels-last views of the token tensors."""

    def __init__(self, arch):
        super().__init__()
        m = arch["mit"]
        dims, heads, depths, srs = m["embed_dims"], m["num_heads"], m["depths"], m["sr_ratios"]
        if not len(dims) == len(heads) == len(depths) == len(srs) == 4:
            raise RbaHipError(f"a MiT arch has four stages, got {m}")
        for C, nH in zip(dims, heads):
            mit_ops._heads(C, nH, "MixVisionTransformer")
            mit_ops._channels4(int(C * m["mlp_ratio"]), "MixVisionTransformer's depthwise convolution")
        cin = 3
        for s in range(4):
            self.add_module(f"patch_embed{s + 1}", OverlapPatchEmbed(7 if s == 0 else 3, 4 if s == 0 else 2, cin, dims[s]))
            cin = dims[s]
        for s in range(4):
            self.add_module(f"block{s + 1}", nn.ModuleList(Block(dims[s], heads[s], m["mlp_ratio"], srs[s]) for _ in range(depths[s])))
            self.add_module(f"norm{s + 1}", nn.LayerNorm(dims[s], eps=BLOCK_EPS))
        self.num_features = list(dims)

    @property
    def size_divisibility(self):
        return 32

    def forward(self, x):
        if x.dim() != 4:
            raise ValueError(f"MixVisionTransformer takes an input of shape (N, C, H, W). Got {tuple(x.shape)} instead!")
        B, _, H, W = x.shape
        if H % 32 or W % 32:
            # the reference's class defines no size_divisibility; its configs pad to 32.  Off that grid the sr convolutions drop rows of the map
            raise RbaHipError(f"MixVisionTransformer needs a padded size that is a multiple of 32, got {H} x {W} "
                              "(MODEL.MASK_FORMER.SIZE_DIVISIBILITY: 32)")
        outs = {}
        x = x.contiguous()
        for s in range(4):
            x, H, W = getattr(self, f"patch_embed{s + 1}")(x, H, W, nchw_in=s == 0)
            pending = None
            for blk in getattr(self, f"block{s + 1}"):
                x, pending = blk(x, H, W, pending)
            norm = getattr(self, f"norm{s + 1}")
            t, tb = pending if pending is not None else (None, None)
            x = ops.add_layer_norm(x, norm.weight, norm.bias, norm.eps, t, tb, inplace_sum=True)[1]
            # [B,C,h,w] as a channels-last VIEW of the token tensor (no copy): same values and shape as the reference's
            # permute(0,3,1,2).contiguous() (:343); the pixel decoder and the next patch embedding consume the token layout directly
            outs[f"res{s + 2}"] = x.view(B, H, W, self.num_features[s]).permute(0, 3, 1, 2)
        return outs


def _variant(name):
    def __init__(self, arch):
        if arch.get("mit") != MIT_VARIANTS[name]:
            raise RbaHipError(f"{name} is built from arch['mit'] == arch.MIT_VARIANTS[{name!r}], got {arch.get('mit')}")
        MixVisionTransformer.__init__(self, arch)

    cls = type(name, (MixVisionTransformer,), {"__init__": __init__, "__doc__": f"MixVisionTransformer with the sizes of arch.MIT_VARIANTS[{name!r}]",
                                               "__module__": __name__})
    return BACKBONE_REGISTRY.register(cls)


BACKBONE_REGISTRY.register(MixVisionTransformer)
mit_b0, mit_b1, mit_b2, mit_b3, mit_b4, mit_b5 = (_variant(n) for n in MIT_VARIANTS)
