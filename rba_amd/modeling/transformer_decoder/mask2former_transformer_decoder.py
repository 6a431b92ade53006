"""Masked-attention transformer decoder (reference: transformer_decoder/mask2former_transformer_decoder.py:232-502, post-norm,
dropout 0).  Same parameter names.  Inference only unless ``MultiScaleMaskedTransformerDecoder.differentiable_heads`` is set (see the class).

MI355X dataflow: memory is kept batch-first [B, S, C]; the cross/self attention cores are the HIP kernel K3 with
the ``sigmoid(mask) < 0.5`` threshold and the all-masked-row fix fused in (the bool [B*h, Q, S] mask of the
reference is never materialised); mask logits are the HIP kernel K4; the bilinear down-sample that feeds the
attention mask is the HIP resampler.
"""
import contextlib
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import ops
from ...lru import ShapeCache, derived, source_key
from ...registry import TRANSFORMER_DECODER_REGISTRY
from ..pixel_decoder.msdeformattn import DeferredMaskFeatures
from .position_encoding import PositionEmbeddingSine


def _qlinear(x, weight, bias=None, relu=False, x_add=None):
    """Linear layer on the query tensor [B, Q, C]: the skinny exact-fp32 MFMA kernel, over blocks of at most 128 rows (one launch for a single image's
    100 queries; a batch of B images takes ceil(100 B / 128) launches -- round 5: no library GEMM for B >= 2 either).
    x_add: the Linear runs on x + x_add (the query position embedding), added inside the kernel."""
    K = x.shape[-1]
    if K % 32:
        raise ops.RbaHipError("query Linears need K % 32 == 0 (hidden_dim 256 in every released architecture)")
    M = x.numel() // K
    x2 = x.contiguous().view(M, K)
    a2 = None if x_add is None else x_add.contiguous().view(M, K)
    if M <= 128:
        return ops.skinny_linear(x2, weight, bias, relu, x_add=a2).view(tuple(x.shape[:-1]) + (weight.shape[0],))
    # more than 128 rows (a batch of B >= 2 images): 128-row blocks, every launch writing ITS rows of the one output tensor (no per-block allocation + copy)
    out = torch.empty((M, weight.shape[0]), dtype=torch.float32, device=x.device)
    for r0 in range(0, M, 128):
        ops.skinny_linear(x2[r0:r0 + 128], weight, bias, relu, x_add=None if a2 is None else a2[r0:r0 + 128], out=out[r0:r0 + 128])
    return out.view(tuple(x.shape[:-1]) + (weight.shape[0],))


class MaskLogitsFunction(Function):
    """``MaskLogitsFunction.apply(embed [B,Q,C], feat [B,C,h,w] | [B,C,N]) -> [B,Q,h,w] | [B,Q,N]``: ``ops.mask_logits`` in the current split mode
    (the very bits of a direct call), differentiable once with respect to both tensors through ``ops.mask_logits_backward`` (exact fp32).  Only the
    inputs the requested gradients read are saved -- ``feat`` for ``embed``'s gradient, ``embed`` for ``feat``'s; a gradient nobody asks for is
    not computed."""

    @staticmethod
    def forward(ctx, embed, feat):
        embed, feat = embed.contiguous(), feat.contiguous()
        need_embed, need_feat = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        ctx.save_for_backward(embed if need_feat else None, feat if need_embed else None)
        return ops.mask_logits(embed, feat)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        embed, feat = ctx.saved_tensors
        need_embed, need_feat = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_embed or need_feat):
            return None, None
        grad_out = grad_out.contiguous()                     # `out.sum().backward()` hands an expanded (stride 0) gradient
        return ops.mask_logits_backward(embed, feat, grad_out, need_embed=need_embed, need_feat=need_feat)


class MaskedXattnFunction(Function):
    """``MaskedXattnFunction.apply(q [B,Q,nH,32], k, v [B,S,nH,32], mask_logits [B,Q,S] | None) -> [B,Q,nH*32]``: ``ops.masked_xattn`` (the very
    bits of a direct call), differentiable once with respect to q, k and v through K3's backward kernel (``ops.masked_xattn_backward``).  The mask
    logits get no gradient (the reference detaches them, :487).  The backward reads all three tensors and the mask whatever is asked for, so they
    are saved only when some gradient is; a gradient nobody asks for is not computed."""

    @staticmethod
    def forward(ctx, q, k, v, mask_logits):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        if mask_logits is not None:
            mask_logits = mask_logits.contiguous()
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(q, k, v, mask_logits)
        return ops.masked_xattn(q, k, v, mask_logits)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        need = ctx.needs_input_grad[:3]
        if not any(need):
            return None, None, None, None
        q, k, v, mask_logits = ctx.saved_tensors
        grad_out = grad_out.contiguous()                     # `out.sum().backward()` hands an expanded (stride 0) gradient
        return ops.masked_xattn_backward(q, k, v, mask_logits, grad_out, *need) + (None,)


# ------------------------------------------------------------------------------------------------ the query-side operations of a training forward
# Every forward below is the inference path's launch, so the values are its bits; the backwards are small library GEMMs / torch's LayerNorm
# backward on [B*Q, C] rows by design, as in ``MSDeformAttn._forward_differentiable``, and K3's backward kernel for the core.
def _rows(t):
    return t.reshape(-1, t.shape[-1])


class _LinearFunction(Function):
    """``_qlinear(x, weight, bias, relu, x_add)`` with gradients for x, x_add (the position embedding: the same rows as x's), weight and bias."""

    @staticmethod
    def forward(ctx, x, x_add, weight, bias, relu):
        y = _qlinear(x, weight, bias, relu, x_add)
        ctx.relu = relu
        ctx.save_for_backward(x, x_add, weight, y if relu else None)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        x, x_add, weight, y = ctx.saved_tensors
        g = _rows(grad_y)
        if ctx.relu:
            g = g * (_rows(y) > 0)
        need = ctx.needs_input_grad
        gx = (g @ weight).view(x.shape) if need[0] or need[1] else None
        gw = g.t() @ _rows(x if x_add is None else x + x_add) if need[2] else None
        return gx if need[0] else None, gx if need[1] else None, gw, g.sum(0) if need[3] else None, None


class _QKVFunction(Function):
    """Self-attention's stacked in_proj in one launch (``ops.skinny_linear(..., add_cols=2E, segments=3)``): q, k from x + x_add, v from x."""

    @staticmethod
    def forward(ctx, x, x_add, weight, bias):
        E = weight.shape[1]
        ctx.save_for_backward(x, x_add, weight)
        return tuple(ops.skinny_linear(x, weight, bias, x_add=None if x_add is None else x_add.contiguous(), add_cols=2 * E, segments=3))

    @staticmethod
    @once_differentiable
    def backward(ctx, gq, gk, gv):
        x, x_add, weight = ctx.saved_tensors
        E = weight.shape[1]
        gqk, gv = torch.cat((_rows(gq), _rows(gk)), 1), _rows(gv)
        need = ctx.needs_input_grad
        ga = (gqk @ weight[:2 * E]).view(x.shape) if need[0] or need[1] else None
        gx = ga + (gv @ weight[2 * E:]).view(x.shape) if need[0] else None
        gw = torch.cat((gqk.t() @ _rows(x if x_add is None else x + x_add), gv.t() @ _rows(x)), 0) if need[2] else None
        gb = torch.cat((gqk.sum(0), gv.sum(0))) if need[3] else None
        return gx, ga if need[1] else None, gw, gb


class _KVFunction(Function):
    """The key / value projections of `_MHAParams._project_kv` (k from key + key_add, v from key) with gradients for key, key_add, the stacked
    in_proj weight and bias (their q rows get zeros) and for `level_row` [C]: a vector that the caller has ALREADY added to every row of `key`
    (``level_embed.weight[i]`` inside the detached memory) -- its gradient is (sum_s dk_s) W_k + (sum_s dv_s) W_v, no d key [B,S,C] needed."""

    @staticmethod
    def forward(ctx, mha, key, key_add, level_row, weight, bias):
        ctx.save_for_backward(key, key_add, weight)
        return mha._project_kv(key, key_add)

    @staticmethod
    @once_differentiable
    def backward(ctx, gk, gv):
        key, key_add, weight = ctx.saved_tensors
        E = weight.shape[1]
        gk, gv = _rows(gk.reshape(key.shape)), _rows(gv.reshape(key.shape))
        wk, wv = weight[E:2 * E], weight[2 * E:]
        _, need_key, need_add, need_level, need_w, need_b = ctx.needs_input_grad
        ga = (gk @ wk).view(key.shape) if need_key or need_add else None
        gkey = ga + (gv @ wv).view(key.shape) if need_key else None
        sk, sv = (gk.sum(0), gv.sum(0)) if need_level or need_b else (None, None)
        glevel = sk @ wk + sv @ wv if need_level else None
        gw = torch.cat((weight.new_zeros(E, E), gk.t() @ _rows(key if key_add is None else key + key_add), gv.t() @ _rows(key)), 0) if need_w else None
        gb = torch.cat((sk.new_zeros(E), sk, sv)) if need_b else None
        return None, gkey, ga if need_add else None, glevel, gw, gb


class _AddLayerNormFunction(Function):
    """``ops.add_layer_norm(x, weight, bias, eps, residual, residual_bias)[1]`` = LayerNorm(x + residual + residual_bias) with gradients for x,
    residual, the folded bias (out_proj.bias / linear2.bias), weight and bias: torch's LayerNorm backward on the [B*Q, C] rows."""

    @staticmethod
    def forward(ctx, x, residual, residual_bias, weight, bias, eps):
        ctx.eps = eps
        s, y = ops.add_layer_norm(x, weight, bias, eps, residual, residual_bias)
        ctx.save_for_backward(s, weight, bias)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_y):
        s, weight, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_s = need[0] or need[1] or need[2]
        with torch.enable_grad():
            z = s.detach().requires_grad_(need_s)
            w, b = weight.detach().requires_grad_(True), bias.detach().requires_grad_(True)
            y = F.layer_norm(z, (z.shape[-1],), w, b, ctx.eps)
        gs, gw, gb = torch.autograd.grad(y, (z, w, b), grad_y) if need_s else (None,) + torch.autograd.grad(y, (w, b), grad_y)
        return (gs if need[0] else None, gs if need[1] else None, _rows(gs).sum(0) if need[2] else None,
                gw if need[3] else None, gb if need[4] else None, None)


# One body per layer: `graph` (always the caller's explicit argument, never read off requires_grad or grad mode) picks the autograd Function
# around the launch; without it the launch is called directly and no Function.apply is entered.
def _linear(graph, x, weight, bias=None, relu=False, x_add=None):
    return _LinearFunction.apply(x, x_add, weight, bias, relu) if graph else _qlinear(x, weight, bias, relu, x_add)


def _add_layer_norm(graph, x, norm, residual=None, residual_bias=None):
    """norm(x + residual + residual_bias): the folded bias (out_proj.bias / linear2.bias) is added inside the launch"""
    if graph:
        return _AddLayerNormFunction.apply(x, residual, residual_bias, norm.weight, norm.bias, norm.eps)
    return ops.add_layer_norm(x, norm.weight, norm.bias, norm.eps, residual, residual_bias)[1]


def _masked_xattn(graph, q, k, v, mask_logits):
    return MaskedXattnFunction.apply(q, k, v, mask_logits) if graph else ops.masked_xattn(q, k, v, mask_logits)


class _MHAParams(nn.Module):
    """Parameter holder with nn.MultiheadAttention's names: in_proj_weight, in_proj_bias, out_proj.{weight,bias}."""

    def __init__(self, d_model, nhead):
        super().__init__()
        self.embed_dim, self.num_heads = d_model, nhead
        self.in_proj_weight = nn.Parameter(torch.zeros(3 * d_model, d_model))
        self.in_proj_bias = nn.Parameter(torch.zeros(3 * d_model))
        self.out_proj = nn.Linear(d_model, d_model)

    def _kv_views(self):
        """the key / value rows of in_proj as Linear views (their packed weight images are cached on the views)"""
        w, b, E = self.in_proj_weight, self.in_proj_bias, self.embed_dim
        return derived(self, "kv_views", (w, b),
                       lambda: (SimpleNamespace(weight=w[E:2 * E], bias=b[E:2 * E]), SimpleNamespace(weight=w[2 * E:], bias=b[2 * E:])))

    def forward(self, query, key, mask_logits=None, key_add=None, query_add=None, level_row=None, graph=False):
        """batch-first: query [B,Q,E], key [B,S,E] (the values too); mask_logits [B,Q,S] (blocked iff sigmoid < 0.5).  key_add / query_add: the
        keys / queries are ``key + key_add`` / ``query + query_add`` (position embeddings, :48-58, :106-118), added inside the projections.
        graph: the same launches with an autograd graph over query, key, the position operands and the four parameters (the mask logits get
        no gradient); level_row: see `_KVFunction`."""
        E, nH = self.embed_dim, self.num_heads
        B, Q, _ = query.shape
        S = key.shape[1]
        w, b = self.in_proj_weight, self.in_proj_bias
        if query is key and key_add is query_add and B * Q <= 128 and E % 32 == 0 and w.is_contiguous() and query.is_contiguous():
            # self-attention: q = W_q (tgt + pos), k = W_k (tgt + pos), v = W_v tgt -- ONE launch over the stacked in_proj weight (was: an add
            # and three launches); q, k, v come back separately contiguous
            if graph:
                q, k, v = _QKVFunction.apply(query, query_add, w, b)
            else:
                q, k, v = ops.skinny_linear(query, w, b, x_add=None if query_add is None else query_add.contiguous(), add_cols=2 * E, segments=3)
            k, v = k.view(B, S, nH, E // nH), v.view(B, S, nH, E // nH)
        else:
            q = _linear(graph, query, w[:E], b[:E], x_add=query_add)
            k, v = _KVFunction.apply(self, key, key_add, level_row, w, b) if graph else self._project_kv(key, key_add)
        o = _masked_xattn(graph, q.view(B, Q, nH, E // nH), k, v, mask_logits)
        return _linear(graph, o, self.out_proj.weight)      # out_proj.bias is added inside the caller's fused add+LN

    def _project_kv(self, key, key_add):
        """k = W_k (key + key_add) + b_k, v = W_v key + b_v as [B,S,nH,hd], by the kernel that pays for the shape"""
        E, nH = self.embed_dim, self.num_heads
        B, S, _ = key.shape
        w, b = self.in_proj_weight, self.in_proj_bias
        if (B * S > 128 and key.is_contiguous() and ops.token_linear_pays(B * S, E, E)
                and (key_add is None or (key_add.is_contiguous() and tuple(key_add.shape) == tuple(key.shape)))):
            # cross-attention: k = W_k (memory + pos) + b_k and v = W_v memory + b_v in ONE launch of the row-complete kernel (was: an add and two
            # library GEMMs per layer)
            lk, lv = self._kv_views()
            k, v = ops.token_linear_multi(key, [(lk, key_add, None, 0, False), (lv, None, None, 0, False)])
            return k.view(B, S, nH, E // nH), v.view(B, S, nH, E // nH)
        value = key
        if key_add is not None:
            key = key + key_add
        if B * S > 128:
            # a memory level beyond the row-complete kernel's range (C5's 14 400-token level): the key / value projections are ordinary token
            # Linears -> K6 where it pays (ops.linear decides; the packed planes are cached on the views), not a library GEMM
            lk, lv = self._kv_views()
            return ops.linear(key.contiguous(), lk).view(B, S, nH, E // nH), ops.linear(value.contiguous(), lv).view(B, S, nH, E // nH)
        # self-attention: key / value are the (<= 128) queries themselves -> the skinny kernel too (hipBLASLt takes 33 us for 100 x 256 x 256)
        return _qlinear(key, w[E:2 * E], b[E:2 * E]).view(B, S, nH, E // nH), _qlinear(value, w[2 * E:], b[2 * E:]).view(B, S, nH, E // nH)


# The three decoder layers (post-norm).  graph: the same launches in the same order -- the same bits -- with an autograd graph over tgt, query_pos
# and the layer's parameters.
class SelfAttentionLayer(nn.Module):
    def __init__(self, d_model, nhead):
        super().__init__()
        self.self_attn = _MHAParams(d_model, nhead)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, tgt, query_pos, graph=False):
        tgt = tgt.contiguous()
        t2 = self.self_attn(tgt, tgt, key_add=query_pos, query_add=query_pos, graph=graph)      # q = k = tgt + query_pos, v = tgt
        return _add_layer_norm(graph, tgt, self.norm, t2, self.self_attn.out_proj.bias)          # forward_post :48-58


class CrossAttentionLayer(nn.Module):
    def __init__(self, d_model, nhead):
        super().__init__()
        self.multihead_attn = _MHAParams(d_model, nhead)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, tgt, memory, mask_logits, pos, query_pos, level_row=None, graph=False):
        """level_row (graph only): a vector already added to every row of `memory` that is to receive its gradient (`_KVFunction`); memory
        itself gets one where it requires grad"""
        t2 = self.multihead_attn(tgt, memory, mask_logits, key_add=pos, query_add=query_pos, level_row=level_row, graph=graph)
        return _add_layer_norm(graph, tgt.contiguous(), self.norm, t2, self.multihead_attn.out_proj.bias)     # forward_post :106-118


class FFNLayer(nn.Module):
    def __init__(self, d_model, dim_feedforward):
        super().__init__()
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm = nn.LayerNorm(d_model)

    def forward(self, tgt, graph=False):
        t2 = _linear(graph, _linear(graph, tgt, self.linear1.weight, self.linear1.bias, relu=True), self.linear2.weight)
        return _add_layer_norm(graph, tgt.contiguous(), self.norm, t2, self.linear2.bias)         # forward_post :171-175


class MLP(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        h = [hidden_dim] * (num_layers - 1)
        self.layers = nn.ModuleList(nn.Linear(n, k) for n, k in zip([input_dim] + h, h + [output_dim]))

    def forward(self, x, graph=False):
        for i, layer in enumerate(self.layers):
            x = _linear(graph, x, layer.weight, layer.bias, relu=i < self.num_layers - 1)
        return x


class BNReluConv(nn.Module):
    """BatchNorm2d -> ReLU -> Conv2d(k=1) with the reference's sub-module names (norm / conv; reference :216-230), evaluated in
    inference mode by one HIP kernel: the running statistics are folded into a per-channel scale and shift."""

    def __init__(self, num_maps_in, num_maps_out):
        super().__init__()
        self.norm = nn.BatchNorm2d(num_maps_in, momentum=0.01)
        self.conv = nn.Conv2d(num_maps_in, num_maps_out, kernel_size=1, bias=True)

    def forward(self, x):
        n = self.norm
        scale = n.weight * torch.rsqrt(n.running_var + n.eps)
        shift = n.bias - n.running_mean * scale
        return ops.bn_relu_conv1x1(x.contiguous(), scale.contiguous(), shift.contiguous(),
                                   self.conv.weight.flatten(1).contiguous(), self.conv.bias)

    def forward_differentiable(self, x):
        """The head in plain torch, with a graph over its four parameters (the DenseHybrid fine-tune trains it; see the decoder's
        ``differentiable_ood_head``): F.batch_norm in the mode ``self.norm.training`` says -- batch statistics and the running-statistics update
        of nn.BatchNorm2d in training mode, the running statistics in eval mode -- then ReLU and the 1x1 convolution as a matmul.  x [B,C,H,W]
        -> [B,out,H,W]."""
        n = self.norm
        if n.training and n.track_running_stats:
            n.num_batches_tracked.add_(1)
        y = F.relu(F.batch_norm(x, n.running_mean, n.running_var, n.weight, n.bias, n.training, n.momentum, n.eps))
        return torch.einsum("oc,bchw->bohw", self.conv.weight.flatten(1), y) + self.conv.bias[None, :, None, None]


@TRANSFORMER_DECODER_REGISTRY.register()
class MultiScaleMaskedTransformerDecoder(nn.Module):
    """``forward`` runs in one of three modes, decided once at its top from two attributes (both default False) and grad mode.  In every mode each
    layer and head is the one body that launches the inference kernels in the inference order, so ``pred_logits`` and ``pred_masks`` are the
    inference forward's bits; a training mode only wraps those launches in autograd Functions.  ``mask_features`` and the memory never receive
    a gradient (frozen pixel decoder), nor do the attention-mask logits (reference :487): their head calls stay sparse, under ``no_grad``.

    None -- inference: no autograd graph is built, whatever ``self.training`` or ``requires_grad`` of the parameters say.
    "heads" -- ``differentiable_heads`` set and grad mode on: the outlier-supervised fine-tune of the two prediction heads
      (FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP).  Decoding runs under ``no_grad`` as in inference; the LAST ``forward_prediction_heads`` call
      (reference :472-479) builds a graph over ``decoder_norm.{weight,bias}``, ``class_embed.{weight,bias}`` and the six ``mask_embed`` tensors,
      not over the decoder-layer output entering it.  The contraction's backward is K4's backward kernel (``MaskLogitsFunction``).
    "decoder" -- ``differentiable_decoder`` set too: the released PEBAL recipe, which freezes the backbone and the pixel decoder and nothing
      else.  The decoder layers carry a graph over every predictor parameter that requires grad (cross-attention, self-attention, FFN, their
      norms, ``query_feat``, ``query_embed``, ``level_embed``), and the head calls that return outputs are differentiable with respect to the
      layer output too.  The attention core's backward is K3's backward kernel, the Linears' and norms' are library GEMMs / torch's LayerNorm
      backward on [B*Q, C] rows.  The cached initial head call is bypassed.

    Two more attributes (default False) are read only in a training mode.  ``deep_supervision`` (the recipe's DEEP_SUPERVISION): ``aux_outputs``
    has ``num_layers`` entries in the reference's ``_set_aux_loss`` order -- the head call before layer 0, then the calls after layers 0 ... L-2
    -- each with ``pred_logits`` and a dense ``pred_masks`` [B,Q,H/4,W/4] carrying the graph of the mode.  They are evaluated behind the
    untouched decoding, on the decoder-layer outputs it held at each head call, and their values are the bits the inference forward returns with
    ``sparse_intermediate_heads = False``; without it ``aux_outputs`` stay as in inference (detached; ``pred_logits`` only on the sparse path).
    ``differentiable_ood_head`` (the DenseHybrid recipe's FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP_AND_OOD_PRED, on a model with that head):
    ``out["ood_pred"]`` is computed in plain torch on the detached ``mask_features`` (``BNReluConv.forward_differentiable``) with a graph over
    ``ood_pred.norm.{weight,bias}`` and ``ood_pred.conv.{weight,bias}`` only; the batch norm runs in the mode ``ood_pred.norm.training`` says and
    updates its running statistics in training mode.  Without it ``ood_pred`` stays the inference kernel's output under ``no_grad``."""

    differentiable_heads = False
    deep_supervision = False
    differentiable_ood_head = False
    differentiable_decoder = False
    # forward() accepts the pixel decoder's DeferredMaskFeatures in place of the mask-feature tensor (MaskFormerHead asks for one when this is set)
    takes_deferred_mask_features = True

    def __init__(self, arch):
        super().__init__()
        a = arch
        d = a["conv_dim"]
        self.num_heads, self.num_layers = a["nheads"], a["dec_layers"]
        self.num_queries, self.num_feature_levels = a["num_queries"], len(a["enc_in"])
        self.pe_layer = PositionEmbeddingSine(d // 2, normalize=True)
        self.transformer_self_attention_layers = nn.ModuleList(SelfAttentionLayer(d, a["nheads"]) for _ in range(self.num_layers))
        self.transformer_cross_attention_layers = nn.ModuleList(CrossAttentionLayer(d, a["nheads"]) for _ in range(self.num_layers))
        self.transformer_ffn_layers = nn.ModuleList(FFNLayer(d, a["dim_feedforward"]) for _ in range(self.num_layers))
        self.decoder_norm = nn.LayerNorm(d)
        self.query_feat = nn.Embedding(a["num_queries"], d)
        self.query_embed = nn.Embedding(a["num_queries"], d)
        self.level_embed = nn.Embedding(self.num_feature_levels, d)
        self.class_embed = nn.Linear(d, a["num_classes"] + 1)
        self.mask_embed = MLP(d, d, a["mask_dim"], 3)
        self.ood_prediction = bool(a.get("dense_hybrid", False))
        if self.ood_prediction:                                  # DenseHybrid head (reference :365-366)
            self.ood_pred = BNReluConv(d, 2)
        # inference-only shortcut, exact: intermediate heads evaluate mask logits only where the attention mask samples them
        # (aux_outputs then carry pred_logits only)
        self.sparse_intermediate_heads = True
        self.cache_initial_heads = True          # the heads of the un-decoded queries are constants of the checkpoint (_initial_query_side)
        self._plan_cache = ShapeCache(8)
        self._row_cache = ShapeCache(8)          # _row_plan: the sparse plans as validated row indices of the gathered projection

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # v1 checkpoints call query_feat "static_query" (reference :237-258)
        for k in list(state_dict.keys()):
            if k.startswith(prefix) and "static_query" in k:
                state_dict[k.replace("static_query", "query_feat")] = state_dict.pop(k)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _sparse_plan(self, feat_hw, target_hw, device):
        """For an even integer down-sampling factor f the align_corners=False bilinear sample of target cell (y, x) is
        0.5*(0.5*v[r0,c0] + 0.5*v[r0,c1]) + 0.5*(0.5*v[r1,c0] + 0.5*v[r1,c1]) with r0 = f*y + f/2 - 1, r1 = r0 + 1 (same for
        columns): exactly 2x2 source pixels.  Returns the flat source indices [4, h*w] or None when the factor is not an
        even integer (then the dense path is used)."""
        key = (tuple(feat_hw), tuple(target_hw), device)

        def build():
            (H, W), (h, w) = feat_hw, target_hw
            if not (h > 0 and w > 0 and H % h == 0 and W % w == 0 and (H // h) % 2 == 0 and (W // w) % 2 == 0 and 4 * h * w < H * W):
                return False
            fy, fx = H // h, W // w
            r0 = torch.arange(h, device=device) * fy + fy // 2 - 1
            c0 = torch.arange(w, device=device) * fx + fx // 2 - 1
            idx = [((r0 + dr)[:, None] * W + (c0 + dc)[None, :]).reshape(-1) for dr in (0, 1) for dc in (0, 1)]
            return torch.stack(idx).contiguous()

        plan = self._plan_cache.get(key, build)
        return None if plan is False else plan

    def _row_plan(self, feat_hw, target_hw, device, B):
        """_sparse_plan as the validated row index [B, 4 h w] of the gathered projection (ops.row_index), or None: no sparse plan for the level, 4 h w not a
        multiple of 128, or the entry is not cached yet and the stream is capturing (validation reads the values back: never inside a capture)."""
        key = (tuple(feat_hw), tuple(target_hw), device, B)
        if key not in self._row_cache and torch.cuda.is_current_stream_capturing():
            return None

        def build():
            plan = self._sparse_plan(feat_hw, target_hw, device)
            if plan is None or plan.numel() % 128:
                return False
            rows = ops.row_index(plan.reshape(1, -1).expand(B, -1), feat_hw[0] * feat_hw[1])
            torch.cuda.current_stream(device).synchronize()          # once per shape: forwards on OTHER streams read the index without an event
            return rows

        rows = self._row_cache.get(key, build)
        return None if rows is False else rows

    def _composed_mask_heads(self, mask_features, size_list):
        """The selection rule of docs/kernels/K4.md: True when this forward never needs the mask-feature map -- every intermediate head call is a sparse one
        that can project its own rows, and the last call contracts the pixels with the composed operand.  (Its grad-mode clause is forward()'s: a forward with
        differentiable heads materialises the map before it gets here.)"""
        if not (ops.COMPOSED_MASK_HEAD and ops.SPLIT_MODE == "f16x3" and self.sparse_intermediate_heads and not self.ood_prediction):
            return False
        md = mask_features.shape[1]
        if self.num_queries > 128 or md > 256 or md % 4 or mask_features.rows_per_image * mask_features.prev.shape[1] >= 1 << 30:
            return False                                              # (the contracts of ops.compose_query_operand / split_linear_nchw_out_gn_rows)
        levels = {size_list[i % self.num_feature_levels] for i in range(self.num_layers)}
        rows = [self._row_plan(mask_features.shape[-2:], lvl, mask_features.device, mask_features.shape[0]) for lvl in sorted(levels)]
        if any(r is None for r in rows):
            return False
        return ops.composed_mask_head_pays(mask_features.rows_per_image, sum(r.data.shape[1] for r in rows))

    def _query_side_heads(self, output, mode=None):
        """decoder_norm -> class_embed, mask_embed MLP on the query tensor [B,Q,C] (reference :473-476): (class logits [B,Q,K+1], mask embedding [B,Q,md]).
        mode (forward()'s): the same launches in the same order with an autograd graph over the ten head tensors -- "decoder": over `output` too."""
        graph = mode is not None
        if mode == "heads":
            output = output.detach()
        dec = _add_layer_norm(graph, output.contiguous(), self.decoder_norm)
        return _linear(graph, dec, self.class_embed.weight, self.class_embed.bias), self.mask_embed(dec, graph).contiguous()

    def _aux_heads_differentiable(self, outputs, mask_features, mode):
        """The intermediate head calls of deep supervision on `outputs` = the decoder-layer outputs [B,Q,C] entering them: the query side once on
        their concatenation along the batch axis (row-wise kernels: the bits of one call each, and one backward pass), then one contraction per
        call against the one `mask_features` -> [{"pred_logits", "pred_masks"}], every tensor with a graph over the ten head tensors only
        (mode "decoder": over `outputs` too)."""
        B = outputs[0].shape[0]
        cls, embed = self._query_side_heads(torch.cat(outputs, dim=0), mode)
        feat = mask_features.detach()
        return [{"pred_logits": cls[l * B:(l + 1) * B], "pred_masks": MaskLogitsFunction.apply(embed[l * B:(l + 1) * B], feat)}
                for l in range(len(outputs))]

    def _initial_query_side(self, B, device):
        """The prediction heads BEFORE the first layer (reference :427-430) see `query_feat.weight` -- learnt parameters, not the image: decoder_norm, class_embed
        and the three mask_embed Linears of that call are constants of the checkpoint.  Computed once per (weights version, batch size) with the same kernels
        (bit-identical to evaluating them per image) and kept: five launches and the query tensor's expand + copy less per image (round 6).
        One entry per (batch size, device, weights) in a ShapeCache: a captured graph reads these tensors by address, so an entry looked up during a capture
        is pinned -- a call with another batch size or other weights adds an entry and never frees one a graph still replays."""
        ps = [self.query_feat.weight, self.decoder_norm.weight, self.decoder_norm.bias, self.class_embed.weight, self.class_embed.bias]
        for ly in self.mask_embed.layers:
            ps += [ly.weight, ly.bias]
        key = (B, device, source_key(*ps))
        cache = self.__dict__.get("_rba_heads0")
        if cache is None:
            cache = self.__dict__["_rba_heads0"] = ShapeCache(4)
        if key not in cache and torch.cuda.is_current_stream_capturing():
            return None                                               # never build a cache entry inside a capture: evaluate in line instead

        def build():
            output = self.query_feat.weight[None].expand(B, -1, -1).contiguous()
            side = self._query_side_heads(output)
            torch.cuda.current_stream(device).synchronize()          # once per checkpoint: forwards on OTHER streams read these tensors without an event
            return output, side

        return cache.get(key, build)

    def forward_prediction_heads(self, output, mask_features, attn_mask_target_size, need_attn_mask=True, need_masks=True,
                                 gathered=None, query_side=None, mode=None):
        """output [B,Q,C] -> class logits [B,Q,K+1], mask logits [B,Q,H/4,W/4] (None unless need_masks), attention-mask
        logits [B,Q,h*w] (reference :472-489; the threshold itself happens inside K3).  When only the attention mask is
        consumed (every call but the last) the mask logits are evaluated just at the 2x2 source pixels each attention
        cell interpolates -- the same arithmetic on 4*h*w instead of H*W/16 columns.  mode: forward()'s, for its last call."""
        if mode is not None:
            # the last call of a training forward (see the class): live heads, never the cached initial ones
            outputs_class, mask_embed = self._query_side_heads(output, mode)
            return outputs_class, MaskLogitsFunction.apply(mask_embed, mask_features.detach()), None
        if query_side is not None:
            outputs_class, mask_embed = query_side
        else:
            outputs_class, mask_embed = self._query_side_heads(output)
        plan = None
        if need_attn_mask and not need_masks and self.sparse_intermediate_heads:
            plan = self._sparse_plan(mask_features.shape[-2:], attn_mask_target_size, mask_features.device)
        if plan is not None:
            B, C = mask_features.shape[:2]
            lvl = tuple(attn_mask_target_size)
            gathered = {} if gathered is None else gathered    # per-call dict owned by forward(): the module stays re-entrant
            if lvl not in gathered:                   # mask_features is the same tensor for every layer: gather once per level
                if isinstance(mask_features, DeferredMaskFeatures):          # the same columns, projected from their own rows: the map is never written
                    gathered[lvl] = mask_features.gather(self._row_plan(mask_features.shape[-2:], lvl, mask_features.device, B))
                else:
                    gathered[lvl] = mask_features.flatten(2).index_select(2, plan.reshape(-1)).contiguous()   # [B,C,4hw]
            cols = gathered[lvl]
            v = ops.mask_logits(mask_embed, cols).view(B, -1, 4, plan.shape[1])
            # = 0.5 * (0.5 * v0 + 0.5 * v1) + 0.5 * (0.5 * v2 + 0.5 * v3), the bilinear sample at the centre of a 2 x 2 cell: scaling by a power
            # of two is exact, so the factors can be collected without changing a bit -- ((v0 + v1) + (v2 + v3)) * 0.25 in one launch
            return outputs_class, None, ops.quad_mean(v)
        if isinstance(mask_features, DeferredMaskFeatures):
            if need_attn_mask:                                              # (not reached under _composed_mask_heads' rule: a dense intermediate call wants the map)
                mask_features = mask_features.materialize()
            else:
                return outputs_class, mask_features.contract(mask_embed), None
        outputs_mask = ops.mask_logits(mask_embed, mask_features)
        attn_logits = None
        if need_attn_mask:
            attn_logits = ops.resample_bilinear(outputs_mask, attn_mask_target_size).flatten(2)
        return outputs_class, outputs_mask, attn_logits

    def _level_pos(self, x, B):
        """sine position embedding of a level as tokens [B, S, C] (contiguous: it is the key projection's `x_add` operand), per (shape, batch)"""
        cache = self.__dict__.setdefault("_pos_tok_cache", ShapeCache(8))
        key = (tuple(x.shape[-2:]), B, x.device)
        return cache.get(key, lambda: self.pe_layer(x).flatten(2).transpose(1, 2).expand(B, -1, -1).contiguous())

    def forward(self, x, mask_features, mask=None):
        """x: list of [B,C,h_l,w_l]; mask_features [B,md,H/4,W/4] -> dict(pred_logits, pred_masks, aux_outputs)
        (reference :398-470).  The mode (see the class) is decided here, once, and passed down: nothing below reads the flags or grad mode."""
        assert len(x) == self.num_feature_levels
        del mask
        mode = None
        if self.differentiable_heads and torch.is_grad_enabled():
            mode = "decoder" if self.differentiable_decoder else "heads"
        frozen = contextlib.nullcontext if mode is None else torch.no_grad
        if mode is not None and isinstance(mask_features, DeferredMaskFeatures):
            mask_features = mask_features.materialize()               # the differentiable last call wants the map (MaskLogitsFunction)
        with (torch.no_grad if mode == "heads" else contextlib.nullcontext)():
            output, mask_features, side, predictions_class, predictions_mask, head_inputs = self._decode(x, mask_features, mode == "decoder")
        cls, msk, _ = self.forward_prediction_heads(output, mask_features, None, need_attn_mask=False, need_masks=True, query_side=side, mode=mode)
        if mode is not None and self.deep_supervision:
            aux = self._aux_heads_differentiable(head_inputs, mask_features, mode) if head_inputs else []
        else:
            aux = [({"pred_logits": a, "pred_masks": b} if b is not None else {"pred_logits": a})
                   for a, b in zip(predictions_class, predictions_mask)]
        out = {"pred_logits": cls, "pred_masks": msk, "aux_outputs": aux}
        if self.ood_prediction:
            if mode is not None and self.differentiable_ood_head:
                out["ood_pred"] = self.ood_pred.forward_differentiable(mask_features.detach())
            else:
                with frozen():
                    out["ood_pred"] = self.ood_pred(mask_features)                   # reference :467-468
        return out

    def _memory_tokens(self, x):
        """the memory of every level as tokens: (src = x + level_embed [B,S,C], sine position embedding [B,S,C], (h, w)) per level"""
        src, pos, size_list = [], [], []
        B = x[0].shape[0]
        for i in range(self.num_feature_levels):
            size_list.append(tuple(int(v) for v in x[i].shape[-2:]))
            pos.append(self._level_pos(x[i], B))                                              # [B,S,C], cached per shape
            t = x[i].permute(0, 2, 3, 1)                                                      # channels-last views (pixel decoder): tokens without a copy
            tok = t.reshape(B, -1, x[i].shape[1]) if t.is_contiguous() else x[i].flatten(2).transpose(1, 2)
            src.append(tok + self.level_embed.weight[i])                                      # [B,S,C] contiguous (:424-426)
        return src, pos, size_list

    def _decode(self, x, mask_features, graph=False):
        """Everything of forward before its last head call -> (decoder-layer output [B,Q,C], contiguous mask_features, the cached query side of that
        call (only a decoder without layers has one), class and mask predictions of the intermediate calls, the decoder-layer outputs that entered
        those calls).  graph: the same launches in the same order with an autograd graph over the decoder layers -- the memory is built under
        no_grad and `mask_features` detached (frozen pixel decoder; level_embed's own gradient goes through `level_row`), the cached initial heads
        are bypassed, and the intermediate head calls run under no_grad on the detached layer output (the mask is detached in the reference,
        :487), sparse as in inference; the returned decoder-layer outputs carry their graph."""
        frozen = torch.no_grad if graph else contextlib.nullcontext
        with frozen():
            src, pos, size_list = self._memory_tokens(x)
        B = x[0].shape[0]
        query_embed = self.query_embed.weight[None].expand(B, -1, -1)
        first = self._initial_query_side(B, mask_features.device) if self.cache_initial_heads and not graph else None
        if first is not None:
            output, side0 = first                                     # constants of the checkpoint (never written: every layer returns new tensors)
        else:
            output, side0 = self.query_feat.weight[None].expand(B, -1, -1).contiguous(), None
        if graph:
            mask_features = mask_features.detach()                    # (forward() has materialised it)
        elif isinstance(mask_features, DeferredMaskFeatures) and not self._composed_mask_heads(mask_features, size_list):
            mask_features = mask_features.materialize()               # today's path from here on, bit for bit
        if not isinstance(mask_features, DeferredMaskFeatures):
            mask_features = mask_features.contiguous()
        level_row = graph and self.level_embed.weight.requires_grad
        predictions_class, predictions_mask, head_inputs = [], [], []
        gathered = {}

        def attn_mask_head(out, level, side=None):
            with frozen():
                cls, msk, logits = self.forward_prediction_heads(out.detach() if graph else out, mask_features, size_list[level], need_attn_mask=True,
                                                                 need_masks=False, gathered=gathered, query_side=side)
            predictions_class.append(cls)
            predictions_mask.append(msk)
            head_inputs.append(out)
            return logits

        if self.num_layers == 0:
            return output, mask_features, side0, predictions_class, predictions_mask, head_inputs
        attn_logits = attn_mask_head(output, 0, side0)
        for i in range(self.num_layers):
            li = i % self.num_feature_levels
            output = self.transformer_cross_attention_layers[i](output, src[li], attn_logits, pos[li], query_embed,     # memory + pos: inside the key projection
                                                                self.level_embed.weight[li] if level_row else None, graph)
            output = self.transformer_self_attention_layers[i](output, query_embed, graph)
            output = self.transformer_ffn_layers[i](output, graph)
            if i == self.num_layers - 1:
                break
            attn_logits = attn_mask_head(output, (i + 1) % self.num_feature_levels)
        return output, mask_features, None, predictions_class, predictions_mask, head_inputs
