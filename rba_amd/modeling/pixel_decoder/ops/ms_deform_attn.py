"""Multi-scale deformable attention: the reference's ``MSDeformAttn`` module and ``MSDeformAttnFunction`` surface
(pixel_decoder/ops/modules/ms_deform_attn.py:34-125, ops/functions/ms_deform_attn_func.py:32-49) on the HIP
kernels K2 (forward and backward).  Difference by design: unlike the reference's bare ``except`` (ms_deform_attn.py:116-121)
that silently falls back to grid_sample, a failure of the native op raises.  ``MSDeformAttn`` runs the fused inference path
unless its ``differentiable`` attribute is set (see the class)."""
from types import SimpleNamespace

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .... import ops
from ....lru import derived


class MSDeformAttnFunction(Function):
    """``MSDeformAttnFunction.apply(value, shapes, level_start_index, sampling_locations, attention_weights,
    im2col_step)`` -- the reference's autograd Function (ops/functions/ms_deform_attn_func.py:32-49) on the HIP forward and
    backward kernels.  Gradients flow to value, sampling_locations and attention_weights; once differentiable."""

    @staticmethod
    def forward(ctx, value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights,
                im2col_step=128):
        ctx.im2col_step = im2col_step
        output = ops.ms_deform_attn_forward(value, value_spatial_shapes, value_level_start_index, sampling_locations,
                                            attention_weights, im2col_step)
        ctx.save_for_backward(value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights)
        return output

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights = ctx.saved_tensors
        # `out.sum().backward()` hands an expanded (stride 0) gradient
        grad_value, grad_sampling_loc, grad_attn_weight = ops.ms_deform_attn_backward(
            value, value_spatial_shapes, value_level_start_index, sampling_locations, attention_weights, grad_output.contiguous(),
            ctx.im2col_step)
        need = ctx.needs_input_grad
        return (grad_value if need[0] else None, None, None, grad_sampling_loc if need[3] else None,
                grad_attn_weight if need[4] else None, None)


class MSDeformAttn(nn.Module):
    """``differentiable`` (attribute, default False) is the explicit opt-in to training: with it set and grad mode on, ``forward`` runs
    the reference formulation (torch Linears, softmax and location arithmetic around ``MSDeformAttnFunction.apply``), so every parameter
    and input receives a gradient.  Otherwise -- whatever ``self.training`` or ``requires_grad`` of the parameters say -- the fused
    inference path runs, which builds no autograd graph."""

    differentiable = False

    def __init__(self, d_model=256, n_levels=4, n_heads=8, n_points=4):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"d_model must be divisible by n_heads, but got {d_model} and {n_heads}")
        self.im2col_step = 128
        self.d_model, self.n_levels, self.n_heads, self.n_points = d_model, n_levels, n_heads, n_points
        self.sampling_offsets = nn.Linear(d_model, n_heads * n_levels * n_points * 2)
        self.attention_weights = nn.Linear(d_model, n_heads * n_levels * n_points)
        self.value_proj = nn.Linear(d_model, d_model)
        self.output_proj = nn.Linear(d_model, d_model)

    def _sampling_linear(self):
        """[sampling_offsets ; attention_weights] stacked along the output dimension, rebuilt when either weight changes."""
        so, aw = self.sampling_offsets, self.attention_weights

        def build():
            lin = SimpleNamespace(weight=torch.cat([so.weight.detach(), aw.weight.detach()], 0).contiguous(),
                                  bias=torch.cat([so.bias.detach(), aw.bias.detach()], 0).contiguous())
            lin.parts = [(SimpleNamespace(weight=lin.weight[c:c + 256], bias=lin.bias[c:c + 256]), c) for c in range(0, lin.weight.shape[0], 256)]
            return lin

        return derived(self, "sampling_linear", (so.weight, aw.weight, so.bias, aw.bias), build)

    def _sampling_parts(self):
        """the stacked sampling Linear cut into row chunks of <= 256 outputs for the row-complete token kernel: [(linear view, first column)]"""
        return self._sampling_linear().parts

    def forward(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                input_padding_mask=None, query_pos=None, post=None):
        """query [N,Lq,C]; reference_points [N,Lq,L,2] in [0,1]; input_flatten [N,S,C] -> [N,Lq,C].
        query_pos: the attention runs on ``query + query_pos`` (the encoder's `self.with_pos_embed(src, pos)`, msdeformattn.py:133) -- handed
        over separately so that the add happens inside the Linear that consumes it.  post = (residual, LayerNorm): return
        ``norm(residual + output)`` (msdeformattn.py:134-135), in the output projection's epilogue where the row-complete kernel applies."""
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        M, L, P = self.n_heads, self.n_levels, self.n_points
        if reference_points.shape[-1] != 2:
            raise ValueError(f"Last dim of reference_points must be 2 on this path, got {reference_points.shape[-1]}")
        C = self.d_model
        if self.differentiable and torch.is_grad_enabled():
            return self._forward_differentiable(query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                                                input_padding_mask, query_pos, post)
        fused = ops.msda_fused_ok(C // M, L, P, S, M) and input_padding_mask is None
        parts = self._sampling_parts()
        tok = (fused and query is input_flatten and len(parts) <= 2 and query.is_contiguous() and ops.token_linear_pays(N * S, C, C)
               and all(ops.token_linear_pays(N * Lq, pl.weight.shape[0], C) for pl, _ in parts)
               and (query_pos is None or (query_pos.is_contiguous() and tuple(query_pos.shape) == tuple(query.shape))))
        if tok:
            # value = value_proj(src) and the sampling Linears of src + pos: ONE launch (was: an add and two GEMMs)
            raw = torch.empty((N, Lq, M * L * P * 3), dtype=torch.float32, device=query.device)
            outs = ops.token_linear_multi(query, [(self.value_proj, None, None, 0, False)] + [(pl, query_pos, raw, c0, False) for pl, c0 in parts])
            out = ops.msda_fused(outs[0].view(N, S, M, C // M), input_spatial_shapes, input_level_start_index, raw, reference_points.contiguous(),
                                 M, L, P)
            if post is not None and ops.token_linear_pays(N * Lq, C, C):
                return ops.token_linear(out, self.output_proj, residual=post[0].contiguous(), norm=post[1])
            return self._finish(ops.linear(out, self.output_proj), post)
        if query_pos is not None:
            query = query + query_pos
        return self._finish(self._forward_general(query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                                                  input_padding_mask), post)

    def _forward_differentiable(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                                input_padding_mask, query_pos, post):
        """The reference formulation (ops/modules/ms_deform_attn.py:95-125) in torch ops around the autograd Function: the four
        projections are library GEMMs by design (training path only; never taken under torch.no_grad)."""
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        M, L, P = self.n_heads, self.n_levels, self.n_points
        if query_pos is not None:
            query = query + query_pos
        value = F.linear(input_flatten, self.value_proj.weight, self.value_proj.bias)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], 0.0)
        value = value.view(N, S, M, self.d_model // M)
        offsets = F.linear(query, self.sampling_offsets.weight, self.sampling_offsets.bias).view(N, Lq, M, L, P, 2)
        weights = F.linear(query, self.attention_weights.weight, self.attention_weights.bias).view(N, Lq, M, L * P)
        weights = F.softmax(weights, -1).view(N, Lq, M, L, P)
        normalizer = torch.stack([input_spatial_shapes[..., 1], input_spatial_shapes[..., 0]], -1)
        loc = reference_points[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
        out = MSDeformAttnFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index, loc.contiguous(),
                                         weights.contiguous(), self.im2col_step)
        y = F.linear(out, self.output_proj.weight, self.output_proj.bias)
        if post is None:
            return y
        res, norm = post
        return F.layer_norm(res + y, (self.d_model,), norm.weight, norm.bias, norm.eps)

    @staticmethod
    def _finish(y, post):
        if post is None:
            return y
        res, norm = post
        return ops.add_layer_norm(res, norm.weight, norm.bias, norm.eps, y.contiguous())[1]

    def _forward_general(self, query, reference_points, input_flatten, input_spatial_shapes, input_level_start_index,
                         input_padding_mask=None):
        N, Lq, _ = query.shape
        S = input_flatten.shape[1]
        M, L, P = self.n_heads, self.n_levels, self.n_points
        value = ops.linear(input_flatten, self.value_proj)
        if input_padding_mask is not None:
            value = value.masked_fill(input_padding_mask[..., None], 0.0)
        value = value.view(N, S, M, self.d_model // M)
        # sampling_offsets and attention_weights as ONE Linear (rows [offsets | logits]), then one kernel for
        # loc = reference + offset / (W_l, H_l) and the softmax over the L*P logits (reference :95-115)
        raw = ops.linear(query, self._sampling_linear())
        if ops.msda_fused_ok(self.d_model // M, L, P, S, M) and input_padding_mask is None:
            # locations + softmax inside the gather kernel: one launch, no [N,Lq,M,L,P,3] round trip
            out = ops.msda_fused(value.contiguous(), input_spatial_shapes, input_level_start_index, raw.contiguous(),
                                 reference_points.contiguous(), M, L, P)
            return ops.linear(out, self.output_proj)
        loc, weights = ops.msda_prepare(raw, reference_points.contiguous(), input_spatial_shapes, M, L, P)
        out = MSDeformAttnFunction.apply(value.contiguous(), input_spatial_shapes, input_level_start_index, loc, weights,
                                         self.im2col_step)
        return ops.linear(out, self.output_proj)
