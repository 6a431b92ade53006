"""Shared by tests/test_mask_logits_backward_cpu.py, tests/test_mask_logits_backward_gpu.py and tests/test_finetune_heads_gpu.py: the case table of
K4's backward with its seeded inputs and fp64 truth, and the torch restatement of the reference's last prediction-head call.

The restatement (``ref_heads``) is written from mask2former_transformer_decoder.py:472-479 of the reference (decoder_norm -> class_embed /
three-layer mask_embed -> einsum); like the outlier loss of tests/_rba_bwd_cases.py it is checked against the mathematics (gradcheck in double,
test_mask_logits_backward_cpu.py) and is the truth the GPU tests use.  Error metric, bar and check are those of tests/_rba_bwd_cases.py.
"""
import functools

import torch
import torch.nn.functional as F

from tests._rba_bwd_cases import bar, check, err, ref_outlier_loss  # noqa: F401  (re-exported: one metric, one bar)

HEAD_TENSORS = ("decoder_norm.weight", "decoder_norm.bias", "class_embed.weight", "class_embed.bias") + tuple(
    f"mask_embed.layers.{i}.{n}" for i in range(3) for n in ("weight", "bias"))


def ref_heads(output, mask_features, p, eps=1e-5):
    """:473-479.  output [B,Q,C] (a decoder layer's output), mask_features [B,md,h,w], p = {name: tensor} over HEAD_TENSORS ->
    (pred_logits [B,Q,K+1], pred_masks [B,Q,h,w])"""
    dec = F.layer_norm(output, (output.shape[-1],), p["decoder_norm.weight"], p["decoder_norm.bias"], eps)      # :473
    cls = F.linear(dec, p["class_embed.weight"], p["class_embed.bias"])                                         # :475
    e = dec
    for i in range(3):                                                                                          # :476, MLP :198-212
        e = F.linear(e, p[f"mask_embed.layers.{i}.weight"], p[f"mask_embed.layers.{i}.bias"])
        if i < 2:
            e = F.relu(e)
    return cls, torch.einsum("bqc,bchw->bqhw", e, mask_features)                                                # :479


# ---- K4 backward: (name, B, Q, C, N)
CASES = (
    ("crop", 1, 100, 256, 32768),      # the fine-tune's own size: many slices
    ("batch", 2, 100, 256, 2048),      # a different image per entry
    ("tail", 1, 100, 256, 4100),       # N % 4 == 0, not a multiple of any tile or slice
    ("odd", 1, 7, 12, 130),            # N % 4 != 0, C % 4 == 0, a single partial tile
    ("oddc", 1, 20, 30, 257),          # nothing aligned
    ("one", 1, 1, 1, 1),               # degenerate sizes
    ("bigq", 1, 250, 32, 515),         # Q > 112
    ("c264", 1, 100, 264, 516),        # C % 32 != 0
    ("c360", 1, 100, 360, 516),        # the forward's MFMA cap
    ("wide", 1, 33, 512, 260),         # beyond the released widths
    ("bigq4", 1, 250, 32, 516),        # Q > 112 with N % 4 == 0: three query blocks / two query chunks on the matrix-pipe kernels
)
CASE = {c[0]: c for c in CASES}
NAMES = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    """(E [B,Q,C], F [B,C,N], G [B,Q,N]) fp32 on the CPU, seeded by the case: G = randn * rand(Q,1) * 1e-3 (the size of a mean's gradient, a
    different weight per query), F = 0.25 randn with channel 0 constant 1, E = randn"""
    _, B, Q, C, N = CASE[name]
    return inputs_for(B, Q, C, N, 4000 + NAMES.index(name))


def inputs_for(B, Q, C, N, seed):
    """`case_inputs` for any shape, seeded: the named cases and the random-shape sweep draw here"""
    gen = torch.Generator().manual_seed(seed)
    G = torch.randn(B, Q, N, generator=gen) * torch.rand(B, Q, 1, generator=gen) * 1e-3
    Fm = 0.25 * torch.randn(B, C, N, generator=gen)
    Fm[:, 0] = 1.0
    E = torch.randn(B, Q, C, generator=gen)
    return E, Fm, G


def _autograd(E, Fm, G):
    e, f = E.detach().clone().requires_grad_(True), Fm.detach().clone().requires_grad_(True)
    (torch.einsum("bqc,bchw->bqhw", e, f[:, :, None, :]) * G[:, :, None, :]).sum().backward()
    return e.grad, f.grad


@functools.lru_cache(maxsize=None)
def case_truth(name):
    """fp64 CPU autograd of torch.einsum on .double() of the very inputs, and b = the same metric for fp32 CPU autograd:
    (grad_embed64, grad_feat64, b_embed, b_feat)"""
    E, Fm, G = case_inputs(name)
    ge64, gf64 = _autograd(E.double(), Fm.double(), G.double())
    ge32, gf32 = _autograd(E, Fm, G)
    return ge64, gf64, err(ge32, ge64), err(gf32, gf64)


def head_truth(output, mask_features, params, labels, dtype):
    """CPU autograd of ref_outlier_loss(ref_heads(...)) in `dtype` on copies of the given tensors (labels [B,H,W], or [H,W] with B = 1) ->
    (loss, {name: grad} over HEAD_TENSORS)"""
    p = {n: params[n].detach().cpu().to(dtype).clone().requires_grad_(True) for n in HEAD_TENSORS}
    cls, masks = ref_heads(output.detach().cpu().to(dtype), mask_features.detach().cpu().to(dtype), p)
    labels = labels.cpu()
    loss = ref_outlier_loss(cls, masks, labels if labels.dim() == 3 else labels[None])
    loss.backward()
    return loss.detach(), {n: t.grad for n, t in p.items()}
