"""Inputs, truth and error metric shared by tests/test_masked_xattn_backward_gpu.py and tools/k3_bwd_probe.py --errors.  Test infrastructure,
not product code.

Truth = double autograd through oracle.ref_ops.attention_core(q, k, v, blocked) with blocked = attn_mask_from_logits(ml) evaluated in fp32 on
the very logits the kernel sees (the threshold is a decision, not arithmetic: it is taken once, in the kernel's precision).  Metric and bar are
tests/_msda_cases.py's: e(T) = max|T - T64| / max|T64|, bar 4 max(b, 2^-20) with b the same metric for fp32 CPU autograd on the same inputs."""
import torch

from oracle import ref_ops
from tests._msda_cases import bar               # noqa: F401  (one bar)


def err(t, t64):
    """e(T) = max|T - T64| / max|T64| (tests/_msda_cases.err).  Where the truth is identically zero -- grad_q and grad_k of the one-key case: a
    softmax over one key is the constant 1 -- the ratio does not exist and the tensor has to be exactly zero: 0.0 then, inf otherwise."""
    d, m = float((t.detach().cpu().double() - t64).abs().max()), float(t64.abs().max())
    if m == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / m

# name -> (B, Q, S, nH, masked)
CASES = {
    "s1": (1, 5, 1, 1, True),
    "q16_s77": (2, 16, 77, 2, True),
    "q37_s301": (1, 37, 301, 3, True),
    "q130_s301": (1, 130, 301, 2, True),              # Q > 128
    "self_100": (1, 100, 100, 8, False),              # mask None: self-attention
    "s512": (1, 100, 512, 8, True),
    "b2_s2048": (2, 100, 2048, 8, True),
    "s8192": (1, 100, 8192, 8, True),
    "q37_s1023": (1, 37, 1023, 2, True),              # either side of the row pass's short-row / long-row switch (S >= 1024)
    "q37_s1024": (1, 37, 1024, 2, True),
}
ALL = list(CASES)
NAMES = ("grad_q", "grad_k", "grad_v")


def make(name, zero_col=None, seed=None):
    """-> dict(q, k, v, ml | None, go), CPU fp32.  Planted rows as in test_k3_masked_xattn: row 0 fully blocked (attends everywhere), row 1 fully
    open, where S > 300 row 2 open only in its last 150 keys; the others randn * 3.  zero_col = s: no fully blocked row, and key s is blocked in
    every row instead."""
    B, Q, S, nH, masked = CASES[name]
    return make_shape(B, Q, S, nH, masked, Q + S if seed is None else seed, zero_col=zero_col)


def make_shape(B, Q, S, nH, masked, seed, zero_col=None, blocked_row=None):
    """`make` for any shape (the named cases and the random-shape sweep draw here).  blocked_row: whether row 0 is fully blocked; None = as
    `make` plants it, exactly when no zero_col is given.  The sweep plants both (zero_col with blocked_row=True)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, n, nH, 32, generator=g) for n in (Q, S, S))
    go = torch.randn(B, Q, nH * 32, generator=g)
    ml = None
    if masked:
        ml = torch.randn(B, Q, S, generator=g) * 3
        if zero_col is None if blocked_row is None else blocked_row:
            ml[:, 0] = -5.0
        if Q > 1:
            ml[:, 1] = 5.0
        if S > 300 and Q > 2:
            ml[:, 2, : S - 150] = -5.0
            ml[:, 2, S - 150] = 5.0                    # (at least one key of the open tail really is open)
        if zero_col is not None:
            ml[:, :, zero_col] = -5.0
    return dict(q=q, k=k, v=v, ml=ml, go=go)


def cpu_grads(inp, dtype, go=None):
    q, k, v = (inp[n].to(dtype).clone().requires_grad_(True) for n in ("q", "k", "v"))
    blocked = None if inp["ml"] is None else ref_ops.attn_mask_from_logits(inp["ml"].clone())     # fp32, the kernel's own logits
    go = inp["go"] if go is None else go
    ref_ops.attention_core(q, k, v, blocked).backward(go.to(dtype))
    return q.grad, k.grad, v.grad
