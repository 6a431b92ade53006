"""K4 backward on the GPU: both gradients of the mask-logit contraction against fp64 CPU autograd of torch.einsum on .double() of the very
inputs, the exact-fp32 decision, reproducibility, the argument contract of the entry point, and the autograd Function.

Bar (the project's gradient convention, tests/test_rba_backward_gpu.py): e(T) = max|T_gpu - T64| / max|T64| per gradient tensor,
e(T) <= 4 max(b(T), 2^-20), b the same metric for fp32 CPU autograd of the same case.  No case and no element is left out.  Every test runs
under the guard-banded, NaN-poisoned allocations of tests/_guard.py: outputs and the workspace come from torch.empty inside rba_amd.ops.
"""
import pytest
import torch

from tests import _k4_bwd_cases as C

pytestmark = pytest.mark.gpu


def _dev(*ts):
    return [t.cuda().contiguous() for t in ts]


def _launch(name, scale=None, **kw):
    from rba_amd import ops
    E, Fm, G = _dev(*C.case_inputs(name))
    if scale is not None:
        G = G * scale
    return ops.mask_logits_backward(E, Fm, G, **kw)


@pytest.mark.parametrize("name", C.NAMES)
def test_kernel_meets_the_bar(name):
    _, B, Q, Cd, N = C.CASE[name]
    ge64, gf64, b_embed, b_feat = C.case_truth(name)
    ge, gf = _launch(name)
    assert tuple(ge.shape) == (B, Q, Cd) and tuple(gf.shape) == (B, Cd, N)
    C.check(f"{name} grad_embed", ge.cpu(), ge64, b_embed)
    C.check(f"{name} grad_feat", gf.cpu(), gf64, b_feat)


@pytest.mark.parametrize("name", ["tail", "odd"])
def test_power_of_two_scaling_is_exact(name):
    """On the fp32 path a power-of-two factor on G commutes with every product and sum (nothing here nears the subnormals: |G| ~ 1e-3 * 2^-40
    ~ 1e-15), so the results scale bit for bit.  Any f16-split arithmetic loses G at this size: this test holds the exact-fp32 decision."""
    s = 2.0 ** -40
    ge, gf = _launch(name)
    ge_s, gf_s = _launch(name, scale=s)
    assert float(ge.abs().max()) > 0 and float(gf.abs().max()) > 0
    assert torch.equal(ge_s, ge * s) and torch.equal(gf_s, gf * s)


@pytest.mark.parametrize("name", ["crop", "oddc"])
def test_bitwise_reproducible(name):
    runs = [_launch(name) for _ in range(3)]
    for ge, gf in runs[1:]:
        assert torch.equal(ge, runs[0][0]) and torch.equal(gf, runs[0][1])


@pytest.mark.parametrize("name", ["batch", "oddc"])
def test_null_outputs(name):
    from rba_amd import _lib, ops
    ge, gf = _launch(name)
    none, gf_only = _launch(name, need_embed=False)
    ge_only, none2 = _launch(name, need_feat=False)
    assert none is None and none2 is None
    assert torch.equal(gf_only, gf) and torch.equal(ge_only, ge)
    with pytest.raises(ops.RbaHipError):
        _launch(name, need_embed=False, need_feat=False)
    # the operand a gradient does not read may be absent: at the wrapper (None) and at the raw entry point (NULL)
    E, Fm, G = _dev(*C.case_inputs(name))
    assert torch.equal(ops.mask_logits_backward(None, Fm, G, need_feat=False)[0], ge)
    assert torch.equal(ops.mask_logits_backward(E, None, G, need_embed=False)[1], gf)
    _, B, Q, Cd, N = C.CASE[name]
    lib = _lib.load()
    out, ws = torch.full((B, Q, Cd), float("nan"), device="cuda"), torch.empty(1 << 20, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.rba_mask_logits_bwd_f32(0, Fm.data_ptr(), G.data_ptr(), out.data_ptr(), 0, B, Q, Cd, N, ws.data_ptr(), ws.numel() * 4, st) == 0
    assert torch.equal(out, ge)


def test_argument_errors():
    """hipErrorInvalidValue from the entry point, without a launch: both outputs NULL, a NULL input that would be read, grad_embed with a NULL or
    too small workspace, negative sizes.  B = 0 and N = 0 return 0 and touch nothing."""
    import ctypes
    from rba_amd import _lib
    lib = _lib.load()
    B, Q, Cd, N = 2, 5, 8, 12
    dev = "cuda"
    E, Fm, G = torch.zeros(B, Q, Cd, device=dev), torch.zeros(B, Cd, N, device=dev), torch.zeros(B, Q, N, device=dev)
    ge, gf = torch.full((B, Q, Cd), 7.0, device=dev), torch.full((B, Cd, N), 7.0, device=dev)
    n = ctypes.c_int64(-1)
    assert lib.rba_mask_logits_bwd_workspace_f32(B, Q, Cd, N, ctypes.addressof(n)) == 0 and n.value >= B * Q * Cd * 4
    ws = torch.empty(n.value // 4, device=dev)
    ok = (E.data_ptr(), Fm.data_ptr(), G.data_ptr(), ge.data_ptr(), gf.data_ptr(), B, Q, Cd, N, ws.data_ptr(), n.value, 0)
    bad = {"no output": ok[:3] + (0, 0) + ok[5:], "null grad_out": ok[:2] + (0,) + ok[3:], "null feat for grad_embed": ok[:1] + (0,) + ok[2:],
           "null embed for grad_feat": (0,) + ok[1:], "grad_embed without workspace": ok[:9] + (0, n.value, 0),
           "workspace too small": ok[:10] + (n.value - 1, 0), "negative B": ok[:5] + (-1,) + ok[6:], "negative Q": ok[:6] + (-1,) + ok[7:],
           "C = 0": ok[:7] + (0,) + ok[8:], "negative N": ok[:8] + (-1,) + ok[9:], "B > 65535": ok[:5] + (65536,) + ok[6:]}
    for what, a in bad.items():
        assert lib.rba_mask_logits_bwd_f32(*a) == 1, what
    assert lib.rba_mask_logits_bwd_workspace_f32(B, Q, Cd, -1, ctypes.addressof(n)) == 1
    assert lib.rba_mask_logits_bwd_workspace_f32(B, Q, Cd, N, 0) == 1
    for what, a in {"B = 0": ok[:5] + (0,) + ok[6:], "N = 0": ok[:8] + (0,) + ok[9:]}.items():
        assert lib.rba_mask_logits_bwd_f32(*a) == 0, what
    torch.cuda.synchronize()
    assert bool((ge == 7.0).all()) and bool((gf == 7.0).all())
    assert lib.rba_mask_logits_bwd_f32(*ok) == 0                 # and the valid call writes every element (zeros here)
    torch.cuda.synchronize()
    assert bool((ge == 0).all()) and bool((gf == 0).all())


# ---- the autograd Function

def _batch4():
    E, Fm, G = C.case_inputs("batch")
    return E, Fm.view(2, 256, 32, 64), G.view(2, 100, 32, 64)


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_function_forward_is_mask_logits(mode):
    from rba_amd import ops
    from rba_amd.modeling.transformer_decoder.mask2former_transformer_decoder import MaskLogitsFunction
    E, Fm, _ = _dev(*_batch4())
    with ops.split_mode(mode):
        out = MaskLogitsFunction.apply(E, Fm)
        assert tuple(out.shape) == (2, 100, 32, 64)
        assert torch.equal(out, ops.mask_logits(E, Fm))


@pytest.mark.parametrize("need", [(True, True), (True, False), (False, True)])
def test_function_backward(need):
    """B = 2, a different image per batch entry; needs_input_grad honoured"""
    from rba_amd.modeling.transformer_decoder.mask2former_transformer_decoder import MaskLogitsFunction
    E, Fm, G = _dev(*_batch4())
    E.requires_grad_(need[0])
    Fm.requires_grad_(need[1])
    (MaskLogitsFunction.apply(E, Fm) * G).sum().backward()
    assert (E.grad is not None) == need[0] and (Fm.grad is not None) == need[1]
    ge64, gf64, b_embed, b_feat = C.case_truth("batch")
    if need[0]:
        C.check("batch grad_embed", E.grad.cpu(), ge64, b_embed)
    if need[1]:
        C.check("batch grad_feat", Fm.grad.cpu().view(2, 256, 2048), gf64, b_feat)
