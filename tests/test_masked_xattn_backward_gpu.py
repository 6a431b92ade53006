"""GPU: the backward of the masked cross-attention core K3 (rba_masked_xattn_bwd_f32 through rba_amd.ops and MaskedXattnFunction) against
fp64 CPU autograd through the oracle.

Truth T64 = gradients of oracle.ref_ops.attention_core in double with the blocked set taken in fp32 from the very logits the kernel sees
(tests/_xattn_bwd_cases.py); e(T) = max|T_gpu - T64| / max|T64| per gradient tensor; bar e <= 4 max(b, 2^-20), b = the same metric for the
oracle's fp32 CPU autograd on the same inputs, computed per case and printed.  No case and no element is left out.  The header declares all
three gradients bitwise reproducible (no atomics), so two launches are compared for equality."""
import pytest
import torch

from tests import _xattn_bwd_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


@pytest.fixture(scope="module")
def Fn():
    from rba_amd.modeling.transformer_decoder.mask2former_transformer_decoder import MaskedXattnFunction
    return MaskedXattnFunction


def dev(t):
    return None if t is None else t.cuda().contiguous()


_truth = {}


def truth(name, go=None, key=None, **kw):
    k = (name, key, tuple(sorted(kw.items())))
    if k not in _truth:
        inp = C.make(name, **kw)
        t64 = C.cpu_grads(inp, torch.float64, go)
        b = [C.err(t, r) for t, r in zip(C.cpu_grads(inp, torch.float32, go), t64)]
        _truth[k] = (inp, t64, b)
    return _truth[k]


def check(got, name, what, go=None, key=None, **kw):
    inp, t64, b = truth(name, go, key, **kw)
    for t, r, bi, tn in zip(got, t64, b, C.NAMES):
        assert t.shape == r.shape and t.dtype == torch.float32
        e = C.err(t, r)
        print(f"{what} {name} {tn}: e = {e:.3e} b = {bi:.3e} bar = {C.bar(bi):.3e}")
        assert e <= C.bar(bi), f"{what}, case {name}, {tn}: e = {e:.3e}, b = {bi:.3e}, bar = {C.bar(bi):.3e}"


def run_op(ops, inp, **need):
    return ops.masked_xattn_backward(dev(inp["q"]), dev(inp["k"]), dev(inp["v"]), dev(inp["ml"]), dev(inp["go"]), **need)


def run_autograd(Fn, inp, go=None, need=(True, True, True), reduce_sum=False):
    a = [dev(inp[n]).requires_grad_(r) for n, r in zip(("q", "k", "v"), need)]
    out = Fn.apply(*a, dev(inp["ml"]))
    assert out.grad_fn is not None
    if reduce_sum:
        out.sum().backward()                                    # autograd hands an expanded, stride-0 gradient
    else:
        out.backward(dev(inp["go"] if go is None else go))
    return tuple(t.grad for t in a)


@pytest.mark.parametrize("name", C.ALL)
def test_backward(ops, Fn, name):
    inp = truth(name)[0]
    check(run_op(ops, inp), name, "op")
    if name in ("q37_s301", "self_100", "s512"):
        check(run_autograd(Fn, inp), name, "autograd")


@pytest.mark.parametrize("name,col", [("q16_s77", 70), ("q37_s301", 3), ("s512", 511), ("q37_s1024", 1000)])
def test_blocked_column_gets_exact_zeros(ops, name, col):
    """a key blocked in every row (no fully blocked row in the case): its dk and dv rows are exactly 0.0 -- outputs start NaN-poisoned"""
    inp = truth(name, zero_col=col)[0]
    from oracle import ref_ops
    blocked = ref_ops.attn_mask_from_logits(inp["ml"].clone())
    assert bool(blocked[:, :, col].all()) and not bool((inp["ml"].sigmoid() < 0.5).all(-1).any())
    got = run_op(ops, inp)
    check(got, name, "blocked column", zero_col=col)
    assert bool((got[1][:, col] == 0.0).all()) and bool((got[2][:, col] == 0.0).all())


def test_partial_needs_and_expanded_gradient(ops, Fn):
    name = "q37_s301"
    inp = truth(name)[0]
    full = run_op(ops, inp)
    for i, kw in enumerate(({"need_k": False, "need_v": False}, {"need_q": False, "need_v": False}, {"need_q": False, "need_k": False})):
        got = run_op(ops, inp, **kw)
        assert all((g is None) == (j != i) for j, g in enumerate(got))
        assert torch.equal(got[i], full[i])
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError):
        run_op(ops, inp, need_q=False, need_k=False, need_v=False)
    ones = torch.ones_like(inp["go"])
    g = run_autograd(Fn, inp, reduce_sum=True)
    check(g, name, "out.sum().backward()", go=ones, key="ones")
    for i in range(3):
        need = tuple(j == i for j in range(3))
        got = run_autograd(Fn, inp, go=ones, need=need)
        assert all((t is None) == (j != i) for j, t in enumerate(got)) and torch.equal(got[i], g[i])


@pytest.mark.parametrize("name", ["q130_s301", "self_100", "q37_s1024", "b2_s2048"])
def test_two_launches_are_bit_equal(ops, name):
    inp = truth(name)[0]
    r1, r2 = run_op(ops, inp), run_op(ops, inp)
    assert all(torch.equal(a, b) for a, b in zip(r1, r2))


@pytest.mark.parametrize("name", ["q37_s301", "self_100"])
def test_forward_unchanged(ops, Fn, name):
    inp = C.make(name)
    a = [dev(inp[n]) for n in ("q", "k", "v", "ml")]
    ref = ops.masked_xattn(*a)
    with torch.no_grad():
        assert torch.equal(Fn.apply(*a), ref)
    out = Fn.apply(*a)                                          # nothing requires grad
    assert out.grad_fn is None and torch.equal(out, ref)
    a[1].requires_grad_(True)
    with torch.no_grad():
        out = Fn.apply(*a)
    assert out.grad_fn is None and torch.equal(out, ref)
    assert torch.equal(Fn.apply(*a).detach(), ref)


def test_argument_errors_and_empty_shapes(ops):
    from rba_amd._lib import RbaHipError
    inp = C.make("q16_s77")
    q, k, v, ml, go = (dev(inp[n]) for n in ("q", "k", "v", "ml", "go"))
    with pytest.raises(RbaHipError):
        ops.masked_xattn_backward(q.double(), k, v, ml, go)                               # mixed dtypes
    with pytest.raises(RbaHipError):
        ops.masked_xattn_backward(q, k, v, ml, go.double())
    with pytest.raises(RbaHipError):
        ops.masked_xattn_backward(q, k, v, ml, go[:, :, :-1].contiguous())                # wrong grad_out shape
    with pytest.raises(RbaHipError, match="contiguous"):
        ops.masked_xattn_backward(q, k, v, ml, go[:, :, :1].expand(2, 16, 64))            # right shape, stride 0
    with pytest.raises(RbaHipError):
        ops.masked_xattn_backward(q.cpu(), k, v, ml, go)
    with pytest.raises(RbaHipError):
        ops.masked_xattn_backward(q, k, v[:, :-1].contiguous(), ml, go)                   # k / v mismatch
    with pytest.raises(RbaHipError):
        ops.masked_xattn_backward(q, k, v, ml[:, :, :-1].contiguous(), go)
    gq, gk, gv = ops.masked_xattn_backward(q[:0].contiguous(), k[:0].contiguous(), v[:0].contiguous(), ml[:0].contiguous(), go[:0].contiguous())
    assert gq.shape == (0, 16, 2, 32) and gk.shape == (0, 77, 2, 32) and gv.shape == (0, 77, 2, 32)
    gq, gk, gv = ops.masked_xattn_backward(q[:, :0].contiguous(), k, v, ml[:, :0].contiguous(), go[:, :0].contiguous())
    assert gq.shape == (2, 0, 2, 32) and gk.shape == k.shape and bool((gk == 0).all()) and bool((gv == 0).all())
    torch.cuda.synchronize()
