"""GPU: the backward pass of multi-scale deformable attention (rba_ms_deform_attn_bwd_f32 / _f64 through rba_amd.ops, the autograd
Function and the `differentiable` path of the MSDeformAttn module) against fp64 CPU autograd through the oracle.

Truth T64 = gradients of oracle.ref_ops.ms_deform_attn in double on `.double()` of the very inputs the kernel sees; metric per gradient
tensor e(T) = max|T_gpu - T64| / max|T64|.  Bars (tests/_msda_cases.py):
  fp32: e(T) <= 4 max(b(T), 2^-20), b(T) = the same metric for the oracle's own fp32 CPU autograd on the same inputs, computed here per case
        (both are fp32 sums of the same terms in another order; a wrong sign, a missing tap or a lost atomic shows at 1e-2 and above);
  fp64: e(T) <= 1e-10;
  entries of grad_sampling_loc / grad_attn_weight of samples outside the window: exactly 0.0 (outputs start NaN-poisoned under the canary).
Inputs keep every pixel coordinate >= 1e-3 away from an integer (the gradient of bilinear sampling jumps there); no sample and no case is
left out."""

import pytest
import torch

from oracle import ref_model
from tests import _msda_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


@pytest.fixture(scope="module")
def Fn():
    from rba_amd.modeling.pixel_decoder.ops.ms_deform_attn import MSDeformAttnFunction
    return MSDeformAttnFunction


def dev(t):
    return t.cuda().contiguous()


def gpu_args(inp):
    return [dev(inp[k]) for k in ("value", "shapes", "lsi", "loc", "w")]


_truth = {}


def truth(name, dtype, go=None, key=None):
    """(inputs, T64 grads, b per tensor | None) -- cached per case: several tests compare against the same truth"""
    k = (name, dtype, key)
    if k not in _truth:
        inp = C.make(name, dtype)
        t64 = C.cpu_grads(inp, torch.float64, go)
        b = [C.err(t, r) for t, r in zip(C.cpu_grads(inp, torch.float32, go), t64)] if dtype == torch.float32 else None
        _truth[k] = (inp, t64, b)
    return _truth[k]


def check(got, name, dtype, what, go=None, key=None):
    inp, t64, b = truth(name, dtype, go, key)
    out = C.outside(inp["loc"], inp["shape_list"])
    for i, (t, r, tn) in enumerate(zip(got, t64, C.NAMES)):
        assert t.shape == r.shape and t.dtype == dtype
        e = C.err(t, r)
        lim = C.FP64_BAR if dtype == torch.float64 else C.bar(b[i])
        print(f"{what} {name} {tn}: e = {e:.3e}" + (f" b = {b[i]:.3e}" if b else "") + f" bar = {lim:.3e}")
        assert e <= lim, f"{what}, case {name}, {tn}: e = {e:.3e}, b = {b[i] if b else None}, bar = {lim:.3e}"
    assert bool((got[1].cpu()[out] == 0.0).all()) and bool((got[2].cpu()[out] == 0.0).all()), \
        f"{what}, case {name}: gradients of out-of-window samples must be exactly 0"


def run_op(ops, inp):
    return ops.ms_deform_attn_backward(*gpu_args(inp), dev(inp["go"]))


def run_autograd(Fn, inp, go=None, need=(True, True, True)):
    a = gpu_args(inp)
    for i, n in zip((0, 3, 4), need):
        a[i].requires_grad_(n)
    out = Fn.apply(*a)
    assert out.grad_fn is not None
    out.backward(dev(inp["go"] if go is None else go))
    return a[0].grad, a[3].grad, a[4].grad


# ---- 1, 2, 3, 4, 5: every case through the op; the marked ones also end to end through the autograd Function
@pytest.mark.parametrize("name", C.FP32_CASES)
def test_backward_fp32(ops, Fn, name):
    inp = truth(name, torch.float32)[0]
    check(run_op(ops, inp), name, torch.float32, "op")
    if name in ("ref_tiny", "model_L3", "model_L1"):
        check(run_autograd(Fn, inp), name, torch.float32, "autograd")


@pytest.mark.parametrize("name", C.FP64_CASES)
def test_backward_fp64(ops, Fn, name):
    inp = truth(name, torch.float64)[0]
    check(run_op(ops, inp), name, torch.float64, "op")
    if name == "ref_tiny":
        check(run_autograd(Fn, inp), name, torch.float64, "autograd")


@pytest.mark.parametrize("name", ["model_L3", "model_L1", "encoder_like", "same_loc_4096"])
def test_backward_generic_form_on_model_shapes(ops, knobs, name):
    """the knobs build forcing the generic kernel where the product dispatches the model form: both forms meet the truth"""
    from rba_amd import _lib
    inp = truth(name, torch.float32)[0]
    knob = _lib.knob("rba_k2_bwd_variant")
    check(run_op(ops, inp), name, torch.float32, "knobs build, dispatch")
    knob.value = 1
    try:
        check(run_op(ops, inp), name, torch.float32, "knobs build, generic")
    finally:
        knob.value = 0


# ---- 6
def test_all_samples_outside_and_empty_shapes(ops):
    inp = C.make("all_outside", torch.float32)
    assert bool(C.outside(inp["loc"], inp["shape_list"]).all())
    gv, gl, ga = run_op(ops, inp)
    assert bool((gv == 0).all()) and bool((gl == 0).all()) and bool((ga == 0).all())
    N, S, M, D = inp["value"].shape
    L, P = len(inp["shape_list"]), 4
    a = gpu_args(inp)
    gv, gl, ga = ops.ms_deform_attn_backward(a[0], a[1], a[2], a[3][:, :0].contiguous(), a[4][:, :0].contiguous(),
                                             torch.empty(N, 0, M * D, device="cuda"))
    assert gv.shape == (N, S, M, D) and bool((gv == 0).all()) and gl.shape == (N, 0, M, L, P, 2) and ga.shape == (N, 0, M, L, P)
    gv, gl, ga = ops.ms_deform_attn_backward(a[0][:0].contiguous(), a[1], a[2], a[3][:0].contiguous(), a[4][:0].contiguous(),
                                             torch.empty(0, 64, M * D, device="cuda"))
    assert gv.shape == (0, S, M, D) and gl.shape == (0, 64, M, L, P, 2) and ga.shape == (0, 64, M, L, P)


# ---- 7
def test_autograd_expanded_gradient_partial_requires_grad_and_second_order(Fn):
    name = "model_L3"
    inp = C.make(name, torch.float32)
    ones = torch.ones_like(inp["go"])
    a = gpu_args(inp)
    for i in (0, 3, 4):
        a[i].requires_grad_(True)
    Fn.apply(*a).sum().backward()                               # autograd hands an expanded, stride-0 gradient
    full = (a[0].grad, a[3].grad, a[4].grad)
    check(full, name, torch.float32, "out.sum().backward()", go=ones, key="ones")
    gv, gl, ga = run_autograd(Fn, inp, go=ones, need=(True, False, False))
    assert gl is None and ga is None
    check((gv, full[1], full[2]), name, torch.float32, "only value requires grad", go=ones, key="ones")
    gv, gl, ga = run_autograd(Fn, inp, go=ones, need=(False, True, False))
    assert gv is None and ga is None and torch.equal(gl, full[1])
    gv, gl, ga = run_autograd(Fn, inp, go=ones, need=(False, True, True))
    assert gv is None and torch.equal(gl, full[1]) and torch.equal(ga, full[2])
    b = gpu_args(inp)
    b[0].requires_grad_(True)
    (g1,) = torch.autograd.grad(Fn.apply(*b).sum(), b[0], create_graph=True)
    with pytest.raises(RuntimeError):                           # a constant incoming gradient: the first-order result carries no graph at all
        g1.sum().backward()
    out = Fn.apply(*b)
    (g1,) = torch.autograd.grad((out * out).sum(), b[0], create_graph=True)     # the incoming gradient 2 out itself requires grad
    with pytest.raises(RuntimeError, match="once_differentiable"):
        g1.sum().backward()


# ---- 8
@pytest.mark.parametrize("name", ["model_L3", "encoder_like", "D71"])
def test_two_launches_deterministic_outputs_are_equal(ops, name):
    inp = truth(name, torch.float32)[0]
    r1, r2 = run_op(ops, inp), run_op(ops, inp)
    assert torch.equal(r1[1], r2[1]) and torch.equal(r1[2], r2[2])
    check(r1, name, torch.float32, "launch 1")
    check(r2, name, torch.float32, "launch 2")


# ---- 9
@pytest.mark.no_canary
@pytest.mark.parametrize("D", [4, 30, 32, 71])
def test_gradcheck_double(Fn, D):
    """the reference's own criterion (ops/test.py:66-89: gradcheck with default eps / atol / rtol) on the tiny geometry.
    nondet_tol: fp64 atomics may reorder <= 64 adds of magnitude <= 1, <= 1e-14."""
    N, M, Lq, L, P = 1, 2, 2, 2, 2
    g = torch.Generator().manual_seed(D)
    sh = torch.tensor(C.TINY, dtype=torch.int64)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    S = int(sh.prod(1).sum())
    value = (torch.rand(N, S, M, D, generator=g, dtype=torch.float64) * 0.01)
    loc = C.nudge(torch.rand(N, Lq, M, L, P, 2, generator=g, dtype=torch.float64), C.TINY)
    assert C.condition(loc, C.TINY)
    w = torch.rand(N, Lq, M, L, P, generator=g, dtype=torch.float64) + 1e-5
    w = w / w.sum((-1, -2), keepdim=True)
    v, l, a = (dev(t).requires_grad_(True) for t in (value, loc, w))
    assert torch.autograd.gradcheck(lambda v_, l_, a_: Fn.apply(v_, dev(sh), dev(lsi), l_, a_, 2), (v, l, a), nondet_tol=1e-12)


# ---- 10
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_forward_unchanged_under_no_grad(ops, Fn, dtype):
    inp = C.make("model_L3" if dtype == torch.float32 else "D30", dtype)
    a = gpu_args(inp)
    ref = ops.ms_deform_attn_forward(*a)
    with torch.no_grad():
        assert torch.equal(Fn.apply(*a), ref) and torch.equal(Fn.apply(*a, 128), ref)
    out = Fn.apply(*a)                                          # nothing requires grad
    assert out.grad_fn is None and torch.equal(out, ref)
    a[0].requires_grad_(True)
    assert torch.equal(Fn.apply(*a).detach(), ref)


# ---- 11
def test_backward_argument_errors(ops):
    from rba_amd._lib import RbaHipError
    inp = C.make("D30", torch.float32)
    v, sh, lsi, loc, w = gpu_args(inp)
    go = dev(inp["go"])
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_backward(v.double(), sh, lsi, loc, w, go)                 # mixed dtypes
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_backward(v, sh, lsi, loc, w, go.double())
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_backward(v, sh, lsi, loc, w, go[:, :, :-1].contiguous())  # wrong grad_output shape
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_backward(v, sh, lsi, loc, w, go.view(1, 37, 3, 30))
    with pytest.raises(RbaHipError, match="contiguous"):
        ops.ms_deform_attn_backward(v, sh, lsi, loc, w, go[:, :, :1].expand(1, 37, 90))  # right shape, stride 0
    with pytest.raises(RbaHipError, match="contiguous"):
        ops.ms_deform_attn_backward(v, sh, lsi, loc.transpose(1, 2).contiguous().transpose(1, 2), w, go)
    v3, loc3, w3, go3 = (t.repeat(3, *([1] * (t.dim() - 1))) for t in (v, loc, w, go))
    with pytest.raises(RbaHipError, match="im2col_step"):
        ops.ms_deform_attn_backward(v3, sh, lsi, loc3, w3, go3, im2col_step=2)       # 3 % 2 != 0
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_backward(v.cpu(), sh, lsi, loc, w, go)


# ---- 12, 13
def _module_problem(dtype=torch.float32):
    """MSDeformAttn(256, 3, 8, 4) with seeded weights; `query` a tensor of its own.  The sampling offsets depend on the query only, so the
    reference points are DRAWN (vectorised rejection: first of 32 candidates per (n, q, level, axis)) such that every pixel coordinate of every
    sample keeps 4e-3 from an integer in double; the test then asserts 1e-3 on the fp32 evaluation of the same expressions."""
    from rba_amd.modeling.pixel_decoder.ops.ms_deform_attn import MSDeformAttn
    N, Lq, C_, M, L, P = 2, 200, 256, 8, 3, 4
    shapes = C.MODEL_L3
    torch.manual_seed(11)
    mod = MSDeformAttn(C_, L, M, P)
    sd = {"m." + k: v.detach().clone() for k, v in mod.state_dict().items()}
    g = torch.Generator().manual_seed(12)
    S = sum(h * w for h, w in shapes)
    query = torch.randn(N, Lq, C_, generator=g)
    src = torch.randn(N, S, C_, generator=g)
    go = torch.randn(N, Lq, C_, generator=g)
    off = torch.nn.functional.linear(query.double(), sd["m.sampling_offsets.weight"].double(), sd["m.sampling_offsets.bias"].double())
    off = off.view(N, Lq, M, L, P, 2)                                                    # in pixels
    wh = torch.tensor(shapes, dtype=torch.float64).flip(-1)                              # [L, 2] = (W, H)
    cand = torch.rand(N, Lq, L, 2, 32, generator=g, dtype=torch.float64)
    pix = cand[:, :, None, :, None] * wh[None, None, None, :, None, :, None] + off[..., None] - 0.5      # [N,Lq,M,L,P,2,32]
    ok = ((pix - pix.round()).abs() >= 4 * C.MARGIN).all(2).all(3)                       # [N,Lq,L,2,32]
    assert bool(ok.any(-1).all())
    first = ok.float().argmax(-1, keepdim=True)
    ref = cand.gather(-1, first).squeeze(-1).float()                                     # [N,Lq,L,2]
    sh = torch.tensor(shapes, dtype=torch.int64)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    for dt in (torch.float32, torch.float64):
        o = torch.nn.functional.linear(query.to(dt), sd["m.sampling_offsets.weight"].to(dt), sd["m.sampling_offsets.bias"].to(dt)).view(N, Lq, M, L, P, 2)
        loc = ref.to(dt)[:, :, None, :, None, :] + o / wh.to(dt)[None, None, None, :, None, :]
        assert C.condition(loc, shapes), "module test inputs: a pixel coordinate within 1e-3 of an integer"
    return mod, sd, query, ref, src, sh, lsi, go, (N, Lq, C_, M, L, P, S)


def _oracle_module_grads(sd, query, ref, src, sh, lsi, go, dims, dtype):
    N, Lq, C_, M, L, P, S = dims
    sdd = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    q, s = query.to(dtype).clone().requires_grad_(True), src.to(dtype).clone().requires_grad_(True)
    ref_model.ms_deform_attn_module(q, ref.to(dtype), s, sh, lsi, sdd, "m", M, L, P).backward(go.to(dtype))
    out = {k[2:]: v.grad for k, v in sdd.items()}
    out["query"], out["input_flatten"] = q.grad, s.grad
    return out


def test_module_differentiable_path(ops):
    mod, sd, query, ref, src, sh, lsi, go, dims = _module_problem()
    t64 = _oracle_module_grads(sd, query, ref, src, sh, lsi, go, dims, torch.float64)
    c32 = _oracle_module_grads(sd, query, ref, src, sh, lsi, go, dims, torch.float32)
    assert len(t64) == 10
    touched = t64["input_flatten"].abs().amax(-1) > 0              # [N, S]: pixels that any sample reaches
    mod = mod.cuda()
    mod.differentiable = True
    q, s = dev(query).requires_grad_(True), dev(src).requires_grad_(True)
    tf32 = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    try:
        out = mod(q, dev(ref), s, dev(sh), dev(lsi))
        assert out.grad_fn is not None
        out.backward(dev(go))
        got = {k: p.grad for k, p in mod.named_parameters()}
        got["query"], got["input_flatten"] = q.grad, s.grad
        for k in sorted(t64):
            e, b = C.err(got[k], t64[k]), C.err(c32[k], t64[k])
            print(f"module {k}: e = {e:.3e} b = {b:.3e} bar = {C.bar(b):.3e}")
            assert e <= C.bar(b), f"module, {k}: e = {e:.3e}, b = {b:.3e}, bar = {C.bar(b):.3e}"
        # the padding mask by property: masked positions of input_flatten receive exactly no gradient, the others do
        N, Lq, C_, M, L, P, S = dims
        mask = torch.zeros(N, S, dtype=torch.bool)
        mask[:, [130, 500, 950, 1200]] = True
        assert bool(touched[mask].all()) and float(touched.float().mean()) > 0.9
        q2, s2 = dev(query).requires_grad_(True), dev(src).requires_grad_(True)
        mod(q2, dev(ref), s2, dev(sh), dev(lsi), dev(mask)).backward(dev(go))
        g = s2.grad.cpu()
        assert bool((g[mask] == 0).all()) and torch.equal(g.abs().amax(-1) > 0, touched & ~mask)
    finally:
        torch.backends.cuda.matmul.allow_tf32 = tf32


def test_module_default_path_untouched(ops):
    """the switch is the attribute alone: a fresh module (training mode, parameters requiring grad) with grad mode on takes the fused inference path"""
    mod, sd, query, ref, src, sh, lsi, go, dims = _module_problem()
    mod = mod.cuda()
    assert mod.training and mod.differentiable is False and all(p.requires_grad for p in mod.parameters())
    a = (dev(query), dev(ref), dev(src), dev(sh), dev(lsi))
    with torch.no_grad():
        want = mod(*a)
    out = mod(*a)
    assert torch.equal(out, want)
    mod.differentiable = True
    with torch.no_grad():
        assert torch.equal(mod(*a), want)                           # differentiable, but grad mode off: still the inference path
