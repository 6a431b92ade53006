"""K15 on the device (rba_grad_sqnorm_f32 + rba_clip_adamw_step_f32 behind rba_amd.solver.ClipAdamW): the case table of tests/_solver_cases.py against the
float64 restatement within the project's bar, bitwise reproducibility, memory safety (the guard bands of tests/_guard.py around every buffer of the feature,
and a parameter carved out of a sentinel-filled buffer), torch's behaviour on non-finite gradients, the version counter, the launch list and a step
that synchronises nothing."""
import contextlib

import pytest
import torch

from tests import _solver_cases as C

pytestmark = pytest.mark.gpu

VIEW_N = C.TENSORS[-1][1][0]


def _margins_untouched(buf):
    return bool((buf[:C.VIEW_OFFSET] == C.SENTINEL).all()) and bool((buf[C.VIEW_OFFSET + VIEW_N:] == C.SENTINEL).all())


@pytest.mark.parametrize("case", C.CASES, ids=C.case_id)
def test_parity_on_the_case_table(case, canary):
    got, opt, buf = C.run_optimizer(case, "cuda")
    t64, b = C.truth(case)
    C.check(C.case_id(case), got, t64, b)
    assert _margins_untouched(buf)
    canary.check()
    g64 = torch.cat([g.double().flatten() for g in C.inputs()[1][case[0] - 1]]) * case[2]
    assert abs(float(opt.grad_norm) - float(g64.norm())) <= 1e-5 * float(g64.norm())
    assert all(torch.equal(q.grad.cpu(), g) for q, g in zip(opt.params, C.inputs()[1][case[0] - 1]))   # .grad keeps the unclipped, unscaled gradient


@pytest.mark.parametrize("chunk", [4, 4096, 16384])
def test_other_chunk_sizes_give_the_same_bits(chunk):
    """the chunk only decides which workgroup steps an element: 4 (every quad its own workgroup), 4096 and the streaming form's 16384 (whole tensors in
    one workgroup's loop) must equal the default's 1024 in every bit"""
    case = (2, 0.01, 0.5)
    want, opt, _ = C.run_optimizer(case, "cuda")
    got, opt2, buf = C.run_optimizer(case, "cuda", chunk=chunk)
    assert opt.plan.chunk == 1024 and opt2.plan.chunk == chunk and opt2.plan.n_blocks != opt.plan.n_blocks
    assert all(torch.equal(a, b) for qa, qb in zip(want, got) for a, b in zip(qa, qb))
    assert _margins_untouched(buf)


def test_two_runs_are_bitwise_equal():
    case = (5, 0.01, 0.5)
    a, opt_a, _ = C.run_optimizer(case, "cuda")
    b, opt_b, _ = C.run_optimizer(case, "cuda")
    assert all(torch.equal(x, y) for qa, qb in zip(a, b) for x, y in zip(qa, qb))
    assert torch.equal(opt_a.stats, opt_b.stats) and torch.equal(opt_a.plan.partials, opt_b.plan.partials)


def test_many_partials_and_a_large_plan(canary):
    """one tensor of 1024 * 4096 + 4100 elements: K15a at its cap of 1024 partials with shares larger than 4096, K15b on the streaming chunk"""
    from rba_amd import ops
    from rba_amd.solver import ClipAdamW
    n = ops.ADAMW_MAX_PARTIALS * ops.ADAMW_SHARE + 4100
    gen = torch.Generator().manual_seed(3)
    p0, g = torch.randn(n, generator=gen), 1e-3 * torch.randn(n, generator=gen)
    q = p0.clone().cuda().requires_grad_(True)
    opt = ClipAdamW([("big", q)], [1.0], [0.05], max_norm=0.01)
    assert opt.plan.n_partials == ops.ADAMW_MAX_PARTIALS and opt.plan.chunk == ops.ADAMW_CHUNK_LARGE
    q.grad.copy_(g)
    opt.step(1e-4)
    canary.check()
    t64 = C.restate64([p0], [[g]], [1e-4], 0.01, 1.0, weight_decays=(0.05,), lr_mults=(1.0,))
    t32 = C.torch32([p0], [[g]], [1e-4], 0.01, 1.0, weight_decays=(0.05,), lr_mults=(1.0,))
    got = ([q.detach().cpu()], [opt.exp_avg.cpu()], [opt.exp_avg_sq.cpu()], [q.detach().cpu() - p0])
    C.check("big", got, t64, [[C.err(a, a64) for a, a64 in zip(q32, q64)] for q32, q64 in zip(t32, t64)], names=("big",))
    assert abs(float(opt.grad_norm) - float(g.double().norm())) <= 1e-5 * float(g.double().norm())


def test_a_nan_gradient_poisons_every_parameter():
    """clip_grad_norm_ turns one NaN into a NaN coefficient and torch steps every parameter with it; fminf in the clamp would hide it"""
    got, opt, buf = C.run_optimizer((1, 0.01, 1.0), "cuda", poison=(3, 100, float("nan")))
    assert all(bool(torch.isnan(p).all()) for p in got[0])
    assert bool(torch.isnan(opt.grad_norm).all()) and _margins_untouched(buf)
    # without clipping only the element itself is lost, as in torch
    got, _, _ = C.run_optimizer((1, 0.0, 1.0), "cuda", poison=(3, 100, float("nan")))
    bad = [torch.isnan(p) for p in got[0]]
    assert int(sum(b.sum() for b in bad)) == 1 and bool(bad[3].view(-1)[100])


def test_an_inf_gradient_gives_torchs_pattern():
    """norm = inf, coefficient = 0, inf * 0 = NaN in that element and a zero gradient everywhere else: torch's own result, element for element"""
    poison = (5, 4321, float("inf"))
    got, _, _ = C.run_optimizer((1, 0.01, 1.0), "cuda", poison=poison)
    p0, grads = C.inputs()
    g = [t.clone() for t in grads[0]]
    g[poison[0]].view(-1)[poison[1]] = poison[2]
    want = C.torch32(p0, [g], [C.lr_at(0)], 0.01, 1.0)
    for name, a, w in zip(C.NAMES, got[0], want[0]):
        assert torch.equal(torch.isfinite(a), torch.isfinite(w)), name
    assert int(sum((~torch.isfinite(a)).sum() for a in got[0])) == 1 and not bool(torch.isfinite(got[0][5].view(-1)[4321]))
    finite = [torch.where(torch.isfinite(w), a, torch.zeros_like(a)) for a, w in zip(got[0], want[0])]
    want_finite = [torch.where(torch.isfinite(w), w, torch.zeros_like(w)) for w in want[0]]
    for name, a, w in zip(C.NAMES, finite, want_finite):                     # a zero gradient: weight decay alone, one rounding
        assert float((a - w).abs().max()) <= 2.0 ** -23 * float(w.abs().max()), name


def test_every_stepped_parameter_gets_a_new_version():
    named, _ = C.make_params("cuda")
    from rba_amd.solver import ClipAdamW
    opt = ClipAdamW(named, C.LR_MULTS, C.WEIGHT_DECAYS, max_norm=0.01)
    for (_, q), g in zip(named, C.inputs()[1][0]):
        q.grad.copy_(g)
    before = [q._version for _, q in named]
    opt.step(1e-4)
    assert all(q._version > v for (_, q), v in zip(named, before))


@contextlib.contextmanager
def _recording():
    """tests/test_launch_plans_gpu.py's technique: a stand-in for the ctypes handle that keeps the names of the launches"""
    from rba_amd import _lib

    class Recorder:
        def __init__(self, lib):
            self._lib, self.names = lib, []

        def __getattr__(self, name):
            fn = getattr(self._lib, name)

            def forward(*args):
                self.names.append(name)
                return fn(*args)
            return forward

    rec = Recorder(_lib.load())
    prev, _lib._lib = _lib._lib, rec
    try:
        yield rec.names
    finally:
        _lib._lib = prev


@pytest.mark.no_canary
def test_a_step_is_two_launches_and_synchronises_nothing():
    from rba_amd.solver import ClipAdamW
    named, _ = C.make_params("cuda")
    opt = ClipAdamW(named, C.LR_MULTS, C.WEIGHT_DECAYS, max_norm=0.01)
    for (_, q), g in zip(named, C.inputs()[1][0]):
        q.grad.copy_(g)
    opt.step(C.lr_at(0))                                         # (nothing is built lazily; the recorded step is a second one all the same)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with _recording() as names:
            opt.zero_grad()
            opt.step(C.lr_at(1))
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert names == ["rba_grad_sqnorm_f32", "rba_clip_adamw_step_f32"]
    # the mode is honoured by this build: the same block with a read-back in it raises
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            float(opt.grad_norm)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert float(opt.grad_norm) == 0.0                            # the second step ran on the zeroed buffer


def test_wrappers_refuse_what_the_kernels_cannot_take():
    from rba_amd import ops
    q = torch.zeros(10, device="cuda")
    with pytest.raises(ops.RbaHipError, match="listed twice"):
        ops.adamw_plan([q, q], [1.0, 1.0], [0.0, 0.0])
    with pytest.raises(ops.RbaHipError, match="multiple of 4"):
        ops.adamw_plan([q], [1.0], [0.0], chunk=6)
    with pytest.raises(ops.RbaHipError, match="contiguous"):
        ops.adamw_plan([torch.zeros(4, 4, device="cuda").t()], [1.0], [0.0])
    plan = ops.adamw_plan([q], [1.0], [0.0])
    flat = ops.adamw_flat(plan)
    assert plan.total == 12 and flat.numel() == 12
    with pytest.raises(ops.RbaHipError, match="12 elements"):
        ops.grad_sqnorm(plan, torch.zeros(16, device="cuda"))
    with pytest.raises(ops.RbaHipError, match="16-byte aligned"):
        ops.grad_sqnorm(plan, torch.zeros(16, device="cuda")[1:13])
    with pytest.raises(ops.RbaHipError, match="step >= 1"):
        ops.clip_adamw_step(plan, flat, flat.clone(), flat.clone(), 0, 1e-4)
    plan.params[0] = torch.zeros(10, device="cuda")
    with pytest.raises(ops.RbaHipError, match="moved or resized"):
        ops.clip_adamw_step(plan, flat, flat.clone(), flat.clone(), 1, 1e-4)
