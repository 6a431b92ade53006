"""GPU: a boundary list and seeded random shapes through the training kernels whose launch FORM depends on the shape -- K1 backward in its three
score modes and its per-class adjoint, K4 / K3 / K2 backward, K8's matching cost -- and a size-pair sweep of the align-corners taps of K9, K10, K11a
and K11b: every (in, out) of [1, 40]^2 and a list of large pairs, each on the row axis and on the column axis (tests/_train_fuzz_cases.py; the CPU
test of the generators is tests/test_training_kernel_fuzz_cpu.py).

Truth, metric and bar are each family's own: fp64 CPU autograd of its torch restatement on .double() of the very inputs; e(T) = max|T - T64| /
max|T64| per tensor (T64 == 0: exactly 0); e <= 4 max(b, 2^-20) with b the same metric for fp32 CPU autograd, computed per draw and printed with
e; scalars by _point_loss_cases.check_scalar; counts exact.  No draw and no element is left out.

Stale workspaces: every draw runs twice, first with every floating-point buffer of ops._STREAM_WORKSPACES filled with NaN, then with 3.0e38 (the
int32 "tiles" kind is K1's counter and stays zero).  Both runs meet the bar and are bit-equal wherever include/rba_hip.h declares the output
bitwise reproducible -- everything here but K2's grad_value.  A family's draws run in a seeded shuffled order, so small shapes follow large ones
on the grown buffer, and each family with a stream workspace (K1, K4, K8, K9 - K11) asserts that at least one of its draws reused a buffer larger
than it needed.  K3 and K2 backward keep no stream workspace (K3's scratch is allocated per call, NaN-poisoned by tests/_guard.py): they run twice
for the bit-equality alone.

One stated condition beyond the generators' own: in the pair sweep "a source pixel nobody samples is exactly 0 on the device" is asked where
neither reference names the pixel.  At (in, out) = (27, 12), (32, 8) and (32, 15) fp32 ATen itself names one source row more than fp64 ATen (the
floor of scale * dst is taken one ulp below in - 1); the kernels restate fp32 ATen, and that row is held by the bar like every other element
(`_train_fuzz_cases.AC_FP32_NAMES_MORE`, asserted exhaustive by the CPU test).
"""
import ctypes

import pytest
import torch

from tests import _dense_hybrid_cases as D
from tests import _msda_cases as M2
from tests import _pebal_cases as G
from tests import _point_loss_cases as P
from tests import _train_fuzz_cases as T
from tests import _xattn_bwd_cases as X

pytestmark = pytest.mark.gpu

WHICH = ("boundary",) + T.SEEDS


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


def dev(t):
    return None if t is None else t.cuda().contiguous()


def _fill(ops, value):
    for (_, _, kind), buf in ops._STREAM_WORKSPACES.items():
        if kind != "tiles" and buf.is_floating_point():
            buf.fill_(value)


def _twice(ops, run):
    """`run` on NaN-filled, then on 3.0e38-filled workspaces"""
    _fill(ops, T.NAN)
    first = run()
    _fill(ops, T.HUGE)
    return first, run()


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        assert (x is None and y is None) or torch.equal(x, y), f"{what}: the NaN-filled and the 3.0e38-filled run differ"


class Reuse:
    """did a draw run on a stream workspace that was already there and larger than the draw needs?"""

    def __init__(self, ops):
        self.ops, self.seen = ops, set()

    def _buffer(self, kind):
        found = [b for (_, _, k), b in self.ops._STREAM_WORKSPACES.items() if k == kind]
        return found[0] if len(found) == 1 else None

    def before(self, kind):
        b = self._buffer(kind)
        return None if b is None else (b.data_ptr(), b.numel())

    def after(self, kind, was, query, *dims):
        n = ctypes.c_int64(0)
        assert self.ops._query(query, *dims, ctypes.addressof(n)) == 0
        b = self._buffer(kind)
        if was is not None and b is not None and was == (b.data_ptr(), b.numel()) and b.numel() > max(n.value // 4, 1):
            self.seen.add(kind)


# ---------------------------------------------------------------------------------------------------------------- 1. K1 backward, the per-class adjoint
@pytest.mark.parametrize("which", WHICH)
def test_k1_backward_and_per_class_adjoint(ops, which):
    reuse = Reuse(ops)
    if which != "boundary":                                               # a large draw first: the seed's own draws then run on a grown buffer
        ops.rba_reduce_backward(torch.zeros(200, 1, 600, device="cuda"), torch.zeros(200, 100, device="cuda"), torch.zeros(1, 600, device="cuda"))
    for d in T.shuffled(T.k1_draws(which), 7):
        Q, K, HW = d
        mask, prob, g, gsem = (dev(t) for t in T.k1_inputs(d))
        m3 = mask.view(Q, 1, HW)
        T.count_draw("K1 backward")
        for what in ("rba", "energy", "neg_logit_sum", "sem_seg"):
            gm64, gp64, b_mask, b_prob = T.k1_truth(d, what)
            if what == "sem_seg":
                run = lambda **kw: ops.sem_seg_backward(m3, prob, gsem.view(K, 1, HW), **kw)
            else:
                run = lambda **kw: ops.rba_reduce_backward(m3, prob, g.view(1, HW), score=what, **kw)
            was = reuse.before("grad_prob")
            r1, r2 = _twice(ops, run)
            reuse.after("grad_prob", was, "rba_reduce_bwd_workspace_f32", Q, K, HW)
            for r in (r1, r2):
                assert tuple(r[0].shape) == (Q, 1, HW) and tuple(r[1].shape) == (Q, K)
                T.check("K1 backward", f"{d} {what} grad_mask", r[0].view(Q, HW), gm64, b_mask)
                T.check("K1 backward", f"{d} {what} grad_prob", r[1], gp64, b_prob)
            _same_bits(r1, r2, f"K1 backward {d} {what}")
            _fill(ops, T.HUGE)
            assert torch.equal(run(need_mask=False)[1], r1[1])
    T.report("K1 backward")
    assert "grad_prob" in reuse.seen, "no draw reused a workspace larger than it needed"


# ---------------------------------------------------------------------------------------------------------------- 2. K4 backward
@pytest.mark.parametrize("which", WHICH)
def test_k4_backward(ops, which):
    reuse = Reuse(ops)
    if which != "boundary":
        ops.mask_logits_backward(torch.zeros(2, 200, 300, device="cuda"), torch.zeros(2, 300, 4000, device="cuda"), torch.zeros(2, 200, 4000, device="cuda"))
    for d in T.shuffled(T.k4_draws(which), 8):
        E, Fm, Gm = (dev(t) for t in T.k4_inputs(d))
        ge64, gf64, b_embed, b_feat = T.k4_truth(d)
        T.count_draw("K4 backward")
        was = reuse.before("grad_embed")
        r1, r2 = _twice(ops, lambda: ops.mask_logits_backward(E, Fm, Gm))
        reuse.after("grad_embed", was, "rba_mask_logits_bwd_workspace_f32", *d)
        for r in (r1, r2):
            T.check("K4 backward", f"{d} grad_embed", r[0], ge64, b_embed)
            T.check("K4 backward", f"{d} grad_feat", r[1], gf64, b_feat)
        _same_bits(r1, r2, f"K4 backward {d}")
        a1, a2 = _twice(ops, lambda: (ops.mask_logits_backward(None, Fm, Gm, need_feat=False)[0], ops.mask_logits_backward(E, None, Gm, need_embed=False)[1]))
        _same_bits(a1, r1, f"K4 backward {d}, each gradient alone")
        _same_bits(a2, r1, f"K4 backward {d}, each gradient alone")
    T.report("K4 backward")
    assert "grad_embed" in reuse.seen, "no draw reused a workspace larger than it needed"


# ---------------------------------------------------------------------------------------------------------------- 3. K3 backward
@pytest.mark.parametrize("which", WHICH)
def test_k3_backward(ops, which):
    for d in T.shuffled(T.k3_draws(which), 9):
        inp = T.k3_inputs(d)
        t64, b = T.k3_truth(d)
        a = [dev(inp[n]) for n in ("q", "k", "v", "ml", "go")]
        T.count_draw("K3 backward")
        r1, r2 = _twice(ops, lambda: ops.masked_xattn_backward(*a))
        for r in (r1, r2):
            for t, t64_i, bi, name in zip(r, t64, b, X.NAMES):
                assert t.dtype == torch.float32
                T.check("K3 backward", f"{d} {name}", t, t64_i, bi)
                assert (name in T.k3_zero_truth(d)) == (float(t64_i.abs().max()) == 0.0)
        _same_bits(r1, r2, f"K3 backward {d}")
    T.report("K3 backward")


# ---------------------------------------------------------------------------------------------------------------- 4. K2 backward
@pytest.mark.parametrize("which", WHICH)
def test_k2_backward(ops, which):
    for d in T.shuffled(T.k2_draws(which), 10):
        inp = T.k2_inputs(d)
        t64, b = T.k2_truth(d)
        a = [dev(inp[k]) for k in ("value", "shapes", "lsi", "loc", "w", "go")]
        out = M2.outside(inp["loc"], inp["shape_list"])
        T.count_draw("K2 backward")
        r1, r2 = _twice(ops, lambda: ops.ms_deform_attn_backward(*a))
        for r in (r1, r2):
            for t, t64_i, bi, name in zip(r, t64, b, M2.NAMES):
                T.check("K2 backward", f"{d} {name}", t, t64_i, bi)
            assert bool((r[1].cpu()[out] == 0.0).all()) and bool((r[2].cpu()[out] == 0.0).all())
        _same_bits(r1[1:], r2[1:], f"K2 backward {d}")                    # grad_value is summed with atomics: no bit-equality claim
    T.report("K2 backward")


# ---------------------------------------------------------------------------------------------------------------- 5. K8: the matching cost
@pytest.mark.parametrize("which", WHICH)
def test_k8_match_cost(ops, which):
    reuse = Reuse(ops)
    wm, wc, wd = P.COST_WEIGHTS
    if which != "boundary":
        ops.match_cost(torch.zeros(120, 4, 4, device="cuda"), torch.zeros(80, 4, 4, device="cuda"), torch.zeros(400, 2, device="cuda"),
                       torch.full((120, 2), 0.5, device="cuda"), torch.zeros(80, dtype=torch.int64, device="cuda"))
    for d in T.shuffled(T.k8_draws(which), 11):
        pred, tgt, coords, logits, ids = T.k8_inputs(d)
        c64, b = T.k8_truth(d)
        a = [dev(t) for t in (pred, tgt, coords, logits.softmax(-1), ids)]
        T.count_draw("K8 match_cost")
        was = reuse.before("match_cost")
        r1, r2 = _twice(ops, lambda: (ops.match_cost(*a, cost_mask=wm, cost_class=wc, cost_dice=wd),))
        reuse.after("match_cost", was, "rba_match_cost_workspace_f32", *d)
        for r in (r1, r2):
            T.check("K8 match_cost", f"{d} cost", r[0], c64, b)
        _same_bits(r1, r2, f"K8 {d}")
    T.report("K8 match_cost")
    assert "match_cost" in reuse.seen, "no draw reused a workspace larger than it needed"


# ---------------------------------------------------------------------------------------------------------------- 6. the align-corners size pairs
def _scalars(family, what, got, t):
    for name, value in got.items():
        if name in t["n"]:
            assert float(value) == t["n"][name], f"{family} {what} {name}: {float(value)} != {t['n'][name]}"
        else:
            P.check_scalar(f"{family} {what} {name}", value, t["l32"][name], t["l64"][name])


def _gradients(family, what, grads, t):
    for g, g64, b, zero in zip(grads, t["g64"], t["b"], T.unsampled(t)):
        T.check(family, what, g, g64, b, quiet=True)
        assert not g.cpu()[zero].any(), f"{family} {what}: a pixel nobody samples is not exactly 0"


def _run_k9(ops, score, labels):
    loss, stats = ops.outlier_tail(score, labels, "mse", T.THR_IN, T.THR_OUT)
    g = ops.outlier_tail_backward(score, labels, stats, torch.ones((), device="cuda"), "mse", T.THR_IN, T.THR_OUT)
    return loss, stats, g


def _run_k11b(ops, score, labels):
    losses, stats = ops.score_reg(score, labels)
    return losses, stats, ops.score_reg_backward(score, labels, stats, None, torch.ones((), device="cuda"))


def _run_k10(ops, sem, ood, labels):
    losses, stats, lse = ops.dense_hybrid_loss(sem, ood, labels, D.BETA)
    return (losses, stats, lse) + ops.dense_hybrid_loss_backward(sem, ood, labels, stats, lse, torch.ones((), device="cuda"), D.BETA)


def _run_k11a(ops, sem, labels):
    losses, stats, R = ops.gambler_loss(sem, labels, G.OOD_REG)
    return losses, stats, R, ops.gambler_loss_backward(sem, labels, stats, R, torch.ones((), device="cuda"), G.OOD_REG)


K10_STATS = ("S_seg", "S_ood", "S_th", "S_x", "n_seg", "n_ood", "n_all", "m")
PAIR = {  # kernel -> (family, run, the workspace's kind, its size query, the query's arguments of a launch)
    "K9": ("K9 pairs", _run_k9, "outlier_tail", "rba_outlier_tail_workspace_f32", lambda h, w, H, W: (T.PAIR_B, H, W)),
    "K11b": ("K11b pairs", _run_k11b, "score_reg", "rba_score_reg_workspace_f32", lambda h, w, H, W: (T.PAIR_B, h, w, H, W)),
    "K10": ("K10 pairs", _run_k10, "dense_hybrid_loss", "rba_dense_hybrid_loss_workspace_f32", lambda h, w, H, W: (T.PAIR_B, H, W)),
    "K11a": ("K11a pairs", _run_k11a, "gambler_loss", "rba_gambler_loss_workspace_f32", lambda h, w, H, W: (T.PAIR_B, H, W)),
}


def _pair_launch(ops, reuse, kernel, launch):
    family, run, kind, query, dims = PAIR[kernel]
    inputs = T.pair_inputs(kernel, launch)
    assert T.pair_condition(kernel, inputs), (kernel, launch)
    t = T.pair_truth(kernel, inputs)
    a = [dev(x) for x in inputs]
    was = reuse.before(kind)
    r1, r2 = _twice(ops, lambda: run(ops, *a))
    reuse.after(kind, was, query, *dims(*launch))
    T.count_draw(family)
    what = f"{launch}"
    _same_bits(r1, r2, f"{family} {launch}")
    for r in (r1, r2):
        r = [x.cpu() for x in r]                                          # one copy each: the scalar checks below read them element by element
        if kernel == "K9":
            _scalars(family, what, {"loss": r[0][0], "sum_in": r[1][0], "n_in": r[1][1], "sum_out": r[1][2], "n_out": r[1][3]}, t)
            grads = r[2:]
        elif kernel == "K11b":
            _scalars(family, what, {"smoothness": r[0][0], "sparsity": r[0][1]}, t)
            grads = r[2:]
        elif kernel == "K10":
            _scalars(family, what, {"loss": r[0][0], "loss_seg": r[0][1], "loss_ood": r[0][2], "loss_th": r[0][3],
                                    **{n: r[1][i] for i, n in enumerate(K10_STATS)}}, t)
            grads = r[3:]
        else:
            _scalars(family, what, {"loss": r[0][0], "in_mean": r[0][1], "out_mean": r[0][2], "S_in": r[1][0], "S_out": r[1][1],
                                    "n_in": r[1][2], "n_ood": r[1][3]}, t)
            grads = r[3:]
        _gradients(family, what, grads, t)


def _grow(ops):
    """one launch of each kernel on a label map larger than any small pair's, so that every small pair runs on a reused, larger workspace"""
    big = (3, 3, 64, 64)
    for kernel in T.PAIR_KERNELS:
        PAIR[kernel][1](ops, *[dev(x) for x in T.pair_inputs(kernel, big)])


@pytest.mark.parametrize("chunk", T.small_chunks())
def test_align_corners_small_pairs(ops, chunk):
    """200 launches of the 1600: pair a on the rows, pair b on the columns, through K9 (mse), K11b (the sparsity leg), K10 (K = 2) and, one admitted
    launch in five, K11a"""
    reuse = Reuse(ops)
    _grow(ops)
    base = chunk * T.PAIR_CHUNK
    for i, launch in enumerate(T.chunk_launches(chunk)):
        for kernel in T.PAIR_KERNELS[:3]:
            _pair_launch(ops, reuse, kernel, launch)
        if T.k11a_runs(launch, base + i):
            _pair_launch(ops, reuse, "K11a", launch)
    for kernel in T.PAIR_KERNELS:
        T.report(PAIR[kernel][0])
        assert PAIR[kernel][2] in reuse.seen, f"{kernel}: no launch reused a workspace larger than it needed"


@pytest.mark.parametrize("axis", ["rows", "columns"])
def test_align_corners_large_pairs(ops, axis):
    """the listed and 20 seeded large pairs on one axis, the other at 2 -> 2 (K11a: 2 -> 4, its blur needs four label columns)"""
    reuse = Reuse(ops)
    pick = slice(0, None, 2) if axis == "rows" else slice(1, None, 2)
    for kernel in T.PAIR_KERNELS:
        launches = T.large_launches((2, 4) if kernel == "K11a" else (2, 2))[pick]
        for launch in T.shuffled(launches, 12):
            _pair_launch(ops, reuse, kernel, launch)
        T.report(PAIR[kernel][0])
        assert PAIR[kernel][2] in reuse.seen, f"{kernel}: no launch reused a workspace larger than it needed"
