"""Shared by tests/test_training_kernel_fuzz_cpu.py and tests/test_training_kernel_fuzz_gpu.py: the shape generators of the random-shape sweep of
the training kernels -- K1 backward and its per-class adjoint, K4 / K3 / K2 backward, K8's matching cost and the align-corners taps of K9, K10,
K11a and K11b -- the launch rules those shapes have to straddle, restated from the launchers, and the shared checks.  Pure Python and torch.

Every family draws a fixed BOUNDARY list first and then seeded random shapes (``random.Random(seed)``, seeds 0 and 1).  Inputs, truth, metric and
bar are the families' own (tests/_rba_bwd_cases.py, _k4_bwd_cases.py, _xattn_bwd_cases.py, _msda_cases.py, _point_loss_cases.py,
_dense_hybrid_cases.py, _pebal_cases.py): truth = fp64 CPU autograd of the family's torch restatement on ``.double()`` of the very inputs,
e(T) = max|T - T64| / max|T64| (T64 == 0: T must be exactly 0), bar 4 max(b, 2^-20) with b the same metric for fp32 CPU autograd of the same
inputs, scalars by ``_point_loss_cases.check_scalar``, counts exact.  No draw and no element is left out.
"""
import functools
import random

import torch
import torch.nn.functional as F

from tests import _dense_hybrid_cases as D
from tests import _k4_bwd_cases as K4
from tests import _msda_cases as M2
from tests import _pebal_cases as G
from tests import _point_loss_cases as P
from tests import _rba_bwd_cases as R
from tests import _xattn_bwd_cases as X
from tests.test_outlier_tail_gpu import THR_IN, THR_OUT, ref_tail as k9_ref_tail   # K9's restatement lives with its test

SEEDS = (0, 1)
NAN, HUGE = float("nan"), 3.0e38          # what a reused workspace holds on entry: the first run of a draw, the second

err = X.err                               # e(T); a truth that is identically zero: 0.0 if T is exactly zero, inf otherwise
bar = R.bar


def b_of(t32, t64):
    """b = e of fp32 CPU autograd; 0 where the truth is identically zero (the bar is then the floor, and `err` asks for exact zeros anyway)"""
    return err(t32, t64) if float(t64.abs().max()) > 0 else 0.0


RECORDS = {}                              # family -> {"draws", "e", "b", "ratio"}: the worst of what `check` saw, for docs/measurements.md


def count_draw(family, n=1):
    RECORDS.setdefault(family, {"draws": 0, "e": 0.0, "b": 0.0, "ratio": 0.0})["draws"] += n


def check(family, what, t, t64, b, quiet=False):
    """e(T) <= 4 max(b, 2^-20), every element finite; prints e and b (quiet: the pair sweep prints its worst per test instead of 10^4 lines)"""
    t = t.detach().cpu()
    assert tuple(t.shape) == tuple(t64.shape), f"{what}: shape {tuple(t.shape)} != {tuple(t64.shape)}"
    e, lim = err(t, t64), bar(b)
    if not quiet:
        print(f"{family} {what}: e = {e:.3e}  b = {b:.3e}  bar = {lim:.3e}  e/bar = {e / lim:.3f}")
    rec = RECORDS.setdefault(family, {"draws": 0, "e": 0.0, "b": 0.0, "ratio": 0.0})
    if e > rec["e"]:
        rec["e"], rec["b"] = e, b
    rec["ratio"] = max(rec["ratio"], e / lim)
    assert torch.isfinite(t).all(), f"{family} {what}: not finite"
    assert e <= lim, f"{family} {what}: e = {e:.3e} > 4 max(b, 2^-20) = {lim:.3e} (b = {b:.3e})"
    return e


def report(family):
    r = RECORDS.get(family)
    if r:
        print(f"RECORD {family}: draws {r['draws']}  worst e = {r['e']:.3e} (its b = {r['b']:.3e})  worst e/bar = {r['ratio']:.3f}")


def shuffled(draws, seed):
    """the draws of a family in a seeded order, so that small shapes follow large ones on the grown workspace"""
    order = list(draws)
    random.Random(seed).shuffle(order)
    return order


def _bounded(rnd, n, draw, ok, tries=4000):
    """n draws that satisfy `ok`, from at most `tries` proposals (asserted: the sequence is bounded)"""
    out = []
    for _ in range(tries):
        d = draw(rnd)
        if ok(d):
            out.append(d)
            if len(out) == n:
                return tuple(out)
    raise AssertionError(f"generator: {len(out)} of {n} draws in {tries} proposals")


# ================================================================================================ 1. K1 backward, the per-class adjoint
# rba_reduce_bwd.hip: launch_bwd<20 | 32 | 80 | 160> by K; 128-pixel tiles; the sig tile stays resident while Q + K <= 124 LDS rows, otherwise the
# queries go in chunks of max(16, 124 - K); the sum kernel takes 64 of the Q K entries per workgroup
K1_TILE, K1_ROWS, K1_SCALE, K1_WORK = 128, 124, 6.0, 2_500_000


def k1_kmax(K):
    return 20 if K <= 20 else 32 if K <= 32 else 80 if K <= 80 else 160


def k1_chunk(Q, K):
    return Q if Q + K <= K1_ROWS else min(Q, max(16, K1_ROWS - K))


def k1_in_domain(Q, K, HW):
    return Q >= 1 and 1 <= K <= 160 and HW >= 1


def k1_boundary():
    """(Q, K, HW)"""
    out = []
    for K in (20, 21, 27, 32, 33, 80, 81, 108, 109, 160):
        out += [(s - K, K, 129 + K % 3) for s in (K1_ROWS, K1_ROWS + 1) if s - K >= 1]      # resident | chunked
        if K > 108:                                                                          # there that Q is < 16 (or none): the 16-row chunk floor
            out += [(16, K, 129), (17, K, 257)]
    out += [(1, 19, 515), (250, 19, 515), (250, 27, 127), (1, 160, 128), (1, 1, 1)]
    out += [(7, 3, hw) for hw in (1, 127, 128, 129, 513, 515)]                               # tiles 1, 1, 1, 2, 5, 5: not multiples of 4
    out += [(9, 7, 200), (8, 8, 200), (13, 5, 200), (16, 8, 130), (43, 3, 130)]              # Q K = 63, 64, 65, 128, 129
    return tuple(out)


def k1_random(seed, n=12):
    return _bounded(random.Random(seed), n, lambda r: (r.randint(1, 260), r.randint(1, 160), r.randint(1, 1500)),
                    lambda d: d[0] * d[1] * d[2] <= K1_WORK)


def k1_draws(which):
    """which: "boundary" | a seed"""
    return k1_boundary() if which == "boundary" else k1_random(which)


def _stable_seed(*ints):
    s = 0
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


@functools.lru_cache(maxsize=256)
def k1_inputs(draw):
    """(mask [Q,HW], prob [Q,K], g [HW], gsem [K,HW]) fp32 on the CPU"""
    Q, K, HW = draw
    mask, prob, g = R.inputs_for(Q, K, HW, K1_SCALE, _stable_seed(1, Q, K, HW))
    gsem = torch.randn(K, HW, generator=torch.Generator().manual_seed(_stable_seed(11, Q, K, HW)))
    return mask, prob, g, gsem


def _sem_autograd(mask, prob, gsem):
    m, p = mask.detach().clone().requires_grad_(True), prob.detach().clone().requires_grad_(True)
    (torch.einsum("qk,qn->kn", p, m.sigmoid()) * gsem).sum().backward()
    return m.grad, p.grad


def k1_truth(draw, what):
    """what: a score mode of K1 backward, or "sem_seg" (the per-class adjoint) -> (grad_mask64, grad_prob64, b_mask, b_prob)"""
    mask, prob, g, gsem = k1_inputs(draw)
    if what == "sem_seg":
        gm64, gp64 = _sem_autograd(mask.double(), prob.double(), gsem.double())
        gm32, gp32 = _sem_autograd(mask, prob, gsem)
    else:
        gm64, gp64 = R._autograd(mask.double(), prob.double(), g.double(), what)
        gm32, gp32 = R._autograd(mask, prob, g, what)
    return gm64, gp64, b_of(gm32, gm64), b_of(gp32, gp64)


# ================================================================================================ 2. K4 backward
# mask_logits_bwd.hip: the matrix-pipe kernels need N % 4 == 0 (and 16-byte aligned pointers), otherwise the VALU kernels; grad_embed: blocks of
# 112 queries x 64 channels and slices of `len` pixels; grad_feat: 128-query chunks, 64-channel blocks, 256 columns per workgroup
K4_QB, K4_CB, K4_QC, K4_COLS, K4_WORK = 112, 64, 128, 256, 30_000_000


def k4_slices(B, Q, C, N):
    """slices_of: (len, count) -- len a multiple of 32, at least 512, aiming at 512 workgroups"""
    units = B * ((Q + K4_QB - 1) // K4_QB) * ((C + K4_CB - 1) // K4_CB)
    target = 1 if units >= 512 else (512 + units - 1) // units
    length = max(512, ((N + target - 1) // target + 31) // 32 * 32)
    return length, (N + length - 1) // length


def k4_matrix_form(N):
    return N % 4 == 0


def k4_in_domain(B, Q, C, N):
    return 1 <= B <= 65535 and Q >= 1 and C >= 1 and N >= 1


def k4_boundary():
    """(B, Q, C, N).  Slice length at these sizes is 512 (asserted by the CPU test from `k4_slices`): N sits on both sides of 512 and 1024"""
    return ((1, 111, 63, 255), (1, 112, 64, 256), (1, 113, 65, 257), (2, 127, 1, 511), (1, 128, 256, 512), (1, 129, 264, 513),
            (1, 224, 64, 1023), (1, 225, 65, 1024), (3, 1, 360, 1025), (1, 112, 64, 1026), (2, 128, 63, 516), (1, 1, 1, 1),
            (1, 100, 256, 1028), (1, 7, 12, 2))


def _around(rnd, centres, spread=1):
    return max(1, rnd.choice(centres) + rnd.randint(-spread, spread))


def k4_random(seed, n=10):
    def draw(r):
        N = r.choice([r.randint(1, 5000), _around(r, (256, 512, 1024), 3), 4 * r.randint(1, 1250)])
        return (r.choice((1, 2, 3)), r.choice([_around(r, (1, 112, 128, 224)), r.randint(1, 230)]),
                r.choice([_around(r, (1, 64, 256, 264, 360)), r.randint(1, 370)]), N)
    return _bounded(random.Random(100 + seed), n, draw, lambda d: d[0] * d[1] * d[2] * d[3] <= K4_WORK)


def k4_draws(which):
    return k4_boundary() if which == "boundary" else k4_random(which)


@functools.lru_cache(maxsize=64)
def k4_inputs(draw):
    return K4.inputs_for(*draw, _stable_seed(2, *draw))


def k4_truth(draw):
    """(grad_embed64, grad_feat64, b_embed, b_feat)"""
    E, Fm, Gm = k4_inputs(draw)
    ge64, gf64 = K4._autograd(E.double(), Fm.double(), Gm.double())
    ge32, gf32 = K4._autograd(E, Fm, Gm)
    return ge64, gf64, b_of(ge32, ge64), b_of(gf32, gf64)


# ================================================================================================ 3. K3 backward
# masked_xattn_bwd.hip: the row pass switches to its long-row form at S >= 1024, which takes 4 queries per workgroup; the key pass takes 64-key
# chunks and four waves that each sweep a quarter of the queries
K3_LONG, K3_ROWS_PER_GROUP, K3_KEYS, K3_WORK = 1024, 4, 64, 1_500_000


def k3_long_rows(S):
    return S >= K3_LONG


def k3_in_domain(B, Q, S, nH):
    return B >= 1 and Q >= 1 and S >= 1 and nH >= 1


def k3_boundary():
    """(B, Q, S, nH, masked): every Q of {1, 2, 3, 4, 5, 7, 129, 130}, every S of {1, 63, 64, 65, 1023, 1024, 1025}, every Q mod 4 under a long row,
    a quarter without a mask"""
    return ((1, 1, 1, 1, True), (1, 2, 63, 3, True), (2, 3, 64, 1, True), (1, 4, 65, 8, True), (1, 5, 1023, 1, True), (1, 4, 1024, 1, True),
            (1, 5, 1024, 3, True), (2, 2, 1025, 1, True), (1, 3, 1025, 1, False), (1, 7, 1024, 1, True), (1, 129, 64, 3, False),
            (1, 130, 65, 1, True), (1, 129, 1025, 1, True), (1, 130, 1023, 1, False), (1, 2, 1024, 1, False), (2, 7, 1, 3, True))


def k3_random(seed, n=8):
    def draw(r):
        S = r.choice([r.randint(1, 2300), _around(r, (64, 128, 1024), 2)])
        return (r.choice((1, 2)), r.choice([r.randint(1, 140), _around(r, (4, 128), 2)]), S, r.choice((1, 3, 8)), r.random() >= 0.25)
    return _bounded(random.Random(200 + seed), n, draw, lambda d: d[0] * d[1] * d[2] * d[3] <= K3_WORK)


def k3_draws(which):
    return k3_boundary() if which == "boundary" else k3_random(which)


def k3_zero_col(draw):
    """the key blocked in every row (planted when Q >= 3 and there is a second key to attend to), or None"""
    B, Q, S, nH, masked = draw
    return _stable_seed(3, *draw[:4]) % S if masked and Q >= 3 and S >= 2 else None


@functools.lru_cache(maxsize=64)
def k3_inputs(draw):
    """`_xattn_bwd_cases.make_shape` with its planted rows -- row 0 fully blocked (it attends everywhere), row 1 fully open -- and, when Q >= 3,
    one key blocked in every row"""
    B, Q, S, nH, masked = draw
    return X.make_shape(B, Q, S, nH, masked, _stable_seed(33, *draw[:4]), zero_col=k3_zero_col(draw), blocked_row=True)


def k3_zero_truth(draw):
    """the gradients whose truth is identically zero: a softmax over one key is the constant 1"""
    return ("grad_q", "grad_k") if draw[2] == 1 else ()


def k3_truth(draw):
    """(T64 x 3, b x 3); the blocked set is taken in fp32 on the kernel's own logits (`_xattn_bwd_cases.cpu_grads`)"""
    inp = k3_inputs(draw)
    t64 = X.cpu_grads(inp, torch.float64)
    return t64, [b_of(t, r) for t, r in zip(X.cpu_grads(inp, torch.float32), t64)]


# ================================================================================================ 4. K2 backward (fp32)
# ms_deform_attn_bwd.hip: the model form needs D == 32, P == 4 and L in {1, 3} and takes 8 (query, head) pairs per workgroup; everything else
# takes the generic kernel, one wave per (n, q, m), 4 to a workgroup
K2_WORK = 3_000_000


def k2_model_form(D, P, L):
    return D == 32 and P == 4 and L in (1, 3)


def k2_in_domain(N, M, D, Lq, shapes, P):
    return N >= 1 and M >= 1 and D >= 1 and Lq >= 1 and P >= 1 and len(shapes) >= 1 and all(h >= 1 and w >= 1 for h, w in shapes)


_L1, _L2, _L3 = ((5, 7),), ((6, 4), (3, 2)), ((9, 7), (5, 3), (2, 2))
_THIN1, _THIN3 = ((1, 5),), ((7, 1), (1, 1), (3, 2))                  # levels with a 1-pixel axis


def k2_boundary():
    """(N, M, D, Lq, shapes, P): both sides of D == 32, P == 4, L in {1, 3}; Lq M = 7, 8, 9, 3, 4, 5, 15, 16, 17; 1-pixel axes in both forms"""
    return ((1, 1, 32, 8, _L1, 4), (2, 1, 32, 7, _L3, 4), (1, 3, 32, 3, _L3, 4), (1, 1, 31, 8, _L1, 4), (1, 1, 33, 9, _L3, 4),
            (1, 1, 32, 4, _L1, 3), (1, 1, 32, 5, _L3, 5), (1, 2, 32, 8, _L2, 4), (1, 1, 32, 3, _THIN1, 4), (1, 5, 32, 3, _THIN3, 4),
            (1, 1, 31, 5, _THIN3, 3), (1, 17, 32, 1, _L3, 4), (2, 1, 33, 4, _L2, 5), (1, 2, 32, 2, _L1, 4))


def k2_random(seed, n=8):
    def draw(r):
        model = r.random() < 0.5                                          # half the draws in the model form, half beside it
        L = r.choice((1, 3)) if model else r.choice((1, 2, 3))
        shapes = tuple((r.randint(1, 24), r.randint(1, 20)) for _ in range(L))
        return (r.choice((1, 2)), r.choice((1, 2, 3, 8)), 32 if model else r.choice((31, 32, 33, r.randint(1, 70))), r.randint(1, 400), shapes,
                4 if model else r.choice((3, 4, 5)))

    def ok(d):
        N, M, D, Lq, shapes, Pn = d
        return sum(h * w for h, w in shapes) <= 1500 and N * M * D * Lq * len(shapes) * Pn <= K2_WORK
    return _bounded(random.Random(300 + seed), n, draw, ok)


def k2_draws(which):
    return k2_boundary() if which == "boundary" else k2_random(which)


@functools.lru_cache(maxsize=64)
def k2_inputs(draw):
    """`_msda_cases.make_shape`, kind "rand": locations in [-0.15, 1.15), nudged off the integer pixel lines; `condition` asserted"""
    N, M, D, Lq, shapes, Pn = draw
    inp = M2.make_shape(N, M, D, Lq, [tuple(s) for s in shapes], Pn, "rand", torch.float32, _stable_seed(4, N, M, D, Lq, Pn, *sum(shapes, ())))
    assert M2.condition(inp["loc"], inp["shape_list"]), f"fixture {draw}: a pixel coordinate within {M2.MARGIN} of an integer"
    return inp


def k2_truth(draw):
    inp = k2_inputs(draw)
    t64 = M2.cpu_grads(inp, torch.float64)
    return t64, [b_of(t, r) for t, r in zip(M2.cpu_grads(inp, torch.float32), t64)]


# ================================================================================================ 5. K8: the matching cost
# point_loss.hip: 32 x 32 tiles over (Q, T), 64-point steps, slices of `len` points (a multiple of 64) aiming at 512 workgroups
K8_QB, K8_TB, K8_PC = 32, 32, 64
K8_PRED, K8_TGT, K8_K = (8, 12), (32, 48), 19


def k8_slices(Q, T, Pn):
    units = ((Q + K8_QB - 1) // K8_QB) * ((T + K8_TB - 1) // K8_TB)
    target = 1 if units >= 512 else (512 + units - 1) // units
    length = max(K8_PC, ((Pn + target - 1) // target + K8_PC - 1) // K8_PC * K8_PC)
    return length, (Pn + length - 1) // length


def k8_in_domain(Q, T, Pn):
    return Q >= 1 and T >= 1 and Pn >= 1


def k8_boundary():
    """(Q, T, P).  Slice length at these sizes is 64 (asserted by the CPU test from `k8_slices`): P sits on both sides of 64 and 128"""
    return ((1, 1, 1), (31, 33, 63), (32, 32, 64), (33, 31, 65), (100, 70, 127), (99, 1, 128), (1, 71, 129), (101, 69, 2), (32, 33, 130),
            (64, 64, 64), (65, 2, 192), (2, 65, 193))


def k8_random(seed, n=8):
    return _bounded(random.Random(400 + seed), n,
                    lambda r: (r.choice([r.randint(1, 110), _around(r, (32, 64, 96))]), r.choice([r.randint(1, 75), _around(r, (32, 64))]),
                               r.choice([r.randint(1, 300), _around(r, (64, 128, 192))])), lambda d: True)


def k8_draws(which):
    return k8_boundary() if which == "boundary" else k8_random(which)


@functools.lru_cache(maxsize=64)
def k8_inputs(draw):
    """(pred_masks [Q,8,12], tgt_masks [T,32,48] binary, coords [P,2], pred_logits [Q,K+1], tgt_ids [T]): `_point_loss_cases.cost_inputs` at small maps"""
    Q, T, Pn = draw
    gen = torch.Generator().manual_seed(_stable_seed(5, Q, T, Pn))
    pred = P.smooth(gen, Q, *K8_PRED, 4.0)
    tgt = (P.smooth(gen, T, *K8_TGT, 1.0) > 0.3).float()
    return pred, tgt, torch.rand(Pn, 2, generator=gen), 2.0 * torch.randn(Q, K8_K + 1, generator=gen), torch.randint(0, K8_K + 1, (T,), generator=gen)


def k8_truth(draw):
    """(C64 [Q,T], b)"""
    pred, tgt, coords, logits, ids = k8_inputs(draw)
    c64 = P.ref_match_cost(pred.double(), tgt.double(), coords.double(), logits.double(), ids, *P.COST_WEIGHTS)
    return c64, b_of(P.ref_match_cost(pred, tgt, coords, logits, ids, *P.COST_WEIGHTS), c64)


# ================================================================================================ 6. the align-corners taps: a size-pair sweep
# K9, K10, K11a and K11b resample rows and columns with the same code (bilinear_ac.h), so one launch (h, w, H, W) = (in_a, in_b, out_a, out_b) tests
# pair a on the rows and pair b on the columns.  Two images per launch: there are always two label pixels to plant both classes on.
PAIR_MAX, PAIR_CHUNK, PAIR_B = 40, 200, 2
LARGE_LISTED = ((128, 512), (256, 1024), (160, 640), (129, 512), (128, 513), (255, 1024), (512, 128), (2, 2048), (511, 2047))
PAIR_KERNELS = ("K9", "K11b", "K10", "K11a")


def small_pairs():
    return tuple((i, o) for i in range(1, PAIR_MAX + 1) for o in range(1, PAIR_MAX + 1))


@functools.lru_cache(maxsize=None)
def small_launches():
    """1600 launches (h, w, H, W): the row pairs are [1, 40]^2 in a seeded order, the column pairs a seeded permutation of them"""
    rows = list(small_pairs())
    random.Random(600).shuffle(rows)
    cols = list(rows)
    random.Random(601).shuffle(cols)
    return tuple((a[0], b[0], a[1], b[1]) for a, b in zip(rows, cols))


def small_chunks():
    n = len(small_launches())
    return tuple(range((n + PAIR_CHUNK - 1) // PAIR_CHUNK))


def chunk_launches(chunk):
    return small_launches()[chunk * PAIR_CHUNK:(chunk + 1) * PAIR_CHUNK]


@functools.lru_cache(maxsize=None)
def large_pairs():
    rnd = random.Random(602)
    return LARGE_LISTED + tuple((rnd.randint(1, 512), rnd.randint(1, 2048)) for _ in range(20))


def large_launches(other=(2, 2)):
    """every large pair once on the rows and once on the columns, the other axis at `other` (2 -> 2; K11a's blur needs 4 label columns: 2 -> 4)"""
    out = []
    for i, o in large_pairs():
        out += [(i, other[0], o, other[1]), (other[0], i, other[1], o)]
    return tuple(out)


# Which source rows a destination names is a DECISION (the floor of scale * dst), and the two references take it in their own precision.  At these
# pairs -- and at no other pair of the sweep, asserted by the CPU test -- fp32 ATen names one source row that fp64 ATen does not: the last
# destination's coordinate (in - 1) / (out - 1) * (out - 1) is in - 1 exactly in fp64 and one ulp below it in fp32, so row in - 2 gets a weight of
# about 2^-22 there.  The kernels restate fp32 ATen (bilinear_ac.h), so "nobody samples this pixel: exactly 0" is asked where NEITHER reference
# names the pixel; the named-by-fp32-only row is held by the bar like every other element.  No pair and no element is left out.
AC_FP32_NAMES_MORE = ((27, 12), (32, 8), (32, 15))


def ac_named(size_in, size_out, dtype):
    """bool [size_in]: the source rows that get a gradient from F.interpolate(align_corners=True) along one axis, in `dtype`"""
    x = torch.zeros(1, 1, size_in, 1, dtype=dtype, requires_grad=True)
    F.interpolate(x, size=(size_out, 1), mode="bilinear", align_corners=True).sum().backward()
    return x.grad.flatten() != 0


def unsampled(t):
    """per gradient of `pair_truth`: the elements that are exactly zero in both references"""
    return [(g64 == 0) & (g32 == 0) for g64, g32 in zip(t["g64"], t["g32"])]


def k11a_runs(launch, index):
    """K11a's blur needs H, W >= 4; of the launches it admits, one in five (it shares AcOwner with K10, which runs them all)"""
    return launch[2] >= 4 and launch[3] >= 4 and index % 5 == 0


def pair_in_domain(launch, kernel):
    h, w, H, W = launch
    return min(h, w, H, W) >= 1 and (kernel != "K11a" or min(H, W) >= 4)


def _plant(labels, first, last):
    labels.view(-1)[0], labels.view(-1)[-1] = first, last
    return labels


def _binary_labels(gen, H, W):
    """0 (inlier) 60 %, of which 1 (outlier) 25 %, 255 (void) the rest; both classes planted"""
    r = torch.rand(PAIR_B, H, W, generator=gen)
    labels = torch.full((PAIR_B, H, W), 255, dtype=torch.int64)
    labels[r < 0.6] = 0
    labels[r < 0.25] = 1
    return _plant(labels, 0, 1)


def _class_labels(gen, K, H, W):
    """`_dense_hybrid_cases.draw_labels`'s mixture -- classes, 15 % 254, 10 % 255, 2 % 200 -- with one class pixel and one outlier pixel planted"""
    labels = torch.randint(0, K, (PAIR_B, H, W), generator=gen)
    r = torch.rand(PAIR_B, H, W, generator=gen)
    labels[r < 0.15] = D.OUTLIER
    labels[(r >= 0.15) & (r < 0.25)] = 255
    labels[(r >= 0.25) & (r < 0.27)] = 200
    return _plant(labels, K - 1, D.OUTLIER)


PAIR_K = 2


def pair_inputs(kernel, launch):
    """the kernel's inputs on the CPU.  K9: (score, labels in {0, 1, 255}); K11b: (score, labels); K10: (sem [B,2,h,w], ood, labels); K11a: (sem
    [B,3,h,w], labels)"""
    h, w, H, W = launch
    gen = torch.Generator().manual_seed(_stable_seed(6 + PAIR_KERNELS.index(kernel), h, w, H, W))
    if kernel == "K9":
        return -0.55 + 0.5 * torch.randn(PAIR_B, h, w, generator=gen), _binary_labels(gen, H, W)
    if kernel == "K11b":
        return -(3.0 + torch.randn(PAIR_B, h, w, generator=gen)), _binary_labels(gen, H, W)
    if kernel == "K10":
        return (1.5 + 2.0 * torch.randn(PAIR_B, PAIR_K, h, w, generator=gen), 1.5 * torch.randn(PAIR_B, 2, h, w, generator=gen),
                _class_labels(gen, PAIR_K, H, W))
    assert kernel == "K11a"
    return 1.2 * torch.rand(PAIR_B, PAIR_K + 1, h, w, generator=gen), _class_labels(gen, PAIR_K, H, W)


def pair_condition(kernel, inputs):
    """both label classes present (the means exist); K11a: the fp64 blurred reward stays above `_pebal_cases.MIN_R`"""
    labels = inputs[-1]
    if kernel in ("K9", "K11b"):
        return bool((labels == 0).any()) and bool((labels == 1).any())
    ok = bool(((labels >= 0) & (labels < PAIR_K)).any()) and bool((labels == D.OUTLIER).any())
    if kernel == "K11a":
        ok = ok and float(G.ref_gambler_tail(inputs[0].double(), labels)[1]["R"].min()) >= G.MIN_R
    return ok


def _num(v):
    return float(v.detach()) if isinstance(v, torch.Tensor) else float(v)


def pair_truth(kernel, inputs):
    """fp64 and fp32 CPU autograd of the kernel's restatement -> {"l64", "l32": {name: scalar}, "n": {name: exact count}, "g64": [gradients],
    "b": [fp32 autograd's error of each]}"""
    out = {}
    for tag, dtype in (("64", torch.float64), ("32", torch.float32)):
        leaves = [t.to(dtype).clone().requires_grad_(True) for t in inputs[:-1]]
        labels = inputs[-1]
        if kernel == "K9":
            loss, (s_in, n_in, s_out, n_out) = k9_ref_tail(leaves[0], labels, "mse")
            scalars, counts = {"loss": loss, "sum_in": s_in, "sum_out": s_out}, {"n_in": n_in, "n_out": n_out}
            loss.backward()
        elif kernel == "K11b":
            smooth, sparse = G.ref_smoothness(leaves[0]), G.ref_sparsity(leaves[0], labels)
            scalars, counts = {"smoothness": smooth, "sparsity": sparse}, {}
            sparse.backward()                                           # the sparsity leg alone: the resampling walk
        elif kernel == "K10":
            loss, parts = D.ref_tail(leaves[0], leaves[1], labels, D.BETA)
            scalars = {"loss": loss, **{k: parts[k] for k in ("loss_seg", "loss_ood", "loss_th", "S_seg", "S_ood", "S_th", "S_x", "m")}}
            counts = {k: parts[k] for k in ("n_seg", "n_ood", "n_all")}
            loss.backward()
        else:
            loss, parts = G.ref_gambler_tail(leaves[0], labels)
            scalars = {"loss": loss, **{k: parts[k] for k in ("in_mean", "out_mean", "S_in", "S_out")}}
            counts = {k: parts[k] for k in ("n_in", "n_ood")}
            loss.backward()
        out["l" + tag] = {k: _num(v) for k, v in scalars.items()}
        out["g" + tag] = [t.grad for t in leaves]
        out["n"] = {k: int(v) for k, v in counts.items()}
    out["b"] = [b_of(a, r) for a, r in zip(out["g32"], out["g64"])]
    return out
