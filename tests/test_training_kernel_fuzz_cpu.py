"""The generators of the training-kernel shape sweep (tests/_train_fuzz_cases.py), without a GPU: every draw list is a pure function of its seed,
lies inside the domain include/rba_hip.h documents (the sweep probes no refusal), hits both sides of every launch-rule boundary -- computed from
the rules restated beside the generators -- and meets its fixture conditions; and the fp32 CPU restatement of a sample of draws stays inside
4 max(b, 2^-20) of the fp64 one (b is its own error) with no truth that is identically zero unless the family declares it."""
import importlib

import pytest
import torch

from tests import _msda_cases as M2
from tests import _train_fuzz_cases as T

WHICH = ("boundary",) + T.SEEDS


def _all(draws_of):
    return [d for w in WHICH for d in draws_of(w)]


def _both(values, what):
    values = set(values)
    assert values == {False, True}, f"{what}: only {values} drawn"


@pytest.mark.parametrize("draws_of", [T.k1_draws, T.k4_draws, T.k3_draws, T.k2_draws, T.k8_draws], ids=["k1", "k4", "k3", "k2", "k8"])
def test_draw_lists_are_pure_functions_of_the_seed(draws_of):
    first = {w: draws_of(w) for w in WHICH}
    importlib.reload(T)
    again = {w: getattr(T, draws_of.__name__)(w) for w in WHICH}
    assert first == again
    assert first[0] != first[1]
    assert all(len(set(v)) == len(v) for v in first.values())


def test_pair_sweep_lists_are_pure_functions_of_the_seed():
    first = (T.small_launches(), T.large_pairs(), T.large_launches())
    importlib.reload(T)
    assert first == (T.small_launches(), T.large_pairs(), T.large_launches())


# ---------------------------------------------------------------------------------------------------------------- 1. K1 backward
def test_k1_draws_straddle_every_launch_rule():
    draws = _all(T.k1_draws)
    assert all(T.k1_in_domain(*d) for d in draws)
    assert len(T.k1_random(0)) == len(T.k1_random(1)) == 12 and all(d[0] <= 260 and d[1] <= 160 and d[2] <= 1500 for d in draws)
    bd = T.k1_boundary()
    assert {T.k1_kmax(d[1]) for d in bd} == {20, 32, 80, 160} and {T.k1_kmax(d[1]) for s in T.SEEDS for d in T.k1_random(s)} >= {32, 160}
    ks = {d[1] for d in bd}
    assert {20, 21, 27, 32, 33, 80, 81, 160} <= ks                                        # both sides of each K switch
    for K in (20, 21, 27, 32, 33, 80, 81, 108):                                           # Q + K = 124 | 125: resident | chunked
        assert {d[0] + K for d in bd if d[1] == K} >= {124, 125}
        assert T.k1_chunk(124 - K, K) == 124 - K and T.k1_chunk(125 - K, K) == max(16, 124 - K) < 125 - K
    for K in (109, 160):                                                                  # K > 108: the 16-row floor of the chunk, Q = 16 | 17
        assert {d[0] for d in bd if d[1] == K} >= {16, 17} and T.k1_chunk(16, K) == 16 == T.k1_chunk(17, K)
    assert {d[0] for d in bd} >= {1, 250}
    assert {d[2] for d in bd} >= {1, 127, 128, 129, 513, 515}
    tiles = {(d[2] + T.K1_TILE - 1) // T.K1_TILE for d in bd}
    assert {1, 2, 5} <= tiles and any(t % 4 for t in tiles)
    assert {d[0] * d[1] for d in bd} >= {63, 64, 65}
    _both((d[0] + d[1] <= T.K1_ROWS for s in T.SEEDS for d in T.k1_random(s)), "random K1 draws, resident form")


# ---------------------------------------------------------------------------------------------------------------- 2. K4 backward
def test_k4_draws_straddle_every_launch_rule():
    draws = _all(T.k4_draws)
    assert all(T.k4_in_domain(*d) for d in draws) and all(d[3] <= 5000 for d in draws)
    assert len(T.k4_random(0)) == len(T.k4_random(1)) == 10
    bd = T.k4_boundary()
    assert {d[0] for d in bd} == {1, 2, 3}
    assert {d[1] for d in bd} >= {1, 111, 112, 113, 127, 128, 129, 224, 225}
    assert {d[2] for d in bd} >= {1, 63, 64, 65, 256, 264, 360}
    assert {d[3] % 4 for d in bd} == {0, 1, 2, 3} and {d[3] for d in bd} >= {255, 256, 257}
    _both((T.k4_matrix_form(d[3]) for s in T.SEEDS for d in T.k4_random(s)), "random K4 draws, matrix-pipe form")
    counts = set()
    for d in draws:
        length, count = T.k4_slices(*d)
        assert length >= 512 and length % 32 == 0 and (count - 1) * length < d[3] <= count * length
        counts.add(count)
    for d in bd:                                                                          # N on both sides of one and of two slice lengths
        assert T.k4_slices(*d)[0] == 512
    ns = {d[3] for d in bd}
    assert {511, 512, 513, 1023, 1024, 1025} <= ns and {1, 2, 3} <= counts
    assert T.k4_slices(1, 100, 256, 32768) == (512, 64) and T.k4_slices(1, 100, 256, 131072) == (1024, 128)     # the launcher's own examples


# ---------------------------------------------------------------------------------------------------------------- 3. K3 backward
def test_k3_draws_straddle_every_launch_rule_and_plant_their_rows():
    from oracle import ref_ops
    draws = _all(T.k3_draws)
    assert all(T.k3_in_domain(*d[:4]) for d in draws) and all(d[1] <= 140 and d[2] <= 2300 for d in draws)
    assert len(T.k3_random(0)) == len(T.k3_random(1)) == 8
    bd = T.k3_boundary()
    assert {d[1] for d in bd} >= {1, 2, 3, 4, 5, 7, 129, 130} and {d[2] for d in bd} >= {1, 63, 64, 65, 1023, 1024, 1025}
    assert {d[3] for d in bd} == {1, 3, 8} and {d[0] for d in bd} == {1, 2}
    assert {d[1] % T.K3_ROWS_PER_GROUP for d in bd if T.k3_long_rows(d[2])} == {0, 1, 2, 3}
    assert 0.2 <= sum(not d[4] for d in bd) / len(bd) <= 0.35
    for s in T.SEEDS:
        _both((T.k3_long_rows(d[2]) for d in T.k3_random(s)), f"random K3 draws of seed {s}, long rows")
    _both((d[4] for s in T.SEEDS for d in T.k3_random(s)), "random K3 draws, masked")
    planted_col = 0
    for d in bd + T.k3_random(0):
        B, Q, S, nH, masked = d
        inp = T.k3_inputs(d)
        assert (inp["ml"] is not None) == masked
        if not masked:
            continue
        raw = inp["ml"].sigmoid() < 0.5                                                   # fp32, the kernel's own logits
        assert bool(raw[:, 0].all())                                                      # a fully blocked row ...
        blocked = ref_ops.attn_mask_from_logits(inp["ml"].clone())
        assert not bool(blocked[:, 0].any())                                              # ... which attends everywhere
        col = T.k3_zero_col(d)
        if Q > 1:
            assert not bool(raw[:, 1, [s for s in range(S) if s != col]].any())           # a fully open row (but for the blocked column)
        assert (col is not None) == (Q >= 3 and S >= 2)
        if col is not None:
            planted_col += 1
            assert bool(raw[:, :, col].all()) and bool(blocked[:, 1:, col].all())
        assert float(inp["ml"].abs().min()) > 0.0                                         # no logit on the threshold
    assert planted_col >= 8


# ---------------------------------------------------------------------------------------------------------------- 4. K2 backward
def test_k2_draws_straddle_the_model_form_and_keep_off_the_pixel_lines():
    draws = _all(T.k2_draws)
    assert all(T.k2_in_domain(*d) for d in draws)
    assert len(T.k2_random(0)) == len(T.k2_random(1)) == 8
    assert all(sum(h * w for h, w in d[4]) <= 1500 and d[3] <= 400 for d in draws)
    bd = T.k2_boundary()
    forms = [(d[2], d[5], len(d[4])) for d in bd]
    _both((T.k2_model_form(*f) for f in forms), "K2 boundary draws, model form")
    for i, values in enumerate(((31, 32, 33), (3, 4, 5), (1, 2, 3))):                     # each condition fails alone, on each side
        for v in values:
            others = [f for f in forms if f[i] == v and all(f[j] in ((32,), (4,), (1, 3))[j] for j in range(3) if j != i)]
            assert others, f"no boundary draw with condition {i} at {v} and the other two met"
    lqm = {d[3] * d[1] for d in bd}
    assert {7, 8, 9, 3, 4, 5, 15, 16, 17} <= lqm
    for model in (False, True):                                                           # 1-pixel axes through both kernels
        assert any(any(1 in s for s in d[4]) for d in bd if T.k2_model_form(d[2], d[5], len(d[4])) == model)
    for s in T.SEEDS:
        _both((T.k2_model_form(d[2], d[5], len(d[4])) for d in T.k2_random(s)), f"random K2 draws of seed {s}, model form")
    for d in draws:
        inp = T.k2_inputs(d)                                                              # asserts `condition` itself
        assert M2.condition(inp["loc"], inp["shape_list"]) and inp["loc"].dtype == torch.float32
        assert float(inp["loc"].min()) < 0.0 and float(inp["loc"].max()) > 1.0 or inp["loc"].numel() < 64
    assert any(bool(M2.outside(T.k2_inputs(d)["loc"], T.k2_inputs(d)["shape_list"]).any()) for d in bd)


# ---------------------------------------------------------------------------------------------------------------- 5. K8
def test_k8_draws_straddle_tiles_and_slices():
    draws = _all(T.k8_draws)
    assert all(T.k8_in_domain(*d) for d in draws) and len(T.k8_random(0)) == len(T.k8_random(1)) == 8
    bd = T.k8_boundary()
    assert {d[0] for d in bd} >= {1, 31, 32, 33, 100} and {d[1] for d in bd} >= {1, 31, 32, 33, 70}
    assert {d[2] for d in bd} >= {1, 63, 64, 65, 127, 128, 129}
    counts = set()
    for d in draws:
        length, count = T.k8_slices(*d)
        assert length >= 64 and length % 64 == 0 and (count - 1) * length < d[2] <= count * length
        counts.add(count)
    assert all(T.k8_slices(*d)[0] == 64 for d in bd) and {1, 2, 3} <= counts
    assert T.k8_slices(100, 19, 12544) == (128, 98)                                       # the launcher's own example


# ---------------------------------------------------------------------------------------------------------------- 6. the pair sweep
def test_pair_sweep_covers_the_square_on_both_axes():
    launches = T.small_launches()
    square = set(T.small_pairs())
    assert len(square) == 1600 == len(launches)
    rows, cols = [(h, H) for h, w, H, W in launches], [(w, W) for h, w, H, W in launches]
    assert set(rows) == set(cols) == square and rows != cols
    assert sum(len(T.chunk_launches(c)) for c in T.small_chunks()) == 1600 and max(len(T.chunk_launches(c)) for c in T.small_chunks()) <= 200
    large = T.large_pairs()
    assert large[:len(T.LARGE_LISTED)] == T.LARGE_LISTED and len(large) == len(T.LARGE_LISTED) + 20
    assert all(1 <= i <= 512 and 1 <= o <= 2048 for i, o in large)
    for other in ((2, 2), (2, 4)):
        ll = T.large_launches(other)
        assert {(h, H) for h, w, H, W in ll if (w, W) == other} >= set(large) and {(w, W) for h, w, H, W in ll if (h, H) == other} >= set(large)
    for kernel in T.PAIR_KERNELS[:3]:
        assert all(T.pair_in_domain(l, kernel) for l in launches + T.large_launches())
    eleven = [l for i, l in enumerate(launches) if T.k11a_runs(l, i)]
    assert len(eleven) >= 200 and all(T.pair_in_domain(l, "K11a") for l in eleven + list(T.large_launches((2, 4))))
    assert any(h > H for h, w, H, W in eleven) and any(w < W for h, w, H, W in eleven)


def test_pair_sweep_references_agree_on_the_named_rows_but_at_three_pairs():
    """fp32 and fp64 ATen name the same source rows at every pair of the sweep except `AC_FP32_NAMES_MORE`, where fp32 names exactly one more: the
    stated condition under which "nobody samples it" is asked of the device"""
    more = []
    for i, o in T.small_pairs() + T.large_pairs():
        n64, n32 = T.ac_named(i, o, torch.float64), T.ac_named(i, o, torch.float32)
        assert bool((n32 | ~n64).all()), (i, o)                                           # fp32 never names fewer
        if not torch.equal(n32, n64):
            assert int((n32 & ~n64).sum()) == 1
            more.append((i, o))
    assert tuple(more) == T.AC_FP32_NAMES_MORE


@pytest.mark.parametrize("kernel", T.PAIR_KERNELS)
def test_pair_sweep_fixtures_and_reference(kernel):
    """every 16th small launch and a few large ones: the planted classes, and the fp32 restatement against the fp64 one"""
    other = (2, 4) if kernel == "K11a" else (2, 2)
    sample = [l for i, l in enumerate(T.small_launches()) if i % 16 == 0] + list(T.large_launches(other)[:6]) + [(1, 1, 4, 4), (40, 40, 4, 4)]
    sample = [l for l in sample if T.pair_in_domain(l, kernel)]
    some_zero = False
    for launch in sample:
        inputs = T.pair_inputs(kernel, launch)
        assert T.pair_condition(kernel, inputs), (kernel, launch)
        t = T.pair_truth(kernel, inputs)
        for g32, g64, b in zip(t["g32"], t["g64"], t["b"]):
            assert float(g64.abs().max()) > 0 and T.err(g32, g64) <= T.bar(b)
            some_zero |= bool((g64 == 0).any())
        for name, l64 in t["l64"].items():
            assert abs(t["l32"][name] - l64) <= T.P.scalar_bar(t["l32"][name], l64)
    assert some_zero                                                                      # down-sampling: source pixels nobody samples


# ---------------------------------------------------------------------------------------------------------------- the references alone
def _reference_alone(triples, zero=()):
    for name, t32_b, t64 in triples:
        if name in zero:
            assert float(t64.abs().max()) == 0.0, name
        else:
            assert float(t64.abs().max()) > 0.0, f"{name}: the truth is identically zero and not declared so"
        assert t32_b <= T.bar(t32_b)


def test_reference_alone_k1():
    for d in T.k1_boundary()[::4] + T.k1_random(0)[:3]:
        for what in ("rba", "energy", "neg_logit_sum", "sem_seg"):
            gm64, gp64, bm, bp = T.k1_truth(d, what)
            _reference_alone((("grad_mask", bm, gm64), ("grad_prob", bp, gp64)))


def test_reference_alone_k4_k3_k2_k8():
    for d in T.k4_boundary()[::3] + T.k4_random(0)[:2]:
        ge64, gf64, be, bf = T.k4_truth(d)
        _reference_alone((("grad_embed", be, ge64), ("grad_feat", bf, gf64)))
    for d in T.k3_boundary()[::3] + T.k3_random(0)[:2] + ((2, 7, 1, 3, True),):
        t64, b = T.k3_truth(d)
        _reference_alone(zip(T.X.NAMES, b, t64), zero=T.k3_zero_truth(d))
    assert T.k3_zero_truth((2, 7, 1, 3, True)) == ("grad_q", "grad_k")
    for d in T.k2_boundary()[::3] + T.k2_random(0)[:2]:
        t64, b = T.k2_truth(d)
        _reference_alone(zip(M2.NAMES, b, t64))
    for d in T.k8_boundary()[::3] + T.k8_random(0)[:2]:
        c64, b = T.k8_truth(d)
        _reference_alone((("cost", b, c64),))


def test_draws_stay_inside_their_work_caps():
    """what keeps the fp64 truth of one draw well under 0.2 s: the product of the sizes its restatement multiplies"""
    assert all(d[0] * d[1] * d[2] <= T.K1_WORK for d in _all(T.k1_draws))
    assert all(d[0] * d[1] * d[2] * d[3] <= T.K4_WORK for d in _all(T.k4_draws))
    assert all(d[0] * d[1] * d[2] * d[3] <= T.K3_WORK for d in _all(T.k3_draws))
    assert all(d[0] * d[1] * d[2] * d[3] * len(d[4]) * d[5] <= T.K2_WORK for d in _all(T.k2_draws))
