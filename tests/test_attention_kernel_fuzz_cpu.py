"""The generators of the attention-kernel shape sweep (tests/_attn_fuzz_cases.py), without a GPU: every draw list is a pure function of its seed and
bounded; the boundary list plus the two seeds' draws reach every launch form the restated rules name -- the count of cases per form is pinned here,
so a form that loses its last case, or a rule that moves, fails -- and land on both sides of every threshold; the fixtures hold what they promise
(planted mask rows, planted sampling locations, a qkv tensor that is exact); and each family's fp32 CPU restatement stays inside the family's bound
of its fp64 truth with a finite b."""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops
from tests import _attn_fuzz_cases as A

WHICH = ("boundary",) + A.SEEDS

FAMILIES = {  # family -> (draws, forms of a case, every form the launcher has)
    "k3": ("k3_draws", "k3_forms", A.K3_FORMS),
    "k4": ("k4_draws", "k4_forms", tuple(f"fp32: {f}" for f in A.K4_FP32_FORMS) + tuple(f"f16x3: {f}" for f in A.K4_H3_FORMS + A.K4_FP32_FORMS)),
    "k5": ("k5_draws", "k5_forms", A.K5_FORMS),
    "k7": ("k7_draws", "k7_forms", A.K7_FORMS),
    "k2": ("k2_draws", "k2_forms", A.K2_FORMS),
}

# cases per launch form over the boundary list and both seeds (a K3 case counts once per split_keys value, a K4 case once per mode)
COUNTS = {
    "k3": {"scalar": 48, "mfma-partial 1 strips": 12, "mfma-partial 2 strips": 4, "mfma-partial 3 strips": 3, "mfma-partial 4 strips": 3,
           "mfma-partial 5 strips": 2, "mfma-partial 6 strips": 5, "mfma-partial 7 strips": 7, "mfma-partial 8 strips": 6, "fall-back Q > 128": 3,
           "fall-back nH > 32": 3},
    "k4": {"fp32: mfma<8,2>": 3, "fp32: mfma<4,4>": 17, "fp32: launch<52,2>": 24, "fp32: launch<52,1>": 17,
           "f16x3: h3<1,1>": 5, "f16x3: h3<1,1> persistent": 8, "f16x3: h3<1,2>": 7, "f16x3: h3<1,2> persistent": 3, "f16x3: h3<2,1>": 1,
           "f16x3: h3<2,1> persistent": 4, "f16x3: h3<2,2>": 4, "f16x3: h3<2,2> persistent": 4,
           "f16x3: mfma<8,2>": 1, "f16x3: mfma<4,4>": 6, "f16x3: launch<52,2>": 13, "f16x3: launch<52,1>": 5},
    "k5": {"h3": 11, "mfma<4>": 12, "mfma<3>": 5, "scalar<16>": 23, "scalar<32>": 16, "scalar<64>": 27},
    "k7": {"block C=128": 19, "qkv C=128": 7, "qkv C=192": 6, "qkv C=256": 8},
    "k2": {"gather L=1": 7, "gather L=3": 9, "generic float4": 14, "generic scalar": 8, "f64": 2},
}


def _all(draws_of):
    return [d for w in WHICH for d in draws_of(w)]


def _both(values, what):
    values = set(values)
    assert values == {False, True}, f"{what}: only {values} drawn"


@pytest.mark.parametrize("family", list(FAMILIES))
def test_draw_lists_are_pure_functions_of_the_seed_and_bounded(family):
    name = FAMILIES[family][0]
    first = {w: getattr(A, name)(w) for w in WHICH}
    importlib.reload(A)
    assert first == {w: getattr(A, name)(w) for w in WHICH}
    assert first[0] != first[1]
    assert all(len(set(v)) == len(v) for v in first.values())
    assert len(first[0]) == len(first[1]) <= 10                                           # `_bounded`: n draws from at most 4000 proposals, or it raises
    with pytest.raises(AssertionError):
        A._bounded(__import__("random").Random(0), 1, lambda r: 0, lambda d: False, tries=50)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_every_launch_form_is_reached_and_counted(family):
    draws, forms, every = FAMILIES[family]
    counts = A.form_counts(_all(getattr(A, draws)), getattr(A, forms))
    print(family, dict(sorted(counts.items())))
    assert set(counts) == set(every), f"{family}: forms without a case {set(every) - set(counts)}, unnamed forms {set(counts) - set(every)}"
    assert all(counts[f] > 0 for f in every)
    assert counts == COUNTS[family]
    boundary = A.form_counts(getattr(A, draws)("boundary"), getattr(A, forms))
    assert set(boundary) == set(every), f"{family}: the boundary list alone misses {set(every) - set(boundary)}"


# ---------------------------------------------------------------------------------------------------------------- 1. K3
def test_k3_draws_straddle_every_launch_rule_and_plant_their_rows():
    bd, draws = A.k3_boundary(), _all(A.k3_draws)
    assert all(min(d) >= 1 and d[0] * d[1] * d[2] * d[3] <= A.K3_WORK for d in draws)
    assert {d[2] for d in bd} >= {1, 3, 4, 143, 144, 145, 287, 288, 289}
    assert {d[1] for d in bd} >= {1, 15, 16, 17, 100, 112, 113, 127, 128, 129, 200}
    assert {d[3] for d in bd} >= {1, 3, 8, 32, 33}
    for w in range(1, 8):                                                                 # Q on both sides of every strip-count switch
        assert {16 * w, 16 * w + 1} <= {d[1] for d in bd}, w
    sixty_four = {d[2]: A.k3_plan(d[0], d[2], d[3]) for d in bd if d[0] * d[3] == 64}
    assert set(sixty_four) >= {8 * 144, 8 * 144 + 1, 16 * 144 + 1} and all(p[3] == 8 for p in sixty_four.values())
    assert [sixty_four[s][:3] for s in (8 * 144, 8 * 144 + 1, 16 * 144 + 1)] == [(1, 8, 8), (2, 5, 9), (3, 6, 17)]   # nchunks = target, target + 1, 2 target + 1
    clamped = [d for d in bd if d[0] * d[3] > 512]
    assert clamped and all(A.k3_plan(d[0], d[2], d[3])[3] == 1 and A.k3_plan(d[0], d[2], d[3])[0] == A.k3_plan(d[0], d[2], d[3])[2] > 1 for d in clamped)
    assert A.k3_plan(1, 14720, 8) == (2, 52, 103, 64)                                     # the workload's own shape
    _both((A.k3_vec_mask_tail(d[2]) for d in bd), "K3 boundary, 16-byte mask reads beside a padded chunk")
    assert {d[2] for d in bd if A.k3_vec_mask_tail(d[2])} >= {4, 148, 292} and {d[2] % 4 for d in bd} == {0, 1, 2, 3}
    assert any(d[1] > 128 and d[3] > 32 for d in bd)                                      # both fall-back reasons at once
    for s in A.SEEDS:
        _both((A.k3_plan(d[0], d[2], d[3])[2] > 1 for d in A.k3_random(s)), f"random K3 draws of seed {s}, more than one chunk")
    for d in bd[::3] + A.k3_random(0)[:3]:
        B, Q, S, nH = d
        ml = A.k3_inputs(d)["ml"]
        assert float(ml.abs().min()) > A.K3_LOGIT_MARGIN
        raw = ml.sigmoid() < 0.5
        assert bool(raw[:, 0].all()) and not bool(ref_ops.attn_mask_from_logits(ml.clone())[:, 0].any())   # fully blocked: attends everywhere
        if Q > 1:
            assert not bool(raw[:, 1].any())
        if Q > 2:
            lo = A.k3_last_chunk(S)
            assert bool(raw[:, 2, :lo].all()) and not bool(raw[:, 2, lo:].any()) and lo < S
            assert lo // A.K3_XC == (S - 1) // A.K3_XC                                    # the open keys lie in the last chunk


# ---------------------------------------------------------------------------------------------------------------- 2. K4
def test_k4_draws_straddle_every_launch_rule():
    bd, draws = A.k4_boundary(), _all(A.k4_draws)
    assert all(min(d) >= 1 and A.k4_in_budget(d) for d in draws)
    assert {d[1] for d in bd} >= {1, 16, 52, 53, 100, 104, 105, 112, 113, 150}
    assert {d[2] for d in bd} >= {1, 3, 4, 8, 32, 36, 96, 256, 288, 360, 364, 512}
    assert {d[3] for d in bd} >= {1, 2, 3, 4, 6, 510, 512, 514}
    # launch<52, 2>, each reason alone
    alone = {"N % 4 == 2": lambda B, Q, C, N: N % 4 == 2 and Q <= 112 and C % 4 == 0 and C <= 360, "Q > 112": lambda B, Q, C, N: N % 4 == 0 and Q > 112 and C % 4 == 0 and C <= 360,
             "C > 360": lambda B, Q, C, N: N % 4 == 0 and Q <= 112 and C % 4 == 0 and C > 360, "C % 4 != 0": lambda B, Q, C, N: N % 4 == 0 and Q <= 112 and C % 4 != 0}
    for why, rule in alone.items():
        assert any(rule(*d) and A.k4_form(d, "fp32") == "launch<52,2>" for d in bd), why
    ns = {B: {d[3] for d in bd if d[0] == B} for B in (1, 2, 3)}
    for B in (1, 2, 3):                                                                   # the smallest N % 4 == 0 across ceil(N / 512) B >= 256, and the one below
        n = next(n for n in range(4, 1 << 20, 4) if A.k4_wide_blocks(B, n))
        assert {n - 4, n} <= ns[B] and not A.k4_wide_blocks(B, n - 4)
    for B in (1, 3):                                                                      # N B >= 32768: the smallest even and odd N on each side
        n = math.ceil(A.K4_CT_WORK / B)
        assert {n - 2, n - 1, n, n + 1} <= ns[B] or {n - 1, n, n + 1, n + 2} <= ns[B]
        assert {A.k4_ct(B, m) for m in (n - 2, n - 1)} == {1} and {A.k4_ct(B, m) for m in (n, n + 1)} == {1, 2}
        first = next(m for m in range(1, 1 << 20) if A.k4_persistent(B, m))               # the f16x3 kernel turns persistent; 1 and 2 columns beyond
        assert {first - 1, first, first + 1, first + 2} <= ns[B] and not A.k4_persistent(B, first - 1)
        two = next(m for m in range(2, 1 << 20, 2) if A.k4_ct(B, m) == 2 and A.k4_persistent(B, m))
        assert {two - 2, two, two + 2} <= ns[B] and not A.k4_persistent(B, two - 2) and A.k4_ct(B, two - 2) == 2
    assert A.k4_form((1, 100, 256, 256 * 512), "f16x3") == "h3<2,2> persistent" and A.k4_form((1, 100, 256, 128 * 512), "f16x3") == "h3<2,2>"   # the workload's own
    assert A.k4_form((1, 100, 256, 32 * 64), "f16x3") == "h3<1,2>" and A.k4_form((1, 100, 256, 256 * 512), "fp32") == "mfma<8,2>"


# ---------------------------------------------------------------------------------------------------------------- 3. K5
def test_k5_draws_cover_every_geometry_and_keep_qkv_exact():
    bd, draws = A.k5_boundary(), _all(A.k5_draws)
    assert all(A.k5_in_domain(d) for d in draws)
    assert {(d[5], d[3]) for d in bd} >= {(hd, ws) for hd in A.K5_HD for ws in A.K5_WS}
    assert {d[0] for d in bd} == set(A.K5_B) and {d[4] for d in bd} == set(A.K5_NH)
    for ws in A.K5_WS:
        mine = [d for d in bd if d[3] == ws]
        assert {d[1] for d in mine} | {d[2] for d in mine} >= set(A.k5_sizes(ws)), ws
        assert {d[6] for d in mine} >= set(A.k5_shifts(ws)), ws
    for rel in range(6):                                                                  # each relative size on each axis, somewhere
        size = lambda ws: (1, ws - 1, ws, ws + 1, 2 * ws, 2 * ws + 1)[rel]
        assert any(d[1] == size(d[3]) for d in bd) and any(d[2] == size(d[3]) for d in bd), rel
    assert any(d[3] == 8 and d[5] == 32 and d[1] % 8 == 0 and d[2] % 8 == 0 for d in bd)   # N = 64, no padded key, no padded token
    scalar = [d for d in bd if A.k5_form(d).startswith("scalar")]
    _both((A.k5_scalar_lds(d) > A.K5_LDS_CAP for d in scalar), "K5 scalar forms, LDS tile above 64 KiB")
    assert {(d[5], d[3]) for d in scalar if A.k5_scalar_lds(d) > A.K5_LDS_CAP} >= {(32, 16), (64, 12), (64, 13), (64, 16)}
    assert max(A.k5_scalar_lds(d) for d in draws) <= 160 * 1024
    split = [d for d in bd if A.k5_split_ok(d)]
    assert len(split) >= 4 and all(A.k5_form(d) == "h3" for d in split)
    _both(((d[0] * d[1] * d[2]) % 32 == 0 for d in split), "K5 split_out cases, whole 32-row groups only")
    for s in A.SEEDS:
        _both((A.k5_takes_frag(d) for d in A.k5_random(s)), f"random K5 draws of seed {s}, matrix-pipe form")
    for d in bd[::5] + A.k5_random(0)[:3]:
        inp = A.k5_inputs(d)
        assert torch.equal(inp["qkv"].double(), F.linear(inp["x"].double(), inp["qkv_w"].double(), inp["qkv_b"].double())), d


# ---------------------------------------------------------------------------------------------------------------- 4. K7
def test_k7_draws_cover_both_entry_points_and_restate_the_reference():
    bd, draws = A.k7_boundary(), _all(A.k7_draws)
    assert all(A.k7_in_domain(d) and d[2] * d[3] * d[4] <= A.K7_TOKENS for d in draws)
    assert all(set(A.K7_SUPPORTED[e]) <= set(A.K7_C) for e in A.K7_SUPPORTED) and set(A.K7_C) - set(A.K7_SUPPORTED["qkv"]) == {96, 384}
    for entry in ("block", "qkv"):
        mine = [d for d in bd if d[0] == entry]
        assert {d[3] for d in mine} >= set(A.K7_SIZES) and {d[4] for d in mine} >= set(A.K7_SIZES), entry
        assert {d[2] for d in mine} == {1, 2, 3} and {d[5] for d in mine} == set(A.K7_SHIFTS), entry
        rows = [d[2] * d[3] * d[4] for d in mine]
        assert any(r < 32 for r in rows) and any(r > 32 and r % 32 for r in rows) and any(r % 32 == 0 for r in rows), entry
    for d in (("block", 128, 2, 12, 13, 1), ("qkv", 192, 1, 1, 11, 0)):
        inp = A.k7_inputs(d)
        for mine, theirs in zip(A.k7_restate(d, inp, torch.float64), A.k7_reference(d, inp)):
            assert torch.equal(mine, theirs), d
    inp = A.k7_inputs(("qkv", 192, 1, 1, 11, 0))
    assert torch.equal(inp["proj_w"], torch.eye(192)) and not inp["proj_b"].any()


# ---------------------------------------------------------------------------------------------------------------- 5. K2
def test_k2_draws_cover_every_form_and_plant_their_locations():
    bd, draws = A.k2_boundary(), _all(A.k2_draws)
    assert all(A.k2_in_domain(d) for d in draws)
    assert all(max(max(s) for s in d[4]) <= 24 for d in draws)                            # fp32 pixel coordinates stay below 24: their rounding stays inside the bound
    assert {(d[2], len(d[4]), d[5]) for d in bd if d[6] == "f32"} == set(A.K2_DLP)
    assert {d[1] for d in bd} == {1, 3, 8} and {d[0] for d in bd} == {1, 2, 3}
    assert sum(d[6] == "f64" for d in bd) == 2
    size = lambda d: sum(h * w for h, w in d[4])
    for form in ("gather L=1", "gather L=3"):
        mine = [d for d in bd if A.k2_form(d) == form]
        assert {d[3] for d in mine if d[3] != size(d)} >= {1, 31, 32, 33} and any(d[3] == size(d) for d in mine), form
    for form in A.K2_FORMS[:4]:
        assert any(any(1 in s for s in d[4]) for d in bd if A.k2_form(d) == form), f"{form}: no level with a 1-pixel axis"
    levels = {s for d in bd for s in d[4]}
    assert (1, 1) in levels and any(h == 1 and w > 1 for h, w in levels) and any(w == 1 and h > 1 for h, w in levels)
    for s in A.SEEDS:
        _both((A.k2_form(d).startswith("gather") for d in A.k2_random(s)), f"random K2 draws of seed {s}, gather form")
    seen = set()
    for d in draws:
        inp = A.k2_inputs(d)
        seen |= inp["planted"]
        assert len(inp["planted"]) >= 2 or inp["loc"].numel() < 16, d
        assert float(inp["loc"].min()) < 0.0 < 1.0 < float(inp["loc"].max()) or inp["loc"].numel() < 64
    assert seen == set(A.K2_PLANTED)
    inp = A.k2_inputs(bd[4])                                                              # (1, 3, 32, 35, 5 x 7, 4): the planted values are what they say
    pix = inp["loc"] * torch.tensor([7.0, 5.0]) - 0.5                                  # fp32, as the kernel computes it
    assert bool((pix == pix.round()).all(-1).any()) and bool(((pix + 1.0).abs() < 1e-6).any()) and bool((pix.abs() > 1e4).any())
    assert bool(((pix + 0.5) == (pix + 0.5).round()).all(-1).any())


# ---------------------------------------------------------------------------------------------------------------- the references alone
def _self_consistent(t64, b, bound, what):
    assert torch.isfinite(t64).all() and math.isfinite(b) and b >= 0.0, what
    assert b * float(t64.abs().max()) < bound, f"{what}: fp32 CPU torch itself misses the bound"


def test_reference_alone_k3_k4():
    for d in A.k3_boundary()[::6] + A.k3_random(0)[:2]:
        for name, (t64, b) in A.k3_truth(d).items():
            _self_consistent(t64, b, A.K3_BOUND, f"K3 {d} {name}")
    for d in A.k4_boundary()[:19:3] + A.k4_random(1)[:2]:
        t64, b = A.k4_truth(d)
        _self_consistent(t64, b, A.k4_bound(d[2]), f"K4 {d}")


def test_reference_alone_k5_k7_k2():
    for d in A.k5_boundary()[::7] + A.k5_random(0)[:2]:
        t64, b = A.k5_truth(d)
        _self_consistent(t64, b, A.K5_BOUND, f"K5 {d}")
    for d in A.k7_boundary()[1::9] + A.k7_random(1)[3:4]:
        x64, y64, bx, by = A.k7_truth(d)
        _self_consistent(x64, bx, A.K7_BOUND_X, f"K7 {d} x")
        _self_consistent(y64, by, A.K7_BOUND_Y2, f"K7 {d} y2")
    for d in A.k2_boundary()[::4] + A.k2_random(0)[:2]:
        t64, b = A.k2_truth(d)
        _self_consistent(t64, b, A.K2_BOUND if d[6] == "f32" else 1.0, f"K2 {d}")
