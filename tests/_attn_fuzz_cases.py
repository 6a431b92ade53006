"""Shared by tests/test_attention_kernel_fuzz_cpu.py and tests/test_attention_kernel_fuzz_gpu.py: the shape generators of the random-shape sweep
of the forward attention kernels -- K3 masked cross-attention, K4 mask logits, K5 Swin window attention, K7 the fused Swin attention half block and
K2 deformable attention -- the launch rules those shapes have to straddle, restated from the launchers (the launcher is the truth: the CPU test
pins the count of cases per launch form, so a rule that moves is seen), the input builders and the fp64 truths.  Pure Python and torch.

Every family draws a fixed BOUNDARY list first and then seeded random shapes (``random.Random(seed)``, seeds 0 and 1).  `form_of`-style functions
(`k3_form`, `k4_form`, `k5_form`, `k7_form`, `k2_form`) name the launch form a case takes.

Truth = the oracle's torch restatement of the operation on ``.double()`` of the very inputs.  The metric is the training sweep's
(tests/_train_fuzz_cases.py): e(T) = max|T - T64| / max|T64|, b = the same for fp32 CPU torch on the same inputs.  What is ASSERTED is the absolute
bound of the family's fixed-shape test in tests/test_kernels_gpu.py, on that test's input distribution; e, b and e / max(b, 2^-24) are RECORDED per
family and form (`check`, `report`) for docs/measurements.md.  No draw and no element is left out.
"""
import functools
import random

import torch
import torch.nn.functional as F

from oracle import ref_ops
from tests import _train_fuzz_cases as T
from tests.test_kernels_gpu import _k7_reference                 # K7's fp64 restatement lives with its fixed-shape test

SEEDS = T.SEEDS
err, b_of, shuffled = T.err, T.b_of, T.shuffled                   # one metric, one order
_bounded, _stable_seed, _around = T._bounded, T._stable_seed, T._around

B_FLOOR = 2.0 ** -24                                              # e / b is recorded against max(b, half an fp32 ulp): fp32 torch is exact at the tiniest shapes

RECORDS = {}                                                      # family -> form -> {"draws", "e", "b", "ratio"}: the worst of what `check` saw


def _rec(family, form):
    return RECORDS.setdefault(family, {}).setdefault(form, {"draws": 0, "e": 0.0, "b": 0.0, "ratio": 0.0})


def count_draw(family, form, n=1):
    _rec(family, form)["draws"] += n


def check(family, form, what, t, t64, b, bound, quiet=True):
    """max|T - T64| < bound, every element finite; records e(T), its b and e / max(b, 2^-24) under (family, form)"""
    t = t.detach().cpu()
    assert tuple(t.shape) == tuple(t64.shape), f"{family} {what}: shape {tuple(t.shape)} != {tuple(t64.shape)}"
    d, e = float((t.double() - t64).abs().max()), err(t, t64)
    ratio = e / max(b, B_FLOOR)
    if not quiet:
        print(f"{family} [{form}] {what}: max|d| = {d:.3e}  bound = {bound:.3e}  e = {e:.3e}  b = {b:.3e}  e/b = {ratio:.2f}")
    rec = _rec(family, form)
    if e > rec["e"]:
        rec["e"], rec["b"] = e, b
    rec["ratio"] = max(rec["ratio"], ratio)
    assert torch.isfinite(t).all(), f"{family} [{form}] {what}: not finite"
    assert d < bound, f"{family} [{form}] {what}: max|d| = {d:.3e} >= {bound:.3e} (e = {e:.3e}, b = {b:.3e})"
    return d


def report(family):
    forms = RECORDS.get(family, {})
    if forms:
        parts = [f"{form}: draws {r['draws']} worst e = {r['e']:.3e} (its b = {r['b']:.3e}) worst e/b = {r['ratio']:.2f}" for form, r in sorted(forms.items())]
        print(f"RECORD {family}: draws {sum(r['draws'] for r in forms.values())} | " + " | ".join(parts))


def form_counts(cases, form_of):
    out = {}
    for c in cases:
        for f in form_of(c):
            out[f] = out.get(f, 0) + 1
    return out


def _ceil(a, b):
    return (a + b - 1) // b


# ================================================================================================ 1. K3: masked cross-attention
# masked_xattn.hip, rba_masked_xattn_f32: with a workspace (split_keys=True), Q <= 128 and nH <= 32 the three-launch matrix-pipe form -- row flags,
# xattn_partial_mfma_kernel<W> with W = min(ceil(Q / 16), 8) waves of 16-query strips, merge -- otherwise (no workspace, Q > 128 or nH > 32) the
# scalar kernel, one workgroup per (query, head).  xattn_plan: keys in chunks of XC = 144; target = max(1, 512 / (nH B)) splits; chunks_per_split =
# ceil(nchunks / target); splits = ceil(nchunks / chunks_per_split).  The mask row is read 16 bytes at a time where S % 4 == 0 and k0i + 3 < S.
K3_XC, K3_MAX_Q, K3_MAX_NH, K3_BOUND, K3_WORK = 144, 128, 32, 5e-6, 1_500_000
K3_FORMS = ("scalar",) + tuple(f"mfma-partial {w} strips" for w in range(1, 9)) + ("fall-back Q > 128", "fall-back nH > 32")
K3_LOGIT_MARGIN = 2.0 ** -20


def k3_plan(B, S, nH):
    """xattn_plan -> (chunks_per_split, splits, nchunks, target)"""
    nchunks = _ceil(S, K3_XC)
    target = max(1, 512 // (nH * B))
    cps = max(1, _ceil(nchunks, target))
    return cps, _ceil(nchunks, cps), nchunks, target


def k3_form(case, split):
    B, Q, S, nH = case
    if not split:
        return "scalar"
    if Q > K3_MAX_Q:
        return "fall-back Q > 128"
    if nH > K3_MAX_NH:
        return "fall-back nH > 32"
    return f"mfma-partial {min(_ceil(Q, 16), 8)} strips"


def k3_forms(case):
    return (k3_form(case, True), k3_form(case, False))


def k3_vec_mask_tail(S):
    """16-byte mask reads that stop next to the row tail: S % 4 == 0 and the last chunk is padded (k0i + 3 < S fails only beyond the row)"""
    return S % 4 == 0 and S % K3_XC != 0


def k3_boundary():
    """(B, Q, S, nH).  S in {1, 3, 4, 143 .. 145, 287 .. 289} and 144 k + 4 (vector mask reads beside a padded chunk); B nH = 64 (target 8) at
    nchunks = 8, 9, 17 (chunks_per_split 1, 2, 3); B nH = 544 > 512 (target clamps to 1); every strip count, Q on both sides of each; both fall-backs"""
    return ((1, 5, 1, 1), (1, 3, 3, 1), (2, 4, 4, 3), (1, 15, 143, 1), (1, 16, 144, 8), (1, 17, 145, 3), (1, 100, 287, 8), (1, 7, 288, 1),
            (1, 112, 289, 1), (1, 113, 148, 3), (1, 127, 292, 1), (1, 128, 145, 8), (1, 1, 289, 32), (1, 129, 145, 3), (1, 200, 289, 1),
            (1, 5, 145, 33), (1, 130, 77, 33), (1, 2, 144, 1),
            (1, 32, 146, 1), (1, 33, 145, 1), (1, 48, 77, 2), (1, 49, 200, 1), (1, 64, 150, 3), (1, 65, 144, 1), (1, 80, 300, 1), (1, 81, 143, 2),
            (1, 96, 146, 1), (1, 97, 160, 1),
            (2, 20, 8 * 144, 32), (8, 9, 8 * 144 + 1, 8), (2, 6, 16 * 144 + 1, 32), (17, 4, 289, 32))


def k3_random(seed, n=8):
    def draw(r):
        S = r.choice([r.randint(1, 2400), _around(r, (144, 288, 432, 1152), 2), 4 * r.randint(1, 300)])
        Q = r.choice([r.randint(1, 140), _around(r, (16, 112, 128), 1)])
        return (r.choice((1, 2, 3)), Q, S, r.choice((1, 2, 3, 8, 8, 32, 33)))
    return _bounded(random.Random(700 + seed), n, draw, lambda d: d[0] * d[1] * d[2] * d[3] <= K3_WORK)


def k3_draws(which):
    """which: "boundary" | a seed"""
    return k3_boundary() if which == "boundary" else k3_random(which)


def k3_last_chunk(S):
    """first key of the row whose only open keys lie in the last chunk (one chunk: its last key alone)"""
    start = (_ceil(S, K3_XC) - 1) * K3_XC
    return start if start > 0 else S - 1


@functools.lru_cache(maxsize=64)
def k3_inputs(case):
    """dict(q, k, v, ml), fp32 on the CPU: `test_k3_masked_xattn`'s distribution (randn, logits randn * 3) with its planted rows -- row 0 fully
    blocked (it attends everywhere), row 1 (Q > 1) fully open, row 2 (Q > 2) open only from `k3_last_chunk` on.  No logit within 2^-20 of zero:
    the fixture is re-drawn with the next seed otherwise (decisions on the threshold stay with test_k3_threshold_decision_at_the_boundary)."""
    B, Q, S, nH = case
    for attempt in range(16):
        g = torch.Generator().manual_seed(_stable_seed(3, B, Q, S, nH, attempt))
        q, k, v = (torch.randn(B, n, nH, 32, generator=g) for n in (Q, S, S))
        ml = torch.randn(B, Q, S, generator=g) * 3
        ml[:, 0] = -5.0
        if Q > 1:
            ml[:, 1] = 5.0
        if Q > 2:
            lo = k3_last_chunk(S)
            ml[:, 2, :lo] = -5.0
            ml[:, 2, lo:] = 5.0
        if float(ml.abs().min()) > K3_LOGIT_MARGIN:
            return dict(q=q, k=k, v=v, ml=ml)
    raise AssertionError(f"K3 fixture {case}: a logit within 2^-20 of zero in 16 seeds")


@functools.lru_cache(maxsize=64)
def k3_truth(case):
    """{"mask": (T64, b), "none": (T64, b)}; the blocked set is taken in fp32 on the kernel's own logits"""
    inp = k3_inputs(case)
    q, k, v = inp["q"], inp["k"], inp["v"]
    out = {}
    for name, blocked in (("mask", ref_ops.attn_mask_from_logits(inp["ml"].clone())), ("none", None)):
        t64 = ref_ops.attention_core(q.double(), k.double(), v.double(), blocked)
        out[name] = (t64, b_of(ref_ops.attention_core(q, k, v, blocked), t64))
    return out


# ================================================================================================ 2. K4: mask logits
# mask_logits.hip.  rba_mask_logits_f32: Q <= 112, C % 4 == 0, C <= 360 and N % 4 == 0 (and 16-byte aligned pointers) take the matrix pipe,
# launch_mfma<8, 2> when ceil(N / 512) B >= 256, otherwise launch_mfma<4, 4>; everything else the VALU kernel, launch<52, 2> for even N,
# launch<52, 1> for odd N.  rba_mask_logits_f16x3_f32: Q <= 112, C % 32 == 0 and C <= 256 take mask_logits_h3_kernel<CT, PF, 8> -- CT = 2 columns
# per lane when N is even and N B >= 32768, otherwise 1; PF = 2 when C / 32 is even, otherwise 1; wave tiles of 16 CT columns, 8 to a workgroup,
# persistent once the workgroups exceed 256 / B (rba_even_grid) -- and every other shape the exact-fp32 entry above.
K4_MAX_Q, K4_MAX_C, K4_H3_MAX_C, K4_CT_WORK, K4_CAP, K4_WAVES = 112, 360, 256, 32768, 256, 8
K4_BYTES, K4_WORK = 64 << 20, 300_000_000
K4_MODES = ("fp32", "f16x3")
K4_FP32_FORMS = ("mfma<8,2>", "mfma<4,4>", "launch<52,2>", "launch<52,1>")
K4_H3_FORMS = tuple(f"h3<{ct},{pf}>{p}" for ct in (1, 2) for pf in (1, 2) for p in ("", " persistent"))


def k4_wide_blocks(B, N):
    """the 8-wave against 4-wave switch of the exact-fp32 matrix-pipe kernel"""
    return _ceil(N, 512) * B >= 256


def k4_ct(B, N):
    return 2 if N % 2 == 0 and N * B >= K4_CT_WORK else 1


def k4_persistent(B, N):
    wave_tiles = _ceil(N, 16 * k4_ct(B, N))
    return _ceil(wave_tiles, K4_WAVES) > (1 if B >= K4_CAP else K4_CAP // B)


def k4_form(case, mode):
    B, Q, C, N = case
    if mode == "f16x3" and Q <= K4_MAX_Q and C % 32 == 0 and C <= K4_H3_MAX_C:
        return f"h3<{k4_ct(B, N)},{2 if (C // 32) % 2 == 0 else 1}>" + (" persistent" if k4_persistent(B, N) else "")
    if Q <= K4_MAX_Q and C % 4 == 0 and C <= K4_MAX_C and N % 4 == 0:
        return "mfma<8,2>" if k4_wide_blocks(B, N) else "mfma<4,4>"
    return "launch<52,2>" if N % 2 == 0 else "launch<52,1>"


def k4_forms(case):
    return tuple(f"{mode}: {k4_form(case, mode)}" for mode in K4_MODES)


def k4_bound(C):
    return 2e-4 * (C / 256) ** 0.5 + 1e-5


def k4_in_budget(case):
    B, Q, C, N = case
    return (Q + C) * N * B * 4 <= K4_BYTES and B * Q * C * N <= K4_WORK


def k4_boundary():
    """(B, Q, C, N).  Small shapes: every Q, C and N the rules name, launch<52, 2> for each of its four reasons (N % 4 == 2, Q > 112, C > 360,
    C % 4 != 0).  Long rows at small Q and C: both sides of ceil(N / 512) B >= 256 for B = 1, 2, 3, of N B >= 32768 (even and odd N), and of the
    persistent grid of the f16x3 kernel for B = 1, 3 at one and at two columns per lane, with one and two columns beyond"""
    small = ((1, 1, 1, 1), (2, 16, 3, 2), (1, 52, 4, 3), (3, 53, 8, 4), (1, 100, 32, 6), (1, 104, 36, 510), (2, 105, 96, 512), (1, 112, 256, 514),
             (1, 113, 288, 512), (1, 150, 360, 510), (1, 112, 364, 512), (1, 100, 512, 4), (1, 113, 64, 6), (1, 112, 360, 516), (1, 16, 256, 6),
             (1, 100, 3, 512), (2, 112, 64, 3), (1, 105, 128, 2), (3, 100, 256, 512))
    wide = ((1, 16, 32, 255 * 512), (1, 16, 32, 255 * 512 + 4), (2, 16, 64, 127 * 512), (2, 16, 64, 127 * 512 + 4), (3, 16, 8, 85 * 512),
            (3, 16, 8, 85 * 512 + 4))
    ct = ((1, 100, 32, 32766), (1, 16, 64, 32767), (1, 112, 32, 32768), (1, 16, 64, 32770), (3, 16, 32, 10921), (3, 16, 64, 10922),
          (3, 16, 32, 10923), (3, 16, 64, 10924))
    persistent = ((1, 16, 32, 32769), (1, 16, 64, 32771), (1, 16, 64, 65536), (1, 16, 32, 65538), (1, 16, 64, 65540),
                  (3, 16, 32, 10880), (3, 16, 32, 10881), (3, 16, 64, 10882), (3, 16, 32, 10883), (3, 16, 64, 21760), (3, 16, 64, 21762), (3, 16, 32, 21764))
    return small + wide + ct + persistent


def k4_random(seed, n=8):
    def draw(r):
        N = r.choice([r.randint(1, 3000), _around(r, (512, 1024), 3), 4 * r.randint(1, 700), r.randint(30000, 70000)])
        Q = r.choice([_around(r, (52, 104, 112)), r.randint(1, 150)]) if N < 30000 else r.randint(1, 40)
        C = r.choice([4 * r.randint(1, 90), 32 * r.randint(1, 8), r.randint(1, 520)]) if N < 30000 else r.choice((32, 64, 96, r.randint(1, 40)))
        return (r.choice((1, 2, 3)), Q, C, N)
    return _bounded(random.Random(800 + seed), n, draw, k4_in_budget)


def k4_draws(which):
    return k4_boundary() if which == "boundary" else k4_random(which)


@functools.lru_cache(maxsize=8)
def k4_inputs(case):
    """(embed [B,Q,C], feat [B,C,N]): `test_k4_mask_logits`'s distribution (randn)"""
    B, Q, C, N = case
    g = torch.Generator().manual_seed(_stable_seed(4, B, Q, C, N))
    return torch.randn(B, Q, C, generator=g), torch.randn(B, C, N, generator=g)


@functools.lru_cache(maxsize=8)
def k4_truth(case):
    e, f = k4_inputs(case)
    t64 = torch.einsum("bqc,bcn->bqn", e.double(), f.double())
    return t64, b_of(torch.einsum("bqc,bcn->bqn", e, f), t64)


# ================================================================================================ 3. K5: Swin window attention
# swin_window_attn.hip, rba_swin_window_attn_f32: head_dim in {16, 32, 64}, ws^2 <= 256, 0 <= shift < ws.  head_dim 32 takes the matrix pipe by
# NT = ceil(ws^2 / 16): 9 -> the f16x3 kernel (launch_h3<9, 9>), 4 -> launch_mfma<4, 4>, 3 -> launch_mfma<3, 3>; every other geometry the scalar
# kernel swin_window_attn_kernel<head_dim>, whose K and V tile (2 N head_dim floats + N region ids) is dynamic LDS -- up to 132 096 B, launched
# without raising a per-kernel cap (the runtime takes it on gfx950: 160 KiB per workgroup), so the sweep stands on both sides of 64 KiB.
# bias_frag is read by the matrix-pipe forms only; split_out needs head_dim 32 and ws 12.
K5_WS, K5_HD, K5_B, K5_NH, K5_BOUND, K5_LDS_CAP = (1, 2, 5, 6, 7, 8, 9, 12, 13, 16), (16, 32, 64), (1, 2, 3), (1, 3, 6), 1e-5, 64 * 1024
K5_FORMS = ("h3", "mfma<4>", "mfma<3>", "scalar<16>", "scalar<32>", "scalar<64>")


def k5_form(case):
    B, H, W, ws, nH, hd, shift = case
    nt = _ceil(ws * ws, 16)
    if hd == 32 and nt in (9, 4, 3):
        return "h3" if nt == 9 else f"mfma<{nt}>"
    return f"scalar<{hd}>"


def k5_forms(case):
    return (k5_form(case),)


def k5_takes_frag(case):
    return not k5_form(case).startswith("scalar")


def k5_split_ok(case):
    return case[5] == 32 and case[3] == 12                           # ops.swin_window_attn_split_ok


def k5_scalar_lds(case):
    """dynamic LDS bytes of the scalar kernel"""
    ws, hd = case[3], case[5]
    return 2 * ws * ws * hd * 4 + ws * ws * 4


def k5_in_domain(case):
    B, H, W, ws, nH, hd, shift = case
    return B >= 1 and H >= 1 and W >= 1 and nH >= 1 and hd in K5_HD and 1 <= ws and ws * ws <= 256 and 0 <= shift < ws


def k5_sizes(ws):
    return tuple(sorted({v for v in (1, ws - 1, ws, ws + 1, 2 * ws, 2 * ws + 1) if v >= 1}))


def k5_shifts(ws):
    return tuple(sorted({s for s in (0, 1, ws // 2, ws - 1) if 0 <= s < ws}))


def k5_boundary():
    """(B, H, W, ws, nH, head_dim, shift): two cases per (head_dim, ws) with H, W, shift, B and nH cycling through their lists on co-prime strides,
    then the listed ones -- ws = 8 (N = 64: exactly four full key tiles), more of the matrix-pipe forms, whole and broken 32-row groups for
    split_out, and the shapes whose scalar tile exceeds 64 KiB of LDS (head_dim 32 at ws 16, head_dim 64 from ws 12)"""
    out = []
    for hi, hd in enumerate(K5_HD):
        for wi, ws in enumerate(K5_WS):
            sizes, shifts = k5_sizes(ws), k5_shifts(ws)
            for k in (2 * hi, 2 * hi + 1):                                                  # k = 0 .. 5 over the six cases of a window size
                out.append((K5_B[(k + wi) % 3], sizes[k % len(sizes)], sizes[(k + 1 + wi) % len(sizes)], ws, K5_NH[(k // 2 + wi) % 3], hd, shifts[k % len(shifts)]))
    out += [(2, 8, 8, 8, 3, 32, 0), (1, 16, 9, 8, 1, 32, 4), (1, 17, 7, 8, 6, 32, 7),
            (2, 7, 13, 6, 3, 32, 3), (1, 5, 6, 6, 1, 32, 5), (3, 12, 1, 6, 6, 32, 1), (2, 15, 7, 7, 3, 32, 3),
            (1, 12, 12, 12, 1, 32, 0), (3, 1, 11, 12, 3, 32, 6), (2, 13, 25, 12, 6, 32, 11), (1, 24, 12, 12, 3, 32, 1),
            (1, 16, 17, 16, 1, 32, 8), (1, 13, 12, 12, 3, 64, 6), (2, 17, 16, 16, 1, 64, 15), (1, 14, 13, 13, 1, 64, 0)]
    return tuple(dict.fromkeys(out))


def k5_random(seed, n=10):
    turn = iter(range(1 << 30))

    def draw(r):
        pipe = next(turn) % 3 == 0                                         # one draw in three in a matrix-pipe form, the others anywhere
        ws = r.choice((6, 7, 8, 12, 12)) if pipe else r.randint(1, 16)
        return (r.choice(K5_B), r.randint(1, 2 * ws + 3), r.randint(1, 2 * ws + 3), ws, r.choice(K5_NH), 32 if pipe else r.choice(K5_HD), r.randint(0, ws - 1))
    return _bounded(random.Random(900 + seed), n, draw, k5_in_domain)


def k5_draws(which):
    return k5_boundary() if which == "boundary" else k5_random(which)


def _on_grid(t, steps, limit):
    """`t` rounded to multiples of 1 / steps and clipped to +- limit"""
    return (t * steps).round().clamp(-limit * steps, limit * steps) / steps


@functools.lru_cache(maxsize=64)
def k5_inputs(case):
    """dict(x [B,HW,C], qkv_w, qkv_b, table, qkv, bias), fp32 on the CPU: `test_k5_window_attn_core`'s distribution, with x, the weight and the
    bias of the qkv Linear on binary grids (1/8 within +-4, 1/128 within +-1, 1/256) so that every sum of the Linear is an fp32 number: the qkv
    tensor the kernel reads is then EXACTLY what the fp64 truth computes from x (asserted by the CPU test), and the truth is one of the very inputs"""
    B, H, W, ws, nH, hd, shift = case
    C, N = nH * hd, ws * ws
    g = torch.Generator().manual_seed(_stable_seed(5, *case))
    x = _on_grid(torch.randn(B, H * W, C, generator=g), 8, 4)
    qkv_w = _on_grid(torch.randn(3 * C, C, generator=g) * C ** -0.5, 128, 1)
    qkv_b = _on_grid(torch.randn(3 * C, generator=g) * 0.2, 256, 1)
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5
    bias = table[ref_ops.relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).contiguous()
    return dict(x=x, qkv_w=qkv_w, qkv_b=qkv_b, table=table, qkv=F.linear(x, qkv_w, qkv_b), bias=bias)


def k5_restate(case, inp, dtype):
    """`test_k5_window_attn_core`'s oracle: pad -> roll -> partition -> window attention (identity proj) -> reverse -> un-roll -> crop"""
    B, H, W, ws, nH, hd, shift = case
    C = nH * hd
    x, qkv_w, qkv_b, table = (inp[k].to(dtype) for k in ("x", "qkv_w", "qkv_b", "table"))
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    xp = F.pad(x.view(B, H, W, C), (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = xp.shape[1], xp.shape[2]
    if shift:
        xp = torch.roll(xp, (-shift, -shift), (1, 2))
    xw = xp.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    mask = ref_ops.shift_attn_mask(H, W, ws, shift).to(dtype) if shift else None
    aw = ref_ops.window_attention(xw, qkv_w, qkv_b, torch.eye(C, dtype=dtype), torch.zeros(C, dtype=dtype), table, ws, nH, mask)
    y = aw.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    return y[:, :H, :W].reshape(B, H * W, C)


@functools.lru_cache(maxsize=64)
def k5_truth(case):
    inp = k5_inputs(case)
    t64 = k5_restate(case, inp, torch.float64)
    return t64, b_of(k5_restate(case, inp, torch.float32), t64)


# ================================================================================================ 4. K7: the fused Swin attention half block
# swin_attn_block.hip: 12 x 12 windows, head_dim 32, f16x3 mode.  rba_swin_attn_block_supported: C == 128; rba_swin_attn_qkv_supported: C in
# {128, 192, 256}.  Both entry points accept every 0 <= shift < 12.  One workgroup per window; the qkv entry writes SplitActivations, whose rows
# come in groups of 32 (the last group's padding rows are not written).
K7_WS, K7_C, K7_SIZES, K7_SHIFTS, K7_TOKENS = 12, (96, 128, 192, 256, 384), (1, 11, 12, 13, 24, 25, 37), (0, 6, 1, 11), 2600
K7_SUPPORTED = {"block": (128,), "qkv": (128, 192, 256)}
K7_FORMS = tuple(f"{entry} C={C}" for entry in ("block", "qkv") for C in K7_SUPPORTED[entry])
K7_BOUND_X, K7_BOUND_Y2, K7_BOUND_UNFUSED = 2e-5, 3e-5, 1e-5


def k7_form(case):
    return f"{case[0]} C={case[1]}"


def k7_forms(case):
    return (k7_form(case),)


def k7_in_domain(case):
    entry, C, B, H, W, shift = case
    return C in K7_SUPPORTED[entry] and B >= 1 and H >= 1 and W >= 1 and 0 <= shift < K7_WS


def k7_boundary():
    """(entry, C, B, H, W, shift): every supported C of both entry points; H and W through {1, 11, 12, 13, 24, 25, 37}; B H W = 1, 33, 37 (below and
    beside one 32-row group) and multiples of 32; shifts 0, 6, 1, 11"""
    block = ((1, 1, 1, 0), (1, 11, 12, 6), (2, 12, 13, 1), (3, 13, 11, 11), (1, 24, 25, 6), (2, 25, 24, 0), (1, 37, 1, 6), (1, 12, 37, 1),
             (3, 1, 11, 0), (1, 37, 37, 11), (2, 24, 12, 6), (1, 13, 13, 0))
    qkv = {128: ((1, 1, 1, 6), (2, 11, 13, 0), (1, 12, 24, 1), (3, 25, 1, 11), (1, 37, 12, 6), (1, 24, 37, 0)),
           192: ((1, 1, 11, 0), (2, 13, 11, 6), (1, 24, 12, 11), (3, 1, 25, 1), (1, 12, 37, 0), (1, 37, 24, 6)),
           256: ((2, 1, 1, 0), (1, 11, 11, 11), (3, 12, 12, 6), (1, 13, 25, 1), (2, 24, 24, 0), (1, 37, 37, 6))}
    return tuple(("block", 128) + c for c in block) + tuple(("qkv", C) + c for C in K7_SUPPORTED["qkv"] for c in qkv[C])


def k7_random(seed, n=5):
    def draw(r):
        entry = r.choice(("block", "qkv"))
        return (entry, r.choice(K7_SUPPORTED[entry]), r.choice((1, 2, 3)), r.randint(1, 40), r.randint(1, 40), r.choice(K7_SHIFTS + (r.randint(0, 11),)))
    return _bounded(random.Random(1000 + seed), n, draw, lambda d: d[2] * d[3] * d[4] <= K7_TOKENS)


def k7_draws(which):
    return k7_boundary() if which == "boundary" else k7_random(which)


@functools.lru_cache(maxsize=16)
def k7_inputs(case):
    """`test_k7_swin_attn_block`'s distribution; the qkv entry point has no proj and no norm2: identity and zero there, so that the one truth is
    x + attention for both"""
    entry, C, B, H, W, shift = case
    nH, ws = C // 32, K7_WS
    g = torch.Generator().manual_seed(_stable_seed(7, C, B, H, W, shift, entry == "qkv"))
    x = torch.randn(B, H * W, C, generator=g) * 1.5 + 0.3
    n1 = (torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2, 1e-5)
    n2 = (torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2, 1e-5)
    qkv_w, qkv_b = torch.randn(3 * C, C, generator=g) * C ** -0.5, torch.randn(3 * C, generator=g) * 0.2
    proj_w, proj_b = torch.randn(C, C, generator=g) * C ** -0.5, torch.randn(C, generator=g) * 0.2
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5
    if entry == "qkv":
        proj_w, proj_b, n2 = torch.eye(C), torch.zeros(C), (torch.ones(C), torch.zeros(C), 1e-5)
    N = ws * ws
    bias = table[ref_ops.relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).contiguous()
    return dict(x=x, n1=n1, n2=n2, qkv_w=qkv_w, qkv_b=qkv_b, proj_w=proj_w, proj_b=proj_b, table=table, bias=bias)


def k7_restate(case, inp, dtype):
    """`_k7_reference` in `dtype` (it computes in fp64 only; the CPU test asserts that this one equals it there, bit for bit) -> (x, y2)"""
    entry, C, B, H, W, shift = case
    nH, ws, L = C // 32, K7_WS, H * W
    c = lambda t: t.to(dtype)
    x, n1, n2 = c(inp["x"]), inp["n1"], inp["n2"]
    y = F.layer_norm(x, (C,), c(n1[0]), c(n1[1]), n1[2]).view(B, H, W, C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    xp = F.pad(y, (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = xp.shape[1], xp.shape[2]
    if shift:
        xp = torch.roll(xp, (-shift, -shift), (1, 2))
    xw = xp.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    mask = c(ref_ops.shift_attn_mask(H, W, ws, shift)) if shift else None
    aw = ref_ops.window_attention(xw, c(inp["qkv_w"]), c(inp["qkv_b"]), c(inp["proj_w"]), c(inp["proj_b"]), c(inp["table"]), ws, nH, mask)
    o = aw.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    xn = x + o[:, :H, :W].reshape(B, L, C)
    return xn, F.layer_norm(xn, (C,), c(n2[0]), c(n2[1]), n2[2])


def k7_reference(case, inp):
    entry, C, B, H, W, shift = case
    return _k7_reference(inp["x"], inp["n1"], inp["qkv_w"], inp["qkv_b"], inp["proj_w"], inp["proj_b"], inp["table"], H, W, K7_WS, C // 32, shift, inp["n2"])


@functools.lru_cache(maxsize=16)
def k7_truth(case):
    """(x64, y2_64, b_x, b_y2): x = shortcut + proj(attention) -- for the qkv entry point shortcut + attention"""
    inp = k7_inputs(case)
    x64, y64 = k7_reference(case, inp)
    x32, y32 = k7_restate(case, inp, torch.float32)
    return x64, y64, b_of(x32, x64), b_of(y32, y64)


# ================================================================================================ 5. K2: deformable attention
# ms_deform_attn.hip, rba_ms_deform_attn_fwd_f32: D == 32, P == 4 and L in {1, 3} (16-byte aligned operands) take the gather form
# msda_fwd_lp_kernel<L, 4>, a workgroup of 32 consecutive queries of one head on a ((Lq + 31) / 32, M, N) grid; every other shape the generic
# kernel, 4 channels per thread when D % 4 == 0 (float4), otherwise one.  rba_ms_deform_attn_fwd_f64: the generic kernel in double.
# rba_msda_fused_f32 (sampling locations and softmax inside the gather kernel) exists for the gather form's shapes only.
K2_BOUND, K2_BOUND_F64 = 1e-5, 1e-12                              # test_k2_shapes; test_k2_reference_test_set's double check
K2_FORMS = ("gather L=1", "gather L=3", "generic float4", "generic scalar", "f64")
K2_DLP = ((32, 1, 4), (32, 3, 4), (32, 2, 4), (32, 3, 2), (16, 2, 1), (5, 1, 3), (64, 3, 4))
K2_FAR = 1.0e4

_LV1, _LV2, _LV3 = ((5, 7),), ((6, 4), (3, 2)), ((9, 7), (5, 3), (2, 2))
_THIN1, _THIN2, _THIN3 = ((1, 6),), ((1, 1), (4, 1)), ((7, 1), (1, 1), (1, 5))          # 1 x W, 1 x 1 and H x 1 levels


def k2_gather_form(D, L, P):
    return D == 32 and P == 4 and L in (1, 3)                          # = ops.msda_fused_ok


def k2_form(case):
    N, M, D, Lq, shapes, P, dt = case
    if dt == "f64":
        return "f64"
    if k2_gather_form(D, len(shapes), P):
        return f"gather L={len(shapes)}"
    return "generic float4" if D % 4 == 0 else "generic scalar"


def k2_forms(case):
    return (k2_form(case),)


def k2_in_domain(case):
    N, M, D, Lq, shapes, P, dt = case
    return min(N, M, D, Lq, P) >= 1 and len(shapes) >= 1 and all(h >= 1 and w >= 1 for h, w in shapes) and dt in ("f32", "f64")


def k2_boundary():
    """(N, M, D, Lq, shapes, P, dtype): every (D, L, P) of `K2_DLP`; Lq in {1, 31, 32, 33, S} (the gather form's 32-query workgroups, Lq != S);
    M in {1, 3, 8}; N in {1, 2, 3}; levels with a 1-pixel axis in every form; two fp64 cases"""
    f = "f32"
    return ((1, 1, 32, 1, _LV1, 4, f), (2, 3, 32, 31, _LV1, 4, f), (1, 8, 32, 32, _THIN1, 4, f), (3, 1, 32, 33, _LV1, 4, f), (1, 3, 32, 35, _LV1, 4, f),
            (1, 8, 32, 1, _LV3, 4, f), (2, 1, 32, 31, _THIN3, 4, f), (1, 3, 32, 32, _LV3, 4, f), (1, 1, 32, 33, _LV3, 4, f), (3, 3, 32, 82, _LV3, 4, f),
            (1, 3, 32, 33, _LV2, 4, f), (2, 8, 32, 31, _LV2, 4, f), (1, 1, 32, 1, _THIN2, 4, f),
            (1, 3, 32, 32, _LV3, 2, f), (2, 1, 32, 13, _THIN3, 2, f),
            (3, 8, 16, 30, _LV2, 1, f), (1, 1, 16, 33, _THIN2, 1, f),
            (1, 3, 5, 35, _LV1, 3, f), (2, 1, 5, 1, _THIN1, 3, f), (1, 8, 5, 31, _LV1, 3, f),
            (1, 3, 64, 33, _LV3, 4, f), (2, 1, 64, 82, _LV3, 4, f),
            (1, 3, 32, 33, _LV3, 4, "f64"), (2, 3, 5, 31, _LV1, 3, "f64"))


def k2_random(seed, n=8):
    def draw(r):
        D, L, P = r.choice(K2_DLP + ((32, 1, 4), (32, 3, 4), (r.randint(1, 70), r.randint(1, 3), r.randint(1, 5))))
        shapes = tuple((r.randint(1, 24), r.randint(1, 20)) for _ in range(L))
        return (r.choice((1, 2, 3)), r.choice((1, 3, 8)), D, r.choice([r.randint(1, 400), _around(r, (32, 64, 96))]), shapes, P, "f32")
    return _bounded(random.Random(1100 + seed), n, draw, lambda d: d[0] * d[1] * d[2] * d[3] * len(d[4]) * d[5] <= 3_000_000)


def k2_draws(which):
    return k2_boundary() if which == "boundary" else k2_random(which)


K2_PLANTED = ("centre", "edge", "border -0.5 px", "border +0.5 px", "far", "zero or one")


def k2_planted(H, W):
    """[(kind, x, y)] of one level: exactly on pixel centres, exactly on pixel edges, half a pixel outside either border, far outside, and 0 and 1"""
    pts = [("centre", (i % W + 0.5) / W, (i % H + 0.5) / H) for i in range(max(H, W))]
    pts += [("edge", (i % (W + 1)) / W, ((i + 1) % (H + 1)) / H) for i in range(max(H, W) + 1)]
    pts += [("border -0.5 px", -0.5 / W, 0.5 / H), ("border -0.5 px", 0.5 / W, -0.5 / H), ("border +0.5 px", 1 + 0.5 / W, 0.5 / H),
            ("border +0.5 px", 0.5 / W, 1 + 0.5 / H), ("border -0.5 px", -0.5 / W, 1 + 0.5 / H)]
    pts += [("far", K2_FAR, 0.5), ("far", 0.5, -K2_FAR), ("far", -K2_FAR, K2_FAR)]
    pts += [("zero or one", 0.0, 0.0), ("zero or one", 1.0, 1.0), ("zero or one", 0.0, 1.0), ("zero or one", 1.0, 0.5)]
    return pts


def _k2_dtype(case):
    return torch.float64 if case[6] == "f64" else torch.float32


@functools.lru_cache(maxsize=64)
def k2_inputs(case):
    """dict(value, shapes, lsi, loc, w, planted): `test_k2_shapes`'s distribution (value randn, locations uniform in [-0.2, 1.2], softmaxed
    weights) with every second sample of a level moved onto that level's planted set, in the order of `k2_planted`.  planted: the kinds that
    made it into the tensor"""
    N, M, D, Lq, shapes, P, dt = case
    dtype, L = _k2_dtype(case), len(shapes)
    g = torch.Generator().manual_seed(_stable_seed(2, N, M, D, Lq, P, dt == "f64", *sum(shapes, ())))
    sh = torch.as_tensor(shapes, dtype=torch.long)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    S = int(sh.prod(1).sum())
    value = torch.randn(N, S, M, D, generator=g, dtype=dtype)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g, dtype=dtype) * 1.4 - 0.2
    w = F.softmax(torch.randn(N, Lq, M, L * P, generator=g, dtype=dtype), -1).view(N, Lq, M, L, P)
    planted = set()
    for l, (H, W) in enumerate(shapes):
        pts = k2_planted(H, W)
        flat = loc[:, :, :, l].reshape(-1, 2).clone()
        n = (flat.shape[0] + 1) // 2
        pick = [pts[(j + l) % len(pts)] for j in range(n)]
        flat[0::2] = torch.tensor([[x, y] for _, x, y in pick], dtype=dtype)
        planted |= {kind for kind, _, _ in pick}
        loc[:, :, :, l] = flat.view(N, Lq, M, P, 2)
    return dict(value=value, shapes=sh, lsi=lsi, loc=loc, w=w, planted=frozenset(planted))


@functools.lru_cache(maxsize=64)
def k2_truth(case):
    inp = k2_inputs(case)
    t64 = ref_ops.ms_deform_attn(inp["value"].double(), inp["shapes"], inp["loc"].double(), inp["w"].double())
    t32 = ref_ops.ms_deform_attn(inp["value"].float(), inp["shapes"], inp["loc"].float(), inp["w"].float())
    return t64, b_of(t32, t64)


def k2_fused_inputs(case):
    """(raw [N,Lq,3 M L P], reference_points [N,Lq,L,2]) for msda_fused against msda_prepare + ms_deform_attn_forward: offsets and reference points
    that push samples across and beyond the border, as the `edge` cases of test_msda_fused_equals_prepare_plus_forward"""
    N, M, D, Lq, shapes, P, dt = case
    L = len(shapes)
    g = torch.Generator().manual_seed(_stable_seed(22, N, M, Lq, L))
    return torch.randn(N, Lq, 3 * M * L * P, generator=g) * 3.0, torch.rand(N, Lq, L, 2, generator=g) * 1.4 - 0.2
