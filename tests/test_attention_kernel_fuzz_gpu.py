"""GPU: a boundary list and seeded random shapes through the forward attention kernels -- K3 masked cross-attention, K4 mask logits, K5 Swin window
attention, K7 the fused Swin attention half block and K2 deformable attention -- whose launch FORM depends on the shape (tests/_attn_fuzz_cases.py:
the generators, the restated launch rules, the inputs and the fp64 truths; their CPU test is tests/test_attention_kernel_fuzz_cpu.py).

Every case runs under conftest's canary (guard-banded, NaN-poisoned allocations: a write outside a tensor or an unwritten output element fails whatever
the numbers say), checked after every case; a family's draws run in a seeded shuffled order, so small shapes follow large ones; each case runs every
output form the wrapper offers for its shape.

Asserted: the absolute bound of the family's fixed-shape test in tests/test_kernels_gpu.py on that test's input distribution -- K2 1e-5 (fp64: 1e-12),
K3 5e-6, K4 2e-4 sqrt(C / 256) + 1e-5 and, for f16x3, 1.5 x the exact kernel's error + 1e-6, K5 1e-5, K7 2e-5 (x), 3e-5 (y2), 1e-5 (against the
unfused sequence) -- every element finite, and torch.equal between the forms the project declares bit-identical (bias against bias_frag, swin_attn_block
with against without norm2, msda_fused against msda_prepare + ms_deform_attn_forward, both K4 column widths by the knob, split_out against
SplitActivations.pack).  Recorded, one RECORD line per family: e = max|T - T64| / max|T64| and b, the same for fp32 CPU torch, per launch form.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import _attn_fuzz_cases as A

pytestmark = pytest.mark.gpu

WHICH = ("boundary",) + A.SEEDS


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


def dev(t):
    return None if t is None else t.cuda().contiguous()


def _guards(canary):
    if canary is not None:
        canary.check()


def _absmax(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


# ---------------------------------------------------------------------------------------------------------------- 1. K3
@pytest.mark.parametrize("which", WHICH)
def test_k3_masked_xattn(ops, canary, which):
    for c in A.shuffled(A.k3_draws(which), 21):
        inp, truth = A.k3_inputs(c), A.k3_truth(c)
        q, k, v, ml = (dev(inp[n]) for n in ("q", "k", "v", "ml"))
        for name, mask in (("mask", ml), ("none", None)):
            t64, b = truth[name]
            for split in (True, False):
                form = A.k3_form(c, split)
                out = ops.masked_xattn(q, k, v, mask, split_keys=split)
                A.count_draw("K3", form)
                A.check("K3", form, f"{c} {name} split_keys={split}", out, t64, b, A.K3_BOUND)
        _guards(canary)
    A.report("K3")


# ---------------------------------------------------------------------------------------------------------------- 2. K4
@pytest.mark.parametrize("which", WHICH)
def test_k4_mask_logits(ops, canary, which):
    from rba_amd import _lib
    both_widths = []
    for c in A.shuffled(A.k4_draws(which), 22):
        B, Q, C, N = c
        e, f = (dev(t) for t in A.k4_inputs(c))
        t64, b = A.k4_truth(c)
        d = {}
        for mode in A.K4_MODES:
            form = f"{mode}: {A.k4_form(c, mode)}"
            out = ops.mask_logits(e, f, mode=mode)
            assert tuple(out.shape) == (B, Q, N)
            A.count_draw("K4", form)
            d[mode] = A.check("K4", form, f"{c}", out, t64, b, A.k4_bound(C))
        assert d["f16x3"] <= 1.5 * d["fp32"] + 1e-6, f"K4 {c}: f16x3 max|d| = {d['f16x3']:.3e} > 1.5 x {d['fp32']:.3e} + 1e-6"
        if A.k4_form(c, "f16x3").startswith("h3") and N % 2 == 0:
            both_widths.append(c)
        _guards(canary)
    assert both_widths or which != "boundary"
    with _lib.use_library(_lib.KNOBS_LIB_PATH) as lib:                                    # one and two columns per lane: the same bits
        knob = ctypes.c_int.in_dll(lib, "rba_k4_variant")
        for c in both_widths:
            e, f = (dev(t) for t in A.k4_inputs(c))
            outs = []
            try:
                for width in (1, 2):
                    knob.value = width
                    outs.append(ops.mask_logits(e, f, mode="f16x3"))
            finally:
                knob.value = 0
            assert torch.equal(outs[0], outs[1]), f"K4 {c}: one and two columns per lane differ"
            _guards(canary)
    A.report("K4")


# ---------------------------------------------------------------------------------------------------------------- 3. K5
@pytest.mark.parametrize("which", WHICH)
def test_k5_swin_window_attn(ops, canary, which):
    for c in A.shuffled(A.k5_draws(which), 23):
        B, H, W, ws, nH, hd, shift = c
        inp = A.k5_inputs(c)
        t64, b = A.k5_truth(c)
        qkv, qkv_b, bias = dev(inp["qkv"]), dev(inp["qkv_b"]), dev(inp["bias"])
        form = A.k5_form(c)
        out = ops.swin_window_attn(qkv, qkv_b, bias, H, W, nH, ws, shift)
        A.count_draw("K5", form)
        A.check("K5", form, f"{c} rel_bias", out, t64, b, A.K5_BOUND)
        frag = ops.swin_bias_fragments(bias, ws)
        out2 = ops.swin_window_attn(qkv, qkv_b, bias, H, W, nH, ws, shift, bias_frag=frag)
        assert torch.equal(out2, out), f"K5 {c}: bias_frag and rel_bias differ"           # the scalar forms do not read it: the same launch twice
        assert ops.swin_window_attn_split_ok(hd, ws) == A.k5_split_ok(c)
        if A.k5_split_ok(c):
            so = ops.swin_window_attn(qkv, qkv_b, bias, H, W, nH, ws, shift, bias_frag=frag, split_out=True)
            want = ops.SplitActivations.pack(out)
            nfull = (B * H * W) // 32 * 32 * nH * hd
            assert so.shape == (B, H * W, nH * hd) and torch.equal(so.data[:nfull], want.data[:nfull]) and torch.equal(so.unpack(), want.unpack())
            assert torch.isfinite(so.unpack()).all()
        else:
            with pytest.raises(ops.RbaHipError):
                ops.swin_window_attn(qkv, qkv_b, bias, H, W, nH, ws, shift, bias_frag=frag, split_out=True)
        _guards(canary)
    A.report("K5")


# ---------------------------------------------------------------------------------------------------------------- 4. K7
def test_k7_supported_geometries_and_refusals(ops):
    for C in A.K7_C:
        assert ops.swin_attn_block_ok(C, C // 32, A.K7_WS) == (C in A.K7_SUPPORTED["block"]), C
        assert ops.swin_attn_qkv_ok(C, C // 32, A.K7_WS) == (C in A.K7_SUPPORTED["qkv"]), C
    for C, entry in ((96, "block"), (384, "block"), (192, "block"), (256, "block"), (96, "qkv"), (384, "qkv")):
        x = torch.zeros(1, 144, C, device="cuda")
        with pytest.raises(ops.RbaHipError):
            if entry == "block":
                ops.swin_attn_block(x, None, None, None, None, None, 12, 12, A.K7_WS, 0)
            else:
                ops.swin_attn_qkv(x, None, None, None, None, 12, 12, A.K7_WS, 0)
        assert not x.any()


@pytest.mark.parametrize("which", WHICH)
def test_k7_swin_attn_half_block(ops, canary, which):
    ws = A.K7_WS
    for c in A.shuffled(A.k7_draws(which), 24):
        entry, C, B, H, W, shift = c
        nH, form = C // 32, A.k7_form(c)
        inp = A.k7_inputs(c)
        x64, y64, bx, by = A.k7_truth(c)
        x, bias, qkv_w, qkv_b, proj_w, proj_b = (dev(inp[n]) for n in ("x", "bias", "qkv_w", "qkv_b", "proj_w", "proj_b"))
        d1, d2 = (dev(inp["n1"][0]), dev(inp["n1"][1]), inp["n1"][2]), (dev(inp["n2"][0]), dev(inp["n2"][1]), inp["n2"][2])
        frag = ops.swin_bias_fragments(bias, ws)
        img = ops.swin_attn_block_weights(qkv_w, proj_w)
        # the unfused sequence of this library on the same inputs: LN -> K6 -> K5 (-> K6)
        y1 = ops.add_layer_norm(x, d1[0], d1[1], d1[2])[1]
        att = ops.swin_window_attn(F.linear(y1, qkv_w, qkv_b), qkv_b, bias, H, W, nH, ws, shift, bias_frag=frag)
        A.count_draw("K7", form)
        if entry == "block":
            xg = x.clone()
            out_x, out_y = ops.swin_attn_block(xg, d1, img, qkv_b, frag, proj_b, H, W, ws, shift, norm2=d2)
            assert out_x.data_ptr() == xg.data_ptr()                                      # in place
            A.check("K7", form, f"{c} x", out_x, x64, bx, A.K7_BOUND_X)
            A.check("K7", form, f"{c} y2", out_y, y64, by, A.K7_BOUND_Y2)
            x2 = x.clone()
            out2, none = ops.swin_attn_block(x2, d1, img, qkv_b, frag, proj_b, H, W, ws, shift)
            assert none is None and torch.equal(out2, out_x), f"K7 {c}: with and without norm2 differ"
            unfused = x + F.linear(att, proj_w, proj_b)
            du = _absmax(out_x, unfused)
        else:
            so = ops.swin_attn_qkv(x, d1, img, qkv_b, frag, H, W, ws, shift)
            assert torch.equal(x.cpu(), inp["x"]) and so.shape == (B, H * W, C)          # x is only read
            got = so.unpack()
            A.check("K7", form, f"{c} x + attention", inp["x"].double() + got.cpu().double(), x64, bx, A.K7_BOUND_X)
            du = _absmax(got, att)
        print(f"K7 [{form}] {c}: against the unfused sequence max|d| = {du:.3e}")
        assert du < A.K7_BOUND_UNFUSED, f"K7 {c}: against the unfused sequence max|d| = {du:.3e} >= {A.K7_BOUND_UNFUSED:.0e}"
        _guards(canary)
    A.report("K7")


# ---------------------------------------------------------------------------------------------------------------- 5. K2
@pytest.mark.parametrize("which", WHICH)
def test_k2_ms_deform_attn(ops, canary, which):
    from oracle import ref_ops
    for c in A.shuffled(A.k2_draws(which), 25):
        N, M, D, Lq, shapes, P, dt = c
        L, form = len(shapes), A.k2_form(c)
        inp = A.k2_inputs(c)
        t64, b = A.k2_truth(c)
        value, sh, lsi, loc, w = (dev(inp[n]) for n in ("value", "shapes", "lsi", "loc", "w"))
        out = ops.ms_deform_attn_forward(value, sh, lsi, loc, w)
        assert out.dtype == value.dtype and tuple(out.shape) == (N, Lq, M * D)
        A.count_draw("K2", form)
        A.check("K2", form, f"{c}", out, t64, b, A.K2_BOUND_F64 if dt == "f64" else A.K2_BOUND)
        S = int(inp["lsi"][-1] + inp["shapes"][-1].prod())
        assert ops.msda_fused_ok(D, L, P, S, M) == A.k2_gather_form(D, L, P)
        if dt == "f32" and A.k2_gather_form(D, L, P):                                     # one launch against prepare + forward: the same bits
            raw, ref_pts = (dev(t) for t in A.k2_fused_inputs(c))
            loc2, w2 = ops.msda_prepare(raw, ref_pts, sh, M, L, P)
            fused = ops.msda_fused(value, sh, lsi, raw, ref_pts, M, L, P)
            two_step = ops.ms_deform_attn_forward(value, sh, lsi, loc2, w2)
            assert torch.equal(fused, two_step), f"K2 {c}: msda_fused and msda_prepare + ms_deform_attn_forward differ"
            l2, w2c = loc2.cpu(), w2.cpu()
            f64 = ref_ops.ms_deform_attn(inp["value"].double(), inp["shapes"], l2.double(), w2c.double())
            A.check("K2", form, f"{c} fused", fused, f64, A.b_of(ref_ops.ms_deform_attn(inp["value"], inp["shapes"], l2, w2c), f64), A.K2_BOUND)
        _guards(canary)
    A.report("K2")
