"""GPU: guard-banded shape sweep ("next" #1).

The reference accepts ANY image size (mask2former/maskformer_model.py:255-257: normalise, ImageList-pad to a multiple of 32; pixel_decoder/msdeformattn.py:352-361:
whatever feature-map sizes come out).  The product picks between >= 10 launch forms by tile-count rules, so parity at five hand-picked sizes says little about the
sizes in between.  Here:

* the guard-band helper (tests/_guard.py, installed for EVERY -m gpu test by tests/conftest.py) is itself tested;
* the round-4 advisor's case -- the GroupNorm-moment epilogues of K6 on `H*W = 128 * odd` rows, on the knobs build with every value of rba_k6_rs and both
  stream hints -- is pinned (it shipped broken once: the moment buffer was written past its end);
* >= 40 image sizes x {tiny1, tiny3} x stream hint {1, 3} x {f16x3, bf16x6}: product vs the oracle at the end-to-end bounds (|d sem_seg|, |d rba| < 1e-4, no argmax
  flip outside the reference's near-ties), both K1 paths -- and, in every run, the product's attention-mask logits vs the oracle's after the oracle's
  `sigmoid < 0.5` decisions have been aligned to the product's (tests/_sweep_align.py: capped, deterministic, each inverted decision provably inside rounding noise);
* the same at REAL channel widths (Swin-B / Swin-L widths, shallow depths so the CPU oracle stays in seconds) over the sizes whose 1/4, 1/8, 1/16 maps are
  128 * odd pixels, 352 x 1216 included -- that is where the wide kernels' launch forms (K6 256 x 128 / K-split / GN-moment / fold, K7 C = 128 / 192 / 256, one-kernel
  MLP) switch -- plus knob-forced forms that must not change a bit;
* batches of two images of different sizes (common canvas, per-image crop).
"""
import ctypes

import pytest
import torch

from oracle import ref_model
from rba_amd import arch as A

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------------------------------------------------------- sizes
# 1/4 map = 128 * odd pixels: (Hp/32)(Wp/32) = 2 * odd ... 352 x 1216 -> 88 x 304 = 128 * 209; 192 x 672 -> 48 x 168 = 128 * 63; 64 x 1120 -> 16 x 280 = 128 * 35
# 1/8 map = 128 * odd: 256 x 736 -> 32 x 92 = 128 * 23 ; 1/16 map = 128 * odd: 128 x 768 -> 8 x 48 = 128 * 3 ; 1024 x 608 -> 64 x 38 = 128 * 19
ODD_TILE_SIZES = [(352, 1216), (192, 672), (64, 1120), (256, 736), (128, 768), (1024, 608), (345, 1210), (190, 650)]
SIZES = ODD_TILE_SIZES + [
    (60, 90), (61, 91), (37, 53), (33, 33), (1, 1), (4, 4), (5, 7), (31, 97), (97, 31), (100, 100), (127, 129), (129, 127), (250, 250), (255, 257),
    (300, 500), (333, 777), (480, 640), (481, 641), (375, 1242), (376, 1241), (370, 1224), (720, 1280), (721, 1281), (540, 960), (360, 640), (363, 637),
    (512, 1024), (513, 1025), (511, 1023), (200, 304), (72, 72), (84, 84), (96, 96), (95, 193), (24, 24), (23, 25), (12, 12), (13, 11), (48, 2000), (2000, 48),
    (32, 32), (64, 64), (65, 63), (8, 8),
]
assert len(set(SIZES)) == len(SIZES) >= 40
# RBA_SWEEP_EXTRA=N: N more (seeded) random sizes for test_size_sweep_tiny -- a one-off soak (profiles/r06_shape_sweep_random_*.txt), not part of the default suite
import os as _os
import random as _random
_rnd = _random.Random(int(_os.environ.get("RBA_SWEEP_SEED", "6")))
EXTRA_SIZES = []
while len(EXTRA_SIZES) < int(_os.environ.get("RBA_SWEEP_EXTRA", "0")):
    _hw = (_rnd.randint(1, 1100), _rnd.randint(1, 2100)) if _rnd.random() < 0.5 else (int(2 ** _rnd.uniform(0, 10)), int(2 ** _rnd.uniform(0, 11)))
    if _hw not in SIZES and _hw not in EXTRA_SIZES:
        EXTRA_SIZES.append(_hw)

WIDE_ARCHS = {
    # Swin-B widths (C = 128 ... 1024: K7 C = 128 / 256 forms, one-kernel MLP, every K6 tile rule), 2 blocks per stage, the released 1-level / 1-layer head
    "wide_b": dict(embed_dim=128, depths=[2, 2, 2, 2], num_heads=[4, 8, 16, 32], window_size=12, conv_dim=256, mask_dim=256, nheads=8, num_queries=100,
                   num_classes=19, dim_feedforward=2048, enc_layers=1, dec_layers=1, enc_in=["res5"]),
    # Swin-L widths (C = 192 ... 1536: K7 C = 192), 3-level encoder, 2 decoder layers
    "wide_l": dict(embed_dim=192, depths=[2, 2, 2, 2], num_heads=[6, 12, 24, 48], window_size=12, conv_dim=256, mask_dim=256, nheads=8, num_queries=100,
                   num_classes=19, dim_feedforward=2048, enc_layers=1, dec_layers=2, enc_in=["res3", "res4", "res5"]),
}
WIDE_SIZES = [(352, 1216), (192, 672), (256, 736), (128, 768), (376, 1241), (60, 90), (333, 777), (363, 637)]      # (the CPU oracle is the cost: seconds per size)

# RBA_SWEEP_EXTRA_WIDE=N: N more seeded random sizes (up to 800 x 1600: the CPU oracle at the released widths takes seconds per size) for test_size_sweep_real_widths
WIDE_EXTRA_SIZES = []
while len(WIDE_EXTRA_SIZES) < int(_os.environ.get("RBA_SWEEP_EXTRA_WIDE", "0")):
    _hw = (_rnd.randint(33, 800), _rnd.randint(33, 1600))
    if _hw not in WIDE_SIZES and _hw not in WIDE_EXTRA_SIZES:
        WIDE_EXTRA_SIZES.append(_hw)

_MODELS = {}


def _arch(name):
    return A.complete(WIDE_ARCHS[name] if name in WIDE_ARCHS else A.ARCHS[name])


def _model(name):
    if name not in _MODELS:
        from rba_amd.checkpoint import load_checkpoint
        from rba_amd.maskformer_model import MaskFormer
        a = _arch(name)
        sd = A.seeded_weights(a, 0)
        m = load_checkpoint(MaskFormer(a), sd).cuda().eval()
        m.graph_replay = False
        _MODELS[name] = (m, a, sd)
    return _MODELS[name]


def _image(h, w, seed=None):
    g = torch.Generator().manual_seed(1000 * h + w if seed is None else seed)
    return torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)


def _err(a, b):
    return (a.detach().cpu().double() - b.double()).abs().max().item()


def _check(out, ref, h, w, what, tol=1e-4):
    assert out["sem_seg"].shape == (19, h, w) and out["rba"].shape == (h, w) and out["argmax"].shape == (h, w), what
    e_sem, e_rba = _err(out["sem_seg"], ref["sem_seg"]), _err(out["rba"], ref["rba"])
    top2 = ref["sem_seg"].topk(2, dim=0).values
    flips = out["argmax"].cpu().long() != ref["argmax"]
    bad = int((flips & ((top2[0] - top2[1]) > tol)).sum())
    ok = e_sem < tol and e_rba < tol and bad == 0          # NaN compares False: a poisoned (unwritten) output fails here
    return ok, (e_sem, e_rba, bad, int(flips.sum()))


def _sweep_one(name, h, w, configs):
    """One case (model, size) over `configs` = (stream hint, arithmetic mode): EVERY run goes through tests/_sweep_align.py -- the product's attention-mask logits are
    tapped, the fp32 and the float64 oracle are aligned to the product's threshold decisions (deterministically: at most one oracle re-run per head call, cached per
    toggle set over the runs of the case), and the run is held to
      * the cap of _sweep_align.MAX_TOGGLES inverted decisions,
      * logit parity |P - R32| <= k * own at every entry of every head call (k = 3 for bf16x6, 5 for f16x3; own = max |R32 - R64| of the aligned oracles),
      * every inverted decision inside the old 2e-5 band (scaled with the output tolerance, as the search this replaces scaled it),
      * the outputs: within 1e-4 of the aligned fp32 oracle, or (1) within tol = max(1e-4, 3 * own_out) of the float64 truth, or -- only for a run with inverted
        decisions, as before -- within tol of the aligned fp32 oracle.
    A run without inverted decisions is compared with the untouched fp32 oracle exactly as before."""
    from rba_amd import ops
    from tests import _sweep_align as SA
    model, a, sd = _model(name)
    image = _image(h, w)
    run32, run64 = SA.oracle_runs(image, sd, a)
    dev_image = image.cuda()
    problems = []
    prev_hint = ops.concurrent_streams()
    try:
        for i, (hint, mode) in enumerate(configs):
            ops.set_concurrent_streams(hint)
            model.fused_upsample = (i + h + w) % 2 == 0                       # both K1 paths over the sweep (fused x4 up-sample / materialised planes)
            with ops.split_mode(mode):
                with SA.tap_attn_logits(model.sem_seg_head.predictor) as P:
                    out = model([{"image": dev_image}], return_argmax=True)[0]
                rba2, arg2 = model.rba_scores([{"image": dev_image}], return_argmax=True)[0]
            what = f"{name} {h}x{w} hint {hint} {mode} fused {model.fused_upsample}"
            assert torch.equal(rba2, out["rba"]) and torch.equal(arg2, out["argmax"]), what       # the score-only path of the evaluator = the dict path, bit for bit
            assert len(P) == a["dec_layers"], (what, len(P))
            want = [SA.blocked(p) for p in P]                                 # K3's own decisions (test_k3_threshold_decision_at_the_boundary)
            try:
                toggles, (R32, ref) = SA.align(run32, want)
                _, (R64, ref64) = SA.align(run64, want)
            except SA.AlignmentError as e:
                problems.append(f"{what}: {e}")
                continue
            # (1) is the SIZE ill-conditioned for fp32 itself?  A 32 x 32 canvas leaves 1 x 1 / 2 x 2 maps: GroupNorm(32) over two values, LayerNorm over near-equal
            # rows -- the reference's own fp32 forward is then 1e-4 ... 4e-4 from the float64 forward of the same weights (measured: tiny3 at 5 x 7, 13 x 11,
            # 32 x 32).  The product must be as close to the float64 truth as the reference's fp32 is (factor 3), and never worse than 1e-4 where the reference is
            # better than that.
            own_out = max(_err(ref["sem_seg"], ref64["sem_seg"]), _err(ref["rba"], ref64["rba"]))
            tol = max(1e-4, 3 * own_out)
            bad, stats = SA.logit_parity(P, R32, R64, toggles, mode, band=SA.OLD_BAND * (tol / 1e-4))
            ok, nums = _check(out, ref, h, w, what)
            if not ok:
                ref64f = {k: (v.float() if v.is_floating_point() else v) for k, v in ref64.items()}
                ok = _check(out, ref64f, h, w, what, tol=tol)[0] or (bool(toggles) and _check(out, ref, h, w, what, tol=tol)[0])
            if not ok:
                bad.append(f"outputs (|d sem|, |d rba|, argmax flips outside near-ties, all flips) {nums} vs the aligned oracle, tol {tol:.1e} "
                           f"(reference fp32 is {own_out:.1e} from its float64)")
            _log_parity(name, h, w, hint, mode, SA.n_toggles(toggles), stats, SA.K_PARITY[mode])
            problems += [f"{what} ({SA.n_toggles(toggles)} inverted decisions, ratio {stats['ratio']:.2f}): {b}" for b in bad]
    finally:
        ops.set_concurrent_streams(prev_hint)
        model.fused_upsample = True
    assert not problems, "\n".join(problems)


def _log_parity(name, h, w, hint, mode, toggles, stats, k):
    """RBA_SWEEP_PARITY_LOG=<file>: one row per run (profiles/sweep_logit_parity.txt is the default sweep's)"""
    path = _os.environ.get("RBA_SWEEP_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{name:7s} {h:5d} {w:5d} {hint:2d} {mode:7s} ratio {stats['ratio']:8.3f} k {k:g} toggles {toggles:2d} near_zero {stats['near_zero']:3d} "
                    f"max|P-R| {stats['max_diff']:.3e} own {stats['own']:.3e} old_band 2e-05\n")


ALL_CONFIGS = [(1, "f16x3"), (3, "f16x3"), (1, "bf16x6"), (3, "bf16x6")]


# ---------------------------------------------------------------------------------------------------------------- the guard itself
def test_guard_catches_out_of_bounds_writes_and_unwritten_outputs(canary):
    """tests/_guard.py: a write one element past a guarded tensor (or before it) fails check(); the payload of a guarded torch.empty is NaN; product allocations
    (rba_amd.ops) are guarded while the fixture is active."""
    from tests import _guard
    from rba_amd import ops
    assert canary is _guard and ops.torch is not torch                     # the proxy is in place
    before = _guard.REGISTRY.allocations
    x = torch.randn(4, 7, 256, device="cuda")
    _, y = ops.add_layer_norm(x, torch.ones(256, device="cuda"), torch.zeros(256, device="cuda"), 1e-5)
    assert _guard.REGISTRY.allocations > before and torch.isfinite(y).all()
    assert _guard.check() >= 1
    t = _guard.empty(16, dtype=torch.float32)
    assert torch.isnan(t).all()                                              # poisoned payload
    t.zero_()
    assert _guard.check() == 1
    t = _guard.empty(16, dtype=torch.float32)
    torch.as_strided(t, (17,), (1,))[16] = 1.0                               # one element past the end
    with pytest.raises(_guard.CanaryError, match="AFTER"):
        _guard.check()
    t = _guard.empty((3, 5), dtype=torch.int32)
    torch.as_strided(t, (1,), (1,), storage_offset=t.storage_offset() - 1)[0] = 7   # one element before the start
    with pytest.raises(_guard.CanaryError, match="BEFORE"):
        _guard.check()
    assert _guard.check() == 0                                               # a failed check forgets its buffers


# ---------------------------------------------------------------------------------------------------------------- the round-4 bug's shapes
@pytest.mark.parametrize("hint", [1, 3])
@pytest.mark.parametrize("rs", [0, 1, 2, 3])
@pytest.mark.parametrize("B,H,W", [(1, 88, 304), (2, 88, 304), (1, 48, 168), (3, 16, 280), (1, 128, 209)])
def test_gn_moment_epilogues_on_128_times_odd_rows(knobs, B, H, W, rs, hint):
    """ADVICE round 4 (high) / VERDICT round 5 missing #4: `conv3x3_nhwc_gn_stats` and `linear_gn_stats` with M = 128 * odd rows per image, on the knobs build with
    rba_k6_rs = 0 .. 3 (3 = the 256 x 128 form from 64 tiles on: the setting that reached the out-of-bounds moment write for 352 x 1216 images) and both stream
    hints.  The moment buffer and the output are guard-banded (conftest's canary fixture): an out-of-bounds slot fails the test even though the merged statistics
    look right.  Values: y bit-identical to the plain kernel, statistics against float64."""
    from rba_amd import _lib, ops
    P, C, N, G = H * W, 256, 256, 32
    assert P % 128 == 0 and (P // 128) % 2 == 1
    k_rs = ctypes.c_int.in_dll(_lib.load(), "rba_k6_rs")
    g = torch.Generator().manual_seed(B * 100000 + P)
    prev = ops.concurrent_streams()
    try:
        k_rs.value = rs
        ops.set_concurrent_streams(hint)
        # 3 x 3 output convolution on its split-image operand
        x = (torch.randn(B, H, W, C, generator=g)).cuda()
        w = (torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5).cuda()
        planes = ops.conv3x3_weight(w, mode="f16x3")
        xs = ops.SplitActivations.pack(x.view(B * P, C))
        xs = ops.SplitActivations(xs.data, (B, H, W, C))
        if ops.conv3x3_emits_gn_moments(B, H, W, N, G):
            y, mr = ops.conv3x3_nhwc_gn_stats(xs, planes, G, 1e-5, None, out_features=N)
            want = ops.conv3x3_nhwc(xs, planes, None, out_features=N)
            assert torch.equal(y, want)
            yd = want.double().view(B, P, G, N // G)
            mean64, var64 = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
            assert _err(mr[..., 0], mean64.cpu()) < 2e-6
            assert ((mr[..., 1].double() * (var64 + 1e-5).sqrt()) - 1).abs().max().item() < 2e-6
        else:
            assert B * P * 2 < 256 * 128                                     # only the small cases may fall outside the moment path
        # lateral 1 x 1 convolution (token Linear, K <= 256)
        for K in (128, 256):
            xl = (torch.randn(B, P, K, generator=g) * 2 + 0.3).cuda()
            lin = torch.nn.Linear(K, N).cuda()
            with torch.no_grad():
                lin.weight.copy_((torch.randn(N, K, generator=g) * K ** -0.5).cuda())
                lin.bias.copy_(torch.randn(N, generator=g).cuda())
                if not ops.linear_emits_gn_moments(B * P, N, K, P, G):
                    continue
                y, mr = ops.linear_gn_stats(xl, lin, G, 1e-5, P)
                want = ops.linear(xl, lin)
            assert torch.equal(y, want)
            yd = want.double().view(B, P, G, N // G)
            mean64, var64 = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
            assert _err(mr[..., 0], mean64.cpu()) < 2e-6
            assert ((mr[..., 1].double() * (var64 + 1e-5).sqrt()) - 1).abs().max().item() < 2e-6
    finally:
        k_rs.value = 0
        ops.set_concurrent_streams(prev)


# ---------------------------------------------------------------------------------------------------------------- the sweep
@pytest.mark.parametrize("name", ["tiny1", "tiny3"])
@pytest.mark.parametrize("h,w", SIZES + EXTRA_SIZES)
def test_size_sweep_tiny(name, h, w):
    """every size x {tiny1 (1 level, 1 decoder layer), tiny3 (3 levels, 4 layers)} x stream hint {1, 3} x {f16x3, bf16x6} against the oracle"""
    _sweep_one(name, h, w, ALL_CONFIGS)


@pytest.mark.parametrize("name", ["wide_b", "wide_l"])
@pytest.mark.parametrize("h,w", WIDE_SIZES + WIDE_EXTRA_SIZES)
def test_size_sweep_real_widths(name, h, w):
    """the released channel widths (shallow depths): the sizes at which the wide kernels change launch form; bf16x6 on the 128 * odd sizes"""
    configs = ALL_CONFIGS if (h, w) in ODD_TILE_SIZES else ALL_CONFIGS[:2]
    _sweep_one(name, h, w, configs)


@pytest.mark.parametrize("name,h,w", [("wide_b", 352, 1216), ("wide_b", 192, 672), ("wide_l", 256, 736), ("wide_l", 352, 1216), ("wide_b", 363, 637)])
def test_forced_launch_forms_do_not_change_a_bit(knobs, name, h, w):
    """knobs build: the 256 x 128 form always / from 64 tiles / never -- same bits as the rule-selected forms; the K-split form wherever legal / never -- same
    result to the last bits' summation order; no guard band touched in any of them"""
    from rba_amd import _lib
    model, a, sd = _model(name)
    image = _image(h, w).cuda()
    k_rs, k_ks = (ctypes.c_int.in_dll(_lib.load(), k) for k in ("rba_k6_rs", "rba_k6_ks"))
    try:
        base = model([{"image": image}], return_argmax=True)[0]
        base = {k: v.clone() for k, v in base.items()}
        for rs, ks in ((1, 1), (2, 0), (3, 0), (0, 2), (2, 2), (3, 1)):
            k_rs.value, k_ks.value = rs, ks
            out = model([{"image": image}], return_argmax=True)[0]
            if ks == 0 or (rs, ks) == (1, 1):
                for k in ("sem_seg", "rba", "argmax"):           # the row-split forms (and no special form at all... where the rule picked none) are bit-identical
                    if not torch.equal(out[k], base[k]):
                        assert ks == 1, (name, h, w, rs, ks, k)  # ks = 1 removes the K-split form where the rule chose it: last bits may move (below)
            # the K-split form sums the two halves of K in its own fixed order: last bits differ from the one-set kernel BY DESIGN (split_linear_h3.h:1020-1025;
            # test_split_linear_k_split_form holds both to the same fp64 bound) -- end to end that stays far inside the parity budget
            assert _err(out["sem_seg"], base["sem_seg"].cpu()) < 2e-5 and _err(out["rba"], base["rba"].cpu()) < 5e-5, (name, h, w, rs, ks)
            top2 = base["sem_seg"].topk(2, dim=0).values
            flips = out["argmax"] != base["argmax"]
            assert int((flips & ((top2[0] - top2[1]) > 1e-4)).sum()) == 0, (name, h, w, rs, ks)
    finally:
        k_rs.value, k_ks.value = 0, 0


@pytest.mark.parametrize("name", ["tiny1", "tiny3", "wide_b"])
def test_batches_of_two_different_sizes(name):
    """ImageList semantics (maskformer_model.py:255-257): both images padded to the common canvas, outputs cropped per image; the oracle runs each image on the
    same canvas.  Includes a pair whose canvas has a 128 * odd quarter map."""
    model, a, sd = _model(name)
    pairs = [((60, 90), (33, 70)), ((352, 1216), (300, 1100)), ((100, 260), (190, 100)), ((5, 7), (64, 64))]
    if name == "wide_b":
        pairs = pairs[1:3]
    for (h0, w0), (h1, w1) in pairs:
        canvas = ((max(h0, h1) + 31) // 32 * 32, (max(w0, w1) + 31) // 32 * 32)
        ims = [_image(h0, w0, seed=1), _image(h1, w1, seed=2)]
        outs = model([{"image": ims[0].cuda()}, {"image": ims[1].cuda()}], return_argmax=True)
        for im, out, (h, w) in zip(ims, outs, ((h0, w0), (h1, w1))):
            ref = ref_model.forward(im, sd, a, canvas=canvas)
            ok, nums = _check(out, ref, h, w, f"{name} {h}x{w} in canvas {canvas}")
            assert ok, (name, (h, w), canvas, nums)


def test_graph_replay_over_changing_sizes_stays_in_bounds():
    """the product default (hipGraph replay from the third call of a shape) over a churn of sizes: replayed = eager, guard bands intact (the graph's private pool is
    guarded like any other allocation)"""
    model, a, sd = _model("tiny1")
    model.graph_replay = True
    try:
        for h, w in [(60, 90), (352, 1216), (60, 90), (37, 53), (352, 1216), (60, 90), (352, 1216), (37, 53), (37, 53)] * 2:
            im = _image(h, w).cuda()
            r = model.rba_scores([{"image": im}])[0]
            model.graph_replay = False
            e = model.rba_scores([{"image": im}])[0]
            model.graph_replay = True
            assert torch.equal(r, e), (h, w)
        assert model.live_graphs() >= 2
    finally:
        model.graph_replay = False
        model.drop_graphs()
