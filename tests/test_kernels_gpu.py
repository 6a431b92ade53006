"""GPU: each HIP kernel (through the C ABI, via rba_amd.ops) against the oracle on the same inputs."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_model, ref_ops

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


def dev(t):
    return t.cuda().contiguous()


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def argmax_ok(arg, sem_ref, tol=1e-5):
    """bit-exact except where the top-2 classes of the reference are closer than `tol`."""
    flips = arg.cpu().long() != sem_ref.argmax(0)
    if sem_ref.shape[0] < 2:
        return int(flips.sum()), int(flips.sum())
    top2 = sem_ref.topk(2, dim=0).values
    gap = top2[0] - top2[1]
    return int((flips & (gap > tol)).sum()), int(flips.sum())


# ----------------------------------------------------------------------------------- K1
def test_k1_golden(ops, golden):
    g = golden("g1_rba_reduce")
    mp, mc = T(g["mask_pred"]), T(g["mask_cls"])
    prob = ref_ops.class_probs(mc)
    rba, sem, arg = ops.rba_reduce(dev(mp), dev(prob), True, True)
    assert maxerr(sem, T(g["sem_seg"])) < 2e-6
    assert maxerr(rba, T(g["rba"])) < 1e-5           # north-star tolerance is 1e-4
    assert np.array_equal(arg.cpu().numpy(), g["argmax"])
    rba2, sem2, arg2 = ops.rba_reduce(dev(mp), dev(prob))
    assert sem2 is None and arg2 is None and torch.equal(rba2, rba)
    # fused x4 upsample + crop
    low = T(g["low"])
    r_up, s_up, a_up = ops.rba_reduce_up4(dev(low), dev(prob), (16, 32), True, True)
    assert maxerr(s_up, T(g["sem_up"])) < 5e-6
    assert maxerr(r_up, T(g["rba_up"])) < 1e-5
    r_c, s_c, _ = ops.rba_reduce_up4(dev(low), dev(prob), (13, 30), True, False)      # ragged crop
    assert maxerr(s_c, T(g["sem_up"])[:, :13, :30]) < 5e-6 and maxerr(r_c, T(g["rba_up"])[:13, :30]) < 1e-5


@pytest.mark.parametrize("Q,K,H,W", [(100, 19, 64, 128), (7, 19, 5, 13), (100, 20, 16, 20), (3, 5, 9, 7),
                                      (50, 65, 8, 24), (1, 1, 1, 1), (100, 19, 1, 4096), (12, 133, 6, 10)])
def test_k1_shapes(ops, Q, K, H, W):
    g = torch.Generator().manual_seed(Q * 1000 + K)
    mp = torch.randn(Q, H, W, generator=g) * 5
    prob = F.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :-1].contiguous()
    sem_r, rba_r, _ = ref_ops.rba_reduce_ordered(mp, prob)
    rba, sem, arg = ops.rba_reduce(dev(mp), dev(prob), True, True)
    assert maxerr(sem, sem_r) < 5e-6 and maxerr(rba, rba_r) < 2e-5
    bad, _ = argmax_ok(arg, sem_r)
    assert bad == 0


@pytest.mark.parametrize("Q,K,H,W", [(100, 19, 32, 64), (9, 7, 5, 6)])
def test_k1_score_modes(ops, Q, K, H, W):
    """energy (evaluate_ood.py:152-159) and negative logit sum (support.py:115-132) epilogues"""
    g = torch.Generator().manual_seed(7)
    mp = torch.randn(Q, H, W, generator=g) * 5
    prob = F.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :-1].contiguous()
    sem_r, _, _ = ref_ops.rba_reduce_ordered(mp, prob)
    want = {"rba": -sem_r.tanh().sum(0), "energy": -torch.logsumexp(sem_r, dim=0), "neg_logit_sum": -sem_r.sum(0)}
    low = torch.randn(Q, H // 4 + 1, W // 4 + 1, generator=g) * 5
    up = ref_ops.upsample_bilinear(low[None], (4 * low.shape[1], 4 * low.shape[2]))[0]
    sem_u, _, _ = ref_ops.rba_reduce_ordered(up, prob)
    want_u = {"rba": -sem_u.tanh().sum(0), "energy": -torch.logsumexp(sem_u, dim=0), "neg_logit_sum": -sem_u.sum(0)}
    for score in want:
        got, _, _ = ops.rba_reduce(dev(mp), dev(prob), score=score)
        assert maxerr(got, want[score]) < 3e-5, score
        if K <= 32:
            got_u, _, _ = ops.rba_reduce_up4(dev(low), dev(prob), (H, W), score=score)
            assert maxerr(got_u, want_u[score][:H, :W]) < 3e-5, score


def test_k1_empty_and_errors(ops):
    from rba_amd._lib import RbaHipError
    prob = torch.full((4, 19), 0.01).cuda()
    rba, _, _ = ops.rba_reduce(torch.zeros(4, 0, 8).cuda(), prob)
    assert rba.shape == (0, 8)
    with pytest.raises(RbaHipError):
        ops.rba_reduce(torch.zeros(4, 2, 2), prob)                  # CPU tensor: no fallback
    with pytest.raises(RbaHipError):
        ops.rba_reduce(torch.zeros(4, 2, 2).cuda().double(), prob)  # wrong dtype
    with pytest.raises(RbaHipError):
        ops.rba_reduce(torch.zeros(5, 2, 2).cuda(), prob)           # Q mismatch
    with pytest.raises(RbaHipError):
        ops.rba_reduce(torch.zeros(4, 2, 4).cuda()[:, :, ::2], prob)   # non-contiguous


def test_k1_extreme_values(ops):
    mp = torch.tensor([[-200.0, 200.0, 0.0, -1e-8], [88.0, -88.0, 30.0, 1e-8]]).view(2, 1, 4)
    prob = torch.tensor([[0.7, 0.2], [0.1, 0.6]])
    sem_r, rba_r, arg_r = ref_ops.rba_reduce_ordered(mp, prob)
    rba, sem, arg = ops.rba_reduce(dev(mp), dev(prob), True, True)
    assert torch.isfinite(rba).all() and maxerr(sem, sem_r) < 1e-6 and maxerr(rba, rba_r) < 1e-6


@pytest.mark.parametrize("h,w,ch,cw", [(8, 16, 32, 64), (5, 7, 20, 28), (6, 9, 21, 33), (1, 1, 4, 4), (184, 320, 720, 1280)])
def test_k1_up4_shapes(ops, h, w, ch, cw):
    g = torch.Generator().manual_seed(h * 100 + w)
    Q = 100 if h < 50 else 12
    low = torch.randn(Q, h, w, generator=g) * 5
    prob = F.softmax(torch.randn(Q, 20, generator=g) * 3, -1)[:, :-1].contiguous()
    up = ref_ops.upsample_bilinear(low[None], (4 * h, 4 * w))[0]
    sem_r, rba_r, _ = ref_ops.rba_reduce_ordered(up, prob)
    sem_r, rba_r = sem_r[:, :ch, :cw], rba_r[:ch, :cw]
    rba, sem, arg = ops.rba_reduce_up4(dev(low), dev(prob), (ch, cw), True, True)
    assert maxerr(sem, sem_r) < 1e-5 and maxerr(rba, rba_r) < 2e-5
    assert argmax_ok(arg, sem_r)[0] == 0


@pytest.mark.parametrize("Q,K,h,w,ch,cw", [(100, 19, 8, 16, 32, 64), (100, 20, 6, 9, 21, 36), (12, 19, 184, 320, 720, 1280), (5, 19, 3, 40, 12, 160),
                                          (33, 19, 7, 33, 26, 132), (100, 19, 1, 1, 4, 4)])
def test_k1_up4_matrix_pipe_form(ops, Q, K, h, w, ch, cw, knobs):
    """score-only rba_reduce_up4 runs the class contraction on the matrix pipe (f16 h + l pairs, three products): against the oracle at the K1
    budget, and against the packed VALU kernel (same taps, same interpolation: only the contraction's rounding differs); all three score modes"""
    import ctypes
    from rba_amd import _lib
    var = ctypes.c_int.in_dll(_lib.load(), "rba_k1_up4_variant")
    g = torch.Generator().manual_seed(Q + h + w)
    low = torch.randn(Q, h, w, generator=g) * 5
    prob = F.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :-1].contiguous()
    up = ref_ops.upsample_bilinear(low[None], (4 * h, 4 * w))[0]
    sem_r, _, _ = ref_ops.rba_reduce_ordered(up, prob)
    sem_r = sem_r[:, :ch, :cw]
    want = {"rba": -sem_r.tanh().sum(0), "energy": -torch.logsumexp(sem_r, dim=0), "neg_logit_sum": -sem_r.sum(0)}
    for score in want:
        got, _, _ = ops.rba_reduce_up4(dev(low), dev(prob), (ch, cw), score=score)
        try:
            var.value = 2
            pk, _, _ = ops.rba_reduce_up4(dev(low), dev(prob), (ch, cw), score=score)
        finally:
            var.value = 0
        assert got.shape == (ch, cw) and torch.isfinite(got).all()
        tol = 6e-5 if score == "neg_logit_sum" else 2e-5                        # a plain sum of K values of magnitude ~3: fp32 round-off of the sum itself
        assert maxerr(got, want[score]) < tol, score
        assert maxerr(got, pk.cpu()) < tol, score
    # round 4: the same kernel with sem_seg and argmax outputs (the evaluator's return_preds path, the stock get_RbA on out["sem_seg"])
    rba0 = ops.rba_reduce_up4(dev(low), dev(prob), (ch, cw))[0]
    for ws_, wa_ in ((True, True), (True, False), (False, True)):
        rba, sem, arg = ops.rba_reduce_up4(dev(low), dev(prob), (ch, cw), ws_, wa_)
        assert torch.equal(rba, rba0)                                           # the score does not depend on which outputs are written
        if ws_:
            assert sem.shape == (K, ch, cw) and maxerr(sem, sem_r) < 1e-5
            assert maxerr(-sem.tanh().sum(0), want["rba"]) < 2e-5               # the reference's get_RbA on the dict's sem_seg
        if wa_:
            assert arg.dtype == torch.int32 and argmax_ok(arg, sem_r)[0] == 0   # no flip outside the reference's own near-ties
            if ws_:
                assert torch.equal(sem.gather(0, arg.long()[None])[0], sem.max(0).values)     # a maximum of the kernel's own sem_seg


def test_k1_up4_matrix_pipe_form_full_size_is_stable(ops, knobs):
    """BASELINE C2's map: every pixel within the K1 budget of the packed VALU kernel, and two launches give the same bits (an earlier build of
    this kernel produced intermittently wrong 32-pixel tiles -- only visible at a size that keeps every CU busy with several workgroups)"""
    import ctypes
    from rba_amd import _lib
    var = ctypes.c_int.in_dll(_lib.load(), "rba_k1_up4_variant")
    g = torch.Generator().manual_seed(0)
    low = dev(torch.randn(100, 256, 512, generator=g) * 5)
    prob = dev(F.softmax(torch.randn(100, 20, generator=g) * 3, -1)[:, :-1].contiguous())
    try:
        var.value = 2
        pk = ops.rba_reduce_up4(low, prob, (1024, 2048))[0]
    finally:
        var.value = 0
    a = ops.rba_reduce_up4(low, prob, (1024, 2048))[0]
    b = ops.rba_reduce_up4(low, prob, (1024, 2048))[0]
    assert torch.equal(a, b)
    assert float((a - pk).abs().max()) < 2e-5


K1_FULL = {"pk-19": (5, 19, 3, 8), "pk-20": (5, 20, 3, 8),                      # launch_reduce_pk, static split
           "vec4-5": (5, 5, 3, 8), "unaligned-19": (5, 19, 3, 7),                 # launch_reduce<32, 4>, <32, 1>
           "k65": (5, 65, 2, 3), "k133": (5, 133, 2, 3),                          # launch_reduce<80, 1>, <160, 1>
           "pk-19-dynamic": (3, 19, 8, 131200)}                                   # 1025 tiles on 1024 slots: the smallest dynamic hand-out
K1_FUSED = {"mx-19": (19, (7, 12), 0), "mx-20": (20, (7, 12), 0),                 # (K, crop, rba_k1_up4_variant): matrix pipe
            "pk-19": (19, (7, 12), 2), "pk-20": (20, (7, 12), 2),                 # packed VALU
            "pk-19-ragged": (19, (7, 10), 0),                                     # packed VALU, ragged rows
            "generic-5": (5, (7, 12), 0), "generic-5-ragged": (5, (7, 10), 0),    # generic
            "generic-19": (19, (7, 10), 1)}                                       # generic <19>


@pytest.mark.parametrize("case", ["full-" + k for k in K1_FULL] + ["fused-" + k for k in K1_FUSED])
def test_k1_every_launcher_in_every_output_form(ops, case, request):
    """every K1 launcher with each of the four (sem_seg, argmax) requests: an output-form ladder that paired the flags wrongly would store
    through a null pointer or leave a requested output unwritten.  Tolerances of test_k1_shapes / test_k1_up4_shapes."""
    import ctypes
    from rba_amd import _lib
    kind, name = case.split("-", 1)
    variant = 0
    if kind == "full":
        Q, K, H, W = K1_FULL[name]
        sem_tol = 5e-6
    else:
        (K, crop, variant), Q = K1_FUSED[name], 5
        sem_tol = 1e-5
    g = torch.Generator().manual_seed(Q * 1000 + K)
    prob = F.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :-1].contiguous()
    if kind == "full":
        mp = torch.randn(Q, H, W, generator=g) * 5
        sem_r, rba_r, _ = ref_ops.rba_reduce_ordered(mp, prob)
        x, p = dev(mp), dev(prob)
        run = lambda ws, wa: ops.rba_reduce(x, p, ws, wa)
    else:
        low = torch.randn(Q, 2, 3, generator=g) * 5
        sem_r, rba_r, _ = ref_ops.rba_reduce_ordered(ref_ops.upsample_bilinear(low[None], (8, 12))[0], prob)
        sem_r, rba_r = sem_r[:, :crop[0], :crop[1]], rba_r[:crop[0], :crop[1]]
        x, p = dev(low), dev(prob)
        run = lambda ws, wa: ops.rba_reduce_up4(x, p, crop, ws, wa)
    if variant:
        request.getfixturevalue("knobs")
        var = ctypes.c_int.in_dll(_lib.load(), "rba_k1_up4_variant")
    try:
        if variant:
            var.value = variant
        for ws_ in (False, True):
            for wa_ in (False, True):
                rba, sem, arg = run(ws_, wa_)
                assert (sem is None) == (not ws_) and (arg is None) == (not wa_), (ws_, wa_)
                e_rba, e_sem = maxerr(rba, rba_r), maxerr(sem, sem_r) if ws_ else 0.0
                bad = argmax_ok(arg, sem_r)[0] if wa_ else 0
                print(f"{case} sem={ws_} argmax={wa_}: rba {e_rba:.2e} sem {e_sem:.2e} argmax flips {bad}")
                assert rba.shape == rba_r.shape and e_rba < 2e-5, (ws_, wa_)
                assert e_sem < sem_tol, (ws_, wa_)
                assert bad == 0, (ws_, wa_)
    finally:
        if variant:
            var.value = 0


def test_k1_up4_matrix_pipe_form_soak(ops):
    """2 000 launches of the score-only fused K1 at C2's and C5's maps, round-robin from three streams while a fourth
    stream runs a K6 GEMM loop; every output bit-equal to launch 0 of its map (tools/k1_soak.py reports the pixel pattern otherwise).
    profiles/r04_k1_mx_soak.txt: 6 000 launches + 600 graph-replayed forwards, no differing bit (round 3's build included)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import k1_soak
    r = k1_soak.soak_kernel(2000)
    assert r["launches"] == 2000 and r["mismatching_launches"] == 0, r


# ----------------------------------------------------------------------------------- resample
@pytest.mark.parametrize("C,h,w,H,W", [(100, 8, 16, 32, 64), (3, 23, 40, 46, 80), (5, 64, 128, 8, 16), (2, 184, 320, 23, 40),
                                        (4, 7, 9, 13, 30), (1, 1, 1, 5, 3), (6, 45, 80, 90, 160), (3, 30, 45, 32, 48)])
def test_resample(ops, C, h, w, H, W):
    g = torch.Generator().manual_seed(C + h)
    x = torch.randn(C, h, w, generator=g)
    ref = ref_ops.upsample_bilinear(x[None], (H, W))[0]
    assert maxerr(ops.resample_bilinear(dev(x), (H, W)), ref) < 2e-6
    add = torch.randn(C, H, W, generator=g)
    assert maxerr(ops.resample_bilinear(dev(x), (H, W), add=dev(add)), ref + add) < 2e-6
    x4 = x[None].repeat(2, 1, 1, 1)
    assert maxerr(ops.resample_bilinear(dev(x4), (H, W)), ref[None].repeat(2, 1, 1, 1)) < 2e-6


# ----------------------------------------------------------------------------------- K2
def test_k2_reference_test_set(ops, golden):
    """the reference's own ops/test.py shapes (float variant, :50-63; tolerance there rtol 1e-2 atol 1e-3)."""
    g = golden("g2_ms_deform_attn")
    shapes = T(g["a_shapes"])
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    out = ops.ms_deform_attn_forward(dev(T(g["a32_value"])), dev(shapes), dev(lsi), dev(T(g["a32_loc"])),
                                     dev(T(g["a32_w"])), 2)
    assert maxerr(out, T(g["a32_out"])) < 1e-8
    # the double check comes FIRST in the reference's test (:35-47): its FFI dispatches float and double (ms_deform_attn_cuda.cu:69) -- rba_ms_deform_attn_fwd_f64
    out64 = ops.ms_deform_attn_forward(dev(T(g["a64_value"]).double()), dev(shapes), dev(lsi), dev(T(g["a64_loc"]).double()),
                                       dev(T(g["a64_w"]).double()), 2)
    assert out64.dtype == torch.float64 and maxerr(out64, T(g["a64_out"])) <= 1e-12
    with pytest.raises(ops.RbaHipError):                                              # mixed precisions are refused, as the reference op refuses them
        ops.ms_deform_attn_forward(dev(T(g["a64_value"]).double()), dev(shapes), dev(lsi), dev(T(g["a64_loc"])), dev(T(g["a64_w"]).double()), 2)


def test_k2_golden_3level(ops, golden):
    g = golden("g2_ms_deform_attn")
    shapes = T(g["b_shapes"])
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    out = ops.ms_deform_attn_forward(dev(T(g["b_value"])), dev(shapes), dev(lsi), dev(T(g["b_loc"])), dev(T(g["b_w"])))
    assert maxerr(out, T(g["b_out"])) < 5e-6
    assert maxerr(out, T(g["b_out64"])) < 2e-5


@pytest.mark.parametrize("N,M,D,shapes,P", [(1, 8, 32, [(32, 64)], 4), (2, 8, 32, [(23, 40), (12, 20), (6, 10)], 4),
                                             (1, 2, 2, [(6, 4), (3, 2)], 2), (1, 3, 5, [(4, 7)], 3), (3, 2, 16, [(9, 9), (1, 1)], 1)])
def test_k2_shapes(ops, N, M, D, shapes, P):
    g = torch.Generator().manual_seed(N * 10 + M)
    sh = torch.as_tensor(shapes, dtype=torch.long)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    S = int(sh.prod(1).sum())
    L, Lq = len(shapes), S
    value = torch.randn(N, S, M, D, generator=g)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.4 - 0.2
    w = F.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P)
    ref = ref_ops.ms_deform_attn(value, sh, loc, w)
    out = ops.ms_deform_attn_forward(dev(value), dev(sh), dev(lsi), dev(loc), dev(w))
    assert out.shape == (N, Lq, M * D) and maxerr(out, ref) < 1e-5


def test_k2_errors(ops):
    from rba_amd._lib import RbaHipError
    sh = torch.as_tensor([(2, 2)], dtype=torch.long).cuda()
    lsi = torch.zeros(1, dtype=torch.long).cuda()
    v = torch.zeros(3, 4, 2, 4).cuda()
    loc = torch.zeros(3, 4, 2, 1, 2, 2).cuda()
    w = torch.zeros(3, 4, 2, 1, 2).cuda()
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_forward(v, sh, lsi, loc, w, im2col_step=2)      # 3 % 2 != 0 (ms_deform_attn_cuda.cu:55-57)
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_forward(v.cpu(), sh, lsi, loc, w)
    with pytest.raises(RbaHipError):
        ops.ms_deform_attn_forward(v, sh.int(), lsi, loc, w)


# ----------------------------------------------------------------------------------- K3
@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("B,Q,S,nH", [(1, 100, 2048, 8), (2, 16, 77, 2), (1, 5, 1, 1), (1, 100, 920, 8), (1, 100, 14720, 8),
                                      (1, 100, 100, 8), (1, 37, 301, 3)])
def test_k3_masked_xattn(ops, B, Q, S, nH, split):
    g = torch.Generator().manual_seed(Q + S)
    q, k, v = (torch.randn(B, n, nH, 32, generator=g) for n in (Q, S, S))
    ml = torch.randn(B, Q, S, generator=g) * 3
    ml[:, 0] = -5.0                   # a fully blocked row -> attends everywhere (decoder.py:433)
    if Q > 1:
        ml[:, 1] = 5.0
    blocked = ref_ops.attn_mask_from_logits(ml.clone())
    ref = ref_ops.attention_core(q, k, v, blocked)
    if S > 300:
        ml[:, 2, : S - 150] = -5.0     # everything but the last chunk blocked: exercises the -inf running max across chunks
    blocked = ref_ops.attn_mask_from_logits(ml.clone())
    ref = ref_ops.attention_core(q, k, v, blocked)
    out = ops.masked_xattn(dev(q), dev(k), dev(v), dev(ml), split_keys=split)
    assert maxerr(out, ref) < 5e-6
    ref0 = ref_ops.attention_core(q, k, v, None)
    assert maxerr(ops.masked_xattn(dev(q), dev(k), dev(v), None, split_keys=split), ref0) < 5e-6


def _f32_from_bits(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


_SIGMOID_BOUNDARY = []


def _torch_sigmoid_boundary():
    """Bisection over the bit patterns of the negative floats (more bits = further from zero) for the first x with torch's fp32 `sigmoid(x) < 0.5` -> (bits of the
    last un-blocked float, bits of the first blocked one).  Evaluated on 9 copies so that the vectorised body and the scalar tail of the CPU kernel both answer."""
    if not _SIGMOID_BOUNDARY:
        def is_blocked(bits):
            d = torch.full((9,), _f32_from_bits(bits), dtype=torch.float32).sigmoid() < 0.5
            assert bool(d.all()) == bool(d.any())
            return bool(d.all())
        lo, hi = 0x80000000, 0xBF800000                       # -0.0 (not blocked) ... -1.0 (blocked)
        assert not is_blocked(lo) and is_blocked(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if is_blocked(mid) else (mid, hi)
        _SIGMOID_BOUNDARY.append((lo, hi))
    return _SIGMOID_BOUNDARY[0]


@pytest.mark.parametrize("split", [True, False])
@pytest.mark.parametrize("B,Q,S,nH", [(1, 16, 77, 2), (1, 37, 301, 3), (1, 100, 920, 8)])
def test_k3_threshold_decision_at_the_boundary(ops, B, Q, S, nH, split):
    """K3 fuses the reference's `sigmoid(mask) < 0.5` (mask2former_transformer_decoder.py:486).  The shape sweep aligns the oracle to the product's decisions as
    torch would take them from the product's logits (tests/_sweep_align.py), so all three forms of K3 -- the scalar kernel, the row-flag kernel and the MFMA partial
    kernel -- must decide exactly like torch's fp32 sigmoid for every input, also within 1e-6 of zero where `randn * 3` logits never land: planted +-0, the
    smallest denormals, +-2^-25 ... +-2^-22, +-1e-6 and the two floats on either side of torch's boundary, each at three keys of every row, whose `v` rows are ten
    times larger than the others (one wrong decision moves the output by >~ 1e-4); a row whose only un-blocked key sits at the last un-blocked float; a row whose
    only candidate sits at the first blocked float (fully blocked: attends everywhere, :433); a row whose only un-blocked key lies in the last 144-key chunk."""
    last_open, first_blocked = _torch_sigmoid_boundary()
    assert (last_open, first_blocked) == (0xB43FFFFE, 0xB43FFFFF)           # a torch that moves them must be seen (rba_mask_blocked holds the same constant)
    planted = [0.0, -0.0, 1e-45, -1e-45, 2.0 ** -25, -2.0 ** -25, 2.0 ** -24, -2.0 ** -24, 2.0 ** -23, -2.0 ** -23,
               _f32_from_bits(last_open), _f32_from_bits(first_blocked), 2.0 ** -22, -2.0 ** -22, 1e-6, -1e-6]
    g = torch.Generator().manual_seed(7 * Q + S)
    q, k, v = (torch.randn(B, n, nH, 32, generator=g) for n in (Q, S, S))
    keys = torch.randperm(S - 2, generator=g)[:3 * len(planted) - 1]
    keys = torch.cat([keys, torch.tensor([S - 2])])            # the planted key set (one of them in the last chunk), shared by all rows: v belongs to the key
    v *= 0.1                                                   # the others; the planted keys keep the scale the 5e-6 bound of test_k3_masked_xattn was set for
    v[:, keys] *= 10.0
    ml = torch.where(torch.rand(B, Q, S, generator=g) < 0.5, -5.0, 5.0)
    values = torch.tensor(planted, dtype=torch.float32).repeat(3)
    assert values.view(torch.int32)[3].item() == -(2 ** 31) + 1 and values[1].signbit()     # the denormal and -0.0 survived the trip
    for b in range(B):
        for r in range(Q):
            ml[b, r, keys[torch.randperm(len(keys), generator=g)]] = values
    ml[:, 0] = -5.0
    ml[:, 0, keys[5]] = _f32_from_bits(last_open)              # the only un-blocked key of the row
    ml[:, 1] = -5.0
    ml[:, 1, keys[7]] = _f32_from_bits(first_blocked)          # blocked like all the others: the row attends everywhere
    if S > 300:
        ml[:, 2] = -5.0
        ml[:, 2, S - 2] = -0.0                                  # the only un-blocked key lies in the last chunk
    blocked = ref_ops.attn_mask_from_logits(ml.clone())
    assert int(blocked[0, 0].sum()) == S - 1 and int(blocked[0, 1].sum()) == 0 and (S <= 300 or int(blocked[0, 2].sum()) == S - 1)
    ref = ref_ops.attention_core(q.double(), k.double(), v.double(), blocked)
    out = ops.masked_xattn(dev(q), dev(k), dev(v), dev(ml), split_keys=split)
    assert torch.isfinite(out).all()
    err = maxerr(out, ref)
    print(f"[k3 boundary] Q {Q} S {S} nH {nH} split {split}: max err {err:.3e}")
    assert err < 5e-6


# ----------------------------------------------------------------------------------- K4
@pytest.mark.parametrize("mode", ["fp32", "f16x3"])
@pytest.mark.parametrize("B,Q,C,h,w", [(1, 100, 256, 32, 64), (2, 16, 64, 15, 23), (1, 100, 256, 7, 9), (1, 3, 8, 1, 1), (1, 100, 256, 128, 512),
                                       (2, 112, 96, 24, 46), (1, 100, 256, 1, 14720)])
def test_k4_mask_logits(ops, B, Q, C, h, w, mode):
    g = torch.Generator().manual_seed(Q + C)
    e = torch.randn(B, Q, C, generator=g)
    f = torch.randn(B, C, h, w, generator=g)
    ref = torch.einsum("bqc,bchw->bqhw", e.double(), f.double())
    out = ops.mask_logits(dev(e), dev(f), mode=mode)
    assert out.shape == (B, Q, h, w) and maxerr(out, ref) < 2e-4 * (C / 256) ** 0.5 + 1e-5


def test_k4_f16x3_column_tiles_and_range(ops, knobs):
    """both column-tile widths of the f16x3 kernel give the same bits (the per-element arithmetic does not depend on it), the result is as close
    to fp64 as the exact-fp32 kernel's, and an out-of-range input is NaN, never a wrong number"""
    import ctypes
    from rba_amd import _lib
    knob = ctypes.c_int.in_dll(_lib.load(), "rba_k4_variant")
    g = torch.Generator().manual_seed(5)
    e = dev(torch.randn(1, 100, 256, generator=g) * 3)
    f = dev(torch.randn(1, 256, 4 * 37 * 16, generator=g) * 10)
    ref = torch.einsum("bqc,bcn->bqn", e.double(), f.double())
    outs = []
    try:
        for v in (1, 2):
            knob.value = v
            outs.append(ops.mask_logits(e, f, mode="f16x3"))
    finally:
        knob.value = 0
    assert torch.equal(outs[0], outs[1])
    exact = ops.mask_logits(e, f, mode="fp32")
    assert (outs[0].double() - ref).abs().max() <= 1.5 * (exact.double() - ref).abs().max() + 1e-6
    f2 = f.clone()
    f2[0, 3, 5] = 7e4
    bad = ops.mask_logits(e, f2, mode="f16x3")
    assert torch.isnan(bad[0, :, 5]).all() and torch.isfinite(bad[0, :, 6]).all()
    assert torch.isfinite(ops.mask_logits(e, f2, mode="fp32")).all()


# ----------------------------------------------------------------------------------- K5
def test_k5_swin_block_golden(ops, golden):
    """BasicLayer of the reference on a 13 x 20 grid (window pad, shifted block): product block on GPU vs golden."""
    from rba_amd.modeling.backbone.swin import BasicLayer
    g = golden("g3_swin_parts")
    layer = BasicLayer(32, 2, 2, 6, 4.0, downsample=True)
    sd = {k[len("bl_sd."):]: T(g[k]) for k in g.files if k.startswith("bl_sd.")}
    layer.load_state_dict(sd)
    layer = layer.cuda().eval()
    H, W, Wh, Ww = (int(v) for v in g["bl_hw"])
    x = dev(T(g["bl_x"]))
    with torch.no_grad():
        pending = None
        for blk in layer.blocks:
            x, pending = blk(x, H, W, pending)
        if pending is not None:
            x = x + pending[0] + pending[1]
        down = layer.downsample(x, H, W)
    assert maxerr(x, T(g["bl_out"])) < 2e-5
    assert maxerr(down, T(g["bl_down"])) < 2e-5


@pytest.mark.parametrize("H,W,ws,nH,shift", [(12, 12, 6, 2, 0), (13, 20, 6, 2, 3), (24, 36, 12, 4, 6), (7, 5, 12, 1, 6),
                                              (30, 41, 7, 3, 3)])
def test_k5_window_attn_core(ops, H, W, ws, nH, shift):
    g = torch.Generator().manual_seed(H * W)
    C, B = nH * 32, 2
    qkv_w, qkv_b = torch.randn(3 * C, C, generator=g) * C ** -0.5, torch.randn(3 * C, generator=g) * 0.2
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5
    x = torch.randn(B, H * W, C, generator=g)
    # oracle: pad -> roll -> partition -> window attention (identity proj) -> reverse -> un-roll -> crop
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    xp = F.pad(x.view(B, H, W, C), (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = xp.shape[1], xp.shape[2]
    if shift:
        xp = torch.roll(xp, (-shift, -shift), (1, 2))
    xw = xp.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    mask = ref_ops.shift_attn_mask(H, W, ws, shift) if shift else None
    aw = ref_ops.window_attention(xw, qkv_w, qkv_b, torch.eye(C), torch.zeros(C), table, ws, nH, mask)
    y = aw.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        y = torch.roll(y, (shift, shift), (1, 2))
    ref = y[:, :H, :W].reshape(B, H * W, C)
    qkv = F.linear(x, qkv_w, qkv_b)
    N = ws * ws
    bias = table[ref_ops.relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).contiguous()
    out = ops.swin_window_attn(dev(qkv), dev(qkv_b), dev(bias), H, W, nH, ws, shift)
    assert maxerr(out, ref) < 1e-5
    frag = ops.swin_bias_fragments(dev(bias), ws)            # coalesced fragment-ordered bias: same result
    out2 = ops.swin_window_attn(dev(qkv), dev(qkv_b), dev(bias), H, W, nH, ws, shift, bias_frag=frag)
    assert torch.equal(out2, out)
    if ops.swin_window_attn_split_ok(32, ws):               # the proj Linear's split operand written by the attention kernel itself
        so = ops.swin_window_attn(dev(qkv), dev(qkv_b), dev(bias), H, W, nH, ws, shift, bias_frag=frag, split_out=True)
        want = ops.SplitActivations.pack(out)
        nfull = (B * H * W) // 32 * 32 * C
        assert so.shape == (B, H * W, C) and torch.equal(so.data[:nfull], want.data[:nfull]) and torch.equal(so.unpack(), want.unpack())
    else:
        with pytest.raises(ops.RbaHipError):
            ops.swin_window_attn(dev(qkv), dev(qkv_b), dev(bias), H, W, nH, ws, shift, bias_frag=frag, split_out=True)


def test_k5_register_budgets_are_bit_identical(ops, knobs):
    """Round 4 (late): the f16x3 window-attention kernel at 80 VGPRs (two 9-wave workgroups resident per CU, the default) and at 96 (one: rba_k5_wpe = 5, the
    build of rounds 2-4) is the same arithmetic in the same order -- every output form bit for bit, shifted and unshifted, with window padding, one and two images."""
    import ctypes
    from rba_amd import _lib
    wpe = ctypes.c_int.in_dll(_lib.load(), "rba_k5_wpe")
    assert wpe.value == 6
    g = torch.Generator().manual_seed(5)
    for (B, H, W, nH) in ((2, 40, 70, 3), (1, 130, 150, 4), (1, 12, 12, 1)):
        ws = 12
        C = nH * 32
        qkv = dev(torch.randn(B, H * W, 3 * C, generator=g))
        qb = dev(torch.randn(3 * C, generator=g) * 0.2)
        bias = dev(torch.randn(nH, ws * ws, ws * ws, generator=g) * 0.5)
        frag = ops.swin_bias_fragments(bias, ws)
        for shift in (0, 6):
            got = []
            for w in (6, 5, 7):                                                          # 80 (default) / 96 / 72 VGPRs
                wpe.value = w
                try:
                    so = ops.swin_window_attn(qkv, qb, bias, H, W, nH, ws, shift, bias_frag=frag, split_out=True)
                    nfull = (B * H * W) // 32 * 32 * C                                  # whole 32-row groups of the image (the last group's padding rows are not written)
                    got.append((ops.swin_window_attn(qkv, qb, bias, H, W, nH, ws, shift), ops.swin_window_attn(qkv, qb, bias, H, W, nH, ws, shift, bias_frag=frag),
                                so.data[:nfull].clone(), so.unpack()))
                finally:
                    wpe.value = 6
            for other in got[1:]:
                for a, b in zip(got[0], other):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ----------------------------------------------------------------------------------- K7
def _k7_reference(x, n1, qkv_w, qkv_b, proj_w, proj_b, table, H, W, ws, nH, shift, n2):
    """swin.py:235-293 up to norm2, in float64: norm1 -> pad -> roll -> partition -> window attention -> reverse -> un-roll -> crop -> + shortcut"""
    B, L, C = x.shape
    xd = x.double()
    y = F.layer_norm(xd, (C,), n1[0].double(), n1[1].double(), n1[2]).view(B, H, W, C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    xp = F.pad(y, (0, 0, 0, pad_r, 0, pad_b))
    Hp, Wp = xp.shape[1], xp.shape[2]
    if shift:
        xp = torch.roll(xp, (-shift, -shift), (1, 2))
    xw = xp.view(B, Hp // ws, ws, Wp // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    mask = ref_ops.shift_attn_mask(H, W, ws, shift).double() if shift else None
    aw = ref_ops.window_attention(xw, qkv_w.double(), qkv_b.double(), proj_w.double(), proj_b.double(), table.double(), ws, nH, mask)
    o = aw.view(B, Hp // ws, Wp // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift:
        o = torch.roll(o, (shift, shift), (1, 2))
    xn = xd + o[:, :H, :W].reshape(B, L, C)
    return xn, F.layer_norm(xn, (C,), n2[0].double(), n2[1].double(), n2[2])


@pytest.mark.parametrize("B,H,W,shift", [(1, 24, 36, 0), (2, 30, 41, 6), (1, 7, 5, 6), (1, 12, 12, 0), (1, 50, 26, 6), (3, 13, 24, 0)])
def test_k7_swin_attn_block(ops, B, H, W, shift):
    """round 5: the attention half of a Swin block (norm1 -> qkv -> (shifted-)window attention -> proj -> + shortcut [-> norm2]) as ONE kernel,
    against the float64 restatement of swin.py:235-293 and against the unfused sequence of this library (LN -> K6 -> K5 -> K6)."""
    C, nH, ws = 128, 4, 12
    assert ops.swin_attn_block_ok(C, nH, ws)
    g = torch.Generator().manual_seed(H * W + shift)
    x = torch.randn(B, H * W, C, generator=g) * 1.5 + 0.3
    n1 = (torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2, 1e-5)
    n2 = (torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2, 1e-5)
    qkv_w, qkv_b = torch.randn(3 * C, C, generator=g) * C ** -0.5, torch.randn(3 * C, generator=g) * 0.2
    proj_w, proj_b = torch.randn(C, C, generator=g) * C ** -0.5, torch.randn(C, generator=g) * 0.2
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5
    want_x, want_y = _k7_reference(x, n1, qkv_w, qkv_b, proj_w, proj_b, table, H, W, ws, nH, shift, n2)
    N = ws * ws
    bias = table[ref_ops.relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).contiguous()
    frag = ops.swin_bias_fragments(dev(bias), ws)
    img = ops.swin_attn_block_weights(dev(qkv_w), dev(proj_w))
    d1, d2 = (dev(n1[0]), dev(n1[1]), n1[2]), (dev(n2[0]), dev(n2[1]), n2[2])
    xg = dev(x)
    out_x, out_y = ops.swin_attn_block(xg, d1, img, dev(qkv_b), frag, dev(proj_b), H, W, ws, shift, norm2=d2)
    assert out_x.data_ptr() == xg.data_ptr()                                          # in place
    assert maxerr(out_x, want_x) < 2e-5 and maxerr(out_y, want_y) < 3e-5
    x2 = dev(x)
    out2, none = ops.swin_attn_block(x2, d1, img, dev(qkv_b), frag, dev(proj_b), H, W, ws, shift)
    assert none is None and torch.equal(out2, out_x)
    # the unfused sequence on the same inputs: same arithmetic family (f16x3), different summation order
    y1 = ops.add_layer_norm(dev(x), d1[0], d1[1], d1[2])[1]
    qkv = F.linear(y1, dev(qkv_w), dev(qkv_b))
    att = ops.swin_window_attn(qkv, dev(qkv_b), dev(bias), H, W, nH, ws, shift, bias_frag=frag)
    unf = dev(x) + F.linear(att, dev(proj_w), dev(proj_b))
    assert maxerr(out_x, unf.double()) < 2e-5
    with pytest.raises(ops.RbaHipError):
        ops.swin_attn_block(dev(x[:, :, :96].contiguous()), d1, img, dev(qkv_b), frag, dev(proj_b), H, W, ws, shift)


@pytest.mark.parametrize("C,B,H,W,shift", [(256, 1, 24, 36, 0), (256, 2, 30, 41, 6), (128, 1, 13, 24, 6), (256, 1, 128, 256, 6), (192, 1, 30, 41, 6), (192, 2, 24, 24, 0)])
def test_k7_attention_only_split_output(ops, C, B, H, W, shift):
    """K7 without proj (Swin-B stage 2, C = 256): norm1 -> qkv -> window attention as one kernel whose output is the proj Linear's split operand --
    against LN -> K6 -> K5(split_out) of this library (same arithmetic family) and, through the proj GEMM, against the float64 half block."""
    nH, ws = C // 32, 12
    assert ops.swin_attn_qkv_ok(C, nH, ws)
    g = torch.Generator().manual_seed(C + H * W + shift)
    x = torch.randn(B, H * W, C, generator=g) * 1.5 + 0.3
    n1 = (torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2, 1e-5)
    n2 = (torch.ones(C), torch.zeros(C), 1e-5)
    qkv_w, qkv_b = torch.randn(3 * C, C, generator=g) * C ** -0.5, torch.randn(3 * C, generator=g) * 0.2
    proj_w, proj_b = torch.randn(C, C, generator=g) * C ** -0.5, torch.randn(C, generator=g) * 0.2
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5
    N = ws * ws
    bias = table[ref_ops.relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).contiguous()
    frag = ops.swin_bias_fragments(dev(bias), ws)
    img = ops.swin_attn_block_weights(dev(qkv_w), dev(proj_w))
    d1 = (dev(n1[0]), dev(n1[1]), n1[2])
    xg = dev(x)
    so = ops.swin_attn_qkv(xg, d1, img, dev(qkv_b), frag, H, W, ws, shift)
    assert torch.equal(xg.cpu(), x) and so.shape == (B, H * W, C)                      # x is only read
    y1 = ops.add_layer_norm(dev(x), d1[0], d1[1], d1[2])[1]
    qkv = F.linear(y1, dev(qkv_w), dev(qkv_b))
    att = ops.swin_window_attn(qkv, dev(qkv_b), dev(bias), H, W, nH, ws, shift, bias_frag=frag)
    assert maxerr(so.unpack(), att.double()) < 1e-5
    want_x, _ = _k7_reference(x, n1, qkv_w, qkv_b, proj_w, proj_b, table, H, W, ws, nH, shift, n2)
    got = dev(x) + F.linear(so.unpack(), dev(proj_w), dev(proj_b))
    assert maxerr(got, want_x) < 3e-5


def test_k7_soak_bit_stable_across_launches_and_streams(ops):
    """K7 shares LDS buffers between waves under two barriers per head and streams its weights with LDS-DMA: 3 x 100 launches of both forms, alternating over
    three HIP streams that run concurrently, must reproduce the first result bit for bit (no floating-point atomics, fixed summation orders)."""
    ws = 12
    g = torch.Generator().manual_seed(99)
    for C, H, W, shift in ((128, 60, 90, 6), (256, 40, 70, 6)):
        nH = C // 32
        x0 = dev(torch.randn(1, H * W, C, generator=g))
        n1 = (dev(torch.randn(C, generator=g) * 0.3 + 1.0), dev(torch.randn(C, generator=g) * 0.2), 1e-5)
        qkv_w, qkv_b = dev(torch.randn(3 * C, C, generator=g) * C ** -0.5), dev(torch.randn(3 * C, generator=g) * 0.2)
        proj_w, proj_b = dev(torch.randn(C, C, generator=g) * C ** -0.5), dev(torch.randn(C, generator=g) * 0.2)
        frag = ops.swin_bias_fragments(dev(torch.randn(nH, ws * ws, ws * ws, generator=g) * 0.5), ws)
        img = ops.swin_attn_block_weights(qkv_w, proj_w)
        torch.cuda.synchronize()
        streams = [torch.cuda.Stream() for _ in range(3)]
        outs = [[] for _ in streams]
        for it in range(100):
            for si, st in enumerate(streams):
                with torch.cuda.stream(st):
                    if C == 128:
                        xx = x0.clone()
                        ops.swin_attn_block(xx, n1, img, qkv_b, frag, proj_b, H, W, ws, shift)
                        outs[si].append(xx)
                    else:
                        outs[si].append(ops.swin_attn_qkv(x0, n1, img, qkv_b, frag, H, W, ws, shift).data)
        torch.cuda.synchronize()
        first = outs[0][0]
        bad = sum(int(not torch.equal(o, first)) for per in outs for o in per)
        assert bad == 0, (C, bad)


def test_k7_f16_range_is_loud(ops):
    """like K5 / K6: a value beyond f16's range gives NaN rows, never a silently wrong finite result"""
    C, nH, ws, H, W = 128, 4, 12, 12, 24
    g = torch.Generator().manual_seed(7)
    x = torch.randn(1, H * W, C, generator=g)
    one, zero = torch.ones(C), torch.zeros(C)
    b1 = zero.clone()
    b1[5] = 1e5                                                                       # norm1 output beyond 65504 in channel 5
    qkv_w, qkv_b = torch.randn(3 * C, C, generator=g) * C ** -0.5, torch.zeros(3 * C)
    proj_w, proj_b = torch.randn(C, C, generator=g) * C ** -0.5, zero
    bias = torch.zeros(nH, ws * ws, ws * ws)
    frag = ops.swin_bias_fragments(dev(bias), ws)
    img = ops.swin_attn_block_weights(dev(qkv_w), dev(proj_w))
    out, _ = ops.swin_attn_block(dev(x), (dev(one), dev(b1), 1e-5), img, dev(qkv_b), frag, dev(proj_b), H, W, ws, 0)
    assert torch.isnan(out).all()


# ----------------------------------------------------------------------------------- GroupNorm
@pytest.mark.parametrize("B,C,h,w,relu", [(1, 256, 32, 64, False), (1, 256, 64, 128, True), (2, 64, 15, 23, True),
                                           (1, 256, 256, 512, True)])
def test_group_norm(ops, B, C, h, w, relu):
    g = torch.Generator().manual_seed(C + h)
    x = torch.randn(B, C, h, w, generator=g) * 3 + 1.5
    wt, bs = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x.double(), 32, wt.double(), bs.double(), 1e-5)
    ref = F.relu(ref) if relu else ref
    out = ops.group_norm(dev(x), 32, dev(wt), dev(bs), 1e-5, relu)
    assert maxerr(out, ref) < 2e-5
    ref32 = F.group_norm(x, 32, wt, bs, 1e-5)       # what the reference runs on CPU
    assert maxerr(out, F.relu(ref32) if relu else ref32) < 2e-5


# ----------------------------------------------------------------------------------- add + LayerNorm
@pytest.mark.parametrize("rows,C", [(1000, 128), (77, 256), (33, 512), (9, 1024), (5, 2048), (3, 3072), (2, 6144), (130, 64),
                                    (7, 32), (4, 192), (6, 1536)])
def test_add_layer_norm(ops, rows, C):
    g = torch.Generator().manual_seed(rows + C)
    x, t = torch.randn(rows, C, generator=g) * 2 + 0.5, torch.randn(rows, C, generator=g)
    tb, w, b = (torch.randn(C, generator=g) for _ in range(3))
    s_ref = x + t + tb
    y_ref = F.layer_norm(s_ref, (C,), w, b, 1e-5)
    s, y = ops.add_layer_norm(dev(x), dev(w), dev(b), 1e-5, residual=dev(t), residual_bias=dev(tb))
    assert maxerr(s, s_ref) < 1e-6 and maxerr(y, y_ref) < 5e-6
    xs = dev(x)
    s2, y2 = ops.add_layer_norm(xs, dev(w), dev(b), 1e-5, residual=dev(t), residual_bias=dev(tb), inplace_sum=True)
    assert s2.data_ptr() == xs.data_ptr() and torch.equal(s2, s) and torch.equal(y2, y)
    s3, y3 = ops.add_layer_norm(dev(x), dev(w), dev(b), 1e-5)                      # plain LayerNorm
    assert maxerr(y3, F.layer_norm(x, (C,), w, b, 1e-5)) < 5e-6 and maxerr(s3, x) == 0
    x3 = x.view(1, rows, C)
    _, y4 = ops.add_layer_norm(dev(x3), dev(w), dev(b), 1e-5, residual=dev(t.view(1, rows, C)))
    assert y4.shape == (1, rows, C) and maxerr(y4, F.layer_norm(x3 + t.view(1, rows, C), (C,), w, b, 1e-5)) < 5e-6


# ----------------------------------------------------------------------------------- skinny linear
@pytest.mark.parametrize("M,N,K,relu,has_bias", [(100, 2048, 256, True, True), (100, 256, 2048, False, False), (100, 20, 256, False, True),
                                                  (16, 64, 64, False, True), (1, 5, 32, True, True), (128, 256, 256, False, True),
                                                  (37, 129, 96, True, False)])
def test_skinny_linear(ops, M, N, K, relu, has_bias, knobs):
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) if has_bias else None
    ref = F.linear(x.double(), w.double(), b.double() if has_bias else None)
    ref = F.relu(ref) if relu else ref
    out = ops.skinny_linear(dev(x), dev(w), dev(b) if has_bias else None, relu)
    assert out.shape == (M, N) and maxerr(out, ref) < 2e-5 * (K / 256) ** 0.5 + 2e-6
    out3 = ops.skinny_linear(dev(x.view(1, M, K)), dev(w), dev(b) if has_bias else None, relu)
    assert out3.shape == (1, M, N) and torch.equal(out3[0], out)
    big = torch.full((M + 5, N), -7.0, device="cuda")                          # out=: the launch fills a row slice of a caller-owned tensor and nothing else
    got = ops.skinny_linear(dev(x), dev(w), dev(b) if has_bias else None, relu, out=big[2:2 + M])
    assert got.data_ptr() == big[2:].data_ptr() and torch.equal(big[2:2 + M], out) and bool((big[:2] == -7).all()) and bool((big[2 + M:] == -7).all())
    # round 3: the per-row-tile decomposition (default) assigns and reduces the k blocks exactly as the round 1-2 kernel: bit-identical
    import ctypes
    from rba_amd import _lib
    var = ctypes.c_int.in_dll(_lib.load(), "rba_skinny_variant")
    try:
        var.value = 1
        old = ops.skinny_linear(dev(x), dev(w), dev(b) if has_bias else None, relu)
        var.value = 2
        new = ops.skinny_linear(dev(x), dev(w), dev(b) if has_bias else None, relu)
    finally:
        var.value = 0
    assert torch.equal(old, out) and torch.equal(new, out)


@pytest.mark.parametrize("relu", [False, True])
def test_relu_helpers_follow_torch_for_infinities_and_nan(ops, relu):
    """csrc/common.h's rba_relu / rba_clamp_below answered +-inf with NaN (max(x, floor) + (x - x)).  Round 6: compare + select -- exactly
    torch.relu / identity for +inf, -inf, NaN, -0.0.  Driven through the bias of the skinny Linear (one row of zeros -> the output IS the bias after the
    activation) and of the row-complete token Linear."""
    vals = torch.tensor([float("inf"), float("-inf"), float("nan"), -0.0, 0.0, -3.5, 2.25, 1e-30] * 4)
    N, K = vals.numel(), 64
    x, w = torch.zeros(5, K), torch.randn(N, K)
    out = ops.skinny_linear(dev(x), dev(w), dev(vals), relu).cpu()
    pre = torch.zeros(5, N) + vals                                             # what F.linear gives: (+0) + (-0.0) is +0.0 already
    want = torch.relu(pre) if relu else pre
    assert torch.equal(torch.isnan(out), torch.isnan(want))
    assert torch.equal(out.nan_to_num(7.0), want.nan_to_num(7.0))            # +-inf kept, -inf -> 0 under ReLU
    if not relu:
        assert torch.equal(torch.signbit(out), torch.signbit(want))           # signs (of zeros too) pass untouched when there is no activation


@pytest.mark.parametrize("M,E,K", [(100, 256, 256), (100, 64, 2048), (37, 32, 64), (128, 256, 256)])
def test_skinny_linear_position_add_and_segments(ops, M, E, K, knobs):
    """the q / k / v projections of a decoder self-attention layer as ONE launch over the stacked in_proj weight: columns < 2E see x + x_add,
    the rest x; three separately contiguous outputs -- each bit-equal to its own launch on the separately added input (the add is the same
    fp32 add, the k blocks are reduced in the same order), in both decompositions"""
    import ctypes
    from rba_amd import _lib
    g = torch.Generator().manual_seed(M + E + K)
    x, pos = dev(torch.randn(1, M, K, generator=g)), dev(torch.randn(1, M, K, generator=g))
    w, b = dev(torch.randn(3 * E, K, generator=g) * K ** -0.5), dev(torch.randn(3 * E, generator=g))
    var = ctypes.c_int.in_dll(_lib.load(), "rba_skinny_variant")
    try:
        for v_ in (0, 1, 2):
            var.value = v_
            q, k, v = ops.skinny_linear(x, w, b, x_add=pos, add_cols=2 * E, segments=3)
            xp = x + pos
            assert q.shape == (1, M, E) and q.is_contiguous() and k.is_contiguous() and v.is_contiguous()
            assert torch.equal(q, ops.skinny_linear(xp, w[:E].contiguous(), b[:E].contiguous()))
            assert torch.equal(k, ops.skinny_linear(xp, w[E:2 * E].contiguous(), b[E:2 * E].contiguous()))
            assert torch.equal(v, ops.skinny_linear(x, w[2 * E:].contiguous(), b[2 * E:].contiguous()))
            assert torch.equal(ops.skinny_linear(x, w, b, x_add=pos), ops.skinny_linear(xp, w, b))              # every column, one output
            assert torch.equal(ops.skinny_linear(x, w, b, relu=True, x_add=pos, add_cols=0), ops.skinny_linear(x, w, b, relu=True))
    finally:
        var.value = 0


# ----------------------------------------------------------------------------------- bf16x6 (split-bf16) linear
@pytest.mark.parametrize("M,N,K,gelu,has_bias", [(128, 128, 32, False, True), (1000, 256, 128, False, True), (777, 128, 256, True, True),
                                                 (4096, 384, 512, False, False), (130, 256, 1024, True, True), (1, 128, 64, False, True),
                                                 (2048, 512, 2048, False, True), (3600, 1024, 96, True, False),
                                                 (500, 192, 192, False, True), (900, 576, 192, True, True), (300, 100, 64, False, False),
                                                 (257, 1, 32, False, True),
                                                 # the software-pipelined form (K > 256, >= 160 tiles): even / odd block counts, ragged M and N
                                                 (8192, 1536, 512, False, True), (3000, 1100, 544, True, True), (2600, 1280, 288, False, False)])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_split_linear_vs_fp64(ops, M, N, K, gelu, has_bias, mode):
    """Six bf16 MFMAs (three f16 MFMAs) per product reproduce the fp32 Linear: error against fp64 at the level of an fp32 GEMM's own
    rounding."""
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) if has_bias else None
    ref = F.linear(x.double(), w.double(), b.double() if has_bias else None)
    ref = F.gelu(ref) if gelu else ref
    planes = ops.split_weight(dev(w), mode=mode)
    Np = (N + 127) // 128 * 128
    flat = ops.unpack_split_weight(planes)
    if mode == "bf16x6":
        assert planes.shape == (Np // 128, K // 16, 3, 128, 2, 8) and planes.dtype == torch.bfloat16
        assert flat.shape == (3, Np, K)
        assert torch.equal(flat[:, :N].float().sum(0).cpu(), w), "the three bf16 planes must sum to the fp32 weight exactly"
    else:
        assert planes.shape == (Np // 128, K // 16, 2, 128, 2, 8) and planes.dtype == torch.float16
        assert flat.shape == (2, Np, K)
        h = w.half()
        assert torch.equal(flat[0, :N].cpu(), h), "plane 0 = f16(w)"
        assert torch.equal(flat[1, :N].cpu(), ((w - h.float()) * 2048.0).half()), "plane 1 = f16((w - h) 2^11)"
        assert ((flat[0, :N].double() + flat[1, :N].double() / 2048.0).cpu() - w.double()).abs().max() <= 2.0 ** -22 * w.abs().max()
    assert not flat[:, N:].float().any(), "padding rows must be zero"
    out = ops.split_linear(dev(x), planes, dev(b) if has_bias else None, gelu=gelu, out_features=N)
    fp32 = F.linear(dev(x), dev(w), dev(b) if has_bias else None)
    fp32 = F.gelu(fp32) if gelu else fp32
    tol = 2e-5 * (K / 256) ** 0.5 + 2e-6
    assert out.shape == (M, N) and maxerr(out, ref) < tol
    if not gelu:                                                             # (the epilogue's GELU is the Abramowitz-Stegun 7.1.26 erf polynomial with v_exp_f32 / v_rcp_f32, |error| <= 2e-7: csrc/split_linear_h3.h gelu_erf2)
        assert maxerr(out, ref) < 2.0 * maxerr(fp32, ref) + 1e-6, "not worse than the fp32 GEMM it replaces"
    out3 = ops.split_linear(dev(x.view(1, M, K)), planes, dev(b) if has_bias else None, gelu=gelu, out_features=N)
    assert out3.shape == (1, M, N) and torch.equal(out3[0], out)


@pytest.mark.parametrize("M,N,K,relu,has_bias,has_add", [(2048, 256, 256, False, True, True), (2048, 96, 256, False, True, True), (2048, 256, 1024, False, True, False),
                                                         (4830, 256, 256, True, True, False), (4830, 32, 256, False, False, True), (37, 192, 64, False, True, True),
                                                         (1, 16, 32, False, True, False), (2048, 100, 96, True, True, False), (301, 256, 160, False, False, False),
                                                         (1001, 192, 544, True, True, True), (17, 256, 512, False, True, False)])
def test_token_linear_vs_fp64(ops, M, N, K, relu, has_bias, has_add):
    """Row-complete token Linear (csrc/token_linear.hip): act((x + x_add) W^T + b) against fp64 at the level of the fp32 GEMM it replaces,
    ragged M (rows per workgroup = 16), N not a multiple of 16, odd block counts; x_add is added exactly as the separate torch add did."""
    from types import SimpleNamespace
    from rba_amd._lib import RbaHipError
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) if has_bias else None
    xa = torch.randn(M, K, generator=g) if has_add else None
    xin = x + xa if has_add else x
    ref = F.linear(xin.double(), w.double(), b.double() if has_bias else None)
    ref = F.relu(ref) if relu else ref
    lin = SimpleNamespace(weight=dev(w), bias=dev(b) if has_bias else None)
    assert ops.token_linear_ok(N, K) and ops.token_linear_pays(M, N, K)
    out = ops.token_linear(dev(x), lin, x_add=dev(xa) if has_add else None, relu=relu)
    fp32 = F.linear(dev(xin), dev(w), dev(b) if has_bias else None)
    fp32 = F.relu(fp32) if relu else fp32
    tol = 2e-5 * (K / 256) ** 0.5 + 2e-6
    assert out.shape == (M, N) and maxerr(out, ref) < tol
    assert maxerr(out, ref) < 2.0 * maxerr(fp32, ref) + 1e-6, "not worse than the fp32 GEMM it replaces"
    assert torch.equal(ops.token_linear(dev(x).view(1, M, K), lin, x_add=dev(xa).view(1, M, K) if has_add else None, relu=relu)[0], out)
    with pytest.raises(RbaHipError):
        ops.token_linear(dev(x)[:, : K - 1], lin)                          # K mismatch / non-contiguous
    with pytest.raises(RbaHipError):
        ops.token_linear(dev(x), SimpleNamespace(weight=dev(torch.zeros(272, K)), bias=None))     # N > 256


@pytest.mark.parametrize("M,C,K", [(2048, 256, 256), (2048, 256, 1024), (4830, 256, 256), (50, 64, 128), (999, 128, 96), (1001, 256, 544), (17, 64, 512)])
def test_token_linear_residual_layer_norm(ops, M, C, K, knobs):
    """norm(residual + Linear(x)) in the Linear's epilogue (msdeformattn.py:134-138): against fp64, and against the unfused composition
    (the same Linear, then rba_add_layer_norm_f32) at fp32 round-off"""
    from types import SimpleNamespace
    from rba_amd._lib import RbaHipError
    g = torch.Generator().manual_seed(M + C + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(C, K, generator=g) * K ** -0.5, torch.randn(C, generator=g)
    res = torch.randn(M, C, generator=g) * 3
    norm = torch.nn.LayerNorm(C)
    with torch.no_grad():
        norm.weight.copy_(torch.rand(C, generator=g) + 0.5)
        norm.bias.copy_(torch.randn(C, generator=g))
    ref = F.layer_norm(res.double() + F.linear(x.double(), w.double(), b.double()), (C,), norm.weight.double(), norm.bias.double(), norm.eps)
    lin = SimpleNamespace(weight=dev(w), bias=dev(b))
    norm = norm.cuda()
    out = ops.token_linear(dev(x), lin, residual=dev(res), norm=norm)
    assert out.shape == (M, C) and maxerr(out, ref) < 3e-5 * (K / 256) ** 0.5
    t2 = ops.token_linear(dev(x), lin, use_bias=False)
    unf = ops.add_layer_norm(dev(res), norm.weight, norm.bias, norm.eps, t2, lin.bias)[1]
    assert maxerr(out, unf.cpu()) < 5e-6
    with pytest.raises(RbaHipError):
        ops.token_linear(dev(x), lin, residual=dev(res))                    # residual without norm
    # both workgroup shapes (one / two 16-row tiles per workgroup: rba_token_rt) give the same rows -- same products, same order
    import ctypes
    from rba_amd import _lib
    rt = ctypes.c_int.in_dll(_lib.load(), "rba_token_rt")
    try:
        rt.value = 1
        one = ops.token_linear(dev(x), lin, residual=dev(res), norm=norm)
        rt.value = 2
        two = ops.token_linear(dev(x), lin, residual=dev(res), norm=norm)
    finally:
        rt.value = 0
    assert torch.equal(one, two) and torch.equal(out, one)


def test_token_linear_multi(ops):
    """three Linears over the same rows in one launch, two of them filling column slices of one tensor (the sampling Linear of a 3-level
    MSDeformAttn: 288 outputs = 256 + 32), each with its own x_add: bit-equal to the single-problem launches"""
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(11)
    M, K = 4830, 256
    x, pos = dev(torch.randn(M, K, generator=g)), dev(torch.randn(M, K, generator=g))
    mk = lambda n: SimpleNamespace(weight=dev(torch.randn(n, K, generator=g) * K ** -0.5), bias=dev(torch.randn(n, generator=g)))
    lv, ls = mk(256), mk(288)
    parts = [(SimpleNamespace(weight=ls.weight[c:c + 256], bias=ls.bias[c:c + 256]), c) for c in (0, 256)]
    raw = torch.full((M, 288), float("nan"), device="cuda")
    outs = ops.token_linear_multi(x, [(lv, None, None, 0, False)] + [(pl, pos, raw, c0, False) for pl, c0 in parts])
    assert outs[1] is raw and outs[2] is raw and torch.isfinite(raw).all()
    assert torch.equal(outs[0], ops.token_linear(x, lv))
    for pl, c0 in parts:
        assert torch.equal(raw[:, c0:c0 + pl.weight.shape[0]], ops.token_linear(x, pl, x_add=pos))
    ref = F.linear((x + pos).double().cpu(), ls.weight.double().cpu(), ls.bias.double().cpu())
    assert maxerr(raw, ref) < 2.5e-5
    k, v = ops.token_linear_multi(x, [(lv, pos, None, 0, True), (lv, None, None, 0, False)])      # ReLU on one problem only
    assert torch.equal(k, ops.token_linear(x, lv, x_add=pos, relu=True)) and torch.equal(v, outs[0])


@pytest.mark.parametrize("M,N,K", [(8192, 512, 512), (3000, 1100, 544), (32768, 256, 256), (1000, 128, 128), (2048, 1024, 4096),
                                   (130, 200, 96)])
def test_split_linear_residual_epilogue(ops, M, N, K, knobs):
    """linear(..., residual=r): (r + x W^T) + bias in the GEMM epilogue, in place over r -- bit-identical to the unfused
    composition in the fused add + LayerNorm kernel's order ((r + t) + bias), on every kernel form (LDS-staged, pipelined, 64-column)."""
    g = torch.Generator().manual_seed(M + N + K)
    x, w = dev(torch.randn(M, K, generator=g)), dev(torch.randn(N, K, generator=g) * K ** -0.5)
    b, r = dev(torch.randn(N, generator=g)), dev(torch.randn(M, N, generator=g))
    planes = ops.split_weight(w, mode="f16x3")
    t = ops.split_linear(x, planes, None, out_features=N)
    want = (r + t) + b
    r2 = r.clone()
    out = ops.split_linear(x, planes, b, out_features=N, residual=r2)
    assert out.data_ptr() == r2.data_ptr() and torch.equal(out, want)


@pytest.fixture
def k6_k_split_off(knobs):
    """rba_k6_ks = 1 (knobs build of the library) for the duration of a test that compares launch forms bit for bit."""
    import ctypes
    from rba_amd import _lib
    ks = ctypes.c_int.in_dll(_lib.load(), "rba_k6_ks")
    ks.value = 1
    yield
    ks.value = 0


@pytest.mark.parametrize("M,N,K", [(8192, 512, 512), (8192, 2048, 512), (3000, 1100, 544), (2048, 3072, 1024), (130, 200, 96), (31, 128, 32),
                                   (8192, 512, 2048)])
def test_split_linear_from_split_activations(ops, M, N, K, k6_k_split_off):
    """The f16x3 GEMM reading its A operand as the producer's split fragment image (SplitActivations): bit-identical to the
    fp32-input kernel, with every epilogue (bias, GELU, ReLU, residual), one and two workgroups per CU, ragged M and N.  (The K-split form, which
    only split-image launches run and which sums K in its own order, is held off: test_split_linear_k_split_form covers it.)"""
    g = torch.Generator().manual_seed(M + N + K)
    x, w = dev(torch.randn(M, K, generator=g) * 3), dev(torch.randn(N, K, generator=g) * K ** -0.5)
    b, r = dev(torch.randn(N, generator=g)), dev(torch.randn(M, N, generator=g))
    planes = ops.split_weight(w, mode="f16x3")
    xs = ops.SplitActivations.pack(x)
    assert torch.equal(xs.unpack(), (x.half().float() + ((x - x.half().float()) * 2048).half().float() / 2048))
    for kw in ({}, {"gelu": True}, {"relu": True}):
        assert torch.equal(ops.split_linear(xs, planes, b, out_features=N, **kw), ops.split_linear(x, planes, b, out_features=N, **kw))
    want = ops.split_linear(x, planes, b, out_features=N, residual=r.clone())
    got = ops.split_linear(xs, planes, b, out_features=N, residual=r.clone())
    assert torch.equal(got, want)
    assert torch.equal(ops.split_linear(xs, planes, None, out_features=N), ops.split_linear(x, planes, None, out_features=N))


@pytest.mark.parametrize("M,N,K", [(8192, 2048, 512), (8192, 512, 2048), (8100, 1536, 512), (3680, 2048, 512), (40000, 256, 288), (16500, 640, 544)])
def test_split_linear_256x128_form_is_bit_identical(ops, M, N, K, knobs):
    """Round 4: the 256 x 128 / eight-wave / shared-weight-ring form of the pipelined f16x3 kernel (rba_k6_rs: 1 = off, 3 = from 64 tiles -- what
    ops.set_concurrent_streams(n >= 2) selects) against the 128 x 128 form, on split-image operands: fp32 rows out (plain, GELU, ReLU), the
    residual epilogue, GELU + split image out; M not a multiple of 256 (a whole 128-row half beyond M), N not a multiple of 128."""
    import ctypes
    from rba_amd import _lib
    rs = ctypes.c_int.in_dll(_lib.load(), "rba_k6_rs")
    min_k = ctypes.c_int.in_dll(_lib.load(), "rba_k6_rs_min_k")               # product: the 8-wave form from K = 512 on; here for every K
    prev_min_k = min_k.value
    g = torch.Generator().manual_seed(M + N + K)
    x, w = dev(torch.randn(M, K, generator=g) * 3), dev(torch.randn(N, K, generator=g) * K ** -0.5)
    b, r = dev(torch.randn(N, generator=g)), dev(torch.randn(M, N, generator=g))
    planes = ops.split_weight(w, mode="f16x3")
    xs = ops.SplitActivations.pack(x)

    def run():
        outs = [ops.split_linear(xs, planes, b, out_features=N, **kw) for kw in ({}, {"gelu": True}, {"relu": True})]
        outs.append(ops.split_linear(xs, planes, b, out_features=N, residual=r.clone()))
        if N % 32 == 0:
            so = ops.split_linear(xs, planes, b, gelu=True, out_features=N, split_out=True)
            outs.append(so.data[: M // 32 * 32 * N].clone())
            outs.append(so.unpack())
        return outs
    ks = ctypes.c_int.in_dll(_lib.load(), "rba_k6_ks")                        # the K-split form (its own summation order) off: this test compares tile shapes
    try:
        min_k.value = 0
        ks.value = 1
        rs.value = 1
        want = run()
        rs.value = 3
        got = run()
    finally:
        rs.value = 0
        ks.value = 0
        min_k.value = prev_min_k
    assert prev_min_k == 512
    assert ((M + 255) // 256) * ((N + 127) // 128) >= 64                      # the 8-wave form was reached
    for a_, b_ in zip(got, want):
        assert torch.equal(a_, b_)


@pytest.mark.parametrize("M,N,K", [(8192, 512, 2048), (8100, 500, 1024), (4224, 1024, 3072), (300, 200, 128), (8192, 512, 576)])
def test_split_linear_k_split_form(ops, M, N, K, knobs):
    """Round 4: the K-split 8-wave form of the pipelined f16x3 kernel (KS = 2: two wave sets on the even / odd 32-wide blocks of K, summed through LDS in a
    fixed order) that the single-resident launches with K >= 1024 run on one stream (Swin-B stage-3 fc2).  Not the one-set kernel's summation order, so not
    bit-identical to it: both are held to the same fp64 bound, agree to a few ulp, and the form is deterministic.  rba_k6_ks: 1 = off, 2 = wherever legal."""
    import ctypes
    from rba_amd import _lib
    ks = ctypes.c_int.in_dll(_lib.load(), "rba_k6_ks")
    g = torch.Generator().manual_seed(M + N + K)
    x, w = torch.randn(M, K, generator=g) * 3, torch.randn(N, K, generator=g) * K ** -0.5
    b, r = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    planes = ops.split_weight(dev(w), mode="f16x3")
    xs = ops.SplitActivations.pack(dev(x))
    ref = F.linear(x.double(), w.double(), b.double())

    def run():
        return [ops.split_linear(xs, planes, dev(b), out_features=N), ops.split_linear(xs, planes, dev(b), out_features=N, relu=True),
                ops.split_linear(xs, planes, dev(b), out_features=N, residual=dev(r).clone())]
    try:
        ks.value = 1
        one = run()
        ks.value = 2
        two, again = run(), run()
    finally:
        ks.value = 0
    refs = [ref, ref.relu(), ref + r.double()]
    tol = 2e-5 * (K / 256) ** 0.5 + 2e-6
    for o, t, a2, rf in zip(one, two, again, refs):
        assert torch.equal(t, a2)                                              # deterministic
        assert maxerr(o, rf) < tol and maxerr(t, rf) < tol                     # the same fp64 bound for both forms
        assert maxerr(t, o.double()) < tol                                     # a few ulp of the largest outputs
    if (K & 63) == 0:
        assert not all(torch.equal(t, o) for t, o in zip(two, one)) or K < 256  # the form was reached (a different summation order shows in the last bits)
    else:
        assert all(torch.equal(t, o) for t, o in zip(two, one))               # odd block count: the form does not apply


@pytest.mark.parametrize("M,N,K", [(8192, 2048, 512), (131072, 512, 128), (3000, 1120, 544), (2048, 4096, 1024), (130, 96, 96), (8192, 256, 512)])
def test_split_linear_gelu_split_output(ops, M, N, K):
    """fc1 -> fc2 hand-over: GELU(x W^T + b) written by the operand-swapped GEMM as SplitActivations == pack(fp32 result), bit for bit,
    from fp32 rows and from a split image, ragged M / N % 128, one and two workgroups per CU."""
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = dev(torch.randn(M, K, generator=g)), dev(torch.randn(N, K, generator=g) * K ** -0.5), dev(torch.randn(N, generator=g))
    planes = ops.split_weight(w, mode="f16x3")
    ref = ops.SplitActivations.pack(ops.split_linear(x, planes, b, gelu=True, out_features=N))
    nfull = M // 32 * 32 * N
    for xin in (x, ops.SplitActivations.pack(x)):
        got = ops.split_linear(xin, planes, b, gelu=True, out_features=N, split_out=True)
        assert got.shape == (M, N) and torch.equal(got.data[:nfull], ref.data[:nfull]) and torch.equal(got.unpack(), ref.unpack())
    with pytest.raises(ops.RbaHipError):
        ops.split_linear(x, planes, b, out_features=N, split_out=True)


@pytest.mark.parametrize("M,hidden", [(131072, 512), (3000, 512), (130, 96), (57600, 512), (128, 64)])
def test_swin_mlp_fused(ops, M, hidden):
    """One-kernel Mlp + residual for C = 128: bit-identical to fc1 (GELU, split output) -> fc2 (residual epilogue), and within the GEMM
    tolerance of the fp64 composition."""
    g = torch.Generator().manual_seed(M + hidden)
    C = 128
    fc1, fc2 = torch.nn.Linear(C, hidden).cuda(), torch.nn.Linear(hidden, C).cuda()
    x, r = dev(torch.randn(M, C, generator=g) * 2), dev(torch.randn(M, C, generator=g))
    with torch.no_grad():
        want = ops.linear(ops.linear(x, fc1, gelu=True, split_out=True), fc2, residual=r.clone())
        got = ops.mlp_fused(x, fc1, fc2, r.clone())
        ref = r.double() + F.linear(F.gelu(F.linear(x.double(), fc1.weight.double(), fc1.bias.double())), fc2.weight.double(), fc2.bias.double())
    assert maxerr(got, ref) < 3e-5
    assert torch.equal(got, want)
    assert ops.mlp_fused_ok(131072, 128, 512) and not ops.mlp_fused_ok(131072, 192, 768) and not ops.mlp_fused_ok(8192, 128, 512)


def test_swin_mlp_fused_with_norm2_in_its_prologue(ops):
    """round 5: x <- x + fc2(GELU(fc1(norm2(x)))) with the LayerNorm computed by the MLP kernel itself, against float64 and against LN -> mlp_fused"""
    from torch import nn
    g = torch.Generator().manual_seed(11)
    for M in (32768, 32768 + 77):
        C, hidden = 128, 512
        fc1, fc2 = nn.Linear(C, hidden), nn.Linear(hidden, C)
        with torch.no_grad():
            for p_ in (fc1.weight, fc2.weight):
                p_.copy_(torch.randn(p_.shape, generator=g) * p_.shape[1] ** -0.5)
            fc1.bias.copy_(torch.randn(hidden, generator=g) * 0.2)
            fc2.bias.copy_(torch.randn(C, generator=g) * 0.2)
        fc1, fc2 = fc1.cuda(), fc2.cuda()
        x = torch.randn(M, C, generator=g) * 2.0 + 0.5
        gam, bet = torch.randn(C, generator=g) * 0.3 + 1.0, torch.randn(C, generator=g) * 0.2
        xd = x.double()
        y = F.layer_norm(xd, (C,), gam.double(), bet.double(), 1e-5)
        want = xd + F.linear(F.gelu(F.linear(y, fc1.weight.double().cpu(), fc1.bias.double().cpu())), fc2.weight.double().cpu(), fc2.bias.double().cpu())
        xg = dev(x)
        out = ops.mlp_fused_ln(xg, (dev(gam), dev(bet), 1e-5), fc1, fc2)
        assert out.data_ptr() == xg.data_ptr() and maxerr(out, want) < 3e-5
        x2 = dev(x)
        y2 = ops.add_layer_norm(x2, dev(gam), dev(bet), 1e-5)[1]
        two = ops.mlp_fused(y2, fc1, fc2, x2)
        assert maxerr(out, two.double()) < 5e-6


@pytest.mark.parametrize("rows,C", [(8192, 512), (2048, 1024), (1000, 96), (33, 32), (4100, 1536), (70, 2048)])
def test_add_layer_norm_split_output(ops, rows, C):
    """add_layer_norm(frag=True): the LayerNorm output written directly as SplitActivations == pack(fp32 output), bit for bit, with and
    without the fused residual add; the summed tensor is unchanged."""
    g = torch.Generator().manual_seed(rows + C)
    x, t = dev(torch.randn(rows, C, generator=g) * 2), dev(torch.randn(rows, C, generator=g))
    tb, w, b = dev(torch.randn(C, generator=g)), dev(torch.randn(C, generator=g)), dev(torch.randn(C, generator=g))
    for res, rb in ((None, None), (t, tb)):
        s0, y0 = ops.add_layer_norm(x, w, b, 1e-5, res, rb)
        s1, y1 = ops.add_layer_norm(x, w, b, 1e-5, res, rb, frag=True)
        assert isinstance(y1, ops.SplitActivations) and y1.shape == tuple(x.shape)
        ref = ops.SplitActivations.pack(y0)
        K = C
        nfull = rows // 32 * 32 * K                                            # the padding rows of the last group are never written
        assert torch.equal(y1.data[:nfull], ref.data[:nfull])
        assert torch.equal(y1.unpack(), ref.unpack()) and torch.equal(s0, s1)
    with pytest.raises(ops.RbaHipError):
        ops.add_layer_norm(dev(torch.randn(8, 48)), dev(torch.randn(48)), dev(torch.randn(48)), frag=True)


def test_split_linear_relu_epilogue(ops):
    g = torch.Generator().manual_seed(3)
    for M, N, K in ((1000, 1024, 256), (300, 256, 1024)):
        x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
        for mode in ("f16x3", "bf16x6"):
            out = ops.split_linear(dev(x), ops.split_weight(dev(w), mode=mode), dev(b), relu=True)
            assert maxerr(out, F.relu(F.linear(x.double(), w.double(), b.double()))) < 2e-5 * (K / 256) ** 0.5 + 2e-6 and float(out.min()) >= 0.0
        lin = torch.nn.Linear(K, N).cuda()
        xx = torch.randn(40000, K, device="cuda")
        assert maxerr(ops.linear(xx, lin, relu=True), F.relu(F.linear(xx.double(), lin.weight.double(), lin.bias.double()))) < 3e-5


def test_relu_epilogues_keep_nan(ops):
    """the f16x3 kernels answer an operand beyond f16's range with NaN, and the evaluator re-scores an image on bf16x6 when its score map holds a
    NaN -- so no ReLU on the way may turn NaN into 0 (fmaxf does).  Every ReLU form: K6 epilogue, token / skinny Linear, GroupNorm(+ReLU) both layouts."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(256, 128, generator=g)
    x[7, 5] = 7e4                                                                     # beyond 65504: row 7 of every f16x3 product is NaN
    w = torch.randn(128, 128, generator=g) * 0.1
    y = ops.split_linear(dev(x), ops.split_weight(dev(w), mode="f16x3"), None, relu=True, out_features=128)
    assert torch.isnan(y[7]).all() and torch.isfinite(y[8]).all() and (y[8] >= 0).all()
    lin = torch.nn.Linear(128, 128).cuda()
    t = ops.token_linear(dev(x), lin, relu=True)
    assert torch.isnan(t[7]).all() and torch.isfinite(t[6]).all()
    xn = torch.randn(1, 64, 32, generator=g)
    xn[0, 3, 9] = float("nan")
    one, zero = dev(torch.ones(32)), dev(torch.zeros(32))
    assert torch.isnan(ops.group_norm_nhwc(dev(xn), 4, one, zero, relu=True)[0, :, 8:16]).all()          # the NaN's group: statistics and outputs NaN
    assert torch.isnan(ops.group_norm(dev(xn.permute(0, 2, 1).reshape(1, 32, 8, 8).contiguous()), 4, one, zero, relu=True)[0, 8:16]).all()
    sk = ops.skinny_linear(dev(torch.full((4, 128), float("nan"))), dev(w), None, relu=True)
    assert torch.isnan(sk).all()
    # the GroupNorm + ReLU folded into the mask-feature projection's loads (FPN: an overflowed convolution output must not come out as zeros)
    B, P, K, N, G = 2, 256, 256, 128, 32
    xf = torch.randn(B, P, K, generator=g)
    xf[1, 17, 40] = float("nan")
    p3 = ops.split_weight(dev(torch.randn(N, K, generator=g) * K ** -0.5), mode="f16x3")
    mr = ops.group_norm_nhwc_stats(dev(xf), G, 1e-5)
    o = ops.split_linear_nchw_out_gn(dev(xf).view(B * P, K), mr, dev(torch.ones(K)), dev(torch.zeros(K)), G, True, p3, None, P, out_features=N)
    assert torch.isfinite(o[0]).all() and torch.isnan(o[1]).all()


def test_split_linear_extreme_values(ops):
    """Exactness of the split over the exponent range, zeros, and values whose low planes vanish."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(256, 64, generator=g) * torch.logspace(-12, 12, 64).view(1, 64)
    x[:, 7] = 0.0
    w = torch.zeros(128, 64)
    w[torch.arange(128), torch.arange(128) % 64] = 1.0                       # a selection matrix: output must equal the input
    out = ops.split_linear(dev(x), ops.split_weight(dev(w), mode="bf16x6"))
    assert torch.equal(out.cpu(), x[:, torch.arange(128) % 64])
    w2 = torch.randn(128, 64, generator=g).bfloat16().float()               # weights exactly representable in bf16
    p2 = ops.unpack_split_weight(ops.split_weight(dev(w2), mode="bf16x6"))
    assert torch.equal(p2[0].float().cpu(), w2) and not p2[1:].float().any()


def test_split_linear_f16x3_range(ops):
    """The f16x3 form over ITS exponent range: 22 bits of every input survive from 1e-7 (f16's subnormals: the 2^11-scaled
    residual keeps the bits the high piece lost) to 6e4; zeros are exact; beyond 65504 the output is NaN (never a wrong number)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(256, 64, generator=g) * torch.logspace(-7, 4, 64).view(1, 64)
    x[:, 7] = 0.0
    x = x.clamp(-6.0e4, 6.0e4)
    w = torch.zeros(128, 64)
    w[torch.arange(128), torch.arange(128) % 64] = 1.0
    out = ops.split_linear(dev(x), ops.split_weight(dev(w), mode="f16x3")).cpu()
    want = x[:, torch.arange(128) % 64]
    big = want.abs() >= 6.2e-5                                                # f16 normal range: h carries 11 bits, l the next 11
    assert ((out - want).abs()[big] <= 2.0 ** -21 * want.abs()[big]).all()
    assert ((out - want).abs()[~big] <= 2.0 ** -35).all()                   # below: absolute error of the scaled residual's rounding
    assert torch.equal(out[:, 7], torch.zeros(256))
    x[3, 5] = 7.0e4                                                           # outside f16: that row's outputs that use it are NaN
    out = ops.split_linear(dev(x), ops.split_weight(dev(w), mode="f16x3")).cpu()
    assert torch.isnan(out[3, 5]) and torch.isnan(out[3, 69]) and not torch.isnan(out[4]).any()
    w2 = torch.randn(128, 64, generator=g).half().float()                    # weights exactly representable in f16
    p2 = ops.unpack_split_weight(ops.split_weight(dev(w2), mode="f16x3"))
    assert torch.equal(p2[0].float().cpu(), w2) and not p2[1].float().any()


def test_split_linear_dispatch_and_errors(ops):
    from rba_amd._lib import RbaHipError
    lin = torch.nn.Linear(512, 2048).cuda()
    x = torch.randn(2, 16384, 512, device="cuda")
    assert ops.split_linear_pays(32768, 2048, 512, gelu=True) and not ops.split_linear_pays(100, 2048, 512, gelu=True)
    y = ops.linear(x, lin, gelu=True)
    from rba_amd.lru import peek
    assert peek(lin, ("planes", "f16x3")) is not None and peek(lin, ("planes", "f16x3")).dtype == torch.float16, "f16x3 path not taken"
    assert maxerr(y, F.gelu(F.linear(x.double(), lin.weight.double(), lin.bias.double()))) < 3e-5
    planes_before = peek(lin, ("planes", "f16x3"))
    with torch.no_grad():
        lin.weight.mul_(2.0)                                                 # new weights -> planes are re-split
    y2 = ops.linear(x, lin, use_bias=False)
    assert peek(lin, ("planes", "f16x3")) is not None and peek(lin, ("planes", "f16x3")) is not planes_before
    assert maxerr(y2, F.linear(x.double(), lin.weight.double())) < 3e-5
    small = torch.nn.Linear(96, 100).cuda()                                   # unsupported shape -> hipBLASLt, same result contract
    assert maxerr(ops.linear(x[..., :96].contiguous(), small), F.linear(x[..., :96].double(), small.weight.double(), small.bias.double())) < 3e-5
    planes = ops.split_weight(lin.weight.detach())
    with pytest.raises(RbaHipError):
        ops.split_linear(x.cpu(), planes)
    with pytest.raises(RbaHipError):
        ops.split_linear(x[..., :256], planes)                                # non-contiguous / wrong K
    with pytest.raises(RbaHipError):
        ops.split_linear(x, planes.float())
    with pytest.raises(RbaHipError):
        ops.split_weight(torch.randn(128, 48, device="cuda"))                    # K % 32 != 0
    with pytest.raises(RbaHipError):
        ops.split_linear(x, planes, out_features=1000)                           # does not match the packed tiles
    assert ops.split_linear(x[:0], planes).shape == (0, 16384, 2048)


# ----------------------------------------------------------------------------------- bf16x6 conv3x3 (NHWC) and NCHW-out Linear
@pytest.mark.parametrize("B,H,W,C,N,has_bias", [(1, 16, 24, 32, 128, False), (2, 9, 13, 64, 256, True), (1, 33, 20, 256, 256, False),
                                                (1, 5, 3, 32, 40, True), (1, 64, 128, 256, 256, False)])
@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_conv3x3_nhwc_vs_fp64(ops, B, H, W, C, N, has_bias, mode):
    """Implicit-GEMM 3x3 convolution (pad 1) on NHWC activations against F.conv2d in fp64, borders included."""
    g = torch.Generator().manual_seed(B * 1000 + H * W + C)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5
    b = torch.randn(N, generator=g) if has_bias else None
    ref = F.conv2d(x.double(), w.double(), b.double() if has_bias else None, padding=1).permute(0, 2, 3, 1)
    planes = ops.conv3x3_weight(dev(w), mode=mode)
    out = ops.conv3x3_nhwc(dev(x.permute(0, 2, 3, 1).contiguous()), planes, dev(b) if has_bias else None, out_features=N)
    assert out.shape == (B, H, W, N)
    assert maxerr(out, ref) < 2e-5 * (9 * C / 256) ** 0.5 + 2e-6


@pytest.mark.parametrize("B,H,W,C,N,has_bias", [(1, 128, 256, 256, 256, False), (2, 100, 167, 64, 256, True), (1, 256, 512, 256, 256, False),
                                                  (3, 131, 90, 32, 200, True)])
def test_conv3x3_nhwc_from_split_activations(ops, B, H, W, C, N, has_bias):
    """The FPN hand-over: `lateral + upsample` written by the resample kernel as the convolution's split operand, and the pipelined
    convolution gathering neighbour-pixel pieces from it: both bit-identical to the fp32-row forms (borders, ragged M, several images)."""
    g = torch.Generator().manual_seed(B * 1000 + H * W + C)
    assert ops.conv3x3_takes_split(B * H * W, N)
    h2, w2 = (H + 1) // 2, (W + 1) // 2
    prev, cur = dev(torch.randn(B, h2, w2, C, generator=g)), dev(torch.randn(B, H, W, C, generator=g))
    w = dev(torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5)
    b = dev(torch.randn(N, generator=g)) if has_bias else None
    y32 = torch.stack([ops.resample_bilinear_nhwc(prev[i], (H, W), add=cur[i]) for i in range(B)])
    ys = ops.SplitActivations.empty((B, H, W, C), prev.device)
    for i in range(B):
        assert ops.resample_bilinear_nhwc(prev[i], (H, W), add=cur[i], split_into=ys, image=i) is ys
    want = ops.SplitActivations.pack(y32)
    nfull = (B * H * W) // 32 * 32 * C
    assert torch.equal(ys.data[:nfull], want.data[:nfull]) and torch.equal(ys.unpack(), want.unpack())
    planes = ops.conv3x3_weight(w, mode="f16x3")
    z32 = ops.conv3x3_nhwc(y32, planes, b, out_features=N)
    zs = ops.conv3x3_nhwc(ys, planes, b, out_features=N)
    ref = F.conv2d(y32.permute(0, 3, 1, 2).double(), w.double(), b.double() if has_bias else None, padding=1).permute(0, 2, 3, 1)
    assert maxerr(zs, ref) < 2e-5 * (9 * C / 256) ** 0.5 + 2e-6
    assert torch.equal(zs, z32)                           # same products, same order as the LDS-staged fp32-row kernel
    no_add = ops.SplitActivations.empty((1, H, W, C), prev.device)
    ops.resample_bilinear_nhwc(prev[0], (H, W), split_into=no_add)
    assert torch.equal(no_add.unpack()[0], ops.SplitActivations.pack(ops.resample_bilinear_nhwc(prev[0], (H, W))).unpack())


@pytest.mark.parametrize("B,P,K,N", [(1, 1000, 64, 128), (2, 384, 256, 256), (1, 777, 128, 40), (3, 130, 32, 300), (2, 640, 512, 256)])
def test_split_linear_nchw_out(ops, B, P, K, N):
    g = torch.Generator().manual_seed(B + P + K + N)
    x, w, b = torch.randn(B * P, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ref = F.linear(x.double(), w.double(), b.double()).view(B, P, N).permute(0, 2, 1)
    planes = ops.split_weight(dev(w), mode="bf16x6")
    out = ops.split_linear_nchw_out(dev(x), planes, dev(b), P, out_features=N)
    assert out.shape == (B, N, P) and maxerr(out, ref) < 2e-5 * (K / 256) ** 0.5 + 2e-6
    same = ops.split_linear(dev(x), planes, dev(b), out_features=N).view(B, P, N).permute(0, 2, 1)
    assert maxerr(out, same.double()) < 1e-5      # same six terms; the operand roles (and so the summation order) are swapped
    # round 3: the f16x3 form (what the mask-feature projection runs): the LDS-staged kernel with a channel-major epilogue -- the same
    # accumulators as the row-major Linear, so the two agree bit for bit; P % 4 != 0 takes the scalar-store path, bias may be absent
    p3 = ops.split_weight(dev(w), mode="f16x3")
    out3 = ops.split_linear_nchw_out(dev(x), p3, dev(b), P, out_features=N)
    same3 = ops.split_linear(dev(x), p3, dev(b), out_features=N).view(B, P, N).permute(0, 2, 1)
    assert out3.shape == (B, N, P) and maxerr(out3, ref) < 2e-5 * (K / 256) ** 0.5 + 2e-6
    if K <= 256:                                  # the row-major Linear runs the same LDS-staged kernel there
        assert torch.equal(out3, same3.contiguous())
    nb = ops.split_linear_nchw_out(dev(x), p3, None, P, out_features=N)
    assert maxerr(nb, ref - b.double()[None, :, None]) < 2e-5 * (K / 256) ** 0.5 + 2e-6


@pytest.mark.parametrize("B,P,K,N,G,relu", [(1, 1024, 256, 256, 32, True), (2, 384, 256, 256, 32, True), (1, 256, 128, 40, 32, False), (3, 128, 64, 300, 4, True),
                                              (1, 131072, 256, 256, 32, True)])
def test_split_linear_nchw_out_with_folded_group_norm(ops, B, P, K, N, G, relu):
    """round 4: GroupNorm (+ ReLU) of the input rows applied inside the projection's loads == group_norm_nhwc followed by the projection, bit for bit
    (`mask_features(layer_1(y))`, pixel_decoder/msdeformattn.py:357-362)."""
    g = torch.Generator().manual_seed(B + P + K + N)
    x = torch.randn(B, P, K, generator=g) * 3 + 0.7
    w, b = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ga, be = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    xd = dev(x)
    p3 = ops.split_weight(dev(w), mode="f16x3")
    assert ops.split_linear_nchw_out_takes_gn(p3, P, K, G)
    two = ops.split_linear_nchw_out(ops.group_norm_nhwc(xd, G, dev(ga), dev(be), 1e-5, relu=relu).view(B * P, K), p3, dev(b), P, out_features=N)
    mr = ops.group_norm_nhwc_stats(xd, G, 1e-5)
    one = ops.split_linear_nchw_out_gn(xd.view(B * P, K), mr, dev(ga), dev(be), G, relu, p3, dev(b), P, out_features=N)
    assert one.shape == (B, N, P) and torch.equal(one, two)
    if P >= 65536:
        # round 5: builds of this kernel in which the compiler used a packed multiply with the cross select on source 1 (`v_pk_mul_f32 ... op_sel:[0,1]`) for
        # a = gamma * rstd staged a few hundred rows per launch with a = 0 -- a different set in every launch (csrc/split_linear_gnf.hip,
        # profiles/r05_gnfold_select.txt).  The translation unit is compiled without packed fp32 since; every launch must give the same bits.
        for _ in range(6):
            again = ops.split_linear_nchw_out_gn(xd.view(B * P, K), mr, dev(ga), dev(be), G, relu, p3, dev(b), P, out_features=N)
            assert torch.equal(again, two)
    y = F.group_norm(x.double().permute(0, 2, 1), G, ga.double(), be.double(), 1e-5)
    ref = F.linear((y.relu() if relu else y).permute(0, 2, 1), w.double(), b.double()).permute(0, 2, 1)
    assert maxerr(one, ref) < 4e-5 * (K / 256) ** 0.5 + 4e-6
    assert not ops.split_linear_nchw_out_takes_gn(p3, P + 4, K, G)                 # ragged images keep the two-call form
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError):
        ops.split_linear_nchw_out_gn(xd.view(B * P, K), mr[:, :1].contiguous(), dev(ga), dev(be), G, relu, p3, dev(b), P, out_features=N)


@pytest.mark.parametrize("B,P,K,N,G,has_bias", [(1, 32768, 256, 256, 32, False), (2, 16384, 128, 256, 32, True), (1, 131072, 128, 256, 32, False), (1, 20480, 64, 128, 8, False)])
def test_linear_with_gn_moments_epilogue(ops, B, P, K, N, G, has_bias):
    """round 4: the FPN's lateral 1 x 1 convolution leaves the GroupNorm moments of its output in its epilogue: the output is the plain Linear's bit for bit,
    the merged (mean, rstd) equal the statistics pass over the output (and fp64) up to the summation order (pixel_decoder/msdeformattn.py:222-235)."""
    g = torch.Generator().manual_seed(B + P + K + N)
    x = dev(torch.randn(B, P, K, generator=g) * 2 + 0.3)
    lin = torch.nn.Linear(K, N).cuda()
    with torch.no_grad():
        lin.weight.copy_(dev(torch.randn(N, K, generator=g) * K ** -0.5))
        lin.bias.copy_(dev(torch.randn(N, generator=g)))
    assert ops.linear_emits_gn_moments(B * P, N, K, P, G)
    with torch.no_grad():
        y, mr = ops.linear_gn_stats(x, lin, G, 1e-5, P, use_bias=has_bias)
        want = ops.linear(x, lin, use_bias=has_bias)
    assert torch.equal(y, want)
    ref = ops.group_norm_nhwc_stats(want, G, 1e-5)
    yd = want.double().view(B, P, G, N // G)
    mean64, var64 = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
    assert mr.shape == (B, G, 2)
    assert maxerr(mr[..., 0], mean64) < 2e-6 and maxerr(ref[..., 0], mean64) < 2e-6
    assert ((mr[..., 1].double().cpu() * (var64 + 1e-5).sqrt().cpu()) - 1).abs().max() < 2e-6
    assert not ops.linear_emits_gn_moments(B * P, N, K, P + 64, G) and not ops.linear_emits_gn_moments(B * P, N, 512, P, G)


@pytest.mark.parametrize("B,H,W,C,N,G", [(1, 128, 256, 256, 256, 32), (2, 64, 128, 64, 256, 32), (1, 256, 512, 256, 256, 32)])
def test_conv3x3_with_gn_moments_epilogue(ops, B, H, W, C, N, G):
    """round 4: the same for the FPN's 3 x 3 output convolution on its split-image operand (both tile forms of the pipelined kernel)."""
    g = torch.Generator().manual_seed(B * 1000 + H * W + C)
    x = dev(torch.randn(B, H, W, C, generator=g))
    w = dev(torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5)
    planes = ops.conv3x3_weight(w, mode="f16x3")
    xs = ops.SplitActivations.pack(x.view(B * H * W, C))
    xs = ops.SplitActivations(xs.data, (B, H, W, C))
    assert ops.conv3x3_emits_gn_moments(B, H, W, N, G)
    y, mr = ops.conv3x3_nhwc_gn_stats(xs, planes, G, 1e-5, None, out_features=N)
    want = ops.conv3x3_nhwc(xs, planes, None, out_features=N)
    assert torch.equal(y, want)
    yd = want.double().view(B, H * W, G, N // G)
    mean64, var64 = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
    assert maxerr(mr[..., 0], mean64) < 2e-6
    assert ((mr[..., 1].double().cpu() * (var64 + 1e-5).sqrt().cpu()) - 1).abs().max() < 2e-6
    assert not ops.conv3x3_emits_gn_moments(B, 75, 50, N, G) and not ops.conv3x3_emits_gn_moments(B, H, W, N, 2)      # ragged tiles / 128-channel groups


# ----------------------------------------------------------------------------------- channels-last GroupNorm / resample
@pytest.mark.parametrize("B,P,C,G,relu", [(1, 1000, 256, 32, True), (2, 257, 256, 32, False), (1, 131072, 256, 32, True),
                                          (1, 77, 128, 32, False), (3, 5, 64, 4, True), (1, 300, 1024, 32, False)])
def test_group_norm_nhwc(ops, B, P, C, G, relu):
    g = torch.Generator().manual_seed(P + C)
    x = torch.randn(B, P, C, generator=g) * 2.0 + 0.7
    w, b = torch.randn(C, generator=g), torch.randn(C, generator=g)
    ref = F.group_norm(x.double().permute(0, 2, 1), G, w.double(), b.double(), 1e-5).permute(0, 2, 1)
    ref = F.relu(ref) if relu else ref
    out = ops.group_norm_nhwc(dev(x), G, dev(w), dev(b), 1e-5, relu=relu)
    assert out.shape == x.shape and maxerr(out, ref) < 2e-5
    same = ops.group_norm(dev(x.permute(0, 2, 1).reshape(B, C, P, 1).contiguous()), G, dev(w), dev(b), 1e-5, relu=relu)
    assert maxerr(out, same.view(B, C, P).permute(0, 2, 1).double()) < 2e-5


@pytest.mark.parametrize("h,w,H,W,C,has_add", [(32, 64, 64, 128, 256, True), (7, 9, 14, 18, 8, False), (45, 80, 90, 160, 256, True),
                                               (5, 5, 12, 7, 4, False), (64, 128, 256, 512, 256, True)])
def test_resample_bilinear_nhwc(ops, h, w, H, W, C, has_add):
    g = torch.Generator().manual_seed(h * w + C)
    x = torch.randn(h, w, C, generator=g)
    add = torch.randn(H, W, C, generator=g) if has_add else None
    ref = F.interpolate(x.permute(2, 0, 1)[None].double(), size=(H, W), mode="bilinear", align_corners=False)[0].permute(1, 2, 0)
    ref = ref + add.double() if has_add else ref
    out = ops.resample_bilinear_nhwc(dev(x), (H, W), add=dev(add) if has_add else None)
    assert out.shape == (H, W, C) and maxerr(out, ref) < 1e-5
    nchw = ops.resample_bilinear(dev(x.permute(2, 0, 1).contiguous()), (H, W),
                                 add=dev(add.permute(2, 0, 1).contiguous()) if has_add else None)
    assert maxerr(out, nchw.permute(1, 2, 0).double()) < 2e-6      # same taps and weights (fma contraction may differ)


# ----------------------------------------------------------------------------------- gaussian smoothing of the score map
@pytest.mark.parametrize("B,Q,S", [(1, 100, 2048), (2, 16, 77), (1, 3, 1), (1, 100, 8192)])
def test_quad_mean_is_the_centre_sample_bit_for_bit(ops, B, Q, S):
    """rba_quad_mean_f32 == ((v0 + v1) + (v2 + v3)) * 0.25 (the torch expression it replaced in the sparse prediction head) exactly, and equals
    F.interpolate(bilinear, align_corners=False) of a [2h, 2w] map down to [h, w] at the same four pixels"""
    g = torch.Generator().manual_seed(S + Q)
    v = dev(torch.randn(B, Q, 4, S, generator=g) * 7)
    want = ((v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])) * 0.25
    got = ops.quad_mean(v)
    assert got.shape == (B, Q, S) and torch.equal(got, want)
    assert ops.quad_mean(v[:, :0]).shape == (B, 0, S)
    with pytest.raises(Exception):
        ops.quad_mean(dev(torch.zeros(2, 3, 5)))


@pytest.mark.parametrize("R,K1", [(100, 20), (1, 2), (257, 64), (300, 9)])
def test_softmax_drop_last_vs_torch(ops, R, K1):
    """rba_softmax_drop_last_f32 against F.softmax(x, -1)[..., :-1] in fp64; rows still sum to 1 with the dropped column; extreme logits"""
    g = torch.Generator().manual_seed(R + K1)
    x = torch.randn(R, K1, generator=g) * 6
    x[0, 0] = 80.0                                                   # one dominant class: the others underflow towards 0, no NaN
    if R > 2:
        x[2] = -1.0e4
        x[2, -1] = 0.0                                               # everything in the dropped "no object" column
    want = F.softmax(x.double(), -1)[..., :-1]
    got = ops.softmax_drop_last(dev(x))
    assert got.shape == (R, K1 - 1) and got.is_contiguous()
    assert torch.isfinite(got).all()
    assert float((got.double().cpu() - want).abs().max()) < 3e-7
    ref32 = F.softmax(dev(x), -1)[..., :-1]
    assert float((got - ref32).abs().max()) < 3e-7
    assert ops.softmax_drop_last(dev(x).view(1, R, K1)).shape == (1, R, K1 - 1)
    with pytest.raises(Exception):
        ops.softmax_drop_last(dev(torch.zeros(4, 65)))


@pytest.mark.parametrize("H,W,k,sigma", [(1024, 2048, 7, 1.0), (60, 90, 7, 1.0), (33, 70, 5, 0.8), (4, 5, 7, 1.0), (129, 65, 15, 2.5)])
def test_gaussian_blur_vs_oracle(ops, H, W, k, sigma):
    from oracle import ref_ops
    from rba_amd._lib import RbaHipError
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(H, W, generator=g) * 3.0
    out = ops.gaussian_blur(dev(x), k, sigma)
    assert out.shape == (H, W) and maxerr(out, ref_ops.gaussian_blur(x.double(), k, sigma)) < 5e-6
    with pytest.raises(RbaHipError):
        ops.gaussian_blur(dev(x), 6, 1.0)
    with pytest.raises(RbaHipError):
        ops.gaussian_blur(dev(x[:3, :3]), 7, 1.0)                                  # reflect padding needs pad < size


# ----------------------------------------------------------------------------------- open-set panoptic epilogue
@pytest.mark.parametrize("H,W,p,seed", [(64, 96, 0.5, 0), (200, 300, 0.4, 1), (33, 17, 0.7, 2), (512, 1024, 0.45, 3)])
def test_ood_components_vs_oracle(ops, H, W, p, seed):
    """threshold -> 3x3 open -> 3x3 close -> 4-connected components numbered in raster order, against the oracle (and so SciPy)."""
    from scipy import ndimage
    g = np.random.default_rng(seed)
    score = ndimage.gaussian_filter(g.standard_normal((H, W)), 2.0).astype(np.float32) * 5
    thr = float(np.quantile(score, 1 - p))
    labels, n = ops.ood_components(dev(torch.from_numpy(score)), thr)
    box = np.ones((3, 3), bool)
    b = score > thr
    opened = ndimage.binary_dilation(ndimage.binary_erosion(b, box, border_value=1), box, border_value=0)
    closed = ndimage.binary_erosion(ndimage.binary_dilation(opened, box, border_value=0), box, border_value=1)
    want, wn = ndimage.label(closed)
    assert n == wn and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
    if H * W <= 64 * 96:
        from oracle import ref_ops
        lab2, n2 = ref_ops.ood_components(score, thr)
        assert n2 == n and np.array_equal(lab2, want)
    empty, n0 = ops.ood_components(dev(torch.zeros(8, 8)), 1.0)
    assert n0 == 0 and not empty.any()
    full, n1 = ops.ood_components(dev(torch.ones(8, 8)), 0.0)
    assert n1 == 1 and bool((full == 1).all())


def test_k1_dynamic_tiles_match_static_and_workspace_self_resets(ops):
    """rba_reduce_ws_f32 (tiles fetched from an atomic counter) against rba_reduce_f32 (static split): identical bits, the
    workspace is zero again after every launch, and two streams with their own workspaces do not interfere."""
    import ctypes
    from rba_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(11)
    Q, K, H, W = 100, 19, 256, 512
    mask = dev(torch.randn(Q, H, W, generator=g) * 5)
    prob = dev(torch.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :K].contiguous())
    st = torch.cuda.current_stream().cuda_stream
    static = torch.empty(H, W, device="cuda")
    sem_s = torch.empty(K, H, W, device="cuda")
    arg_s = torch.empty(H, W, dtype=torch.int32, device="cuda")
    assert lib.rba_reduce_f32(mask.data_ptr(), prob.data_ptr(), static.data_ptr(), sem_s.data_ptr(), arg_s.data_ptr(), Q, K, H * W, 0, st) == 0
    for _ in range(3):                                                     # the same cached workspace is reused
        rba, sem, arg = ops.rba_reduce(mask, prob, True, True)
        assert torch.equal(rba, static) and torch.equal(sem, sem_s) and torch.equal(arg, arg_s)
        ws = ops._k1_workspace(mask.device)
        torch.cuda.synchronize()
        assert ws.tolist() == [0, 0], "the last workgroup must leave the counters zeroed"
    s2 = torch.cuda.Stream()
    s2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s2):
        r2 = ops.rba_reduce(mask, prob)[0]
    r1 = ops.rba_reduce(mask, prob)[0]
    torch.cuda.synchronize()
    assert torch.equal(r1, static) and torch.equal(r2, static) and len(ops._STREAM_WORKSPACES) >= 2


# ----------------------------------------------------------------------------------- size-independent properties at BASELINE sizes
def test_k1_full_size_properties(ops):
    """K1 at the BASELINE C2 size (100 x 19 x 1024 x 2048) through properties that need no CPU reference of that size:
    linearity of sem in the queries (two halves add up), one-hot class rows select sigmoid sums, saturated masks give closed forms."""
    g = torch.Generator(device="cuda").manual_seed(5)
    Q, K, H, W = 100, 19, 1024, 2048
    mask = torch.randn(Q, H, W, device="cuda", generator=g) * 5
    prob = torch.softmax(torch.randn(Q, K + 1, device="cuda", generator=g) * 3, -1)[:, :K].contiguous()
    rba, sem, arg = ops.rba_reduce(mask, prob, True, True)
    assert torch.equal(arg.long(), sem.argmax(0)) and maxerr(rba, -sem.double().tanh().sum(0)) < 1e-5
    _, s1, _ = ops.rba_reduce(mask[:40].contiguous(), prob[:40].contiguous(), True)
    _, s2, _ = ops.rba_reduce(mask[40:].contiguous(), prob[40:].contiguous(), True)
    assert (s1 + s2 - sem).abs().max().item() < 5e-6                         # same terms, different association
    onehot = torch.zeros(Q, K, device="cuda")
    cls = torch.arange(Q, device="cuda") % K
    onehot[torch.arange(Q), cls] = 1.0
    _, so, _ = ops.rba_reduce(mask, onehot, True)
    rows = torch.tensor([0, 511, 1023], device="cuda")
    want = torch.zeros(K, 3, W, device="cuda", dtype=torch.float64).index_add_(0, cls, mask[:, rows].double().sigmoid())
    assert (so[:, rows].double() - want).abs().max().item() < 1e-5
    sat = torch.full((Q, H, W), -40.0, device="cuda")
    sat[7] = 40.0                                                             # only query 7 is "on": sem = prob[7], everywhere
    r_sat, s_sat, _ = ops.rba_reduce(sat, prob, True)
    assert (s_sat - prob[7].view(K, 1, 1)).abs().max().item() < 1e-6
    assert (r_sat + prob[7].double().tanh().sum()).abs().max().item() < 1e-6


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_split_linear_full_size_properties(ops, mode):
    """K6 at the largest BASELINE GEMM (Swin-B stage 1, M = 131072): exactness on selection weights, additivity in the input,
    and fp64 agreement on sampled rows."""
    g = torch.Generator(device="cuda").manual_seed(6)
    M, N, K = 131072, 512, 128
    x = torch.randn(M, K, device="cuda", generator=g) * torch.logspace(-3, 3, K, device="cuda").view(1, K)
    sel = torch.zeros(N, K, device="cuda")
    sel[torch.arange(N), torch.arange(N) % K] = 1.0
    out = ops.split_linear(x, ops.split_weight(sel, mode=mode))
    want = x[:, torch.arange(N, device="cuda") % K]
    if mode == "bf16x6":
        assert torch.equal(out, want), "hi + mid + lo must reproduce every fp32 input exactly"
    else:
        assert ((out - want).abs() <= 2.0 ** -21 * want.abs() + 2.0 ** -35).all(), "h + 2^-11 l carries 22 bits of every input"
    w = torch.randn(N, K, device="cuda", generator=g) * K ** -0.5
    b = torch.randn(N, device="cuda", generator=g)
    planes = ops.split_weight(w, mode=mode)
    x1, x2 = torch.randn(M, K, device="cuda", generator=g), torch.randn(M, K, device="cuda", generator=g)
    y1, y2, y12 = ops.split_linear(x1, planes, b), ops.split_linear(x2, planes, b), ops.split_linear(x1 + x2, planes, b)
    assert (y1 + y2 - b - y12).abs().max().item() < 2e-5
    rows = torch.randint(0, M, (256,), device="cuda", generator=g)
    assert maxerr(y1[rows], F.linear(x1[rows].double(), w.double(), b.double())) < 1e-5


# ----------------------------------------------------------------------------------- DenseHybrid head kernels
@pytest.mark.parametrize("B,C,O,h,w", [(1, 64, 2, 16, 24), (2, 256, 2, 9, 7), (1, 32, 1, 5, 5), (1, 48, 4, 8, 16)])
def test_bn_relu_conv1x1(ops, B, C, O, h, w):
    """BNReluConv(C, O, k=1) in eval mode (mask2former_transformer_decoder.py:216-230) against torch's batch_norm/relu/conv2d"""
    g = torch.Generator().manual_seed(B * 100 + C)
    x = torch.randn(B, C, h, w, generator=g)
    bw, bb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mean, var = 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    cw, cb = torch.randn(O, C, 1, 1, generator=g) * C ** -0.5, torch.randn(O, generator=g)
    ref = F.conv2d(F.relu(F.batch_norm(x.double(), mean.double(), var.double(), bw.double(), bb.double(), False, 0.0, 1e-5)),
                   cw.double(), cb.double())
    scale = bw * torch.rsqrt(var + 1e-5)
    shift = bb - mean * scale
    out = ops.bn_relu_conv1x1(dev(x), dev(scale), dev(shift), dev(cw.flatten(1).contiguous()), dev(cb))
    assert out.shape == (B, O, h, w) and maxerr(out, ref) < 1e-5


@pytest.mark.parametrize("C,h,w,H,W", [(2, 16, 24, 60, 90), (3, 5, 7, 5, 7), (1, 4, 4, 1, 9), (2, 8, 8, 3, 2)])
def test_resample_bilinear_align_corners(ops, C, h, w, H, W):
    """F.interpolate(mode="bilinear", align_corners=True) (maskformer_model.py:305)"""
    x = torch.randn(C, h, w, generator=torch.Generator().manual_seed(C + h))
    ref = F.interpolate(x[None].double(), size=(H, W), mode="bilinear", align_corners=True)[0]
    out = ops.resample_bilinear_ac(dev(x), (H, W))
    assert out.shape == (C, H, W) and maxerr(out, ref) < 2e-6


# ----------------------------------------------------------------------------------- fused front end (normalise + pad + patch im2col)
@pytest.mark.parametrize("h,w,Hp,Wp,dtype", [(37, 50, 64, 64, torch.uint8), (64, 96, 64, 96, torch.uint8), (5, 9, 32, 32, torch.float32),
                                             (1024, 2048, 1024, 2048, torch.uint8)])
def test_patch_im2col(ops, h, w, Hp, Wp, dtype):
    """(image - mean) / std, zero padding AFTER normalisation (ImageList) and the im2col of the 4x4 / stride-4 convolution, against
    torch's elementwise ops + F.pad + F.unfold: bit-identical."""
    g = torch.Generator().manual_seed(h * w)
    img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    if dtype == torch.float32:
        img = img.float() + torch.rand(3, h, w, generator=g)
    mean, std = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)
    m32 = torch.tensor(mean, dtype=torch.float32).view(3, 1, 1)
    s32 = torch.tensor(std, dtype=torch.float32).view(3, 1, 1)
    ref = F.pad((img.float() - m32) / s32, (0, Wp - w, 0, Hp - h))
    ref = F.unfold(ref[None], kernel_size=4, stride=4)[0].t()                  # [tokens, 48], column c*16 + ky*4 + kx
    out = ops.patch_im2col(dev(img), [float(v) for v in m32.flatten()], [float(v) for v in s32.flatten()], Hp, Wp)
    assert out.shape == ((Hp // 4) * (Wp // 4), 64)
    assert torch.equal(out[:, :48].cpu(), ref) and not out[:, 48:].any()


@pytest.mark.parametrize("B,H,W,C", [(1, 8, 12, 32), (2, 7, 9, 64), (1, 64, 128, 512), (1, 256, 512, 128), (1, 5, 5, 16)])
def test_merge_layer_norm(ops, B, H, W, C):
    """PatchMerging's gather + LayerNorm in one kernel against pad + the four strided slices + cat + F.layer_norm (swin.py:311-337)"""
    g = torch.Generator().manual_seed(B * H * W + C)
    x = torch.randn(B, H * W, C, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(4 * C, generator=g), 0.1 * torch.randn(4 * C, generator=g)
    xv = x.view(B, H, W, C)
    if H % 2 or W % 2:
        xv = F.pad(xv, (0, 0, 0, W % 2, 0, H % 2))
    cat = torch.cat([xv[:, 0::2, 0::2], xv[:, 1::2, 0::2], xv[:, 0::2, 1::2], xv[:, 1::2, 1::2]], -1).reshape(B, -1, 4 * C)
    ref = F.layer_norm(cat.double(), (4 * C,), gamma.double(), beta.double(), 1e-5)
    out = ops.merge_layer_norm(dev(x), H, W, dev(gamma), dev(beta), 1e-5)
    assert out.shape == ref.shape and maxerr(out, ref) < 5e-6
    same = ops.add_layer_norm(dev(cat.contiguous()), dev(gamma), dev(beta), 1e-5)[1]
    assert torch.equal(out, same), "same arithmetic as the LayerNorm kernel on the materialised concatenation"


@pytest.mark.parametrize("N,Lq,M,L,P", [(1, 2048, 8, 1, 4), (2, 300, 8, 3, 4), (1, 7, 2, 2, 3)])
def test_msda_prepare(ops, N, Lq, M, L, P):
    """offsets / logits of the fused sampling Linear -> sampling locations and softmaxed weights, against MSDeformAttn.forward's
    own torch expressions (ms_deform_attn.py:95-115)"""
    g = torch.Generator().manual_seed(N * Lq + M * L * P)
    raw = torch.randn(N, Lq, 3 * M * L * P, generator=g)
    ref_pts = torch.rand(N, Lq, L, 2, generator=g)
    shapes = torch.tensor([[32 >> l, 64 >> l] for l in range(L)], dtype=torch.int64)
    offsets = raw[..., : 2 * M * L * P].reshape(N, Lq, M, L, P, 2)
    weights = F.softmax(raw[..., 2 * M * L * P:].reshape(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    normalizer = torch.stack([shapes[..., 1], shapes[..., 0]], -1).float()
    loc = ref_pts[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
    loc2, w2 = ops.msda_prepare(dev(raw), dev(ref_pts), dev(shapes), M, L, P)
    assert torch.equal(loc2.cpu(), loc)
    assert maxerr(w2, weights) < 2e-7



@pytest.mark.parametrize("N,Lq,L,edge", [(1, 2048, 1, False), (1, 19320, 3, False), (2, 333, 3, True), (1, 77, 1, True)])
def test_msda_fused_equals_prepare_plus_forward(ops, N, Lq, L, edge, knobs):
    """round 3: the one-launch deformable attention core (sampling locations + softmax computed inside the locality-mapped gather kernel)
    is bit-identical to rba_msda_prepare_f32 + the generic rba_ms_deform_attn_fwd_f32 kernel, which the reference-generated K2 fixtures pin;
    `edge`: reference points and offsets that push samples across and beyond the image border (zero taps, skipped samples)"""
    import ctypes
    from rba_amd import _lib
    M, D, P = 8, 32, 4
    g = torch.Generator().manual_seed(N * Lq + L)
    if L == 3:
        hw = [(92, 160), (46, 80), (23, 40)] if Lq == 19320 else [(12, 20), (6, 10), (3, 5)]
    else:
        hw = [(32, 64)] if Lq == 2048 else [(7, 11)]
    shapes = torch.tensor(hw, dtype=torch.int64)
    S = int(shapes.prod(1).sum())
    lsi = torch.cat((shapes.new_zeros((1,)), shapes.prod(1).cumsum(0)[:-1]))
    value = torch.randn(N, S, M, D, generator=g)
    raw = torch.randn(N, Lq, 3 * M * L * P, generator=g) * (6.0 if edge else 1.5)
    ref_pts = torch.rand(N, Lq, L, 2, generator=g) * (1.4 if edge else 1.0) - (0.2 if edge else 0.0)
    loc, w = ops.msda_prepare(dev(raw), dev(ref_pts), dev(shapes), M, L, P)
    fused = ops.msda_fused(dev(value), dev(shapes), dev(lsi), dev(raw), dev(ref_pts), M, L, P)
    two_step = ops.ms_deform_attn_forward(dev(value), dev(shapes), dev(lsi), loc, w)          # round-3 kernel, parameters from memory
    variant = ctypes.c_int.in_dll(_lib.load(), "rba_k2_variant")
    variant.value = 1
    try:
        generic = ops.ms_deform_attn_forward(dev(value), dev(shapes), dev(lsi), loc, w)       # the kernel the K2 fixtures pin
    finally:
        variant.value = 0
    assert torch.equal(fused, two_step) and torch.equal(fused, generic)
    from oracle import ref_ops
    want = ref_ops.ms_deform_attn(value.double(), shapes, loc.cpu().double(), w.cpu().double())
    assert maxerr(fused, want) < 1e-4            # fp32 sample positions (y H - 0.5 at H = 92..160) against the float64 restatement


@pytest.mark.parametrize("h,w,H,W,C,split", [(8, 16, 16, 32, 256, False), (23, 40, 46, 80, 128, False), (64, 128, 128, 256, 256, True), (7, 9, 14, 18, 128, True)])
def test_resample_nhwc_with_folded_group_norms(ops, h, w, H, W, C, split):
    """round 3: the FPN top-down step with GroupNorm(lateral) and ReLU(GroupNorm(previous conv)) folded into the resample kernel's loads agrees with
    group_norm_nhwc + resample_bilinear_nhwc to an ulp (fp32 rows and the split image), and the statistics entry returns what the
    full GroupNorm uses"""
    g = torch.Generator().manual_seed(h * w + C)
    x = dev(torch.randn(1, h * w, C, generator=g) * 2 + 0.5)
    add = dev(torch.randn(1, H * W, C, generator=g))
    gx, bx, ga, ba = (dev(torch.randn(C, generator=g)) for _ in range(4))
    xn = ops.group_norm_nhwc(x, 32, gx, bx, 1e-5, relu=True)
    an = ops.group_norm_nhwc(add, 32, ga, ba, 1e-5)
    mx, ma = ops.group_norm_nhwc_stats(x, 32, 1e-5), ops.group_norm_nhwc_stats(add, 32, 1e-5)
    xd = x[0].double().view(h * w, 32, C // 32)
    assert maxerr(mx[0, :, 0], xd.mean((0, 2))) < 1e-5
    assert maxerr(mx[0, :, 1], (xd.var((0, 2), unbiased=False) + 1e-5).rsqrt()) < 1e-4
    want = ops.resample_bilinear_nhwc(xn[0].view(h, w, C), (H, W), add=an[0].view(H, W, C))
    got = ops.resample_bilinear_nhwc_gn(x[0].view(h, w, C), (H, W), add[0].view(H, W, C), 32, x_norm=(mx[0], gx, bx, True), add_norm=(ma[0], ga, ba))
    # the same operations per element; the compiler is free to contract a different multiply of `l0 v00 + l1 v01` into the fma in the
    # two instantiations, so the results agree to an ulp of the interpolated value rather than bit for bit
    tol = 4e-7 * float(want.abs().max())
    assert maxerr(got, want.double()) <= tol
    half = ops.resample_bilinear_nhwc_gn(xn[0].view(h, w, C), (H, W), add[0].view(H, W, C), 32, x_norm=None, add_norm=(ma[0], ga, ba))
    assert maxerr(half, want.double()) <= tol
    if split:
        s_want = ops.SplitActivations.empty((1, H, W, C), x.device)
        s_got = ops.SplitActivations.empty((1, H, W, C), x.device)
        s_want.data.zero_(); s_got.data.zero_()
        ops.resample_bilinear_nhwc(xn[0].view(h, w, C), (H, W), add=an[0].view(H, W, C), split_into=s_want)
        ops.resample_bilinear_nhwc_gn(x[0].view(h, w, C), (H, W), add[0].view(H, W, C), 32, x_norm=(mx[0], gx, bx, True), add_norm=(ma[0], ga, ba),
                                      split_into=s_got)
        assert maxerr(s_got.unpack(), s_want.unpack().double()) <= 2 * tol
