"""GPU: operands off the allocator's alignment.

`_chk` demands contiguity, not alignment, so a contiguous view 4 bytes off a 16-byte boundary is a legal argument; the entry points refuse it, dispatch on it
to a scalar form, or only ever take element accesses -- docs/kernels/placement.md classifies every pointer argument of the entry points covered here, from the
code, and the outcomes below are read off that table.  Every alignment-dispatched fallback is otherwise reached through odd shapes only: here the shape is the
smallest at which the ALIGNED call takes the wide or matrix-pipe form (the dispatch line is cited per case), so that the pointer is the only reason to fall back.

Per case: each tensor argument alone is moved (tests/_placement.py: values kept, surroundings poisoned with 0xFF = NaN / 255 / -1), by every shift of its
dtype, then all arguments together.  "refuses": RbaHipError and every guard byte untouched.  "serves": the result meets the reference and the bar of the
wrapper's own value test (named per case, restated here, not widened), and the guard bytes around the moved operand are untouched; the outputs a wrapper
allocates carry the guard bands of tests/_guard.py (the `canary` fixture of conftest.py).  Byte results (resize_u8_pil_bilinear) must equal the aligned call.
argmax maps are compared with the fp64 reference where its top-two gap exceeds the sem_seg bar; at most 1 % of the pixels may be left out, which the
reference alone is checked for.
"""
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_ops
from tests import _ops_surface
from tests import _placement
from tests._placement import ARGMAX_LEFT_OUT_CAP, SHIFTS, place

pytestmark = pytest.mark.gpu

SERVES, REFUSES = "serves", "refuses"


def dev(t):
    return t.cuda().contiguous()


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def _get(kwargs, path):
    """'views[1]' or 'x' -> the tensor"""
    if "[" in path:
        name, i = path[:-1].split("[")
        return kwargs[name][int(i)]
    return kwargs[path]


def _with(kwargs, path, t):
    out = dict(kwargs)
    if "[" in path:
        name, i = path[:-1].split("[")
        seq = list(out[name])
        seq[int(i)] = t
        out[name] = seq
    else:
        out[path] = t
    return out


class Case:
    """fn(**kwargs) with `operands` = {argument path: SERVES | REFUSES} (docs/kernels/placement.md), `verify(result)` asserting the value test's bar"""

    def __init__(self, name, fn, kwargs, operands, verify, bitwise=False, owned=None, reset=None):
        self.name, self.fn, self.kwargs, self.operands, self.verify = name, fn, kwargs, operands, verify
        self.reset = reset                          # reset(kwargs) in front of every call: an operand that the wrapper writes in place gets its values back
        # the caller-owned outputs (argument paths): a refused call must leave every one of them as it was
        self.owned = tuple(owned) if owned is not None else tuple(k for k in ("out",) if k in kwargs)
        self.bitwise = bitwise                      # the docstring calls the results bitwise reproducible: two launches at one placement give equal bits


def _argmax_checker(sem64, bar, name):
    """argmax against the fp64 class map where its top-two gap exceeds `bar`; the share left out is the reference's own property"""
    decided, left_out = _placement.decided_pixels(sem64, bar)
    print(f"[placement] {name}: argmax compared at {100 * (1 - left_out):.2f} % of the pixels, {100 * left_out:.2f} % left out (cap 1 %)")
    assert left_out <= ARGMAX_LEFT_OUT_CAP, f"{name}: choose another seed, {left_out:.3%} of the reference's pixels are near-ties"
    want = sem64.argmax(0)

    def check(arg):
        assert arg.dtype == torch.int32
        assert bool((arg.cpu().long() == want)[decided].all())
    return check


# ---------------------------------------------------------------------------------------------------------------- the cases
def _k1(ops, name):
    """rba_reduce.hip:38 `vec4 = HW % 4 == 0 && ((mask | rba | sem_seg) & 15) == 0`: HW = 64 takes launch_reduce<32, 4> (K = 3) or, with K = 19, the
    dynamic-tile launch_reduce_pk on the `_ws` counter; a moved mask_pred falls to launch_reduce<32, 1>.  cls_prob: element reads (rba_reduce_kernels.h:149).
    Bars: test_kernels_gpu.py::test_k1_shapes (sem_seg 5e-6, rba 2e-5 against the ordered restatement)."""
    mp, prob = _placement.k1_inputs(name)                # seeds checked on the CPU: test_ops_surface_cpu.py
    sem_r, rba_r, _ = ref_ops.rba_reduce_ordered(mp, prob)
    sem64, _, _ = ref_ops.rba_reduce_ordered(mp.double(), prob.double())
    arg_ok = _argmax_checker(sem64, _placement.K1_SEM_SEG_BAR, name)

    def verify(out):
        rba, sem, arg = out
        assert maxerr(sem, sem_r) < 5e-6 and maxerr(rba, rba_r) < 2e-5
        arg_ok(arg)
    return Case(name, ops.rba_reduce, dict(mask_pred=dev(mp), cls_prob=dev(prob), want_sem_seg=True, want_argmax=True),
                {"mask_pred": SERVES, "cls_prob": SERVES}, verify)


def _resample(ops):
    """resample.hip:180 `vec4 = W % 4 == 0 && ((out | add) & 15) == 0`; x: element reads (resample.hip:29-36).  Bar: test_resample (2e-6)."""
    g = torch.Generator().manual_seed(3)
    x, add = torch.randn(3, 4, 6, generator=g), torch.randn(3, 8, 12, generator=g)
    ref = ref_ops.upsample_bilinear(x[None], (8, 12))[0] + add

    def verify(out):
        assert maxerr(out, ref) < 2e-6
    return Case("resample_bilinear", ops.resample_bilinear, dict(x=dev(x), size=(8, 12), add=dev(add)), {"x": SERVES, "add": SERVES}, verify)


def _resample_ac(ops):
    """dense_hybrid.hip:60-75: element reads only.  Bar: test_resample_bilinear_align_corners (2e-6)."""
    x = torch.randn(2, 4, 4, generator=torch.Generator().manual_seed(5))
    ref = F.interpolate(x[None].double(), size=(8, 8), mode="bilinear", align_corners=True)[0]

    def verify(out):
        assert maxerr(out, ref) < 2e-6
    return Case("resample_bilinear_ac", ops.resample_bilinear_ac, dict(x=dev(x), size=(8, 8)), {"x": SERVES}, verify)


def _group_norm(ops):
    """group_norm.hip:28 (statistics: gsize % 4 == 0 && (p & 15) == 0) and :80 (apply: HW % 4 == 0 && ((p | q) & 15) == 0), decided per group inside the
    kernels; weight / bias: element reads (:83, :92).  HW = 16, gsize = 64.  Bar: test_group_norm (2e-5)."""
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 8, 4, 4, generator=g) * 3 + 1.5
    wt, bs = torch.randn(8, generator=g), torch.randn(8, generator=g)
    ref = F.relu(F.group_norm(x.double(), 2, wt.double(), bs.double(), 1e-5))

    def verify(out):
        assert maxerr(out, ref) < 2e-5
    return Case("group_norm", ops.group_norm, dict(x=dev(x), num_groups=2, weight=dev(wt), bias=dev(bs), eps=1e-5, relu=True),
                {"x": SERVES, "weight": SERVES, "bias": SERVES}, verify)


def _bn_relu_conv1x1(ops, h, w):
    """dense_hybrid.hip:85 `RBA_CHECK_ARG(P % 4 != 0 || ((x | out) & 15) == 0)`: with P % 4 == 0 the kernel reads x in 16-byte pieces (:31) and a moved x is
    refused; with P % 4 != 0 it takes the element form (:35).  scale / shift / weight / bias: element reads.  Bar: test_bn_relu_conv1x1 (1e-5)."""
    B, C, O = 2, 8, 2
    g = torch.Generator().manual_seed(B * 100 + C + h)
    x = torch.randn(B, C, h, w, generator=g)
    bw, bb = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    mean, var = 0.2 * torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
    cw, cb = torch.randn(O, C, 1, 1, generator=g) * C ** -0.5, torch.randn(O, generator=g)
    ref = F.conv2d(F.relu(F.batch_norm(x.double(), mean.double(), var.double(), bw.double(), bb.double(), False, 0.0, 1e-5)), cw.double(), cb.double())
    scale = bw * torch.rsqrt(var + 1e-5)
    shift = bb - mean * scale

    def verify(out):
        assert maxerr(out, ref) < 1e-5
    wide = (h * w) % 4 == 0
    return Case(f"bn_relu_conv1x1[P={h * w}]", ops.bn_relu_conv1x1,
                dict(x=dev(x), scale=dev(scale), shift=dev(shift), weight=dev(cw.flatten(1).contiguous()), bias=dev(cb)),
                {"x": REFUSES if wide else SERVES, "scale": SERVES, "shift": SERVES, "weight": SERVES, "bias": SERVES}, verify)


def _mask_logits(ops, mode, C):
    """mask_logits.hip:359 (exact fp32: Q <= 112, C % 4 == 0, N % 4 == 0 and (feat | out | embed) & 15 == 0 -> the MFMA kernel, else :364 the 8-byte or
    scalar kernel) and :380 (f16x3: C % 32 == 0 and the same alignment, else the exact-fp32 entry).  Bar: test_k4_mask_logits."""
    g = torch.Generator().manual_seed(4 + C)
    e, f = torch.randn(2, 4, C, generator=g), torch.randn(2, C, 4, 4, generator=g)
    ref = torch.einsum("bqc,bchw->bqhw", e.double(), f.double())

    def verify(out):
        assert maxerr(out, ref) < 2e-4 * (C / 256) ** 0.5 + 1e-5
    return Case(f"mask_logits[{mode}]", ops.mask_logits, dict(embed=dev(e), feat=dev(f), mode=mode), {"embed": SERVES, "feat": SERVES}, verify)


def _k4_backward(ops):
    """mask_logits_bwd.hip:276 `g16 = N % 4 == 0 && (grad_out & 15) == 0`, :280 (`feat & 15`, the matrix-pipe grad_embed kernel's 16-byte reads :72, :77)
    and :295 (grad_feat, wrapper-owned; 16-byte reads of grad_out :194); embed: element reads (:187, :241).  N = 16.  Truth, metric and bar:
    tests/_k4_bwd_cases.py as test_mask_logits_backward_gpu.py::test_kernel_meets_the_bar uses them (fp64 autograd, e <= 4 max(b, 2^-20))."""
    from tests import _k4_bwd_cases as C
    gen = torch.Generator().manual_seed(4100)
    B, Q, Cd, N = 2, 5, 8, 16
    G = torch.randn(B, Q, N, generator=gen) * torch.rand(B, Q, 1, generator=gen) * 1e-3          # the recipe of C.case_inputs
    Fm = 0.25 * torch.randn(B, Cd, N, generator=gen)
    Fm[:, 0] = 1.0
    E = torch.randn(B, Q, Cd, generator=gen)
    ge64, gf64 = C._autograd(E.double(), Fm.double(), G.double())
    ge32, gf32 = C._autograd(E, Fm, G)
    b_embed, b_feat = C.err(ge32, ge64), C.err(gf32, gf64)

    def verify(out):
        ge, gf = out
        C.check("placement grad_embed", ge.cpu(), ge64, b_embed)
        C.check("placement grad_feat", gf.cpu(), gf64, b_feat)
    return Case("mask_logits_backward", ops.mask_logits_backward, dict(embed=dev(E), feat=dev(Fm), grad_out=dev(G)),
                {"embed": SERVES, "feat": SERVES, "grad_out": SERVES}, verify, bitwise=True)


def _msda_inputs(L, seed):
    M, D, P, N = 2, 32, 4, 2
    hw = [(4, 6), (2, 3), (1, 2)][:L]
    g = torch.Generator().manual_seed(seed)
    sh = torch.tensor(hw, dtype=torch.int64)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    S = int(sh.prod(1).sum())
    return g, N, S, M, D, L, P, sh, lsi


def _k2(ops, L):
    """ms_deform_attn.hip:281 `vec4 = D % 4 == 0 && ((value | out) & 15) == 0` and :282 (D == 32 and (sampling_loc | attn_weight) & 15 == 0 -> the
    locality-mapped kernel with its 8-byte location reads, :152).  spatial_shapes / level_start_index: element reads.  Bar: test_k2_shapes (1e-5)."""
    g, N, S, M, D, L, P, sh, lsi = _msda_inputs(L, 10 + L)
    Lq = 9
    value = torch.randn(N, S, M, D, generator=g)
    loc = torch.rand(N, Lq, M, L, P, 2, generator=g) * 1.4 - 0.2
    w = F.softmax(torch.randn(N, Lq, M, L * P, generator=g), -1).view(N, Lq, M, L, P)
    ref = ref_ops.ms_deform_attn(value, sh, loc, w)

    def verify(out):
        assert maxerr(out, ref) < 1e-5
    return Case(f"ms_deform_attn_forward[L={L}]", ops.ms_deform_attn_forward,
                dict(value=dev(value), spatial_shapes=dev(sh), level_start_index=dev(lsi), sampling_locations=dev(loc), attention_weights=dev(w)),
                {"value": SERVES, "spatial_shapes": SERVES, "level_start_index": SERVES, "sampling_locations": SERVES, "attention_weights": SERVES}, verify)


def _msda_fused(ops, L):
    """ms_deform_attn.hip:326 `RBA_CHECK_ARG(((value | out | raw) & 15) == 0)`; reference_points, spatial_shapes, level_start_index: element reads
    (:140-141, :163, :171).  Reference and bar: test_msda_fused_equals_prepare_plus_forward (the float64 restatement on the prepared locations, 1e-4)."""
    g, N, S, M, D, L, P, sh, lsi = _msda_inputs(L, 20 + L)
    Lq = 9
    value = torch.randn(N, S, M, D, generator=g)
    raw = torch.randn(N, Lq, 3 * M * L * P, generator=g) * 1.5
    ref_pts = torch.rand(N, Lq, L, 2, generator=g)
    loc, w = ops.msda_prepare(dev(raw), dev(ref_pts), dev(sh), M, L, P)
    want = ref_ops.ms_deform_attn(value.double(), sh, loc.cpu().double(), w.cpu().double())

    def verify(out):
        assert maxerr(out, want) < 1e-4
    return Case(f"msda_fused[L={L}]", ops.msda_fused,
                dict(value=dev(value), spatial_shapes=dev(sh), level_start_index=dev(lsi), raw=dev(raw), reference_points=dev(ref_pts), M=M, L=L, P=P),
                {"value": REFUSES, "raw": REFUSES, "spatial_shapes": SERVES, "level_start_index": SERVES, "reference_points": SERVES}, verify)


def _resize_u8(ops, size, flip):
    """resize_u8.hip:127 `aligned(a, b) = W % 4 == 0 && ((a | b) & 3) == 0`: the horizontal pass reads bytes (:50); the vertical pass reads the image in
    dwords when it is the first pass (:74, :142).  (8, 8) -> (12, 8): vertical alone, (8, 12): horizontal alone, (12, 12): both.  The result equals the
    aligned call in every byte (which test_resize_u8_gpu.py holds against Pillow)."""
    image = torch.randint(0, 256, (3, 8, 8), generator=torch.Generator().manual_seed(size[0] * 16 + size[1]), dtype=torch.uint8)
    want = ops.resize_u8_pil_bilinear(dev(image), size, flip=flip).cpu()

    def verify(out):
        assert out.dtype == torch.uint8 and torch.equal(out.cpu(), want)
    return Case(f"resize_u8_pil_bilinear[{size[0]}x{size[1]}{' flip' if flip else ''}]", ops.resize_u8_pil_bilinear,
                dict(image=dev(image), size=size, flip=flip), {"image": SERVES}, verify)


def _tta_merge(ops):
    """tta_merge.hip:134 asks 4-byte alignment of a view and the kernel reads it by elements (:57-58); the case "wide" of tests/_tta_cases.py has W % 4 == 0
    and a flipped view, so the aligned call and the moved one both take the 16-byte stores (:88) of the outputs the wrapper allocates (:129).  Reference and
    bars: test_tta_merge_gpu.py::test_kernel_against_fp64 (G.check against the fp64 restatement; argmax where G.merge_truth calls the pixel decided, whose
    share it asserts to be at least 99 %)."""
    from tests import _tta_cases as G
    name = "wide"
    K, size, spec = G.MERGE_CASES[name]
    t = G.merge_truth(name)
    print(f"[placement] tta_merge: argmax compared at {100 * t['decided'].double().mean().item():.2f} % of the pixels (cap: 1 % left out)")

    def verify(out):
        score, sem, arg = out
        G.check(f"{name} sem_seg", sem.cpu(), t["sem64"], t["b_sem"])
        G.check(f"{name} score (rba)", score.cpu(), t["score64"]["rba"], t["b_score"]["rba"])
        assert arg.dtype == torch.int32 and not ((arg.cpu().long() != t["argmax64"]) & t["decided"]).any()
    return Case("tta_merge", ops.tta_merge, dict(views=[v.cuda() for v in G.merge_inputs(name)], flips=[bool(f) for _, _, f in spec], size=size,
                                                 want_sem_seg=True, want_argmax=True, score="rba"),
                {"views[0]": SERVES, "views[1]": SERVES}, verify)


def _k3(ops, split, S=160):
    """masked_xattn.hip:319 `RBA_CHECK_ARG(((k | v) & 15) == 0)` (16-byte reads :61, :78, :177-178); :323: the matrix-pipe path (split_keys, a workspace)
    needs a 16-byte aligned q (16-byte read :156), a moved q declines it for the plain kernel's element reads (:48-50); mask_logits: element reads in the
    plain kernel (:39, :60) and the row flags (:129), and in the matrix-pipe kernel 16-byte reads (:211) only where `vec_mask` (:164: S % 4 == 0 and a
    16-byte aligned mask) holds.  S = 160: S % 4 == 0, two key chunks of 144, the path forced with split_keys; S = 1024 with split_keys=None: the size from
    which the wrapper itself takes the matrix-pipe path, several key ranges.  Reference and bar: test_k3_masked_xattn (5e-6)."""
    B, Q, nH = 1, 5, 2
    g = torch.Generator().manual_seed(Q + S)
    q, k, v = (torch.randn(B, n, nH, 32, generator=g) for n in (Q, S, S))
    ml = torch.randn(B, Q, S, generator=g) * 3
    ml[:, 0] = -5.0                                # a fully blocked row attends everywhere
    ml[:, 1] = 5.0
    ml[:, 2, : S - 10] = -5.0                      # everything but the last chunk's tail blocked
    ref = ref_ops.attention_core(q, k, v, ref_ops.attn_mask_from_logits(ml.clone()))

    def verify(out):
        assert maxerr(out, ref) < 5e-6
    return Case(f"masked_xattn[{'auto' if split is None else 'split' if split else 'plain'} S={S}]", ops.masked_xattn, dict(q=dev(q), k=dev(k), v=dev(v), mask_logits=dev(ml), split_keys=split),
                {"q": SERVES, "k": REFUSES, "v": REFUSES, "mask_logits": SERVES}, verify)


def _k1_backward(ops):
    """rba_reduce_bwd.hip: every global access of mask, cls_prob and grad_score is one element wide (the only 16-byte accesses, :153-154, are of LDS).
    The case "odd" of tests/_rba_bwd_cases.py; truth, metric and bar as test_rba_backward_gpu.py::test_kernel_meets_the_bar."""
    from tests import _rba_bwd_cases as C
    mask, prob, g = C.case_inputs("odd")
    gm64, gp64, b_mask, b_prob = C.case_truth("odd", "rba")
    Q, N = mask.shape

    def verify(out):
        gm, gp = out
        C.check("placement grad_mask", gm.cpu().view(Q, N), gm64, b_mask)
        C.check("placement grad_prob", gp.cpu(), gp64, b_prob)
    return Case("rba_reduce_backward", ops.rba_reduce_backward, dict(mask_pred=dev(mask.view(Q, 10, N // 10)), cls_prob=dev(prob), grad_score=dev(g.view(10, N // 10)),
                                                                  score="rba"),
                {"mask_pred": SERVES, "cls_prob": SERVES, "grad_score": SERVES}, verify, bitwise=True)


def _quad_mean(ops):
    """decoder_small.hip: element accesses only.  test_quad_mean_is_the_centre_sample_bit_for_bit: the bits of the torch expression."""
    v = dev(torch.randn(2, 3, 4, 9, generator=torch.Generator().manual_seed(12)) * 7)
    want = ((v[:, :, 0] + v[:, :, 1]) + (v[:, :, 2] + v[:, :, 3])) * 0.25

    def verify(out):
        assert torch.equal(out, want)
    return Case("quad_mean", ops.quad_mean, dict(v=v), {"v": SERVES}, verify)


def _softmax_drop_last(ops):
    """decoder_small.hip: element accesses only.  Bar: test_softmax_drop_last_vs_torch (3e-7 against fp64)."""
    x = torch.randn(9, 5, generator=torch.Generator().manual_seed(14)) * 6
    x[0, 0] = 80.0
    want = F.softmax(x.double(), -1)[..., :-1]

    def verify(out):
        assert torch.isfinite(out).all() and maxerr(out, want) < 3e-7
    return Case("softmax_drop_last", ops.softmax_drop_last, dict(logits=dev(x)), {"logits": SERVES}, verify)


def _gaussian_blur(ops):
    """gaussian_blur.hip / gaussian_blur.h: element accesses only.  Bar: test_gaussian_blur_vs_oracle (5e-6)."""
    x = torch.randn(8, 9, generator=torch.Generator().manual_seed(17)) * 3.0
    want = ref_ops.gaussian_blur(x.double(), 7, 1.0)

    def verify(out):
        assert maxerr(out, want) < 5e-6
    return Case("gaussian_blur", ops.gaussian_blur, dict(score=dev(x), kernel_size=7, sigma=1.0), {"score": SERVES}, verify)


def _blur_planes(ops, adjoint):
    """pebal_loss.hip / gaussian_blur.h: element accesses only.  Truth and bar: tests/_pebal_cases.py as test_gaussian_blur_planes_gpu.py uses them."""
    from tests import _pebal_cases as G
    from tests import _rba_bwd_cases as C
    shape = (2, 5, 9)
    u, v = G.blur_inputs(shape)
    t = G.blur_truth(shape)
    if adjoint:
        def verify(out):
            C.check("placement A^T v", out.cpu(), t["g64"], t["b_g"])
        return Case("gaussian_blur_planes_adjoint", ops.gaussian_blur_planes_adjoint, dict(grad_out=dev(v)), {"grad_out": SERVES}, verify, bitwise=True)

    def verify(out):
        C.check("placement A u", out.cpu(), t["y64"], t["b_y"])
    return Case("gaussian_blur_planes", ops.gaussian_blur_planes, dict(planes=dev(u)), {"planes": SERVES}, verify)


def _patch_im2col(ops, dtype):
    """patch_embed.hip:26-29: the image is read by elements (bytes or floats); the 16-byte stores (:32) are of the output the wrapper allocates (:51).
    test_patch_im2col: the bits of torch's elementwise ops + F.pad + F.unfold."""
    h, w, Hp, Wp = 5, 9, 8, 12
    g = torch.Generator().manual_seed(h * w)
    img = torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8)
    if dtype == torch.float32:
        img = img.float() + torch.rand(3, h, w, generator=g)
    m32 = torch.tensor((123.675, 116.28, 103.53), dtype=torch.float32).view(3, 1, 1)
    s32 = torch.tensor((58.395, 57.12, 57.375), dtype=torch.float32).view(3, 1, 1)
    ref = F.unfold(F.pad((img.float() - m32) / s32, (0, Wp - w, 0, Hp - h))[None], kernel_size=4, stride=4)[0].t()

    def verify(out):
        assert torch.equal(out[:, :48].cpu(), ref) and not out[:, 48:].any()
    return Case(f"patch_im2col[{'u8' if dtype == torch.uint8 else 'f32'}]", ops.patch_im2col,
                dict(image=dev(img), mean=[float(x) for x in m32.flatten()], std=[float(x) for x in s32.flatten()], Hp=Hp, Wp=Wp), {"image": SERVES}, verify)


def _ood_components(ops):
    """open_panoptic.hip: element accesses only (the byte maps in between are the wrapper's).  test_ood_components_vs_oracle: equal to SciPy's labels."""
    import numpy as np
    from scipy import ndimage
    H, W, p = 33, 17, 0.7
    score = ndimage.gaussian_filter(np.random.default_rng(2).standard_normal((H, W)), 2.0).astype(np.float32) * 5
    thr = float(np.quantile(score, 1 - p))
    box = np.ones((3, 3), bool)
    opened = ndimage.binary_dilation(ndimage.binary_erosion(score > thr, box, border_value=1), box, border_value=0)
    closed = ndimage.binary_erosion(ndimage.binary_dilation(opened, box, border_value=0), box, border_value=1)
    want, wn = ndimage.label(closed)

    def verify(out):
        labels, n = out
        assert n == wn and labels.dtype == torch.int32 and np.array_equal(labels.cpu().numpy(), want)
    return Case("ood_components", ops.ood_components, dict(score=dev(torch.from_numpy(score)), threshold=thr), {"score": SERVES}, verify)


def _score_reg(ops, backward):
    """pebal_loss.hip with bilinear_ac.h and loss_reduce.h: no wide access of global memory; a label is read as one byte or one int64 (bilinear_ac.h:82-84).
    The first shape of tests/_pebal_cases.py; truth and bars as test_score_reg_gpu.py::test_kernel_against_fp64."""
    from tests import _pebal_cases as G
    from tests import _point_loss_cases as P
    from tests import _rba_bwd_cases as C
    shape = G.REG_SHAPES[0]
    score, labels = G.reg_inputs(shape)
    t = G.reg_truth(shape)
    sd, ld = dev(score), dev(labels)
    if not backward:
        def verify(out):
            losses, stats = out
            P.check_scalar("smoothness", losses[0], t["sm32"], t["sm64"])
            P.check_scalar("sparsity", losses[1], t["sp32"], t["sp64"])
            P.check_scalar("sum of squared differences", stats[0], 2 * t["sm32"], 2 * t["sm64"])
            P.check_scalar("sum of squared samples", stats[1], t["sp32"] ** 2, t["sp64"] ** 2)
        return Case("score_reg", ops.score_reg, dict(score=sd, labels=ld), {"score": SERVES, "labels": SERVES}, verify, bitwise=True)
    up = G.REG_UPSTREAM[2]
    stats = ops.score_reg(sd, ld)[1]

    def verify(out):
        C.check("placement grad_score", out.cpu(), t["g64"][up], t["b"][up])
    return Case("score_reg_backward", ops.score_reg_backward,
                dict(score=sd, labels=ld, stats=stats, grad_smoothness=torch.full((1,), up[0], device="cuda"), grad_sparsity=torch.full((1,), up[1], device="cuda")),
                {"score": SERVES, "labels": SERVES, "stats": SERVES, "grad_smoothness": SERVES, "grad_sparsity": SERVES}, verify, bitwise=True)


def _refusing(name, fn, kwargs, operands, shape, cite, owned=None, reset=None):
    """a wrapper whose entry point lists every caller's pointer in one RBA_CHECK_ARG (`cite`): the refusal is the whole test; the aligned call is only
    asked for its shape"""
    def verify(out):
        out = out[-1] if isinstance(out, tuple) else out
        assert tuple(out.shape) == shape and bool(torch.isfinite(out).all())
    case = Case(name, fn, kwargs, {k: REFUSES for k in operands}, verify, owned=owned, reset=reset)
    case.cite = cite
    return case


def _add_layer_norm(ops):
    g = torch.Generator().manual_seed(31)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    return _refusing("add_layer_norm", ops.add_layer_norm, dict(x=r(8, 32), weight=r(32), bias=r(32), residual=r(8, 32), residual_bias=r(32)),
                     ("x", "weight", "bias", "residual", "residual_bias"), (8, 32), "layer_norm.hip:212-213")


def _merge_layer_norm(ops):
    g = torch.Generator().manual_seed(32)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    return _refusing("merge_layer_norm", ops.merge_layer_norm, dict(x=r(1, 6, 8), H=2, W=3, weight=r(32), bias=r(32)), ("x", "weight", "bias"), (1, 2, 32),
                     "layer_norm.hip:189")


def _group_norm_nhwc(ops, stats):
    g = torch.Generator().manual_seed(33)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    if stats:
        return _refusing("group_norm_nhwc_stats", ops.group_norm_nhwc_stats, dict(x=r(1, 6, 16), num_groups=4), ("x",), (1, 4, 2), "group_norm.hip:240")
    return _refusing("group_norm_nhwc", ops.group_norm_nhwc, dict(x=r(1, 6, 16), num_groups=4, weight=r(16), bias=r(16)), ("x", "weight", "bias"), (1, 6, 16),
                     "group_norm.hip:218")


def _resample_nhwc(ops):
    g = torch.Generator().manual_seed(34)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    return _refusing("resample_bilinear_nhwc", ops.resample_bilinear_nhwc, dict(x=r(2, 3, 8), size=(4, 6), add=r(4, 6, 8)), ("x", "add"), (4, 6, 8),
                     "resample.hip:194")


def _token_linear(ops):
    """token_linear.hip:317: x, x_add, bias (and packed, out: the wrapper's) must be 16-byte aligned.  The Linear is a namespace, so that its bias can move."""
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(35)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    w = r(16, 32)

    def call(x, x_add, bias):
        return ops.token_linear(x, SimpleNamespace(weight=w, bias=bias), x_add=x_add)
    return _refusing("token_linear", call, dict(x=r(8, 32), x_add=r(8, 32), bias=r(16)), ("x", "x_add", "bias"), (8, 16), "token_linear.hip:317")


def _token_linear_norm(ops):
    """token_linear.hip:319: with the post-norm residual step, residual and the LayerNorm's weight and bias are in the refusal too"""
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(36)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    w, b = r(16, 32), r(16)

    def call(x, residual, ln_weight, ln_bias):
        return ops.token_linear(x, SimpleNamespace(weight=w, bias=b), residual=residual, norm=SimpleNamespace(weight=ln_weight, bias=ln_bias, eps=1e-5))
    return _refusing("token_linear[norm]", call, dict(x=r(8, 32), residual=r(8, 16), ln_weight=r(16), ln_bias=r(16)), ("x", "residual", "ln_weight", "ln_bias"),
                     (8, 16), "token_linear.hip:319")


def _token_linear_multi(ops):
    """token_linear.hip:330 (x) and :335 (every problem's x_add, packed, bias, out): all refused; `out` is the caller's, filled with a sentinel that a
    refused call must leave"""
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(37)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    w = r(16, 32)

    def call(x, x_add, bias, out):
        return ops.token_linear_multi(x, [(SimpleNamespace(weight=w, bias=bias), x_add, out, 0, False)])[0]
    return _refusing("token_linear_multi", call, dict(x=r(8, 32), x_add=r(8, 32), bias=r(16), out=torch.full((8, 16), -7.0, device="cuda")),
                     ("x", "x_add", "bias", "out"), (8, 16), "token_linear.hip:330, :335")


def _k3_backward(ops):
    """masked_xattn_bwd.hip:397 `RBA_CHECK_ARG(((k | v | grad_k | grad_v | workspace) & 15) == 0)` (16-byte reads of k and v :75-76, :117-119, :192-193,
    :261-262, :316-317); q, mask_logits and grad_out are read by elements (no wide access of them in the file).  Reference: fp64 autograd of
    ref_ops.attention_core as test_masked_xattn_backward_gpu.py holds it; bar e <= 4 max(b, 2^-20) of tests/_rba_bwd_cases.py."""
    from tests import _rba_bwd_cases as C
    B, Q, S, nH = 1, 5, 40, 2
    g = torch.Generator().manual_seed(41)
    q, k, v = (torch.randn(B, n, nH, 32, generator=g) for n in (Q, S, S))
    ml = torch.randn(B, Q, S, generator=g) * 3
    ml[:, 0] = -5.0
    go = torch.randn(B, Q, nH * 32, generator=g)
    blocked = ref_ops.attn_mask_from_logits(ml.clone())

    def grads(dtype):
        a = [t.to(dtype).clone().requires_grad_(True) for t in (q, k, v)]
        (ref_ops.attention_core(a[0], a[1], a[2], blocked) * go.to(dtype)).sum().backward()
        return [t.grad for t in a]
    g64, g32 = grads(torch.float64), grads(torch.float32)
    b = [C.err(x, y) for x, y in zip(g32, g64)]

    def verify(out):
        for name, t, t64, bb in zip(("grad_q", "grad_k", "grad_v"), out, g64, b):
            C.check(f"placement {name}", t.cpu(), t64, bb)
    return Case("masked_xattn_backward", ops.masked_xattn_backward, dict(q=dev(q), k=dev(k), v=dev(v), mask_logits=dev(ml), grad_out=dev(go)),
                {"q": SERVES, "k": REFUSES, "v": REFUSES, "mask_logits": SERVES, "grad_out": SERVES}, verify, bitwise=True)


def _sem_seg_backward(ops):
    """rba_reduce_bwd.hip (the kernel of K1 backward with the per-class gradient loaded): element accesses of global memory only.  The case "odd";
    truth and bar as test_sem_seg_backward_gpu.py::test_kernel_against_fp64."""
    from tests import _rba_bwd_cases as C
    from tests import test_sem_seg_backward_gpu as T
    mask, prob, gsem = T.inputs("odd")
    gm64, gp64, b_mask, b_prob = T.truth("odd")
    Q, N = mask.shape

    def verify(out):
        gm, gp = out
        C.check("placement grad_mask", gm.cpu().view(Q, N), gm64, b_mask)
        C.check("placement grad_prob", gp.cpu(), gp64, b_prob)
    return Case("sem_seg_backward", ops.sem_seg_backward, dict(mask_pred=dev(mask.view(Q, 10, N // 10)), cls_prob=dev(prob), grad_sem=dev(gsem.view(-1, 10, N // 10))),
                {"mask_pred": SERVES, "cls_prob": SERVES, "grad_sem": SERVES}, verify, bitwise=True)


def _msda_prepare(ops):
    """ms_deform_attn.hip:231-257: raw, reference_points and spatial_shapes are read by elements.  test_msda_prepare: the locations equal torch's
    expression bit for bit, the weights to 2e-7."""
    N, Lq, M, L, P = 1, 7, 2, 2, 3
    g = torch.Generator().manual_seed(N * Lq + M * L * P)
    raw = torch.randn(N, Lq, 3 * M * L * P, generator=g)
    ref_pts = torch.rand(N, Lq, L, 2, generator=g)
    shapes = torch.tensor([[32 >> l, 64 >> l] for l in range(L)], dtype=torch.int64)
    offsets = raw[..., : 2 * M * L * P].reshape(N, Lq, M, L, P, 2)
    weights = F.softmax(raw[..., 2 * M * L * P:].reshape(N, Lq, M, L * P), -1).view(N, Lq, M, L, P)
    normalizer = torch.stack([shapes[..., 1], shapes[..., 0]], -1).float()
    loc = ref_pts[:, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]

    def verify(out):
        assert torch.equal(out[0].cpu(), loc) and maxerr(out[1], weights) < 2e-7
    return Case("msda_prepare", ops.msda_prepare, dict(raw=dev(raw), reference_points=dev(ref_pts), spatial_shapes=dev(shapes), M=M, L=L, P=P),
                {"raw": SERVES, "reference_points": SERVES, "spatial_shapes": SERVES}, verify)


def _confusion(ops, gt_dtype):
    """confusion.hip:195-206: the head of the map is peeled until pred is 16-byte aligned (16-byte reads :130 behind it) and the labels are read in 16-byte
    pieces only where they are aligned there too (:198; :89, :96), else by elements (:107-111); conf and bad are the caller's, 8-byte aligned as every
    int64 tensor (:214), and only added to.  The counts equal the aligned call's and the CPU oracle's (tests/_confusion_cases.py) in every element; conf and
    bad carry guard bytes when they are the moved operands."""
    import numpy as np
    from tests import _confusion_cases as G
    K, n = 3, 1543
    g = torch.Generator().manual_seed(51)
    pred = torch.randint(-1, K + 1, (n,), generator=g, dtype=torch.int32)
    gt = torch.randint(0, 7, (n,), generator=g).to(gt_dtype)
    lut = torch.arange(256, dtype=torch.uint8)
    lut[5], lut[6] = 255, 200
    want_conf, want_bad = G.oracle(pred.numpy(), gt.numpy(), K, 255, lut.numpy())

    def call(pred, gt, lut, conf, bad):
        conf.zero_()
        bad.zero_()
        ops.confusion_accumulate(pred, gt, K, conf, bad, ignore_label=255, lut=lut)
        return conf.clone(), bad.clone()

    def verify(out):
        assert np.array_equal(out[0].cpu().numpy(), want_conf) and np.array_equal(out[1].cpu().numpy(), want_bad)
    return Case(f"confusion_accumulate[{'u8' if gt_dtype == torch.uint8 else 'i64'}]", call,
                dict(pred=dev(pred), gt=dev(gt), lut=dev(lut), conf=torch.zeros(K + 1, K + 1, dtype=torch.int64, device="cuda"),
                     bad=torch.zeros(2, dtype=torch.int64, device="cuda")),
                {"pred": SERVES, "gt": SERVES, "lut": SERVES, "conf": SERVES, "bad": SERVES}, verify)


def _train_view(ops):
    """train_view.hip: img, lab, lut, obj and objmask are read by bytes; the wide stores (:306-311) are of the outputs the wrapper allocates, behind
    `vec` (:361-362).  pad_w % 4 == 0 and cw % 4 == 0, so the aligned call and the moved ones take the wide stores.  All four results (image, sem_seg,
    outlier_mask, hist -- the nearest-neighbour tables decide sem_seg) equal the aligned call in every element, which test_train_view_gpu.py holds against
    the host composition."""
    from rba_amd.dataset_mappers import TrainViewParams
    g = torch.Generator().manual_seed(61)
    img = torch.randint(0, 256, (3, 16, 20), generator=g, dtype=torch.uint8)
    lab = torch.randint(0, 20, (16, 20), generator=g, dtype=torch.uint8)
    lut = torch.randint(0, 19, (256,), generator=g, dtype=torch.uint8)
    obj = torch.randint(0, 256, (3, 4, 5), generator=g, dtype=torch.uint8)
    objmask = (torch.rand(4, 5, generator=g) > 0.4).to(torch.uint8) * 254
    params = TrainViewParams(new_h=24, new_w=30, crop=(2, 3, 16, 20), flip=True, paste=(1, 1))
    kwargs = dict(img=dev(img), lab=dev(lab), params=params, obj=dev(obj), objmask=dev(objmask), lut=dev(lut))
    want = [t.cpu() for t in ops.train_view(**kwargs)]

    def verify(out):
        assert all(a.dtype == b.dtype and torch.equal(a.cpu(), b) for a, b in zip(out, want))
    return Case("train_view", ops.train_view, kwargs, {"img": SERVES, "lab": SERVES, "lut": SERVES, "obj": SERVES, "objmask": SERVES}, verify)


def _k1_up4(ops):
    """rba_reduce.hip:79 refuses misaligned rba / sem_seg (the wrapper's); mask_lowres is read by elements in all three forms (rba_reduce_kernels.h:185-186,
    :375-376, :548: one float per tap), cls_prob too (:204, :391, :506).  K = 19 and crop_w % 4 == 0: the matrix-pipe form (rba_reduce.hip:65).  Bars:
    test_kernels_gpu.py::test_k1_up4_shapes (sem_seg 1e-5, rba 2e-5)."""
    Q, K, h, w = _placement.UP4_CASE
    low, prob = _placement.up4_inputs()                  # seed checked on the CPU: test_ops_surface_cpu.py
    up = ref_ops.upsample_bilinear(low[None], (4 * h, 4 * w))[0]
    sem_r, rba_r, _ = ref_ops.rba_reduce_ordered(up, prob)
    sem64, _, _ = ref_ops.rba_reduce_ordered(ref_ops.upsample_bilinear(low.double()[None], (4 * h, 4 * w))[0], prob.double())
    arg_ok = _argmax_checker(sem64, _placement.UP4_SEM_SEG_BAR, "rba_reduce_up4")

    def verify(out):
        rba, sem, arg = out
        assert maxerr(sem, sem_r) < 1e-5 and maxerr(rba, rba_r) < 2e-5
        arg_ok(arg)
    return Case("rba_reduce_up4", ops.rba_reduce_up4, dict(mask_lowres=dev(low), cls_prob=dev(prob), crop_hw=(4 * h, 4 * w), want_sem_seg=True, want_argmax=True),
                {"mask_lowres": SERVES, "cls_prob": SERVES}, verify)


def _k2_backward(ops):
    """ms_deform_attn_bwd.hip:225: the model form (D = 32) reads the locations in 8-byte pieces (:134) and needs (loc | grad_loc) & 7 == 0, else the
    generic kernel's element reads; value, attn_weight, grad_output, spatial_shapes and level_start_index: element reads.  The case "model_L1" of
    tests/_msda_cases.py; truth and bar as test_msda_backward_gpu.py (fp64 autograd through the oracle, e <= 4 max(b, 2^-20))."""
    from tests import _msda_cases as C
    inp = C.make("model_L1", torch.float32)
    t64 = C.cpu_grads(inp, torch.float64)
    b = [C.err(t, r) for t, r in zip(C.cpu_grads(inp, torch.float32), t64)]

    def verify(out):
        for t, r, bb, name in zip(out, t64, b, C.NAMES):
            e = C.err(t, r)
            print(f"placement {name}: e = {e:.3e} b = {bb:.3e} bar = {C.bar(bb):.3e}")
            assert e <= C.bar(bb), name
    return Case("ms_deform_attn_backward", ops.ms_deform_attn_backward,
                dict(value=dev(inp["value"]), spatial_shapes=dev(inp["shapes"]), level_start_index=dev(inp["lsi"]), sampling_locations=dev(inp["loc"]),
                     attention_weights=dev(inp["w"]), grad_output=dev(inp["go"])),
                {"value": SERVES, "spatial_shapes": SERVES, "level_start_index": SERVES, "sampling_locations": SERVES, "attention_weights": SERVES,
                 "grad_output": SERVES}, verify)


_LOSS_NOTE = """point_loss.hip, outlier_tail.hip, dense_hybrid_loss.hip and pebal_loss.hip with bilinear_ac.h, loss_reduce.h and gaussian_blur.h hold no wide
access of global memory: every operand is read by elements, a label as one byte or one int64 (bilinear_ac.h:82-84); only the workspaces, which the wrappers
allocate, are checked (4 bytes)."""


def _point_sample(ops):
    """K8 (see _LOSS_NOTE).  Shape (2, 1, 7, 64) of tests/_point_loss_cases.py with a plane index; truth and bar: test_point_loss_gpu.py::test_point_sample."""
    from tests import _point_loss_cases as C
    shape = C.SAMPLE_SHAPES[1]
    N = shape[0]
    planes, coords, _ = C.sample_inputs(shape, False)
    index = torch.cat([torch.randperm(N + 2, generator=torch.Generator().manual_seed(1))[:N]] * 1)
    t64 = C.ref_point_sample(planes.double(), coords.double(), index)
    b = C.err(C.ref_point_sample(planes, coords, index), t64)

    def verify(out):
        C.check("placement point_sample", out, t64, b)
    return Case("point_sample", ops.point_sample, dict(planes=dev(planes), coords=dev(coords), plane_index=dev(index)),
                {"planes": SERVES, "coords": SERVES, "plane_index": SERVES}, verify)


def _mask_point_loss(ops, backward):
    """K8 (see _LOSS_NOTE).  Shape (3, 5, 7, 63); truth and bars: test_point_loss_gpu.py::test_mask_point_loss (the scalars, and the gradient of
    W_MASK loss_mask + W_DICE loss_dice)."""
    from tests import _point_loss_cases as C
    shape = C.LOSS_SHAPES[2]
    pred, index, coords, labels, num_masks = C.loss_inputs(shape)
    t = C.loss_truth(shape)
    kw = dict(pred_masks=dev(pred), plane_index=dev(index), point_coords=dev(coords), point_labels=dev(labels), num_masks=num_masks)
    moved = {"pred_masks": SERVES, "plane_index": SERVES, "point_coords": SERVES, "point_labels": SERVES}
    if not backward:
        def verify(out):
            C.check_scalar("placement loss_mask", out[0][0], t["l32"][0], t["l64"][0])
            C.check_scalar("placement loss_dice", out[0][1], t["l32"][1], t["l64"][1])
        return Case("mask_point_loss", ops.mask_point_loss, kw, moved, verify, bitwise=True)
    sums = ops.mask_point_loss(**kw)[1]

    def verify(out):
        C.check("placement grad", out.cpu(), t["g64"], t["b"])
    kw.update(sums=sums, grad_loss_mask=torch.full((1,), C.W_MASK, device="cuda"), grad_loss_dice=torch.full((1,), C.W_DICE, device="cuda"))
    moved.update(sums=SERVES, grad_loss_mask=SERVES, grad_loss_dice=SERVES)
    return Case("mask_point_loss_backward", ops.mask_point_loss_backward, kw, moved, verify)


def _match_cost(ops):
    """K8 (see _LOSS_NOTE).  Shape (3, 1, 64); truth and bar: test_point_loss_gpu.py::test_match_cost."""
    from tests import _point_loss_cases as C
    shape = C.COST_SHAPES[4]
    pred, tgt, coords, logits, ids = C.cost_inputs(shape)
    c64, b = C.cost_truth(shape)
    wm, wc, wd = C.COST_WEIGHTS

    def verify(out):
        C.check("placement match_cost", out.cpu(), c64, b)
    return Case("match_cost", ops.match_cost, dict(pred_masks=dev(pred), tgt_masks=dev(tgt), coords=dev(coords), cls_prob=dev(logits.softmax(-1)), tgt_ids=dev(ids),
                                                   cost_mask=wm, cost_class=wc, cost_dice=wd),
                {"pred_masks": SERVES, "tgt_masks": SERVES, "coords": SERVES, "cls_prob": SERVES, "tgt_ids": SERVES}, verify, bitwise=True)


def _outlier_tail(ops, backward):
    """K9 (see _LOSS_NOTE).  The first shape and "squared_hinge" of test_outlier_tail_gpu.py, its truth and bars."""
    from tests import _point_loss_cases as P
    from tests import _rba_bwd_cases as C
    from tests import test_outlier_tail_gpu as T
    shape, func = T.SHAPES[0], "squared_hinge"
    score, labels = T.inputs(shape)
    t = T.truth(shape, func)
    kw = dict(score=dev(score), labels=dev(labels), func=func, thr_in=T.THR_IN, thr_out=T.THR_OUT)
    if not backward:
        def verify(out):
            loss, stats = out
            P.check_scalar("placement loss", loss[0], t["l32"], t["l64"])
            for i, name in enumerate(("sum_in", "n_in", "sum_out", "n_out")):
                if name.startswith("n_"):
                    assert float(stats[i]) == t["stats64"][i], name
                else:
                    P.check_scalar(name, stats[i], t["stats32"][i], t["stats64"][i])
        return Case("outlier_tail", ops.outlier_tail, kw, {"score": SERVES, "labels": SERVES}, verify, bitwise=True)
    stats = ops.outlier_tail(**kw)[1]

    def verify(out):
        C.check("placement grad_score", out.cpu(), t["g64"], t["b"])
    kw.update(stats=stats, grad_loss=torch.ones(1, device="cuda"))
    return Case("outlier_tail_backward", ops.outlier_tail_backward, kw, {"score": SERVES, "labels": SERVES, "stats": SERVES, "grad_loss": SERVES}, verify,
                bitwise=True)


def _dense_hybrid(ops, backward):
    """K10 (see _LOSS_NOTE).  The first shape of tests/_dense_hybrid_cases.py; truth and bars: test_dense_hybrid_loss_gpu.py::test_kernel_against_fp64."""
    from tests import _dense_hybrid_cases as D
    from tests import _point_loss_cases as P
    from tests import _rba_bwd_cases as C
    shape = D.TAIL_SHAPES[0]
    sem, ood, labels = D.tail_inputs(shape)
    t = D.tail_truth(shape)
    kw = dict(sem=dev(sem), ood=dev(ood), labels=dev(labels), beta=D.BETA)
    if not backward:
        up64 = F.interpolate(sem.double(), size=labels.shape[-2:], mode="bilinear", align_corners=True)
        lse64 = torch.logsumexp(up64, dim=1)
        b_lse = C.err(torch.logsumexp(F.interpolate(sem, size=labels.shape[-2:], mode="bilinear", align_corners=True), dim=1), lse64)

        def verify(out):
            losses, stats, lse = out
            P.check_scalar("placement loss", losses[0], t["l32"], t["l64"])
            for i, name in enumerate(("loss_seg", "loss_ood", "loss_th"), start=1):
                P.check_scalar(name, losses[i], t["parts32"][name], t["parts64"][name])
            for i, name in enumerate(("S_seg", "S_ood", "S_th", "S_x", "n_seg", "n_ood", "n_all", "m")):
                if name.startswith("n_"):
                    assert float(stats[i]) == t["parts64"][name], name
                else:
                    P.check_scalar(name, stats[i], t["parts32"][name], t["parts64"][name])
            C.check("placement lse", lse.cpu(), lse64, b_lse)
        return Case("dense_hybrid_loss", ops.dense_hybrid_loss, kw, {"sem": SERVES, "ood": SERVES, "labels": SERVES}, verify, bitwise=True)
    _, stats, lse = ops.dense_hybrid_loss(**kw)

    def verify(out):
        C.check("placement grad_sem", out[0].cpu(), t["gs64"], t["b_sem"])
        C.check("placement grad_ood", out[1].cpu(), t["go64"], t["b_ood"])
    kw.update(stats=stats, lse=lse, grad_loss=torch.ones(1, device="cuda"))
    return Case("dense_hybrid_loss_backward", ops.dense_hybrid_loss_backward, kw,
                {"sem": SERVES, "ood": SERVES, "labels": SERVES, "stats": SERVES, "lse": SERVES, "grad_loss": SERVES}, verify, bitwise=True)


def _gambler(ops, backward):
    """K11a (see _LOSS_NOTE).  The first shape of tests/_pebal_cases.py; truth and bars: test_gambler_loss_gpu.py::test_kernel_against_fp64."""
    from tests import _pebal_cases as G
    from tests import _point_loss_cases as P
    from tests import _rba_bwd_cases as C
    shape = G.TAIL_SHAPES[0]
    sem, labels = G.tail_inputs(shape)
    t = G.tail_truth(shape)
    kw = dict(sem=dev(sem), labels=dev(labels), ood_reg=G.OOD_REG)
    if not backward:
        def verify(out):
            losses, stats, R = out
            p32, p64 = t["parts32"], t["parts64"]
            P.check_scalar("placement loss", losses[0], t["l32"], t["l64"])
            P.check_scalar("in-mean", losses[1], p32["in_mean"], p64["in_mean"])
            P.check_scalar("out-mean", losses[2], p32["out_mean"], p64["out_mean"])
            P.check_scalar("S_in", stats[0], p32["S_in"], p64["S_in"])
            P.check_scalar("S_out", stats[1], p32["S_out"], p64["S_out"])
            assert float(stats[2]) == p64["n_in"] and float(stats[3]) == p64["n_ood"]
            C.check("placement R", R.cpu(), p64["R"], C.err(p32["R"], p64["R"]))
        return Case("gambler_loss", ops.gambler_loss, kw, {"sem": SERVES, "labels": SERVES}, verify, bitwise=True)
    _, stats, R = ops.gambler_loss(**kw)

    def verify(out):
        C.check("placement grad_sem", out.cpu(), t["g64"], t["b"])
    kw.update(stats=stats, R=R, grad_loss=torch.ones(1, device="cuda"))
    return Case("gambler_loss_backward", ops.gambler_loss_backward, kw, {"sem": SERVES, "labels": SERVES, "stats": SERVES, "R": SERVES, "grad_loss": SERVES},
                verify, bitwise=True)


# ---------------------------------------------------------------------------------------------------------------- K5, K6, K7 and the packers
def _same_bits(want):
    """a moved operand that is read by elements changes no bit of the result"""
    want = [t.clone() for t in (want if isinstance(want, (tuple, list)) else [want])]

    def check(out):
        out = out if isinstance(out, (tuple, list)) else [out]
        assert all(torch.equal(a, b) for a, b in zip(out, want))
    return check


K6_BAR = lambda K: 2e-5 * (K / 256) ** 0.5 + 2e-6          # test_split_linear_vs_fp64, test_split_linear_nchw_out, test_conv3x3_nhwc_vs_fp64


def _split_linear(ops, mode, nchw=False, through_linear=False):
    """K6.  x, the packed planes and the output are in the entry points' refusal (RBA_GEMM_PROLOGUE: split_linear_dma.hip:36 bf16x6, :135 f16x3, :292
    channel-major).  bias is read by elements: the fp32-row and channel-major epilogues (split_linear_h3.h:151, :238; split_linear_dma.h:255, :511) take
    bias[col]; the two 16-byte bias reads of the family are elsewhere -- split_linear_h3.h:717 is the split-output epilogue, whose entry point lists bias
    (split_linear_dma.hip:226), and split_linear_dma.h:488 is behind WIDE, which only the tools' tuning library instantiates
    (tune/split_linear_tune.hip:82).  Reference and bar: test_split_linear_vs_fp64 / test_split_linear_nchw_out."""
    from types import SimpleNamespace
    M, N, K = 8, 128, 32
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ref = F.linear(x.double(), w.double(), b.double())
    if through_linear:
        wd = dev(w)

        def call(x, bias):
            return ops.linear(x, SimpleNamespace(weight=wd, bias=bias))

        def verify(out):
            assert maxerr(out, ref) < K6_BAR(K)
        return Case("linear", call, dict(x=dev(x), bias=dev(b)), {"x": REFUSES, "bias": SERVES}, verify)
    planes = ops.split_weight(dev(w), mode=mode)
    if nchw:
        ref = ref.view(2, 4, N).permute(0, 2, 1)

    def verify(out):
        assert maxerr(out, ref) < K6_BAR(K)
    if nchw:
        return Case("split_linear_nchw_out", ops.split_linear_nchw_out, dict(x=dev(x), planes=planes, bias=dev(b), rows_per_image=4),
                    {"x": REFUSES, "planes": REFUSES, "bias": SERVES}, verify)
    return Case(f"split_linear[{mode}]", ops.split_linear, dict(x=dev(x), planes=planes, bias=dev(b)), {"x": REFUSES, "planes": REFUSES, "bias": SERVES}, verify)


def _packers(ops, which):
    """split_weight: weight (and the planes it allocates) are refused (split_linear_dma.hip:47, split_linear.hip:351).  conv3x3_weight permutes its
    operand with torch and hands split_weight a fresh tensor: a moved weight is served, bit for bit.  swin_attn_block_weights: both weights refused
    (swin_attn_block.hip:72).  swin_bias_fragments: rel_bias is read by elements (swin_window_attn.hip, swin_bias_fragments_kernel: no wide access), the
    result is a permutation -- the aligned call's bits, which test_k5_window_attn_core holds to the attention it feeds."""
    g = torch.Generator().manual_seed(81)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    if which == "split_weight":
        return _refusing("split_weight", ops.split_weight, dict(weight=r(128, 32), mode="f16x3"), ("weight",), (1, 2, 2, 128, 2, 8), "split_linear_dma.hip:47")
    if which == "conv3x3_weight":
        w = r(8, 32, 3, 3)
        return Case("conv3x3_weight", ops.conv3x3_weight, dict(weight=w, mode="f16x3"), {"weight": SERVES}, _same_bits(ops.conv3x3_weight(w, mode="f16x3")))
    if which == "swin_attn_block_weights":
        kw = dict(qkv_weight=r(384, 128), proj_weight=r(128, 128))
        n = ops.swin_attn_block_weights(**kw).numel()
        return _refusing("swin_attn_block_weights", ops.swin_attn_block_weights, kw, ("qkv_weight", "proj_weight"), (n,), "swin_attn_block.hip:72")
    rel = r(2, 36, 36)
    return Case("swin_bias_fragments", ops.swin_bias_fragments, dict(rel_bias=rel, window_size=6), {"rel_bias": SERVES},
                _same_bits(ops.swin_bias_fragments(rel, 6)))


def _conv3x3(ops):
    """K6 implicit GEMM: x, planes, out refused (split_linear_dma.hip:146); bias by elements (split_linear_h3.h:151).  Reference and bar:
    test_conv3x3_nhwc_vs_fp64."""
    B, H, W, C, N = 1, 5, 3, 32, 40
    g = torch.Generator().manual_seed(B * 1000 + H * W + C)
    x = torch.randn(B, C, H, W, generator=g)
    w = torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5
    b = torch.randn(N, generator=g)
    ref = F.conv2d(x.double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    planes = ops.conv3x3_weight(dev(w), mode="f16x3")

    def verify(out):
        assert maxerr(out, ref) < 2e-5 * (9 * C / 256) ** 0.5 + 2e-6
    return Case("conv3x3_nhwc", ops.conv3x3_nhwc, dict(x=dev(x.permute(0, 2, 3, 1).contiguous()), planes=planes, bias=dev(b), out_features=N),
                {"x": REFUSES, "planes": REFUSES, "bias": SERVES}, verify)


def _nchw_out_gn(ops, rows):
    """K6 with the GroupNorm folded into the loads: x, planes, out and the norm's weight / bias are refused (split_linear_gnf.hip:21-22, :45-46); the
    statistics `mr`, the Linear's bias and the row index are read by elements (split_linear_h3.h:238, :516 and the staging loops: no wide access of them).
    Reference and bar: test_split_linear_nchw_out_with_folded_group_norm (fp64, 4e-5 (K / 256)^0.5 + 4e-6); the row form equals the full form's columns."""
    B, P, K, N, G = 1, 128, 32, 128, 8
    g = torch.Generator().manual_seed(B + P + K + N)
    x = torch.randn(B, P, K, generator=g) * 3 + 0.7
    w, b = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ga, be = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g)
    xd = dev(x)
    p3 = ops.split_weight(dev(w), mode="f16x3")
    mr = ops.group_norm_nhwc_stats(xd, G, 1e-5)
    y = F.group_norm(x.double().permute(0, 2, 1), G, ga.double(), be.double(), 1e-5)
    ref = F.linear(y.relu().permute(0, 2, 1), w.double(), b.double()).permute(0, 2, 1)
    kw = dict(x=xd.view(B * P, K), mr=mr, weight=dev(ga), bias_gn=dev(be), num_groups=G, relu=True, planes=p3, bias=dev(b), rows_per_image=P, out_features=N)
    moved = {"x": REFUSES, "planes": REFUSES, "weight": REFUSES, "bias_gn": REFUSES, "mr": SERVES, "bias": SERVES}
    if not rows:
        def verify(out):
            assert maxerr(out, ref) < 4e-5 * (K / 256) ** 0.5 + 4e-6
        return Case("split_linear_nchw_out_gn", ops.split_linear_nchw_out_gn, kw, moved, verify)
    idx = torch.randperm(P, generator=g)[None].to(torch.int32)
    full = ops.split_linear_nchw_out_gn(**kw)

    def call(rows, **k):
        return ops.split_linear_nchw_out_gn_rows(rows=ops.RowIndex(rows, P), **k)

    def verify(out):
        assert torch.equal(out, full[:, :, idx[0].long().cuda()]) and maxerr(out, ref[:, :, idx[0].long()]) < 4e-5 * (K / 256) ** 0.5 + 4e-6
    return Case("split_linear_nchw_out_gn_rows", call, dict(kw, rows=dev(idx)), dict(moved, rows=SERVES), verify)


def _mlp_fused(ops, ln):
    """The one-kernel Swin MLP: x, both weight images, the residual / output and fc1's bias are refused (split_linear_dma.hip:271; with the norm in the
    prologue also its weight and bias, :281); fc2's bias is read by elements (the residual epilogue, split_linear_h3.h:151).  x / residual are written in
    place: a refused call leaves them as they were.  Reference and bar: test_swin_mlp_fused (fp64 composition, 3e-5)."""
    from types import SimpleNamespace
    M, C, hidden = 8, 128, 64
    g = torch.Generator().manual_seed(M + hidden)
    r = lambda *s: torch.randn(*s, generator=g)
    x0, r0 = r(M, C) * 2, r(M, C)
    w1, b1, w2, b2 = r(hidden, C) * C ** -0.5, r(hidden) * 0.2, r(C, hidden) * hidden ** -0.5, r(C) * 0.2
    nw, nb = 1 + 0.1 * r(C), 0.1 * r(C)
    w1d, w2d = dev(w1), dev(w2)
    if not ln:
        ref = r0.double() + F.linear(F.gelu(F.linear(x0.double(), w1.double(), b1.double())), w2.double(), b2.double())
        r0d = dev(r0)

        def call(x, residual, b1, b2):
            return ops.mlp_fused(x, SimpleNamespace(weight=w1d, bias=b1), SimpleNamespace(weight=w2d, bias=b2), residual)

        def verify(out):
            assert maxerr(out, ref) < 3e-5
        return Case("mlp_fused", call, dict(x=dev(x0), residual=dev(r0), b1=dev(b1), b2=dev(b2)),
                    {"x": REFUSES, "residual": REFUSES, "b1": REFUSES, "b2": SERVES}, verify, owned=("residual",),
                    reset=lambda kw: kw["residual"].copy_(r0d))
    y = F.layer_norm(x0.double(), (C,), nw.double(), nb.double(), 1e-5)
    ref = x0.double() + F.linear(F.gelu(F.linear(y, w1.double(), b1.double())), w2.double(), b2.double())
    x0d = dev(x0)

    def call(x, norm_weight, norm_bias, b1, b2):
        return ops.mlp_fused_ln(x, (norm_weight, norm_bias, 1e-5), SimpleNamespace(weight=w1d, bias=b1), SimpleNamespace(weight=w2d, bias=b2))

    def verify(out):
        assert maxerr(out, ref) < 3e-5
    return Case("mlp_fused_ln", call, dict(x=dev(x0), norm_weight=dev(nw), norm_bias=dev(nb), b1=dev(b1), b2=dev(b2)),
                {"x": REFUSES, "norm_weight": REFUSES, "norm_bias": REFUSES, "b1": REFUSES, "b2": SERVES}, verify, owned=("x",),
                reset=lambda kw: kw["x"].copy_(x0d))


def _gn_moments(ops, conv):
    """The GEMMs whose epilogue leaves the GroupNorm moments exist from 160 (Linear) / 256 (convolution) tiles of 128 x 128 on, so these two cases are the
    large ones of the file (20 480 x 32 rows; a 128 x 256 x 32 split image).  x, planes, out refused (split_linear_dma.hip:161; :174 lists the bias too:
    the split-image convolution refuses a moved bias); the Linear's bias is read by elements (split_linear_h3.h:151).  The Linear's output is
    linear()'s bit for bit and its statistics meet test_linear_with_gn_moments_epilogue's bars."""
    from types import SimpleNamespace
    g = torch.Generator().manual_seed(91)
    if not conv:
        B, P, K, N, G = 1, 20480, 32, 128, 8
        x = dev(torch.randn(B, P, K, generator=g) * 2 + 0.3)
        wd, bd = dev(torch.randn(N, K, generator=g) * K ** -0.5), dev(torch.randn(N, generator=g))
        assert ops.linear_emits_gn_moments(B * P, N, K, P, G)
        want = ops.linear(x, SimpleNamespace(weight=wd, bias=bd))
        yd = want.double().view(B, P, G, N // G)
        mean64, var64 = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)

        def call(x, bias):
            return ops.linear_gn_stats(x, SimpleNamespace(weight=wd, bias=bias), G, 1e-5, P)

        def verify(out):
            y, mr = out
            assert torch.equal(y, want) and maxerr(mr[..., 0], mean64) < 2e-6
            assert ((mr[..., 1].double().cpu() * (var64 + 1e-5).sqrt().cpu()) - 1).abs().max() < 2e-6
        return Case("linear_gn_stats", call, dict(x=x, bias=bd), {"x": REFUSES, "bias": SERVES}, verify)
    B, H, W, C, N, G = 1, 128, 256, 32, 128, 8
    assert ops.conv3x3_emits_gn_moments(B, H, W, N, G)
    xs = ops.SplitActivations.pack(dev(torch.randn(B, H, W, C, generator=g)))
    planes = ops.conv3x3_weight(dev(torch.randn(N, C, 3, 3, generator=g) * (9 * C) ** -0.5), mode="f16x3")

    def call(x_data, planes, bias):
        return ops.conv3x3_nhwc_gn_stats(ops.SplitActivations(x_data, (B, H, W, C)), planes, G, 1e-5, bias=bias)
    return _refusing("conv3x3_nhwc_gn_stats", call, dict(x_data=xs.data, planes=planes, bias=dev(torch.randn(N, generator=g))), ("x_data", "planes", "bias"),
                     (B, G, 2), "split_linear_dma.hip:174")


def _compose(ops):
    """split_linear_dma.hip:125: embed, weight (and the planes it allocates) refused; bias is read by elements (:74).  fp32 FMAs in a fixed order: a moved
    bias changes no bit; bias_q against embed @ bias in fp64 at the K6 bar."""
    g = torch.Generator().manual_seed(95)
    r = lambda *s: torch.randn(*s, generator=g)
    E, Wt, b = r(2, 5, 8), r(8, 32), r(8)
    kw = dict(embed=dev(E), weight=dev(Wt), bias=dev(b))
    same = _same_bits(ops.compose_query_operand(**kw))

    def verify(out):
        same(out)
        assert maxerr(out[1], E.double() @ b.double()) < K6_BAR(8)
    return Case("compose_query_operand", ops.compose_query_operand, kw, {"embed": REFUSES, "weight": REFUSES, "bias": SERVES}, verify)


def _k5(ops, frag):
    """swin_window_attn.hip:395 / :427: qkv, qkv_bias, the output and (since the audit) bias_frag are refused.  rel_bias: without bias_frag the
    matrix-pipe kernels read a row of it in 16-byte pieces where N % 4 == 0 (:251, swin_window_attn_h3.h:238) -- `vec_bias` (:199, h3.h:188) now also asks
    for a 16-byte aligned rel_bias, else the element reads of N % 4 != 0; with bias_frag it is not read.  N = 36.  Reference and bar:
    test_k5_window_attn_core (the window-attention oracle, 1e-5)."""
    H, W, ws, nH, shift = 12, 12, 6, 2, 0
    g = torch.Generator().manual_seed(H * W)
    C, B = nH * 32, 2
    qkv_w, qkv_b = torch.randn(3 * C, C, generator=g) * C ** -0.5, torch.randn(3 * C, generator=g) * 0.2
    table = torch.randn((2 * ws - 1) ** 2, nH, generator=g) * 0.5
    x = torch.randn(B, H * W, C, generator=g)
    xw = x.view(B, H // ws, ws, W // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, C)
    aw = ref_ops.window_attention(xw, qkv_w, qkv_b, torch.eye(C), torch.zeros(C), table, ws, nH, None)
    ref = aw.view(B, H // ws, W // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, H * W, C)
    N = ws * ws
    bias = table[ref_ops.relative_position_index(ws).view(-1)].view(N, N, nH).permute(2, 0, 1).contiguous()
    kw = dict(qkv=dev(F.linear(x, qkv_w, qkv_b)), qkv_bias=dev(qkv_b), rel_bias=dev(bias), H=H, W=W, num_heads=nH, window_size=ws, shift=shift)
    moved = {"qkv": REFUSES, "qkv_bias": REFUSES, "rel_bias": SERVES}
    if frag:
        kw["bias_frag"] = ops.swin_bias_fragments(kw["rel_bias"], ws)
        moved["bias_frag"] = REFUSES

    def verify(out):
        assert maxerr(out, ref) < 1e-5
    return Case(f"swin_window_attn[{'frag' if frag else 'rel_bias'}]", ops.swin_window_attn, kw, moved, verify)


def _k7(ops, block):
    """K7: every caller's pointer is in the one refusal (swin_attn_block.hip:56-57 for the attention-only form, :87-88 for the block, which writes x in
    place): the refusal is the whole test."""
    g = torch.Generator().manual_seed(97)
    r = lambda *s: dev(torch.randn(*s, generator=g))
    C, H, W, ws = 128, 12, 12, 12
    assert ops.swin_attn_block_ok(C, 4, ws) and ops.swin_attn_qkv_ok(C, 4, ws)
    image = ops.swin_attn_block_weights(r(3 * C, C) * C ** -0.5, r(C, C) * C ** -0.5)
    frag = ops.swin_bias_fragments(r(4, ws * ws, ws * ws) * 0.5, ws)
    x0 = r(1, H * W, C)

    def call(x, n1w, n1b, image, qkv_bias, bias_frag, proj_bias=None, n2w=None, n2b=None):
        if not block:
            return ops.swin_attn_qkv(x, (n1w, n1b, 1e-5), image, qkv_bias, bias_frag, H, W, ws, 0).unpack()
        return ops.swin_attn_block(x, (n1w, n1b, 1e-5), image, qkv_bias, bias_frag, proj_bias, H, W, ws, 0, norm2=(n2w, n2b, 1e-5))
    kw = dict(x=x0.clone(), n1w=r(C), n1b=r(C), image=image, qkv_bias=r(3 * C), bias_frag=frag)
    if block:
        kw.update(proj_bias=r(C), n2w=r(C), n2b=r(C))
    return _refusing("swin_attn_block" if block else "swin_attn_qkv", call, kw, tuple(kw), (1, H * W, C),
                     "swin_attn_block.hip:87-88" if block else "swin_attn_block.hip:56-57", owned=("x",) if block else (),
                     reset=(lambda kw: kw["x"].copy_(x0)) if block else None)


def _resample_nhwc_gn(ops):
    """resample.hip:238: x, add, out and the two norms' weight / bias are refused; the two statistics pointers are read by elements (:77).  Reference
    and bar: test_resample_nhwc_with_folded_group_norms (group_norm_nhwc + resample_bilinear_nhwc, 4e-7 max|want|)."""
    h, w, H, W, C, G = 3, 4, 6, 8, 32, 8
    g = torch.Generator().manual_seed(h * w + C)
    x = dev(torch.randn(1, h * w, C, generator=g) * 2 + 0.5)
    add = dev(torch.randn(1, H * W, C, generator=g))
    gx, bx, ga, ba = (dev(torch.randn(C, generator=g)) for _ in range(4))
    xn, an = ops.group_norm_nhwc(x, G, gx, bx, 1e-5, relu=True), ops.group_norm_nhwc(add, G, ga, ba, 1e-5)
    mx, ma = ops.group_norm_nhwc_stats(x, G, 1e-5), ops.group_norm_nhwc_stats(add, G, 1e-5)
    want = ops.resample_bilinear_nhwc(xn[0].view(h, w, C), (H, W), add=an[0].view(H, W, C))
    tol = 4e-7 * float(want.abs().max())

    def call(x, add, x_mr, x_weight, x_bias, add_mr, add_weight, add_bias):
        return ops.resample_bilinear_nhwc_gn(x, (H, W), add, G, x_norm=(x_mr, x_weight, x_bias, True), add_norm=(add_mr, add_weight, add_bias))

    def verify(out):
        assert maxerr(out, want.double()) <= tol
    return Case("resample_bilinear_nhwc_gn", call, dict(x=x[0].view(h, w, C), add=add[0].view(H, W, C), x_mr=mx[0].contiguous(), x_weight=gx, x_bias=bx,
                                                        add_mr=ma[0].contiguous(), add_weight=ga, add_bias=ba),
                {"x": REFUSES, "add": REFUSES, "x_weight": REFUSES, "x_bias": REFUSES, "add_weight": REFUSES, "add_bias": REFUSES, "x_mr": SERVES,
                 "add_mr": SERVES}, verify)


def _skinny(ops):
    """skinny_linear.hip:150 `RBA_CHECK_ARG(((x | weight | x_add) & 15) == 0)`; bias and out: element accesses (:69-72, :130-133), so a moved bias or a
    moved caller-owned `out` is served.  Bar: test_skinny_linear (2e-5 (K / 256)^0.5 + 2e-6)."""
    M, N, K = 5, 16, 32
    g = torch.Generator().manual_seed(M + N + K)
    x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ref = F.relu(F.linear(x.double(), w.double(), b.double()))

    def verify(out):
        assert maxerr(out, ref) < 2e-5 * (K / 256) ** 0.5 + 2e-6
    return Case("skinny_linear", ops.skinny_linear, dict(x=dev(x), weight=dev(w), bias=dev(b), relu=True, out=torch.full((M, N), -7.0, device="cuda")),
                {"x": REFUSES, "weight": REFUSES, "bias": SERVES, "out": SERVES}, verify)


def _skinny_add(ops):
    """the `x_add` form of the same entry point (rba_skinny_linear_add_f32): x_add is in the refusal of skinny_linear.hip:150"""
    M, N, K = 5, 16, 32
    g = torch.Generator().manual_seed(M + N + K + 1)
    x, xa = torch.randn(M, K, generator=g), torch.randn(M, K, generator=g)
    w, b = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g)
    ref = F.linear((x + xa).double(), w.double(), b.double())

    def verify(out):
        assert maxerr(out, ref) < 2e-5 * (K / 256) ** 0.5 + 2e-6
    return Case("skinny_linear[x_add]", ops.skinny_linear, dict(x=dev(x), weight=dev(w), bias=dev(b), x_add=dev(xa)),
                {"x": REFUSES, "weight": REFUSES, "x_add": REFUSES, "bias": SERVES}, verify)


CASES = {
    "rba_reduce[K=3]": lambda ops: _k1(ops, "rba_reduce[K=3]"),
    "rba_reduce[K=19]": lambda ops: _k1(ops, "rba_reduce[K=19]"),
    "resample_bilinear": _resample,
    "resample_bilinear_ac": _resample_ac,
    "group_norm": _group_norm,
    "bn_relu_conv1x1[P=16]": lambda ops: _bn_relu_conv1x1(ops, 4, 4),
    "bn_relu_conv1x1[P=15]": lambda ops: _bn_relu_conv1x1(ops, 3, 5),
    "mask_logits[fp32]": lambda ops: _mask_logits(ops, "fp32", 8),
    "mask_logits[f16x3]": lambda ops: _mask_logits(ops, "f16x3", 32),
    "mask_logits_backward": _k4_backward,
    "ms_deform_attn_forward[L=1]": lambda ops: _k2(ops, 1),
    "ms_deform_attn_forward[L=3]": lambda ops: _k2(ops, 3),
    "msda_fused[L=1]": lambda ops: _msda_fused(ops, 1),
    "msda_fused[L=3]": lambda ops: _msda_fused(ops, 3),
    "resize_u8_pil_bilinear[vertical]": lambda ops: _resize_u8(ops, (12, 8), False),
    "resize_u8_pil_bilinear[horizontal]": lambda ops: _resize_u8(ops, (8, 12), True),
    "resize_u8_pil_bilinear[both]": lambda ops: _resize_u8(ops, (12, 12), True),
    "tta_merge": _tta_merge,
    "masked_xattn[split]": lambda ops: _k3(ops, True),
    "masked_xattn[plain]": lambda ops: _k3(ops, False),
    "masked_xattn[auto S=1024]": lambda ops: _k3(ops, None, 1024),
    "masked_xattn_backward": _k3_backward,
    "sem_seg_backward": _sem_seg_backward,
    "msda_prepare": _msda_prepare,
    "confusion_accumulate[u8]": lambda ops: _confusion(ops, torch.uint8),
    "confusion_accumulate[i64]": lambda ops: _confusion(ops, torch.int64),
    "train_view": _train_view,
    "split_linear[f16x3]": lambda ops: _split_linear(ops, "f16x3"),
    "split_linear[bf16x6]": lambda ops: _split_linear(ops, "bf16x6"),
    "split_linear_nchw_out": lambda ops: _split_linear(ops, "f16x3", nchw=True),
    "linear": lambda ops: _split_linear(ops, "f16x3", through_linear=True),
    "split_weight": lambda ops: _packers(ops, "split_weight"),
    "conv3x3_weight": lambda ops: _packers(ops, "conv3x3_weight"),
    "swin_attn_block_weights": lambda ops: _packers(ops, "swin_attn_block_weights"),
    "swin_bias_fragments": lambda ops: _packers(ops, "swin_bias_fragments"),
    "conv3x3_nhwc": _conv3x3,
    "split_linear_nchw_out_gn": lambda ops: _nchw_out_gn(ops, False),
    "split_linear_nchw_out_gn_rows": lambda ops: _nchw_out_gn(ops, True),
    "mlp_fused": lambda ops: _mlp_fused(ops, False),
    "mlp_fused_ln": lambda ops: _mlp_fused(ops, True),
    "linear_gn_stats": lambda ops: _gn_moments(ops, False),
    "conv3x3_nhwc_gn_stats": lambda ops: _gn_moments(ops, True),
    "compose_query_operand": _compose,
    "swin_window_attn[rel_bias]": lambda ops: _k5(ops, False),
    "swin_window_attn[frag]": lambda ops: _k5(ops, True),
    "swin_attn_qkv": lambda ops: _k7(ops, False),
    "swin_attn_block": lambda ops: _k7(ops, True),
    "resample_bilinear_nhwc_gn": _resample_nhwc_gn,
    "rba_reduce_up4": _k1_up4,
    "ms_deform_attn_backward": _k2_backward,
    "point_sample": _point_sample,
    "mask_point_loss": lambda ops: _mask_point_loss(ops, False),
    "mask_point_loss_backward": lambda ops: _mask_point_loss(ops, True),
    "match_cost": _match_cost,
    "outlier_tail": lambda ops: _outlier_tail(ops, False),
    "outlier_tail_backward": lambda ops: _outlier_tail(ops, True),
    "dense_hybrid_loss": lambda ops: _dense_hybrid(ops, False),
    "dense_hybrid_loss_backward": lambda ops: _dense_hybrid(ops, True),
    "gambler_loss": lambda ops: _gambler(ops, False),
    "gambler_loss_backward": lambda ops: _gambler(ops, True),
    "token_linear[norm]": _token_linear_norm,
    "token_linear_multi": _token_linear_multi,
    "rba_reduce_backward": _k1_backward,
    "quad_mean": _quad_mean,
    "softmax_drop_last": _softmax_drop_last,
    "gaussian_blur": _gaussian_blur,
    "gaussian_blur_planes": lambda ops: _blur_planes(ops, False),
    "gaussian_blur_planes_adjoint": lambda ops: _blur_planes(ops, True),
    "patch_im2col[u8]": lambda ops: _patch_im2col(ops, torch.uint8),
    "patch_im2col[f32]": lambda ops: _patch_im2col(ops, torch.float32),
    "ood_components": _ood_components,
    "score_reg": lambda ops: _score_reg(ops, False),
    "score_reg_backward": lambda ops: _score_reg(ops, True),
    "add_layer_norm": _add_layer_norm,
    "merge_layer_norm": _merge_layer_norm,
    "group_norm_nhwc": lambda ops: _group_norm_nhwc(ops, False),
    "group_norm_nhwc_stats": lambda ops: _group_norm_nhwc(ops, True),
    "resample_bilinear_nhwc": _resample_nhwc,
    "token_linear": _token_linear,
    "skinny_linear": _skinny,
    "skinny_linear[x_add]": _skinny_add,
}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


def test_the_cases_are_the_listed_wrappers():
    assert sorted({name.split("[")[0] for name in CASES} | set(_ops_surface.PLACEMENT_ROWS_OUTSIDE_THE_CASE_TABLE)) == sorted(_ops_surface.PLACEMENT_ROWS)


def _run(case, kwargs, placed, expect):
    from rba_amd._lib import RbaHipError
    if kwargs.get("out") is not None:
        kwargs["out"].fill_(-7.0)
    if case.reset is not None:
        case.reset(kwargs)
    if expect == REFUSES:
        before = {path: _get(kwargs, path).clone() for path in case.owned}
        with pytest.raises(RbaHipError):
            case.fn(**kwargs)
        torch.cuda.synchronize()
        for path, t in before.items():
            assert torch.equal(_get(kwargs, path), t), f"a refused call wrote its caller-owned {path}"
    else:
        out = case.fn(**kwargs)
        case.verify(out)
        if case.bitwise:
            if case.reset is not None:
                case.reset(kwargs)
            again = case.fn(**kwargs)
            pairs = zip(out, again) if isinstance(out, (tuple, list)) else [(out, again)]
            assert all(torch.equal(a, b) for a, b in pairs), "two launches at one placement differ in bits"
    assert all(p.untouched() for p in placed), "bytes beside a moved operand were written"


@pytest.mark.parametrize("name", list(CASES))
def test_operands_off_a_16_byte_boundary(ops, name):
    case = CASES[name](ops)
    if case.reset is not None:
        case.reset(case.kwargs)
    case.verify(case.fn(**case.kwargs))                                  # the aligned call meets its bar
    for path, expect in case.operands.items():
        t = _get(case.kwargs, path)
        for nbytes in SHIFTS[t.dtype]:
            p = place(t, nbytes)
            _run(case, _with(case.kwargs, path, p.tensor), [p], expect)
    # all together, each by a shift of its dtype (cycled, so that the operands do not share one offset)
    kwargs, placed = case.kwargs, []
    for i, path in enumerate(case.operands):
        t = _get(case.kwargs, path)
        p = place(t, SHIFTS[t.dtype][i % len(SHIFTS[t.dtype])])
        kwargs = _with(kwargs, path, p.tensor)
        placed.append(p)
    _run(case, kwargs, placed, REFUSES if REFUSES in case.operands.values() else SERVES)


def test_k15_steps_parameters_wherever_they_lie(ops):
    """adamw_step.hip:124: K15b tests each parameter's pointer and steps an unaligned one by elements (the flat grad / exp_avg / exp_avg_sq buffers are
    refused unless 16-byte aligned: :161, :174, and ops._adamw_flat_ok).  Every parameter handed to adamw_plan is carved out 4, 8 or 12 bytes off a
    16-byte boundary between guard bytes; the case table's truth and bar (tests/_solver_cases.py, as test_adamw_step_gpu.py::test_parity_on_the_case_table)
    hold, two runs give equal bits, and no byte beside a parameter changes."""
    from rba_amd.solver import ClipAdamW
    from tests import _solver_cases as S
    case = (2, 0.01, 0.5)
    steps, max_norm, grad_scale = case
    p0, grads = S.inputs()
    t64, b = S.truth(case)
    runs = []
    for _ in range(2):
        placed = [place(t.cuda(), (4, 8, 12)[i % 3]) for i, t in enumerate(p0)]
        named = [(name, p.tensor.requires_grad_(True)) for name, p in zip(S.NAMES, placed)]
        opt = ClipAdamW(named, S.LR_MULTS, S.WEIGHT_DECAYS, betas=S.BETAS, eps=S.EPS, max_norm=max_norm)
        opt.grad_scale = grad_scale
        before = None
        for s in range(steps):
            opt.zero_grad()
            for (_, q), g in zip(named, grads[s]):
                q.grad.copy_(g)
            before = [q.detach().clone() for _, q in named]
            opt.step(S.lr_at(s))
        got = ([q.detach().cpu() for _, q in named], [t.cpu() for t in opt._slices(opt.exp_avg)], [t.cpu() for t in opt._slices(opt.exp_avg_sq)],
               [(q.detach() - x).cpu() for (_, q), x in zip(named, before)])
        S.check("placement", got, t64, b)
        assert all(p.untouched() for p in placed), "bytes beside a moved parameter were written"
        runs.append(got[0])
    assert all(torch.equal(a, c) for a, c in zip(*runs))
