"""K6 forms whose global loads were re-timed: the 3 x 3 convolution on a split image (operand loads in flight across the k block, out-of-image
taps zeroed where the operands are consumed) and the epilogues that fetch bias and residual for all column tiles at once.  Results are the
parent's, bit for bit: every case is held to the fp32-row form with torch.equal and to float64 at the bounds of tests/test_kernels_gpu.py.

Shapes: the smallest launches ops.conv3x3_takes_split accepts (256 tiles of 128 x 128: N = 256, 16 384 rows) with C = 32 / 64 (K = 288 / 576), in
geometries where the 32 rows of one wave span several image rows and two images, so that every combination of invalid taps occurs inside a wave.
Each case runs with the concurrent-streams hint 1 and 3: with 3 (and K >= 512) the launch takes the 256 x 128 form, otherwise the 128 x 128 one."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

N_CONV = 256
GEOMETRIES = [(4, 512, 8), (2, 64, 128), (1, 129, 127), (8, 2048, 1)]            # (B, H, W); (1, 129, 127): ragged M = 16 383
MOMENT_GEOMETRIES = [(4, 512, 8), (2, 64, 128), (8, 2048, 1)]                    # H W % 128 == 0: conv3x3_emits_gn_moments accepts them


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    from rba_amd import ops as o
    return o


@pytest.fixture(params=[1, 3], ids=["streams1", "streams3"])
def hint(request, ops):
    prev = ops.set_concurrent_streams(request.param)
    try:
        yield request.param
    finally:
        ops.set_concurrent_streams(prev)


def maxerr(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


@functools.lru_cache(maxsize=None)
def conv_case(B, H, W, C):
    """Inputs, the fp32-row result and the float64 reference of one geometry: computed once, shared by the tests below and never modified."""
    from rba_amd import ops
    g = torch.Generator().manual_seed(B * 1000 + H * W + C)
    x = torch.randn(B, H, W, C, generator=g)
    w = torch.randn(N_CONV, C, 3, 3, generator=g) * (9 * C) ** -0.5
    b = torch.randn(N_CONV, generator=g)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1).contiguous()
    xd, bd = x.cuda(), b.cuda()
    planes = ops.conv3x3_weight(w.cuda(), mode="f16x3")
    prev = ops.set_concurrent_streams(1)
    try:
        z32 = ops.conv3x3_nhwc(xd, planes, bd, out_features=N_CONV)              # the LDS-staged kernel on fp32 rows
    finally:
        ops.set_concurrent_streams(prev)
    return xd, planes, bd, z32, ref


def split_image(ops, x):
    B, H, W, C = x.shape
    return ops.SplitActivations(ops.SplitActivations.pack(x.reshape(B * H * W, C)).data, (B, H, W, C))


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("B,H,W", GEOMETRIES)
def test_conv3x3_split_image_border_geometries(ops, hint, B, H, W, C):
    x, planes, b, z32, ref = conv_case(B, H, W, C)
    assert ops.conv3x3_takes_split(B * H * W, N_CONV)
    zs = ops.conv3x3_nhwc(split_image(ops, x), planes, b, out_features=N_CONV)
    assert zs.shape == (B, H, W, N_CONV)
    err = maxerr(zs, ref)
    print(f"conv {B}x{H}x{W}x{C} hint {hint}: max |err| vs float64 {err:.3e}")
    assert err < 2e-5 * (9 * C / 256) ** 0.5 + 2e-6                             # test_conv3x3_nhwc_vs_fp64's bound
    assert torch.equal(zs, z32)                                                  # same products, same order as the fp32-row kernel


@pytest.mark.parametrize("C", [32, 64])
@pytest.mark.parametrize("B,H,W", MOMENT_GEOMETRIES)
def test_conv3x3_split_image_moment_form(ops, hint, B, H, W, C):
    G = 32
    x, planes, b, z32, _ = conv_case(B, H, W, C)
    assert ops.conv3x3_emits_gn_moments(B, H, W, N_CONV, G)
    xs = split_image(ops, x)
    y, mr = ops.conv3x3_nhwc_gn_stats(xs, planes, G, 1e-5, b, out_features=N_CONV)
    assert torch.equal(y, ops.conv3x3_nhwc(xs, planes, b, out_features=N_CONV)) and torch.equal(y, z32)
    yd = y.double().view(B, H * W, G, N_CONV // G)
    mean64, var64 = yd.mean(dim=(1, 3)), yd.var(dim=(1, 3), unbiased=False)
    e_mean = maxerr(mr[..., 0], mean64)
    e_rstd = ((mr[..., 1].double().cpu() * (var64 + 1e-5).sqrt().cpu()) - 1).abs().max().item()
    print(f"moments {B}x{H}x{W}x{C} hint {hint}: mean {e_mean:.3e} rstd {e_rstd:.3e}")
    assert mr.shape == (B, G, 2) and e_mean < 2e-6 and e_rstd < 2e-6             # test_conv3x3_with_gn_moments_epilogue's bounds


@pytest.mark.parametrize("B,H,W,where", [(4, 512, 8, (1, 0, 7)), (4, 512, 8, (3, 511, 0)), (2, 64, 128, (1, 63, 127)), (1, 129, 127, (0, 128, 126)),
                                         (1, 129, 127, (0, 64, 0)), (8, 2048, 1, (2, 0, 0)), (8, 2048, 1, (7, 2047, 0))])
def test_conv3x3_split_image_nan_reaches_its_neighbourhood_only(ops, hint, B, H, W, where):
    """A NaN in one pixel must come out in exactly the outputs whose 3 x 3 neighbourhood holds it (every channel of them): the deferred zeroing of the
    out-of-image taps neither lets a neighbour row of another image row / image leak in, nor drops a lane whose tap is inside."""
    C = 64
    x, planes, b, _, _ = conv_case(B, H, W, C)
    bi, yi, xi = where
    xn = x.clone()
    xn[bi, yi, xi, 5] = float("nan")
    hit = torch.zeros(B, 1, H, W)
    hit[bi, 0, yi, xi] = 1.0
    want = (F.conv2d(hit, torch.ones(1, 1, 3, 3), padding=1)[:, 0] > 0).cuda()  # [B, H, W]
    z = ops.conv3x3_nhwc(split_image(ops, xn), planes, b, out_features=N_CONV)
    nan = torch.isnan(z)
    assert torch.equal(nan.all(dim=-1), want) and torch.equal(nan.any(dim=-1), want)


M_EPI, K_EPI = 20480 + 5, 512                                                   # 161 row tiles: >= 160 tiles of 128 x 128 for N > 128, ragged M


@functools.lru_cache(maxsize=None)
def linear_case(N):
    g = torch.Generator().manual_seed(N + K_EPI)
    lin = torch.nn.Linear(K_EPI, N)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(N, K_EPI, generator=g) * K_EPI ** -0.5)
        lin.bias.copy_(torch.randn(N, generator=g))
    x, r = torch.randn(M_EPI, K_EPI, generator=g), torch.randn(M_EPI, N, generator=g)
    ref = F.linear(x.double(), lin.weight.detach().double(), lin.bias.detach().double())
    return lin.cuda().requires_grad_(False), x.cuda(), r.cuda(), ref


_first = {}                                                                      # (test, operand kind) -> result under the first hint that ran


def same_under_every_hint(key, out):
    """The 128 x 128 and 256 x 128 forms are held to each other bit for bit (test_split_linear_256x128_form_is_bit_identical)."""
    if key in _first:
        assert torch.equal(out, _first[key])
    else:
        _first[key] = out.clone()


def test_linear_bias_residual_epilogue(ops, hint):
    N = 128 + 8                                                                  # ragged N: the second column tile of every row tile is partial
    lin, x, r, ref = linear_case(N)
    assert ops.linear_residual_fused(M_EPI, N, K_EPI)
    want = ref + r.double().cpu()
    tol = 2e-5 * (K_EPI / 256) ** 0.5 + 2e-6                                     # the bound of the f16x3 Linear tests
    rows = ops.linear(x, lin, residual=r.clone())
    split = ops.linear(ops.SplitActivations.pack(x), lin, residual=r.clone())
    plain = ops.linear(ops.SplitActivations.pack(x), lin)
    e_rows, e_split, e_plain = maxerr(rows, want), maxerr(split, want), maxerr(plain, ref)
    print(f"linear + residual hint {hint}: rows {e_rows:.3e} split {e_split:.3e} plain {e_plain:.3e} (bound {tol:.3e})")
    assert e_rows < tol and e_split < tol and e_plain < tol
    assert torch.equal(split, rows)                                              # test_split_linear_from_split_activations
    same_under_every_hint(("res", "split"), split)
    same_under_every_hint(("plain", "split"), plain)


def test_linear_gelu_split_output_epilogue(ops, hint):
    N = 256
    lin, x, _, _ = linear_case(N)
    want = ops.SplitActivations.pack(ops.linear(x, lin, gelu=True))             # the fp32-row call
    nfull = M_EPI // 32 * 32 * N
    for kind, xin in (("rows", x), ("split", ops.SplitActivations.pack(x))):
        got = ops.linear(xin, lin, gelu=True, split_out=True)
        assert got.shape == (M_EPI, N) and torch.equal(got.unpack(), want.unpack()) and torch.equal(got.data[:nfull], want.data[:nfull])
        same_under_every_hint(("fc1", kind), got.unpack())
