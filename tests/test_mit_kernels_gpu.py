"""GPU: K19a / K19b / K19c (rba_amd.mit_ops, csrc/mit_attn.hip, csrc/mit_conv.hip) -- the spatial-reduction attention core against float64, the
depthwise 3x3 + GELU against its float64 composition (held to torch's own fp32 error), the im2col gather against F.unfold exactly; bitwise
reproducibility, the wrappers' refusals, graph capture.  Inputs and truths come from tests/_mit_cases.py."""
import pytest
import torch

from tests import _mit_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run rba_amd.mit_ops' allocations under the guard bands too"""
    import rba_amd.mit_ops as mops
    if canary is None:
        yield
        return
    real, mops.torch = mops.torch, canary._PROXY
    try:
        yield
    finally:
        mops.torch = real


# ---------------------------------------------------------------------------------------------------------------- K19a
@pytest.mark.parametrize("nH", C.ATTN_HEADS)
@pytest.mark.parametrize("hd", C.ATTN_HEAD_DIMS)
def test_sr_attention_against_float64(hd, nH):
    from rba_amd import mit_ops
    worst = 0.0
    for B in C.ATTN_BATCHES:
        for N in C.ATTN_N:
            for S in C.ATTN_S:
                q, kv = C.attn_case(B, N, S, nH, hd)
                want = C.attn_truth(q, kv, nH)
                qd, kvd = q.cuda(), kv.cuda()
                got = mit_ops.sr_attention(qd, kvd, nH)
                again = mit_ops.sr_attention(qd, kvd, nH)
                assert got.shape == (B, N, nH * hd) and got.dtype == torch.float32
                assert torch.equal(got, again), f"two launches differ at B={B} N={N} S={S}"
                err = (got.cpu().double() - want).abs().max().item()
                worst = max(worst, err)
                assert err <= C.ATTN_BOUND, f"hd={hd} nH={nH} B={B} N={N} S={S}: max abs error {err:.3g} > {C.ATTN_BOUND}"
    print(f"K19a hd={hd} nH={nH}: worst max abs error {worst:.3g} (bound {C.ATTN_BOUND})")


def test_sr_attention_takes_an_explicit_scale():
    from rba_amd import mit_ops
    q, kv = C.attn_case(1, 65, 63, 2, 32, seed=3)
    got = mit_ops.sr_attention((q * 2.0).cuda(), kv.cuda(), 2, scale=0.5 * 32 ** -0.5)
    assert (got.cpu().double() - C.attn_truth(q, kv, 2)).abs().max().item() <= C.ATTN_BOUND


# ---------------------------------------------------------------------------------------------------------------- K19b
@pytest.mark.parametrize("Cn", C.DW_CHANNELS)
def test_dwconv3x3_gelu_against_the_float64_composition(Cn):
    from rba_amd import mit_ops
    for B in C.DW_BATCHES:
        for H, W in C.DW_MAPS:
            x, weight, bias = C.dwconv_case(B, H, W, Cn)
            want = C.dwconv_compose(x.double(), weight, bias, H, W)
            err_torch32 = (C.dwconv_compose(x, weight, bias, H, W).double() - want).abs().max().item()
            got = mit_ops.dwconv3x3_gelu(x.cuda(), mit_ops.dwconv_taps(weight).cuda(), bias.cuda(), H, W)
            err = (got.cpu().double() - want).abs().max().item()
            bound = 4 * err_torch32 + 4 * 2.0 ** -23 * want.abs().max().item()
            print(f"K19b C={Cn} B={B} {H}x{W}: err {err:.3g}, torch fp32 err {err_torch32:.3g}, bound {bound:.3g}")
            assert err <= bound
            if B > 1:                      # image 0 alone gives the same bits: nothing of image 1 (a constant 1e3) reached it
                alone = mit_ops.dwconv3x3_gelu(x[:1].cuda(), mit_ops.dwconv_taps(weight).cuda(), bias.cuda(), H, W)
                assert torch.equal(got[:1], alone)


# ---------------------------------------------------------------------------------------------------------------- K19c
@pytest.mark.parametrize("k,stride,pad", C.IM2COL_WINDOWS)
def test_im2col_equals_unfold(k, stride, pad):
    from rba_amd import mit_ops
    for B in C.IM2COL_BATCHES:
        for H, W in C.IM2COL_MAPS:
            for Cn in C.IM2COL_CHANNELS:
                x = C.im2col_case(B, H, W, Cn)
                Kp = mit_ops.padded_columns(k, Cn)
                want = C.im2col_reference(x, k, stride, pad, Kp)
                if Cn == 3:
                    assert k != 7 or Kp == 160
                    cols, Ho, Wo = mit_ops.im2col_nhwc(x.cuda(), H, W, k, stride, pad, nchw_in=True)
                else:
                    tokens = x.permute(0, 2, 3, 1).reshape(B, H * W, Cn).contiguous()
                    cols, Ho, Wo = mit_ops.im2col_nhwc(tokens.cuda(), H, W, k, stride, pad)
                where = f"k={k} s={stride} p={pad} B={B} {H}x{W} C={Cn}"
                assert (Ho, Wo) == (mit_ops.conv_out_size(H, k, stride, pad), mit_ops.conv_out_size(W, k, stride, pad)), where
                assert tuple(cols.shape) == tuple(want.shape) == (B, Ho * Wo, Kp), where
                assert torch.equal(cols.cpu(), want), where
                assert not bool(cols[..., k * k * Cn:].any()), where + ": padded columns"


@pytest.mark.parametrize("k,stride,pad", [(3, 2, 1), (2, 2, 0)])
def test_im2col_element_path_on_channels_last_tokens(k, stride, pad):
    """the third path of K19c: channels-last input that is not one 16-byte load per four columns -- C % 4 != 0, and a C % 4 == 0 token tensor that lies
    4, 8 or 12 bytes off a 16-byte boundary"""
    from rba_amd import mit_ops
    B, H, W = 2, 5, 7
    for Cn in (6, 1, 32):
        x = C.im2col_case(B, H, W, Cn, seed=1)
        tokens = x.permute(0, 2, 3, 1).reshape(B, H * W, Cn).contiguous()
        want = C.im2col_reference(x, k, stride, pad, mit_ops.padded_columns(k, Cn))
        for off in ((0,) if Cn % 4 else (1, 2, 3)):
            buf = torch.full((tokens.numel() + 8,), float("nan"), device="cuda")
            placed = buf[off:off + tokens.numel()].view(B, H * W, Cn)
            placed.copy_(tokens)
            assert placed.data_ptr() % 16 == 4 * off and placed.is_contiguous()
            cols, Ho, Wo = mit_ops.im2col_nhwc(placed, H, W, k, stride, pad)
            assert torch.equal(cols.cpu(), want), f"C={Cn}, {4 * off} bytes off"


def test_conv_as_im2col_and_linear_weight():
    """the two repacks agree with the kernels' orders: cols @ conv_linear_weight^T is the convolution, w9 is tap-major"""
    from rba_amd import mit_ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 32, 16, 24, generator=g)
    w = torch.randn(48, 32, 3, 3, generator=g)
    want = torch.nn.functional.conv2d(x.double(), w.double(), stride=2, padding=1).flatten(2).transpose(1, 2)
    cols, Ho, Wo = mit_ops.im2col_nhwc(x.permute(0, 2, 3, 1).reshape(2, 384, 32).contiguous().cuda(), 16, 24, 3, 2, 1)
    got = cols.cpu().double() @ mit_ops.conv_linear_weight(w).double().t()
    assert (Ho, Wo) == (8, 12) and (got - want).abs().max().item() < 1e-12
    dw = torch.randn(8, 1, 3, 3, generator=g)
    assert torch.equal(mit_ops.dwconv_taps(dw)[5], dw[:, 0, 1, 2])


# ---------------------------------------------------------------------------------------------------------------- refusals, graphs
class _Reached(Exception):
    pass


def test_one_fault_is_refused_before_anything_is_allocated_or_launched(monkeypatch):
    from rba_amd import mit_ops
    from rba_amd._lib import RbaHipError

    def reached(name, *args, **kw):
        raise _Reached(name)
    monkeypatch.setattr(mit_ops, "_launch", reached)

    def z(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device="cuda")
    rows = []

    def wrapper(fn, **good):
        rows.append((f"{fn.__name__}: well-formed", lambda: fn(**good), True))

        def add(clause, **bad):
            rows.append((f"{fn.__name__}: {clause}", lambda: fn(**{**good, **bad}), False))
        return add

    add = wrapper(mit_ops.sr_attention, q=z(2, 5, 64), kv=z(2, 3, 128), num_heads=2)
    add("head_dim 16", num_heads=4)
    add("head_dim 128", q=z(2, 5, 128), kv=z(2, 3, 256), num_heads=1)
    add("heads that do not divide C", num_heads=3)
    add("no heads", num_heads=0)
    add("kv of another width", kv=z(2, 3, 64))
    add("kv of another batch", kv=z(1, 3, 128))
    add("no keys", kv=z(2, 0, 128))
    add("no queries", q=z(2, 0, 64))
    add("q of another dtype", q=z(2, 5, 64, dtype=torch.float64))
    add("q not contiguous", q=z(2, 5, 128)[:, :, ::2])
    add("q of rank 2", q=z(10, 64))
    add("q on the CPU", q=torch.zeros(2, 5, 64))
    add("kv of another dtype", kv=z(2, 3, 128, dtype=torch.float16))
    add("kv not contiguous", kv=z(2, 3, 256)[:, :, ::2])
    add("kv on the CPU", kv=torch.zeros(2, 3, 128))
    add = wrapper(mit_ops.dwconv3x3_gelu, x=z(2, 6, 8), w9=z(9, 8), bias=z(8), H=2, W=3)
    add("C % 4 != 0", x=z(2, 6, 6), w9=z(9, 6), bias=z(6))
    add("a map of another size", H=3)
    add("an empty map", x=z(2, 0, 8), H=0)
    add("w9 in the convolution's own layout", w9=z(8, 1, 3, 3))
    add("w9 of another width", w9=z(9, 4))
    add("bias too short", bias=z(4))
    add("x of another dtype", x=z(2, 6, 8, dtype=torch.float64))
    add("x not contiguous", x=z(2, 6, 16)[:, :, ::2])
    add("x of rank 4", x=z(2, 2, 3, 8))
    add("x on the CPU", x=torch.zeros(2, 6, 8))
    add("w9 on the CPU", w9=torch.zeros(9, 8))
    add("bias on the CPU", bias=torch.zeros(8))
    add = wrapper(mit_ops.im2col_nhwc, x=z(2, 6, 8), H=2, W=3, k=3, stride=2, pad=1)
    add("k = 0", k=0)
    add("k = 65", k=65, pad=0)
    add("stride 0", stride=0)
    add("pad = k", pad=3)
    add("negative pad", pad=-1)
    add("a map of another size", W=4)
    add("x of another dtype", x=z(2, 6, 8, dtype=torch.float16))
    add("x not contiguous", x=z(2, 6, 16)[:, :, ::2])
    add("x on the CPU", x=torch.zeros(2, 6, 8))
    add("tokens where the image batch is announced", nchw_in=True)
    add("an image batch of another size", x=z(2, 3, 4, 3), nchw_in=True)

    wrong = []
    for name, call, well_formed in rows:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        try:
            call()
            outcome = "returned"
        except RbaHipError:
            outcome = "refused"
        except _Reached as e:
            outcome = f"reached {e}"
        except Exception as e:                                           # noqa: BLE001 -- the table reports every row, whatever it ran into
            outcome = f"{type(e).__name__}: {e}"
        grew = torch.cuda.memory_allocated() - before
        if not (outcome.startswith("reached") if well_formed else (outcome == "refused" and grew == 0)):
            wrong.append(f"{name}: {outcome}, {grew} bytes allocated")
    assert len(rows) >= 40 and not wrong, "\n".join(wrong)


def test_each_wrapper_is_capturable_and_replays_on_new_inputs():
    from rba_amd import mit_ops
    nH, hd, H, W = 2, 32, 5, 9
    attn = [C.attn_case(2, 65, 63, nH, hd, seed=s) for s in (0, 1, 2)]
    dw = [C.dwconv_case(2, H, W, 132, seed=s) for s in (0, 1, 2)]
    im = [C.im2col_case(2, H, W, 32, seed=s).permute(0, 2, 3, 1).reshape(2, H * W, 32).contiguous() for s in (0, 1, 2)]
    eager = []
    for (q, kv), (x, weight, bias), t in zip(attn, dw, im):
        eager.append((mit_ops.sr_attention(q.cuda(), kv.cuda(), nH),
                      mit_ops.dwconv3x3_gelu(x.cuda(), mit_ops.dwconv_taps(weight).cuda(), bias.cuda(), H, W),
                      mit_ops.im2col_nhwc(t.cuda(), H, W, 3, 2, 1)[0]))
    q, kv = attn[0][0].cuda(), attn[0][1].cuda()
    x, w9, bias = dw[0][0].cuda(), mit_ops.dwconv_taps(dw[0][1]).cuda(), dw[0][2].cuda()
    t = im[0].cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = (mit_ops.sr_attention(q, kv, nH), mit_ops.dwconv3x3_gelu(x, w9, bias, H, W), mit_ops.im2col_nhwc(t, H, W, 3, 2, 1)[0])
    for i in (1, 2, 0):
        q.copy_(attn[i][0]), kv.copy_(attn[i][1]), x.copy_(dw[i][0]), w9.copy_(mit_ops.dwconv_taps(dw[i][1])), bias.copy_(dw[i][2]), t.copy_(im[i])
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(out, eager[i])), f"replay on case {i}"
