"""The blur of B planes and its adjoint (ops.gaussian_blur_planes / ops.gaussian_blur_planes_adjoint, csrc/pebal_loss.hip) against the fp64
restatement of torchvision's GaussianBlur(7, sigma=1) in tests/_pebal_cases.py and fp64 autograd of it.  Bar: e <= 4 max(b, 2^-20), b = the fp32
restatement's error."""
import pytest
import torch

from tests import _pebal_cases as G
from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

_id = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("shape", G.BLUR_SHAPES, ids=_id)
def test_forward_and_adjoint_against_fp64(shape):
    from rba_amd import ops
    u, v = G.blur_inputs(shape)
    t = G.blur_truth(shape)
    for n in (1 << 10, 1 << 16):
        torch.full((n,), float("nan"), device="cuda")                # poisoned allocations
    y = ops.gaussian_blur_planes(u.cuda())
    g = ops.gaussian_blur_planes_adjoint(v.cuda())
    assert y.shape == u.shape and g.shape == v.shape
    C.check("A u", y.cpu(), t["y64"], t["b_y"])
    C.check("A^T v", g.cpu(), t["g64"], t["b_g"])
    # <A u, v> = <u, A^T v>, in fp64 of the fp32 outputs: each side is within the bar of its truth, so the two agree to the sum of the bars
    lhs, rhs = float((y.cpu().double() * v.double()).sum()), float((u.double() * g.cpu().double()).sum())
    scale = float(t["y64"].abs().max() * v.abs().sum() + u.abs().sum() * t["g64"].abs().max())
    print(f"<A u, v> = {lhs:.9g}  <u, A^T v> = {rhs:.9g}")
    assert abs(lhs - rhs) <= (C.bar(t["b_y"]) + C.bar(t["b_g"])) * scale
    assert torch.equal(ops.gaussian_blur_planes_adjoint(v.cuda()), g)


def test_the_adjoint_is_not_the_blur_near_a_border():
    """the fixture separates the two: applying the blur to the cotangent misses the bar by orders of magnitude"""
    shape = G.BLUR_SHAPES[1]
    _, v = G.blur_inputs(shape)
    t = G.blur_truth(shape)
    assert C.err(G.ref_blur(v.double()), t["g64"]) > 100 * C.bar(t["b_g"])


@pytest.mark.parametrize("shape", ((4, 4), (7, 70), (64, 128), (33, 65)), ids=_id)
def test_one_plane_gives_the_bits_of_gaussian_blur(shape):
    from rba_amd import ops
    gen = torch.Generator().manual_seed(11350)
    x = torch.randn(*shape, generator=gen).cuda()
    assert torch.equal(ops.gaussian_blur_planes(x[None])[0], ops.gaussian_blur(x))
    two = torch.stack([x, x.flip(0)])
    out = ops.gaussian_blur_planes(two)
    assert torch.equal(out[0], ops.gaussian_blur(x)) and torch.equal(out[1], ops.gaussian_blur(x.flip(0).contiguous()))


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    x = torch.zeros(1, 4, 4, device="cuda")
    for fn in (ops.gaussian_blur_planes, ops.gaussian_blur_planes_adjoint):
        for bad in (x.cpu(), x.double(), x[0], torch.zeros(1, 3, 4, device="cuda"), torch.zeros(1, 4, 8, device="cuda")[..., ::2]):
            with pytest.raises(RbaHipError):
                fn(bad)
        with pytest.raises(RbaHipError):
            fn(x, kernel_size=6)
        with pytest.raises(RbaHipError):
            fn(x, kernel_size=9)                                     # padding 4 >= size 4
        with pytest.raises(RbaHipError):
            fn(x, sigma=0.0)
