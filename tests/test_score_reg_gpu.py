"""K11b on the GPU: ops.score_reg / ops.score_reg_backward against fp64 CPU torch -- the restatements of the reference's criterion.py:270-279 and
:311-319 in tests/_pebal_cases.py.  Bars (tests/_rba_bwd_cases.py, tests/_point_loss_cases.py): e <= 4 max(b, 2^-20) per tensor, b = fp32 CPU
autograd's error; |l - l64| <= 4 max(|l32 - l64|, 2^-20 |l64|) per scalar."""
import pytest
import torch

from tests import _pebal_cases as G
from tests import _point_loss_cases as P
from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

_id = lambda s: "x".join(map(str, s))


def _poison():
    for n in (1 << 10, 1 << 16, 1 << 20):
        torch.full((n,), float("nan"), device="cuda")
    torch.cuda.synchronize()


def _check_grad(what, g, g64, b):
    if float(g64.abs().max()) == 0.0:
        assert not g.any(), what                             # a zero gradient is exactly zero
    else:
        C.check(what, g.cpu(), g64, b)


@pytest.mark.parametrize("shape", G.REG_SHAPES + G.REG_LAP_SHAPES, ids=_id)
def test_kernel_against_fp64(shape):
    from rba_amd import ops
    score, labels = G.reg_inputs(shape)
    t = G.reg_truth(shape)
    sd, ld = score.cuda(), labels.cuda()
    _poison()
    losses, stats = ops.score_reg(sd, ld)
    assert losses.shape == (2,) and stats.shape == (2,)
    P.check_scalar("smoothness", losses[0], t["sm32"], t["sm64"])
    P.check_scalar("sparsity", losses[1], t["sp32"], t["sp64"])
    P.check_scalar("sum of squared differences", stats[0], 2 * t["sm32"], 2 * t["sm64"])
    P.check_scalar("sum of squared samples", stats[1], t["sp32"] ** 2, t["sp64"] ** 2)
    for up in G.REG_UPSTREAM:
        for scale in (1.0, 2.0 ** -20):
            _poison()
            gsm, gsp = (torch.full((), u * scale, device="cuda") for u in up)
            g = ops.score_reg_backward(sd, ld, stats, gsm, gsp)
            assert g.shape == score.shape
            _check_grad(f"grad_score (upstream {up} x {scale:g})", g / scale, t["g64"][up], t["b"][up])
    # one upstream gradient absent = that gradient 0
    assert torch.equal(ops.score_reg_backward(sd, ld, stats, torch.ones((), device="cuda"), None),
                       ops.score_reg_backward(sd, ld, stats, torch.ones((), device="cuda"), torch.zeros((), device="cuda")))
    assert torch.equal(ops.score_reg_backward(sd, ld, stats, None, torch.ones((), device="cuda")),
                       ops.score_reg_backward(sd, ld, stats, torch.zeros((), device="cuda"), torch.ones((), device="cuda")))


@pytest.mark.parametrize("shape", G.REG_SHAPES[:3], ids=_id)
def test_no_outlier_pixel_and_no_labels_give_sparsity_zero_with_a_zero_gradient(shape):
    from rba_amd import ops
    score, labels = G.reg_inputs(shape)
    t = G.reg_truth(shape, labelled=False)
    none = labels.clone()
    none[labels == 1] = 0
    sd, one, zero = score.cuda(), torch.ones((), device="cuda"), torch.zeros((), device="cuda")
    for lab in (none.cuda(), none.to(torch.uint8).cuda(), None):
        _poison()
        losses, stats = ops.score_reg(sd, lab)
        P.check_scalar("smoothness", losses[0], t["sm32"], t["sm64"])
        assert float(losses[1]) == 0.0 and float(stats[1]) == 0.0
        assert not ops.score_reg_backward(sd, lab, stats, zero, one).any()
        g = ops.score_reg_backward(sd, lab, stats, one, one)
        _check_grad("grad_score", g, t["g64"][(1.0, 0.0)], t["b"][(1.0, 0.0)])


def test_uint8_labels_give_the_bits_of_int64_labels_and_two_runs_agree():
    from rba_amd import ops
    one = torch.ones((), device="cuda")
    for shape in G.REG_SHAPES:
        score, labels = G.reg_inputs(shape)
        sd = score.cuda()
        runs = []
        for lab in (labels.cuda(), labels.cuda(), labels.to(torch.uint8).cuda()):
            _poison()
            losses, stats = ops.score_reg(sd, lab)
            runs.append((losses, stats, ops.score_reg_backward(sd, lab, stats, one, one)))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert torch.equal(a, b), shape


def test_score_reg_function_takes_each_upstream_gradient():
    """ScoreRegFunction: the smoothness output alone, the sparsity output alone, and a weighted sum of both"""
    from rba_amd.modeling.criterion import ScoreRegFunction
    shape = G.REG_SHAPES[0]
    score, labels = G.reg_inputs(shape)
    t = G.reg_truth(shape)
    for up in G.REG_UPSTREAM:
        s = score.cuda().requires_grad_(True)
        smooth, sparse = ScoreRegFunction.apply(s, labels.cuda())
        (smooth if up == (1.0, 0.0) else sparse if up == (0.0, 1.0) else up[0] * smooth + up[1] * sparse).backward()
        C.check(f"d / d score (upstream {up})", s.grad.cpu(), t["g64"][up], t["b"][up])
    s = score.cuda()                                                 # nobody asks for a gradient: none is computed
    assert ScoreRegFunction.apply(s, labels.cuda())[0].grad_fn is None


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    s, l, stats, one = z(1, 2, 2), z(1, 4, 4, dtype=torch.int64), z(2), torch.ones((), device="cuda")
    for bad in (dict(score=s.cpu()), dict(labels=l.cpu()), dict(score=s.double()), dict(labels=l.int()), dict(score=s[0]), dict(labels=l[0]),
                dict(labels=z(2, 4, 4, dtype=torch.int64)), dict(score=z(1, 2, 4)[..., ::2]), dict(score=z(1, 0, 2))):
        a = {"score": s, "labels": l, **bad}
        with pytest.raises(RbaHipError):
            ops.score_reg(a["score"], a["labels"])
        with pytest.raises(RbaHipError):
            ops.score_reg_backward(a["score"], a["labels"], stats, one, one)
    for bad in (dict(stats=z(4)), dict(stats=stats.cpu()), dict(gsm=torch.ones(2, device="cuda")), dict(gsp=one.cpu()), dict(gsm=None, gsp=None)):
        a = {"stats": stats, "gsm": one, "gsp": one, **bad}
        with pytest.raises(RbaHipError):
            ops.score_reg_backward(s, l, a["stats"], a["gsm"], a["gsp"])
