"""K11a on the GPU: ops.gambler_loss / ops.gambler_loss_backward against fp64 CPU torch -- the restatement of the reference's criterion.py:323-388
in tests/_pebal_cases.py -- and criterion.gambler_loss end to end, without a read-back.  Bars (tests/_rba_bwd_cases.py, tests/_point_loss_cases.py):
e(T) = max|T - T64| / max|T64| <= 4 max(b, 2^-20) per tensor, b = fp32 CPU autograd's error on the same inputs;
|l - l64| <= 4 max(|l32 - l64|, 2^-20 |l64|) per scalar; counts exact."""
import pytest
import torch
import torch.nn.functional as F

from tests import _pebal_cases as G
from tests import _point_loss_cases as P
from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

UPSTREAM = (1.0, 2.0 ** -20)
_id = lambda s: "x".join(map(str, s))


def _poison():
    """the allocator's next blocks hold NaN: a workspace or output word that is read before it is written shows"""
    for n in (1 << 10, 1 << 16, 1 << 20):
        torch.full((n,), float("nan"), device="cuda")
    torch.cuda.synchronize()


def _check_forward(losses, stats, R, t):
    p32, p64 = t["parts32"], t["parts64"]
    P.check_scalar("loss", losses[0], t["l32"], t["l64"])
    P.check_scalar("in-mean", losses[1], p32["in_mean"], p64["in_mean"])
    P.check_scalar("out-mean", losses[2], p32["out_mean"], p64["out_mean"])
    P.check_scalar("S_in", stats[0], p32["S_in"], p64["S_in"])
    P.check_scalar("S_out", stats[1], p32["S_out"], p64["S_out"])
    assert float(stats[2]) == p64["n_in"] and float(stats[3]) == p64["n_ood"]
    C.check("R", R.cpu(), p64["R"], C.err(p32["R"], p64["R"]))


@pytest.mark.parametrize("shape", G.TAIL_SHAPES + G.LAP_SHAPES + G.FOUND_SHAPES, ids=_id)
def test_kernel_against_fp64(shape):
    from rba_amd import ops
    sem, labels = G.tail_inputs(shape)
    t = G.tail_truth(shape)
    sd, ld = sem.cuda(), labels.cuda()
    _poison()
    losses, stats, R = ops.gambler_loss(sd, ld, G.OOD_REG)
    assert losses.shape == (3,) and stats.shape == (4,) and R.shape == labels.shape
    _check_forward(losses, stats, R, t)
    if shape == (1, 2, 9, 7, 5, 6):
        assert int((t["g64"] == 0).sum()) > 0                       # down-sampling: pixels nobody samples
    for up in UPSTREAM:
        _poison()
        g = ops.gambler_loss_backward(sd, ld, stats, R, torch.full((), up, device="cuda"), G.OOD_REG)
        assert g.shape == sem.shape
        C.check(f"grad_sem (upstream {up:g})", g.cpu() / up, t["g64"], t["b"])             # 2^-20: an exact scaling
        assert not g.cpu()[t["g64"] == 0].any()


def test_uint8_labels_give_the_bits_of_int64_labels_and_two_runs_agree():
    from rba_amd import ops
    one = torch.ones((), device="cuda")
    for shape in G.TAIL_SHAPES[:4] + G.TAIL_SHAPES[-2:]:
        sem, labels = G.tail_inputs(shape)
        sd = sem.cuda()
        runs = []
        for lab in (labels.cuda(), labels.cuda(), labels.to(torch.uint8).cuda()):
            _poison()
            losses, stats, R = ops.gambler_loss(sd, lab, G.OOD_REG)
            runs.append((losses, stats, R, ops.gambler_loss_backward(sd, lab, stats, R, one, G.OOD_REG)))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert torch.equal(a, b), shape


def test_no_outlier_pixel_is_the_else_branch_and_no_inlier_pixel_is_nan():
    from rba_amd import ops
    sem, labels = G.tail_inputs(G.TAIL_SHAPES[0])
    K = sem.shape[1] - 1
    none = labels.clone()
    none[labels == G.OUTLIER] = 255
    s64 = sem.double().clone().requires_grad_(True)
    l64, p64 = G.ref_gambler_tail(s64, none)
    l64.backward()
    s32 = sem.clone().requires_grad_(True)
    l32, p32 = G.ref_gambler_tail(s32, none)
    l32.backward()
    assert p64["n_ood"] == 0
    losses, stats, R = ops.gambler_loss(sem.cuda(), none.cuda(), G.OOD_REG)
    t = {"l32": l32.detach(), "l64": l64.detach(), "parts32": {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in p32.items()},
         "parts64": {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in p64.items()}}
    _check_forward(losses, stats, R, t)
    assert float(losses[2]) == 0.0 and float(stats[1]) == 0.0 and float(stats[3]) == 0.0
    g = ops.gambler_loss_backward(sem.cuda(), none.cuda(), stats, R, torch.ones((), device="cuda"), G.OOD_REG)
    C.check("grad_sem without outliers", g.cpu(), s64.grad, C.err(s32.grad, s64.grad))
    only_out = labels.clone()
    only_out[labels < K] = 255
    losses, stats, _ = ops.gambler_loss(sem.cuda(), only_out.cuda(), G.OOD_REG)
    assert torch.isnan(losses[0]) and torch.isnan(losses[1]) and float(stats[2]) == 0.0 and float(stats[3]) > 0 and torch.isfinite(losses[2])


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    s, l = z(1, 4, 2, 2), z(1, 4, 4, dtype=torch.int64)
    stats, R, one = z(4), z(1, 4, 4), torch.ones((), device="cuda")
    for bad in (dict(sem=s.cpu()), dict(labels=l.cpu()), dict(sem=s.double()), dict(labels=l.int()), dict(labels=l.float()), dict(sem=s[0]),
                dict(labels=l[0]), dict(labels=z(2, 4, 4, dtype=torch.int64)), dict(sem=z(1, 33, 2, 2)), dict(sem=z(1, 1, 2, 2)),
                dict(labels=z(1, 3, 4, dtype=torch.int64)), dict(labels=z(1, 4, 3, dtype=torch.int64)),
                dict(sem=z(1, 4, 2, 4)[..., ::2]), dict(labels=z(1, 4, 8, dtype=torch.int64)[..., ::2])):
        a = {"sem": s, "labels": l, **bad}
        with pytest.raises(RbaHipError):
            ops.gambler_loss(a["sem"], a["labels"], G.OOD_REG)
        with pytest.raises(RbaHipError):
            ops.gambler_loss_backward(a["sem"], a["labels"], stats, R, one, G.OOD_REG)
    for bad in (dict(stats=z(8)), dict(stats=stats.cpu()), dict(R=z(1, 4, 5)), dict(R=R.cpu()), dict(grad_loss=torch.ones(2, device="cuda")),
                dict(grad_loss=one.cpu())):
        a = {"stats": stats, "R": R, "grad_loss": one, **bad}
        with pytest.raises(RbaHipError):
            ops.gambler_loss_backward(s, l, a["stats"], a["R"], a["grad_loss"], G.OOD_REG)


# ---------------------------------------------------------------------------------------------------------------- criterion.gambler_loss
def _outputs(shape, dtype=torch.int64):
    logits, masks, om, ss = G.loss_inputs(shape)
    leaves = [t.cuda().requires_grad_(True) for t in (logits, masks)]
    targets = [{"outlier_masks": o.to(dtype).cuda(), "sem_seg": s.to(dtype).cuda()} for o, s in zip(om, ss)]
    return leaves, {"pred_logits": leaves[0], "pred_masks": leaves[1]}, targets


@pytest.mark.parametrize("shape", sorted(G.LOSS_SHAPES))
def test_gambler_loss_against_fp64(shape):
    from rba_amd.modeling.criterion import gambler_loss
    K = G.LOSS_SHAPES[shape][2]
    leaves, outputs, targets = _outputs(shape)
    before = [{k: v.clone() for k, v in t.items()} for t in targets]
    t = G.loss_truth(shape)
    loss = gambler_loss(outputs, targets, num_classes=K, ood_reg=G.OOD_REG)["gambler_loss"]
    assert loss.dim() == 0
    P.check_scalar("gambler_loss", loss, t["l32"], t["l64"])
    loss.backward()
    assert leaves[0].grad.shape[-1] == K + 1 and bool(leaves[0].grad[..., -1].any())          # the no-object column has a gradient of its own
    for name, leaf, g64, b in zip(("pred_logits", "pred_masks"), leaves, t["g64"], t["b"]):
        C.check("d / d " + name, leaf.grad.cpu(), g64, b)
    for tgt, b4 in zip(targets, before):
        assert all(torch.equal(tgt[k], b4[k]) for k in tgt)                                  # the targets are not written
    with pytest.raises(ValueError):
        gambler_loss(outputs, targets, num_classes=K + 1)


def test_other_target_dtypes_are_reduced_on_the_device():
    """float / int32 / uint8 targets = the same targets as int64: the result's bits, loss and gradients"""
    from rba_amd.modeling.criterion import gambler_loss
    K = G.LOSS_SHAPES["small"][2]
    want = None
    for dtype in (torch.int64, torch.float32, torch.int32, torch.uint8):
        leaves, outputs, targets = _outputs("small", dtype)
        before = [{k: v.clone() for k, v in t.items()} for t in targets]
        loss = gambler_loss(outputs, targets, num_classes=K)["gambler_loss"]
        loss.backward()
        got = [loss.detach()] + [leaf.grad for leaf in leaves]
        want = got if want is None else want
        for a, b in zip(got, want):
            assert torch.equal(a, b), dtype
        for tgt, b4 in zip(targets, before):
            assert all(tgt[k].dtype == dtype and torch.equal(tgt[k], b4[k]) for k in tgt)


def test_gambler_loss_makes_no_read_back_and_no_torch_tail(monkeypatch):
    """The construction of test_densehybrid_loss_makes_no_read_back_and_no_torch_tail: forward and backward on the "small" fixture, after a warm
    call, with the Python-visible read-back entry points -- Tensor.item / .cpu / .tolist / .__bool__, torch.nonzero -- and the torch functions
    the kernels replace -- F.interpolate, torch.logsumexp, F.conv2d, F.pad, and softmax of anything with more than three dimensions (a map) --
    patched to raise.  The [B,Q,K+1] class softmax in front of K1 is torch and passes."""
    from rba_amd.modeling.criterion import gambler_loss
    K = G.LOSS_SHAPES["small"][2]
    leaves, outputs, targets = _outputs("small")
    gambler_loss(outputs, targets, num_classes=K)["gambler_loss"].backward()                 # warm: workspaces exist
    for leaf in leaves:
        leaf.grad = None
    torch.cuda.synchronize()

    def refuse(name):
        def raiser(*a, **k):
            raise AssertionError(f"call of {name}")
        return raiser

    for name in ("item", "cpu", "tolist", "__bool__", "logsumexp"):
        monkeypatch.setattr(torch.Tensor, name, refuse("Tensor." + name))
    tensor_softmax = torch.Tensor.softmax

    def class_softmax_only(self, *a, **k):                   # F.softmax ends here too
        assert self.dim() <= 3, f"softmax of a map {tuple(self.shape)}"
        return tensor_softmax(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "softmax", class_softmax_only)
    monkeypatch.setattr(torch, "nonzero", refuse("torch.nonzero"))
    monkeypatch.setattr(torch, "logsumexp", refuse("torch.logsumexp"))
    for name in ("interpolate", "conv2d", "pad"):
        monkeypatch.setattr(F, name, refuse("F." + name))
    gambler_loss(outputs, targets, num_classes=K)["gambler_loss"].backward()
    monkeypatch.undo()
    assert all(torch.isfinite(leaf.grad).all() and bool(leaf.grad.any()) for leaf in leaves)
