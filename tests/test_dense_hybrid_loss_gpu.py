"""K10 on the GPU: ops.dense_hybrid_loss / ops.dense_hybrid_loss_backward against fp64 CPU torch -- the restatement of the reference's
criterion.py:390-433 in tests/_dense_hybrid_cases.py -- and criterion.densehybrid_loss end to end, without a read-back.  Bars (tests/_rba_bwd_cases.py,
tests/_point_loss_cases.py): e(T) = max|T - T64| / max|T64| <= 4 max(b, 2^-20) per tensor, b = fp32 CPU autograd's error on the same inputs;
|l - l64| <= 4 max(|l32 - l64|, 2^-20 |l64|) per scalar; counts exact."""
import pytest
import torch
import torch.nn.functional as F

from tests import _dense_hybrid_cases as D
from tests import _point_loss_cases as P
from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

UPSTREAM = (1.0, 2.0 ** -20)
STATS = ("S_seg", "S_ood", "S_th", "S_x", "n_seg", "n_ood", "n_all", "m")
_id = lambda s: "x".join(map(str, s))


def _poison():
    """the allocator's next blocks hold NaN: a workspace or output word that is read before it is written shows"""
    for n in (1 << 10, 1 << 16, 1 << 20):
        torch.full((n,), float("nan"), device="cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("shape", D.TAIL_SHAPES + D.LAP_SHAPES + D.FOUND_SHAPES, ids=_id)
def test_kernel_against_fp64(shape):
    from rba_amd import ops
    sem, ood, labels = D.tail_inputs(shape)
    t = D.tail_truth(shape)
    sd, od, ld = sem.cuda(), ood.cuda(), labels.cuda()
    _poison()
    losses, stats, lse = ops.dense_hybrid_loss(sd, od, ld, D.BETA)
    assert losses.shape == (4,) and stats.shape == (8,) and lse.shape == labels.shape
    P.check_scalar("loss", losses[0], t["l32"], t["l64"])
    for i, name in enumerate(("loss_seg", "loss_ood", "loss_th"), start=1):
        P.check_scalar(name, losses[i], t["parts32"][name], t["parts64"][name])
    for i, name in enumerate(STATS):
        if name.startswith("n_"):
            assert float(stats[i]) == t["parts64"][name], name
        else:
            P.check_scalar(name, stats[i], t["parts32"][name], t["parts64"][name])
    up64 = F.interpolate(sem.double(), size=labels.shape[-2:], mode="bilinear", align_corners=True)
    C.check("lse", lse.cpu(), torch.logsumexp(up64, dim=1),
            C.err(torch.logsumexp(F.interpolate(sem, size=labels.shape[-2:], mode="bilinear", align_corners=True), dim=1), torch.logsumexp(up64, dim=1)))
    if shape == (1, 2, 9, 7, 4, 3):
        assert int((t["gs64"] == 0).sum()) > 0 and int((t["go64"] == 0).sum()) > 0          # down-sampling: pixels nobody samples
    for up in UPSTREAM:
        _poison()
        gs, go = ops.dense_hybrid_loss_backward(sd, od, ld, stats, lse, torch.full((), up, device="cuda"), D.BETA)
        assert gs.shape == sem.shape and go.shape == ood.shape
        C.check(f"grad_sem (upstream {up:g})", gs.cpu() / up, t["gs64"], t["b_sem"])           # 2^-20: an exact scaling
        C.check(f"grad_ood (upstream {up:g})", go.cpu() / up, t["go64"], t["b_ood"])
        assert not gs.cpu()[t["gs64"] == 0].any() and not go.cpu()[t["go64"] == 0].any()


def test_uint8_labels_give_the_bits_of_int64_labels_and_two_runs_agree():
    from rba_amd import ops
    one = torch.ones((), device="cuda")
    for shape in D.TAIL_SHAPES[:3] + D.TAIL_SHAPES[-2:]:
        sem, ood, labels = D.tail_inputs(shape)
        sd, od = sem.cuda(), ood.cuda()
        runs = []
        for lab in (labels.cuda(), labels.cuda(), labels.to(torch.uint8).cuda()):
            _poison()
            losses, stats, lse = ops.dense_hybrid_loss(sd, od, lab, D.BETA)
            runs.append((losses, stats, lse) + ops.dense_hybrid_loss_backward(sd, od, lab, stats, lse, one, D.BETA))
        for other in runs[1:]:
            for a, b in zip(runs[0], other):
                assert torch.equal(a, b), shape


def test_no_outlier_pixel_and_no_class_pixel_are_nan():
    from rba_amd import ops
    sem, ood, labels = D.tail_inputs(D.TAIL_SHAPES[0])
    K = sem.shape[1]
    none = labels.clone()
    none[labels == D.OUTLIER] = 255
    losses, stats, _ = ops.dense_hybrid_loss(sem.cuda(), ood.cuda(), none.cuda(), D.BETA)
    _, p64 = D.ref_tail(sem.double(), ood.double(), none, D.BETA)
    _, p32 = D.ref_tail(sem, ood, none, D.BETA)
    assert torch.isnan(losses[0]) and torch.isnan(losses[2]) and float(stats[5]) == 0.0 and float(stats[1]) == 0.0
    P.check_scalar("loss_seg without outliers", losses[1], p32["loss_seg"], p64["loss_seg"])
    P.check_scalar("loss_th without outliers", losses[3], p32["loss_th"], p64["loss_th"])
    only_out = labels.clone()
    only_out[labels < K] = 255
    losses, stats, _ = ops.dense_hybrid_loss(sem.cuda(), ood.cuda(), only_out.cuda(), D.BETA)
    assert torch.isnan(losses[0]) and torch.isnan(losses[1]) and float(stats[4]) == 0.0 and float(stats[5]) > 0
    assert torch.isfinite(losses[2]) and torch.isfinite(losses[3])


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    z = lambda *s, **k: torch.zeros(*s, device="cuda", **k)
    s, o, l = z(1, 3, 2, 2), z(1, 2, 2, 2), z(1, 4, 4, dtype=torch.int64)
    stats, lse, one = z(8), z(1, 4, 4), torch.ones((), device="cuda")
    for bad in (dict(sem=s.cpu()), dict(ood=o.cpu()), dict(labels=l.cpu()), dict(sem=s.double()), dict(ood=o.half()), dict(labels=l.int()),
                dict(labels=l.float()), dict(sem=s[0]), dict(ood=o[0]), dict(labels=l[0]), dict(labels=z(2, 4, 4, dtype=torch.int64)),
                dict(ood=z(2, 2, 2, 2)), dict(sem=z(1, 33, 2, 2)), dict(ood=z(1, 3, 2, 2)), dict(ood=z(1, 2, 2, 3)),
                dict(sem=z(1, 3, 2, 4)[..., ::2]), dict(labels=z(1, 4, 8, dtype=torch.int64)[..., ::2])):
        a = {"sem": s, "ood": o, "labels": l, **bad}
        with pytest.raises(RbaHipError):
            ops.dense_hybrid_loss(a["sem"], a["ood"], a["labels"], D.BETA)
        with pytest.raises(RbaHipError):
            ops.dense_hybrid_loss_backward(a["sem"], a["ood"], a["labels"], stats, lse, one, D.BETA)
    for bad in (dict(stats=z(4)), dict(stats=stats.cpu()), dict(lse=z(1, 4, 5)), dict(lse=lse.cpu()), dict(grad_loss=torch.ones(2, device="cuda")),
                dict(grad_loss=one.cpu())):
        a = {"stats": stats, "lse": lse, "grad_loss": one, **bad}
        with pytest.raises(RbaHipError):
            ops.dense_hybrid_loss_backward(s, o, l, a["stats"], a["lse"], a["grad_loss"], D.BETA)


# ---------------------------------------------------------------------------------------------------------------- criterion.densehybrid_loss
def _outputs(shape, grad=True):
    logits, masks, ood, labels = D.loss_inputs(shape)
    leaves = [t.cuda().requires_grad_(grad) for t in (logits, masks, ood)]
    return leaves, {"pred_logits": leaves[0], "pred_masks": leaves[1], "ood_pred": leaves[2]}, labels


@pytest.mark.parametrize("shape", sorted(D.LOSS_SHAPES))
def test_densehybrid_loss_against_fp64(shape):
    from rba_amd.modeling.criterion import densehybrid_loss
    K = D.LOSS_SHAPES[shape][2]
    leaves, outputs, labels = _outputs(shape)
    t = D.loss_truth(shape)
    targets = [{"sem_seg": lab.cuda()} for lab in labels]
    loss = densehybrid_loss(outputs, targets, num_classes=K, beta=D.BETA)["densehybrid_loss"]
    assert loss.dim() == 0
    P.check_scalar("densehybrid_loss", loss, t["l32"], t["l64"])
    loss.backward()
    for name, leaf, g64, b in zip(("pred_logits", "pred_masks", "ood_pred"), leaves, t["g64"], t["b"]):
        C.check("d / d " + name, leaf.grad.cpu(), g64, b)
    for tgt, lab in zip(targets, labels):
        assert torch.equal(tgt["sem_seg"].cpu(), lab)                                        # the targets are not written
    with pytest.raises(ValueError):
        densehybrid_loss(outputs, targets, num_classes=K + 1)


def test_other_label_dtypes_are_reduced_on_the_device():
    """float / int32 / uint8 targets = the same targets as int64: the result's bits, loss and gradients"""
    from rba_amd.modeling.criterion import densehybrid_loss
    K = D.LOSS_SHAPES["small"][2]
    want = None
    for dtype in (torch.int64, torch.float32, torch.int32, torch.uint8):
        leaves, outputs, labels = _outputs("small")
        targets = [{"sem_seg": lab.to(dtype).cuda()} for lab in labels]
        before = [t["sem_seg"].clone() for t in targets]
        loss = densehybrid_loss(outputs, targets, num_classes=K, beta=D.BETA)["densehybrid_loss"]
        loss.backward()
        got = [loss.detach()] + [leaf.grad for leaf in leaves]
        want = got if want is None else want
        for a, b in zip(got, want):
            assert torch.equal(a, b), dtype
        for tgt, b4 in zip(targets, before):
            assert tgt["sem_seg"].dtype == dtype and torch.equal(tgt["sem_seg"], b4)


def test_densehybrid_loss_makes_no_read_back_and_no_torch_tail(monkeypatch):
    """The construction of test_outlier_loss_makes_no_read_back: forward and backward on the "small" fixture, after a warm call, with the
    Python-visible read-back entry points -- Tensor.item / .cpu / .tolist / .__bool__, torch.nonzero -- and the torch functions the kernel pair
    replaces -- F.interpolate, F.log_softmax, F.nll_loss, torch.logsumexp -- patched to raise."""
    from rba_amd.modeling.criterion import densehybrid_loss
    K = D.LOSS_SHAPES["small"][2]
    leaves, outputs, labels = _outputs("small")
    targets = [{"sem_seg": lab.cuda()} for lab in labels]
    densehybrid_loss(outputs, targets, num_classes=K)["densehybrid_loss"].backward()          # warm: workspaces exist
    for leaf in leaves:
        leaf.grad = None
    torch.cuda.synchronize()

    def refuse(name):
        def raiser(*a, **k):
            raise AssertionError(f"call of {name}")
        return raiser

    for name in ("item", "cpu", "tolist", "__bool__"):
        monkeypatch.setattr(torch.Tensor, name, refuse("Tensor." + name))
    monkeypatch.setattr(torch, "nonzero", refuse("torch.nonzero"))
    monkeypatch.setattr(torch, "logsumexp", refuse("torch.logsumexp"))
    for name in ("interpolate", "log_softmax", "nll_loss"):
        monkeypatch.setattr(F, name, refuse("F." + name))
    densehybrid_loss(outputs, targets, num_classes=K)["densehybrid_loss"].backward()
    monkeypatch.undo()
    assert all(torch.isfinite(leaf.grad).all() and bool(leaf.grad.any()) for leaf in leaves)
