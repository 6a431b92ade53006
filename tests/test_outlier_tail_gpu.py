"""K9 on the GPU: ops.outlier_tail / ops.outlier_tail_backward against fp64 CPU torch -- F.interpolate(align_corners=True) plus the masked terms,
restated from the reference's criterion.py:474-518 -- and criterion.outlier_loss without a read-back.  Bar (tests/_rba_bwd_cases.py): e(T) =
max|T - T64| / max|T64| <= 4 max(b, 2^-20) per tensor, b = fp32 CPU autograd's error on the same inputs; scalars by _point_loss_cases.check_scalar."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import _point_loss_cases as P
from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

THR_IN, THR_OUT = -1.0, -0.1
# (B, h, w, H, W): a non-integer ratio; an exact x4 with two images; down-sampling (some score pixels get no gradient); single pixels; an axis that does not resample
SHAPES = ((1, 7, 9, 25, 33), (2, 32, 64, 128, 256), (1, 9, 7, 4, 3), (1, 1, 1, 5, 6), (1, 5, 6, 1, 1), (1, 3, 1, 3, 8))
# two laps of the partial / finish reduction, a 16 x 16 score under one large label map (four pixels to a thread before the cap): 259 workgroups (the
# finishing workgroup's threads 0 .. 2 take a second record; a ragged last workgroup), and the 2048 cap (a partial thread walks a fifth pixel)
LAP_SHAPES = ((1, 16, 16, 513, 515), (1, 16, 16, 1449, 1451))
LAP_FUNCS = ("squared_hinge", "binary_cross_entropy")             # one of the thresholded terms, and the cross-entropy: the kernels' two forms
UPSTREAM = (1.0, 2.0 ** -20)


def ref_tail(score, labels, func):
    """criterion.py:474-518 behind the score map.  score [B,h,w], labels [B,H,W] -> (loss, (sum_in, n_in, sum_out, n_out))"""
    ood, ind = labels == 1, labels == 0
    s = F.interpolate(score[:, None], size=labels.shape[-2:], mode="bilinear", align_corners=True)[:, 0]
    if func == "binary_cross_entropy":
        total = F.binary_cross_entropy_with_logits(s, ood.to(s.dtype), reduction="sum")
        return 0.5 * total / s.numel(), (total, s.numel(), 0.0, 0.0)
    d_in, d_out = s[ind] - THR_IN, THR_OUT - s[ood]
    term = {"squared_hinge": lambda d: F.relu(d).pow(2), "mse": lambda d: d.pow(2), "l1": lambda d: d.abs()}[func]
    loss = term(d_in).mean()
    if d_out.numel() > 0:
        loss = 0.5 * (loss + term(d_out).mean())
    return loss, (term(d_in).sum(), d_in.numel(), term(d_out).sum(), d_out.numel())


def _draw(shape, seed):
    """-> (score, labels, whether both classes keep pixels on each side of their threshold)"""
    B, h, w, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    score = -0.55 + 0.5 * torch.randn(B, h, w, generator=gen)
    labels = torch.tensor([0, 1, 255])[torch.randint(0, 3, (B, H, W), generator=gen)]
    if B * H * W <= 32:                                              # the tiny shapes: both classes whatever the draw
        labels.view(-1)[0], labels.view(-1)[-1] = 0, 1
    if B * H * W == 1:
        labels.view(-1)[0] = 0
    s = F.interpolate(score.double()[:, None], size=(H, W), mode="bilinear", align_corners=True)[:, 0]
    labels[(labels == 0) & ((s - THR_IN).abs() < C.KINK)] = 255
    labels[(labels == 1) & ((s - THR_OUT).abs() < C.KINK)] = 255
    ind, ood = labels == 0, labels == 1
    assert ((s[ind] - THR_IN).abs() >= C.KINK).all() and ((s[ood] - THR_OUT).abs() >= C.KINK).all()
    classes = bool(ind.any()) and (bool(ood.any()) or B * H * W == 1)
    sides = bool((s[ind] > THR_IN).any() and (s[ind] < THR_IN).any() and (s[ood] > THR_OUT).any() and (s[ood] < THR_OUT).any())
    return score, labels, classes, sides


@functools.lru_cache(maxsize=None)
def inputs(shape):
    """(score [B,h,w] = -0.55 + 0.5 randn: both thresholds straddled; labels [B,H,W] int64 in {0, 1, 255}, a labelled pixel whose fp64 upsampled score
    lies within KINK of its class threshold relabelled 255).  Asserted: both classes keep pixels (a one-pixel label map keeps its inlier), and with more
    than 16 labelled pixels each class has pixels on each side of its threshold -- except over a one-pixel score map, whose single value lies on one
    side of each.  The three-value map (1,3,1,3,8) takes the first seed of its sequence whose draw does."""
    B, h, w, H, W = shape
    for k in range(64):
        score, labels, classes, sides = _draw(shape, 9000 + (SHAPES + LAP_SHAPES).index(shape) + 100 * k)
        if classes and (sides or int((labels != 255).sum()) <= 16 or h * w == 1):
            return score, labels
    raise AssertionError(f"fixture: no draw of {shape} keeps both classes on both sides of their thresholds")


@functools.lru_cache(maxsize=None)
def truth(shape, func):
    """fp64 and fp32 CPU autograd: {"l64", "l32", "stats64", "stats32", "g64" = d loss / d score, "b"}"""
    score, labels = inputs(shape)
    out = {}
    for name, dtype in (("64", torch.float64), ("32", torch.float32)):
        s = score.to(dtype).clone().requires_grad_(True)
        loss, stats = ref_tail(s, labels, func)
        loss.backward()
        out["l" + name], out["g" + name] = loss.detach(), s.grad
        out["stats" + name] = [float(v.detach()) if isinstance(v, torch.Tensor) else float(v) for v in stats]
    out["b"] = C.err(out["g32"], out["g64"]) if float(out["g64"].abs().max()) > 0 else 0.0
    return out


_id = lambda s: "x".join(map(str, s))


@pytest.mark.parametrize("func,shape", [pytest.param(f, s, id=f"{f}-{_id(s)}") for s in SHAPES for f in C.FUNCS]
                         + [pytest.param(f, s, id=f"{f}-{_id(s)}") for s in LAP_SHAPES for f in LAP_FUNCS])
def test_kernel_against_fp64(shape, func):
    from rba_amd import ops
    score, labels = inputs(shape)
    t = truth(shape, func)
    sd, ld = score.cuda(), labels.cuda()
    loss, stats = ops.outlier_tail(sd, ld, func, THR_IN, THR_OUT)
    assert loss.shape == (1,) and stats.shape == (4,)
    P.check_scalar("loss", loss[0], t["l32"], t["l64"])
    for i, name in enumerate(("sum_in", "n_in", "sum_out", "n_out")):
        if name.startswith("n_"):
            assert float(stats[i]) == t["stats64"][i], name
        else:
            P.check_scalar(name, stats[i], t["stats32"][i], t["stats64"][i])
    if shape == (1, 9, 7, 4, 3):
        assert int((t["g64"] == 0).sum()) > 0                      # down-sampling: score pixels nobody samples
    for up in UPSTREAM:
        g = ops.outlier_tail_backward(sd, ld, stats, torch.full((), up, device="cuda"), func, THR_IN, THR_OUT)
        assert g.shape == score.shape
        if float(t["g64"].abs().max()) > 0:
            C.check(f"grad_score (upstream {up:g})", g.cpu() / up, t["g64"], t["b"])        # 2^-20: an exact scaling
        else:
            assert not g.any()
        assert not g.cpu()[t["g64"] == 0].any()


def test_uint8_labels_give_the_bits_of_int64_labels_and_two_runs_agree():
    from rba_amd import ops
    one = torch.ones((), device="cuda")
    for shape in SHAPES[:3]:
        score, labels = inputs(shape)
        sd = score.cuda()
        for func in C.FUNCS:
            runs = []
            for lab in (labels.cuda(), labels.cuda(), labels.to(torch.uint8).cuda()):
                loss, stats = ops.outlier_tail(sd, lab, func, THR_IN, THR_OUT)
                runs.append((loss, stats, ops.outlier_tail_backward(sd, lab, stats, one, func, THR_IN, THR_OUT)))
            for other in runs[1:]:
                for a, b in zip(runs[0], other):
                    assert torch.equal(a, b), (shape, func)


@pytest.mark.parametrize("func", ["squared_hinge", "mse", "l1"])
def test_no_outlier_pixel_is_not_halved_and_no_inlier_pixel_is_nan(func):
    """the construction of test_outlier_loss_without_outliers_is_not_halved: the halved form is told apart through a label set that differs by one
    outlier pixel"""
    from rba_amd import ops
    score, labels = inputs(SHAPES[0])
    none = labels.clone()
    none[labels == 1] = 255
    l64, _ = ref_tail(score.double(), none, func)
    l32, _ = ref_tail(score, none, func)
    with_one = none.clone()
    up = F.interpolate(score.double()[:, None], size=none.shape[-2:], mode="bilinear", align_corners=True)[:, 0]
    with_one.view(-1)[int((up - THR_OUT).abs().argmin())] = 1      # the pixel whose outlier term is smallest: the halved form is then about half
    halved, _ = ref_tail(score.double(), with_one, func)
    assert float(l64) > 0 and abs(float(halved) - float(l64)) > 0.1 * float(l64)
    loss, stats = ops.outlier_tail(score.cuda(), none.cuda(), func, THR_IN, THR_OUT)
    P.check_scalar("loss without outliers", loss[0], l32, l64)
    assert float(stats[3]) == 0.0 and float(stats[2]) == 0.0
    g = ops.outlier_tail_backward(score.cuda(), none.cuda(), stats, torch.ones((), device="cuda"), func, THR_IN, THR_OUT)
    s = score.double().clone().requires_grad_(True)
    ref_tail(s, none, func)[0].backward()
    s32 = score.clone().requires_grad_(True)
    ref_tail(s32, none, func)[0].backward()
    C.check("grad_score without outliers", g.cpu(), s.grad, C.err(s32.grad, s.grad))
    only_out = labels.clone()
    only_out[labels == 0] = 255
    loss, stats = ops.outlier_tail(score.cuda(), only_out.cuda(), func, THR_IN, THR_OUT)
    assert torch.isnan(loss).all() and float(stats[1]) == 0.0 and float(stats[3]) > 0


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    s, l = torch.zeros(1, 2, 2, device="cuda"), torch.zeros(1, 4, 4, dtype=torch.int64, device="cuda")
    stats, one = torch.zeros(4, device="cuda"), torch.ones((), device="cuda")
    for bad in (dict(score=s.cpu()), dict(labels=l.cpu()), dict(score=s.double()), dict(labels=l.int()), dict(labels=l.float()),
                dict(labels=torch.zeros(2, 4, 4, dtype=torch.int64, device="cuda")), dict(labels=l[0]), dict(score=s[0]), dict(func="kl"), dict(func=0),
                dict(score=torch.zeros(1, 4, 2, device="cuda")[:, ::2])):
        a = {"score": s, "labels": l, "func": "squared_hinge", **bad}
        with pytest.raises(RbaHipError):
            ops.outlier_tail(a["score"], a["labels"], a["func"], THR_IN, THR_OUT)
        with pytest.raises(RbaHipError):
            ops.outlier_tail_backward(a["score"], a["labels"], stats, one, a["func"], THR_IN, THR_OUT)
    for bad in (dict(stats=torch.zeros(3, device="cuda")), dict(stats=stats.cpu()), dict(grad_loss=torch.ones(2, device="cuda")), dict(grad_loss=one.cpu())):
        a = {"stats": stats, "grad_loss": one, **bad}
        with pytest.raises(RbaHipError):
            ops.outlier_tail_backward(s, l, a["stats"], a["grad_loss"], "squared_hinge", THR_IN, THR_OUT)


def test_other_label_dtypes_are_reduced_on_the_device():
    """outlier_loss with float / int32 / bool labels = the same labels as int64 (0 and 1 kept, everything else ignored)"""
    from rba_amd.modeling.criterion import outlier_loss
    logits, masks, labels = C.loss_inputs("small", ("nls", "tanh"))
    out = {"pred_logits": logits.cuda(), "pred_masks": masks.cuda()}
    want = outlier_loss(out, [{"outlier_masks": labels[0].cuda()}])["outlier_loss"]
    assert want.dim() == 0
    for dtype in (torch.float32, torch.int32, torch.uint8):
        got = outlier_loss(out, [{"outlier_masks": labels[0].to(dtype).cuda()}])["outlier_loss"]
        assert torch.equal(got, want), dtype


def test_outlier_loss_makes_no_read_back(monkeypatch):
    """Forward and backward of criterion.outlier_loss on the "small" fixture with the Python-visible read-back entry points patched to raise:
    Tensor.item / .cpu / .tolist / .__bool__ and torch.nonzero.  This catches the read-backs a Python caller can trigger by those names only -- not a
    synchronisation inside a library call (boolean-mask indexing would be caught through nonzero only where torch routes it there)."""
    from rba_amd.modeling.criterion import outlier_loss
    logits, masks, labels = C.loss_inputs("small", ("nls", "tanh"))
    lg, mk = logits.cuda().requires_grad_(True), masks.cuda().requires_grad_(True)
    targets = [{"outlier_masks": labels[0].cuda()}]
    outlier_loss({"pred_logits": lg, "pred_masks": mk}, targets)["outlier_loss"].backward()              # warm: workspaces exist
    lg.grad = mk.grad = None
    torch.cuda.synchronize()

    def refuse(name):
        def raiser(*a, **k):
            raise AssertionError(f"read-back through {name}")
        return raiser

    for name in ("item", "cpu", "tolist", "__bool__"):
        monkeypatch.setattr(torch.Tensor, name, refuse("Tensor." + name))
    monkeypatch.setattr(torch, "nonzero", refuse("torch.nonzero"))
    for func in C.FUNCS:
        loss = outlier_loss({"pred_logits": lg, "pred_masks": mk}, targets, func=func)["outlier_loss"]
        loss.backward()
    monkeypatch.undo()
    assert torch.isfinite(lg.grad).all() and torch.isfinite(mk.grad).all() and bool(mk.grad.any())
