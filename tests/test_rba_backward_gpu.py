"""K1 backward on the GPU: the kernel against fp64 CPU autograd on .double() of the very inputs, the autograd Function, the outlier loss
against the torch restatement of tests/_rba_bwd_cases.py, and the fine-tune recipe in miniature.

Bar (the K2-backward convention): e(T) = max|T_gpu - T64| / max|T64| per gradient tensor, e(T) <= 4 max(b(T), 2^-20), b the same metric for
fp32 CPU autograd of the same case.  No case and no element is left out.  Every test runs under the guard-banded, NaN-poisoned allocations of
tests/_guard.py: outputs and the workspace come from torch.empty inside rba_amd.ops.
"""
import pytest
import torch
import torch.nn as nn

from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu


def _dev(*ts):
    return [t.cuda().contiguous() for t in ts]


def _launch(name, score, **kw):
    from rba_amd import ops
    _, Q, K, N, *_ = C.CASE[name]
    mask, prob, g = _dev(*C.case_inputs(name))
    h = 1 if N < 64 or N % 64 else 64                      # [Q,h,w] with h w = N: the kernel sees the flat pixel axis only
    return ops.rba_reduce_backward(mask.view(Q, h, N // h), prob, g.view(h, N // h), score=score, **kw)


@pytest.mark.parametrize("name,score", C.CASE_MODES)
def test_kernel_meets_the_bar(name, score):
    _, Q, K, N, *_ = C.CASE[name]
    gm64, gp64, b_mask, b_prob = C.case_truth(name, score)
    gm, gp = _launch(name, score)
    assert gm.shape[0] == Q and gm.numel() == Q * N and tuple(gp.shape) == (Q, K)
    C.check(f"{name}/{score} grad_mask", gm.cpu().view(Q, N), gm64, b_mask)
    C.check(f"{name}/{score} grad_prob", gp.cpu(), gp64, b_prob)


@pytest.mark.parametrize("score", C.SCORES)
def test_saturated_logits_give_exact_zeros(score):
    """logits 40 randn clipped to +-120: wherever the correctly rounded fp32 sigmoid is exactly 0 or 1 (fp64 sigmoid rounded to fp32), the
    mask gradient is exactly 0 -- sig (1 - sig) is formed from sig -- and nothing is NaN or inf"""
    mask, _, _ = C.case_inputs("saturated")
    sig = mask.double().sigmoid().float()
    sat = (sig == 0) | (sig == 1)
    assert 0.3 < float(sat.float().mean()) < 0.95 and bool((sig == 0).any()) and bool((sig == 1).any())
    gm, gp = _launch("saturated", score)
    gm = gm.cpu().view_as(mask)
    assert torch.isfinite(gm).all() and torch.isfinite(gp).all()
    assert int((gm[sat] != 0).sum()) == 0
    assert bool((gm[~sat] != 0).any())


@pytest.mark.parametrize("name", ["quarter", "odd"])
def test_bitwise_reproducible(name):
    runs = [_launch(name, "rba") for _ in range(3)]
    for gm, gp in runs[1:]:
        assert torch.equal(gm, runs[0][0]) and torch.equal(gp, runs[0][1])


@pytest.mark.parametrize("name", ["base", "bigq", "odd"])
def test_null_outputs(name):
    from rba_amd import ops
    gm, gp = _launch(name, "rba")
    none, gp_only = _launch(name, "rba", need_mask=False)
    gm_only, none2 = _launch(name, "rba", need_prob=False)
    assert none is None and none2 is None
    assert torch.equal(gp_only, gp) and torch.equal(gm_only, gm)
    with pytest.raises(ops.RbaHipError):
        _launch(name, "rba", need_mask=False, need_prob=False)


def test_argument_errors():
    """K = 0, K = 161 and HW = 0: hipErrorInvalidValue from the entry point (no launch), surfaced as RbaHipError"""
    from rba_amd import _lib, ops
    dev = "cuda"
    for Q, K, h, w in [(4, 0, 2, 3), (4, 161, 2, 3), (4, 3, 0, 3)]:
        args = (torch.zeros(Q, h, w, device=dev), torch.zeros(Q, K, device=dev), torch.zeros(h, w, device=dev))
        for kw in (dict(), dict(need_prob=False), dict(need_mask=False)):
            with pytest.raises(ops.RbaHipError, match="hipError 1 "):
                ops.rba_reduce_backward(*args, **kw)
    lib = _lib.load()
    m, p, g = torch.zeros(4, 6, device=dev), torch.zeros(4, 3, device=dev), torch.zeros(6, device=dev)
    out, ws = torch.empty(4, 6, device=dev), torch.empty(64, device=dev)
    ok = (m.data_ptr(), p.data_ptr(), g.data_ptr(), out.data_ptr(), 0, 4, 3, 6, 0, 0, 0, 0)
    assert lib.rba_reduce_bwd_f32(*ok) == 0
    bad = {"score_mode": ok[:8] + (3,) + ok[9:], "no output": ok[:3] + (0, 0) + ok[5:], "null mask": (0,) + ok[1:],
           "grad_prob without workspace": ok[:4] + (ws.data_ptr(),) + ok[5:],
           "workspace too small": ok[:4] + (out.data_ptr(),) + ok[5:9] + (ws.data_ptr(), 4 * 3 * 4 - 1, 0)}
    for what, a in bad.items():
        assert lib.rba_reduce_bwd_f32(*a) == 1, what
    torch.cuda.synchronize()


# ---- the autograd Function

def _batch():
    (m0, p0, g0), (m1, p1, g1) = C.case_inputs("base"), C.case_inputs("saturated")
    return torch.stack([m0, m1]).view(2, 100, 64, 64), torch.stack([p0, p1]), torch.stack([g0, g1]).view(2, 64, 64)


def test_function_forward_is_rba_reduce():
    from rba_amd import ops
    from rba_amd.modeling.criterion import RbaScoreFunction
    mask, prob, _ = _dev(*_batch())
    for score in C.SCORES:
        out = RbaScoreFunction.apply(mask, prob, score)
        assert tuple(out.shape) == (2, 64, 64)
        for i in range(2):
            assert torch.equal(out[i], ops.rba_reduce(mask[i], prob[i], score=score)[0])


@pytest.mark.parametrize("need", [(True, True), (False, True), (True, False)])
def test_function_backward(need):
    """B = 2, a different image per batch entry; needs_input_grad honoured"""
    from rba_amd.modeling.criterion import RbaScoreFunction
    mask, prob, g = _dev(*_batch())
    mask.requires_grad_(need[0])
    prob.requires_grad_(need[1])
    (RbaScoreFunction.apply(mask, prob, "rba") * g).sum().backward()
    assert (mask.grad is not None) == need[0] and (prob.grad is not None) == need[1]
    for i, name in enumerate(["base", "saturated"]):
        gm64, gp64, b_mask, b_prob = C.case_truth(name, "rba")
        if need[0]:
            C.check(f"batch[{i}] grad_mask", mask.grad[i].cpu().view(100, 4096), gm64, b_mask)
        if need[1]:
            C.check(f"batch[{i}] grad_prob", prob.grad[i].cpu(), gp64, b_prob)


# ---- the loss

def _gpu_loss(shape, combo, func, outliers=True):
    from rba_amd.modeling.criterion import outlier_loss
    logits, masks, labels = _dev(*C.loss_inputs(shape, combo, outliers))
    logits.requires_grad_(True)
    masks.requires_grad_(True)
    out = outlier_loss({"pred_logits": logits, "pred_masks": masks}, [{"outlier_masks": lb} for lb in labels],
                       target=combo[0], score_norm=combo[1], func=func)
    assert set(out) == {"outlier_loss"} and out["outlier_loss"].dim() == 0
    out["outlier_loss"].backward()
    return float(out["outlier_loss"]), logits.grad.cpu(), masks.grad.cpu()


@pytest.mark.parametrize("shape", sorted(C.LOSS_SHAPES))
@pytest.mark.parametrize("combo", C.COMBOS)
@pytest.mark.parametrize("func", C.FUNCS)
def test_outlier_loss_against_the_restatement(shape, combo, func):
    l64, gl64, gm64, b_logits, b_masks = C.loss_truth(shape, combo, func)
    loss, gl, gm = _gpu_loss(shape, combo, func)
    print(f"loss {loss:.8g} truth {float(l64):.8g}")
    assert abs(loss - float(l64)) <= 1e-5 * abs(float(l64))
    C.check("grad pred_logits", gl, gl64, b_logits)
    C.check("grad pred_masks", gm, gm64, b_masks)


@pytest.mark.parametrize("func", ["squared_hinge", "mse", "l1"])
def test_outlier_loss_without_outliers_is_not_halved(func):
    combo = ("nls", "tanh")
    l64, gl64, gm64, b_logits, b_masks = C.loss_truth("small", combo, func, False)
    logits, masks, labels = C.loss_inputs("small", combo, False)
    # the value the halved form would give is half of this one: tell them apart through a label set that differs by one outlier pixel
    with_one = labels.clone()
    with_one[0, 0, 0] = 1
    halved = C.ref_outlier_loss(logits.double(), masks.double(), with_one, combo[0], combo[1], func)
    assert float(l64) > 0 and abs(float(halved) - float(l64)) > 0.1 * float(l64)
    loss, gl, gm = _gpu_loss("small", combo, func, False)
    assert abs(loss - float(l64)) <= 1e-5 * abs(float(l64))
    C.check("grad pred_logits", gl, gl64, b_logits)
    C.check("grad pred_masks", gm, gm64, b_masks)


# ---- the fine-tune recipe in miniature: frozen decoder output and mask features, trainable class_embed and three-layer mask_embed

class _Heads(nn.Module):
    def __init__(self, K=19, C_=256):
        super().__init__()
        self.class_embed = nn.Linear(C_, K + 1)
        self.mask_embed = nn.Sequential(nn.Linear(C_, C_), nn.ReLU(), nn.Linear(C_, C_), nn.ReLU(), nn.Linear(C_, C_))

    def forward(self, decoder_output, mask_features):
        return {"pred_logits": self.class_embed(decoder_output),
                "pred_masks": torch.einsum("bqc,bchw->bqhw", self.mask_embed(decoder_output), mask_features)}


def _recipe_inputs():
    gen = torch.Generator().manual_seed(2024)
    dec = torch.randn(1, 100, 256, generator=gen)
    feat = 0.25 * torch.randn(1, 256, 32, 64, generator=gen)
    feat[:, 0] = 1.0                                       # a constant channel: with the bias below the mask logits sit around -7, the scores around the thresholds
    r = torch.rand(1, 128, 256, generator=gen)
    labels = torch.full((1, 128, 256), 255, dtype=torch.int64)
    labels[r < 0.6] = 0
    labels[r < 0.25] = 1
    torch.manual_seed(7)
    heads = _Heads()
    with torch.no_grad():
        heads.mask_embed[-1].bias[0] = -7.0
    return dec, feat, labels, heads


def test_finetune_recipe_in_miniature():
    import copy
    from rba_amd.modeling.criterion import outlier_loss
    dec, feat, labels, heads = _recipe_inputs()

    def cpu_run(dtype):
        h = copy.deepcopy(heads).to(dtype)
        out = h(dec.to(dtype), feat.to(dtype))
        loss = C.ref_outlier_loss(out["pred_logits"], out["pred_masks"], labels)
        loss.backward()
        return loss.detach(), {n: p.grad for n, p in h.named_parameters()}

    l64, g64 = cpu_run(torch.float64)
    _, g32 = cpu_run(torch.float32)
    assert all(float(g.abs().max()) > 0 for g in g64.values())

    h = copy.deepcopy(heads).cuda()
    dec_d, feat_d, labels_d = dec.cuda(), feat.cuda(), labels.cuda()
    run = lambda: outlier_loss(h(dec_d, feat_d), [{"outlier_masks": labels_d[0]}])["outlier_loss"]
    loss = run()
    loss.backward()
    assert abs(float(loss) - float(l64)) <= 1e-5 * abs(float(l64))
    for n, p in h.named_parameters():
        C.check(f"grad {n}", p.grad.cpu(), g64[n], C.err(g32[n], g64[n]))
    # one SGD step sized for a first-order decrease of 1 % of the loss
    sq = sum(float((p.grad.double() ** 2).sum()) for p in h.parameters())
    lr = 0.01 * float(loss) / sq
    with torch.no_grad():
        for p in h.parameters():
            p -= lr * p.grad
        after = float(run())
    print(f"loss {float(loss):.6f} -> {after:.6f}")
    assert after < float(loss)


# ---- the dynamic-LDS cap of the K > 108 launches must not depend on which call came first

_LDS_ORDER_SCRIPT = """
import sys, torch
import torch.nn.functional as F
from rba_amd import ops
from tests import _rba_bwd_cases as C
for K in {ks}:
    gen = torch.Generator().manual_seed(K)
    Q, N = 40, 300
    mask, g = 6.0 * torch.randn(Q, N, generator=gen), torch.randn(N, generator=gen)
    prob = F.softmax(2.0 * torch.randn(Q, K + 1, generator=gen), dim=-1)[:, :-1].contiguous()
    gm64, gp64 = C._autograd(mask.double(), prob.double(), g.double(), "rba")
    gm32, gp32 = C._autograd(mask, prob, g, "rba")
    gm, gp = ops.rba_reduce_backward(mask.cuda().view(Q, 1, N), prob.cuda(), g.cuda().view(1, N))
    torch.cuda.synchronize()
    C.check(f"K = {{K}} grad_mask", gm.cpu().view(Q, N), gm64, C.err(gm32, gm64))
    C.check(f"K = {{K}} grad_prob", gp.cpu(), gp64, C.err(gp32, gp64))
print("ORDER OK")
"""


@pytest.mark.parametrize("ks", [(120, 160, 109), (160, 120)])
def test_lds_cap_does_not_depend_on_call_order(ks):
    """A fresh process (the cap is per-process state, and the other tests of this file have already run K = 160 in this one): K = 120 asks
    for 71 808 bytes of dynamic LDS, K = 160 for 92 928.  Every call must succeed and meet the bar in either order."""
    import os
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _LDS_ORDER_SCRIPT.format(ks=repr(ks))], cwd=repo, capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ORDER OK" in r.stdout
