"""The per-class adjoint of K1 on the GPU: ops.sem_seg_backward against fp64 CPU autograd of the class map einsum("qk,qn->kn", cls_prob,
sigmoid(mask)) on the (Q, K, N) of K1 backward's case table (tests/_rba_bwd_cases.py) with a random grad_sem [K,N], and SemSegFunction.  Bar:
e(T) = max|T - T64| / max|T64| <= 4 max(b, 2^-20), b = fp32 CPU autograd's error on the same inputs."""
import functools

import pytest
import torch

from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

NAMES = ("base", "odd", "one", "mapillary", "kmax", "bigq", "k27")  # resident and chunked (kmax, bigq, k27) forms, every KMAX instantiation (20, 80, 160, 32)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(mask [Q,N], prob [Q,K] of the K1 case, grad_sem [K,N] seeded by the case)"""
    mask, prob, _ = C.case_inputs(name)
    gen = torch.Generator().manual_seed(11000 + NAMES.index(name))
    return mask, prob, torch.randn(prob.shape[1], mask.shape[1], generator=gen)


def _autograd(mask, prob, gsem):
    m, p = mask.detach().clone().requires_grad_(True), prob.detach().clone().requires_grad_(True)
    (torch.einsum("qk,qn->kn", p, m.sigmoid()) * gsem).sum().backward()
    return m.grad, p.grad


@functools.lru_cache(maxsize=None)
def truth(name):
    mask, prob, gsem = inputs(name)
    gm64, gp64 = _autograd(mask.double(), prob.double(), gsem.double())
    gm32, gp32 = _autograd(mask, prob, gsem)
    return gm64, gp64, C.err(gm32, gm64), C.err(gp32, gp64)


def _device(name):
    mask, prob, gsem = inputs(name)
    N = mask.shape[1]
    return mask.cuda().view(-1, 1, N), prob.cuda(), gsem.cuda().view(-1, 1, N)


@pytest.mark.parametrize("name", NAMES)
def test_kernel_against_fp64(name):
    from rba_amd import ops
    gm64, gp64, b_mask, b_prob = truth(name)
    m, p, g = _device(name)
    torch.full((1 << 20,), float("nan"), device="cuda")              # the allocator's next blocks hold NaN (the workspace is read only where written)
    gm, gp = ops.sem_seg_backward(m, p, g)
    assert gm.shape == m.shape and gp.shape == p.shape
    C.check("grad_mask", gm.cpu().view(gm64.shape), gm64, b_mask)
    C.check("grad_prob", gp.cpu(), gp64, b_prob)
    only_m, none = ops.sem_seg_backward(m, p, g, need_prob=False)
    assert none is None and torch.equal(only_m, gm)
    none, only_p = ops.sem_seg_backward(m, p, g, need_mask=False)
    assert none is None and torch.equal(only_p, gp)
    gm2, gp2 = ops.sem_seg_backward(m, p, g)
    assert torch.equal(gm2, gm) and torch.equal(gp2, gp)             # two runs, equal bits


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    m, p, g = _device("odd")
    for bad in (dict(mask_pred=m.cpu()), dict(cls_prob=p.double()), dict(grad_sem=g[0]), dict(grad_sem=g[:-1]), dict(cls_prob=p[:-1]),
                dict(mask_pred=m.repeat(1, 1, 2)[..., ::2]), dict(need_mask=False, need_prob=False)):
        a = {"mask_pred": m, "cls_prob": p, "grad_sem": g, "need_mask": True, "need_prob": True, **bad}
        with pytest.raises(RbaHipError):
            ops.sem_seg_backward(a["mask_pred"], a["cls_prob"], a["grad_sem"], a["need_mask"], a["need_prob"])


def test_sem_seg_function_forward_bits_and_gradients():
    """SemSegFunction on two images: the forward is ops.rba_reduce's sem_seg output bit for bit, the backward is ops.sem_seg_backward's, and a
    gradient nobody needs is not computed"""
    from rba_amd import ops
    from rba_amd.modeling.criterion import SemSegFunction
    mask, prob, gsem = inputs("odd")
    Q, N = mask.shape
    m = torch.stack([mask, mask.flip(0)]).view(2, Q, 10, 13).cuda()
    p = torch.stack([prob, prob.flip(0)]).cuda()
    g = torch.stack([gsem, 2.0 * gsem]).view(2, -1, 10, 13).cuda()
    mg, pg = m.clone().requires_grad_(True), p.clone().requires_grad_(True)
    sem = SemSegFunction.apply(mg, pg)
    for b in range(2):
        assert torch.equal(sem[b], ops.rba_reduce(m[b], p[b], want_sem_seg=True)[1])
    sem.backward(g)
    for b in range(2):
        gm, gp = ops.sem_seg_backward(m[b], p[b], g[b])
        assert torch.equal(mg.grad[b], gm) and torch.equal(pg.grad[b], gp)
    only = m.clone().requires_grad_(True)
    SemSegFunction.apply(only, p).backward(g)
    assert torch.equal(only.grad, mg.grad)
