"""Shared by tests/test_solver_cpu.py, tests/test_adamw_step_gpu.py and tests/test_train_net_gpu.py: the float64 restatement of
``clip_grad_norm_(params, max_norm)`` + ``torch.optim.AdamW`` (amsgrad=False), the case table of K15, the error metric and its bar.

The bar is the project's own (tests/_rba_bwd_cases.py): e <= 4 max(b, 2^-20) with e(T) = max|T - T64| / max|T64| and b the same distance for fp32
``torch.optim.AdamW(foreach=False)`` behind ``clip_grad_norm_`` on the CPU, on the very inputs.  It is applied per tensor to exp_avg, exp_avg_sq, the
parameter and the last step's update p_after - p_before, each separately.
"""
import functools
import itertools
import os
import shutil

import torch

FLOOR = 2.0 ** -20
BETAS, EPS = (0.9, 0.999), 1e-8

# (name, shape, weight decay, lr multiplier).  Sizes: 1 and 3 (no full 16-byte group: the tail path alone), 255 / 257 (vector path with a tail), 4097 (past
# the chunk boundaries 1024 .. 4096 by one element), 256 x 256 (a tensor that spans 64 workgroups).  "view" lives one element past a 16-byte boundary
# inside a larger sentinel-filled buffer: the parameter's element path.
TENSORS = (
    ("t1", (1,), 0.0, 1.0),
    ("t3", (3,), 0.05, 1.0),
    ("t255", (255,), 0.0, 0.1),
    ("t257", (257,), 0.05, 1.0),
    ("t4097", (4097,), 0.05, 0.1),
    ("t64k", (256, 256), 0.05, 1.0),
    ("view", (131,), 0.0, 1.0),
)
NAMES = tuple(t[0] for t in TENSORS)
WEIGHT_DECAYS = tuple(t[2] for t in TENSORS)
LR_MULTS = tuple(t[3] for t in TENSORS)
VIEW_OFFSET, VIEW_MARGIN, SENTINEL = 33, 64, 7.0        # 33 * 4 bytes = 8 * 16 + 4
MAX_STEPS = 5
# (steps, max_norm, grad_scale): clipping active (the gradient norm is about 2.6), inactive, disabled
CASES = tuple(itertools.product((1, 2, 5), (0.01, 1e9, 0.0), (1.0, 0.5)))


def case_id(case):
    return f"steps{case[0]}-clip{case[1]:g}-scale{case[2]:g}"


def lr_at(step):
    """a schedule-like learning rate for step 0, 1, ...: it changes every step"""
    return 1e-4 * (1.0 - step / 10.0) ** 0.9


@functools.lru_cache(maxsize=None)
def inputs():
    """(p0 [tensor], grads [step][tensor]) fp32 on the CPU, seeded; never modified"""
    gen = torch.Generator().manual_seed(1515)
    p0 = [0.5 * torch.randn(shape, generator=gen) for _, shape, _, _ in TENSORS]
    grads = [[1e-2 * torch.randn(shape, generator=gen) for _, shape, _, _ in TENSORS] for _ in range(MAX_STEPS)]
    return p0, grads


def restate64(p0, grads, lrs, max_norm, grad_scale, weight_decays=WEIGHT_DECAYS, lr_mults=LR_MULTS, betas=BETAS, eps=EPS):
    """float64 clip_grad_norm_ + AdamW over len(lrs) steps -> (p, exp_avg, exp_avg_sq, last update), lists of float64 tensors.  ``grads[s][t]`` is the
    gradient of tensor t at step s before the scale and the clip."""
    p = [t.double().clone() for t in p0]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    before = None
    for s, lr in enumerate(lrs):
        g = [t.double() * grad_scale for t in grads[s]]
        if max_norm > 0:
            total = torch.sqrt(sum((t * t).sum() for t in g))
            coef = min(max_norm / (float(total) + 1e-6), 1.0)
            g = [t * coef for t in g]
        before = [t.clone() for t in p]
        step = s + 1
        bc1, bc2 = 1 - betas[0] ** step, 1 - betas[1] ** step
        for i in range(len(p)):
            lr_t = lr * lr_mults[i]
            p[i] = p[i] * (1 - lr_t * weight_decays[i])
            m[i] = m[i] + (g[i] - m[i]) * (1 - betas[0])
            v[i] = betas[1] * v[i] + (1 - betas[1]) * g[i] * g[i]
            p[i] = p[i] - (lr_t / bc1) * m[i] / (v[i].sqrt() / bc2 ** 0.5 + eps)
    return p, m, v, [a - b for a, b in zip(p, before)]


def torch32(p0, grads, lrs, max_norm, grad_scale, weight_decays=WEIGHT_DECAYS, lr_mults=LR_MULTS):
    """the same with fp32 torch.optim.AdamW(foreach=False) + clip_grad_norm_ on the CPU"""
    params = [torch.nn.Parameter(t.clone()) for t in p0]
    opt = torch.optim.AdamW([{"params": [q], "weight_decay": wd} for q, wd in zip(params, weight_decays)], lr=1.0, betas=BETAS, eps=EPS, foreach=False)
    before = None
    for s, lr in enumerate(lrs):
        for q, g, group, mult in zip(params, grads[s], opt.param_groups, lr_mults):
            q.grad = g.clone() * grad_scale
            group["lr"] = lr * mult
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(params, max_norm)
        before = [q.detach().clone() for q in params]
        opt.step()
    return ([q.detach() for q in params], [opt.state[q]["exp_avg"] for q in params], [opt.state[q]["exp_avg_sq"] for q in params],
            [q.detach() - b for q, b in zip(params, before)])


def err(t, t64):
    d = (t.detach().cpu().double() - t64).abs().max()
    return float(d / t64.abs().max()) if float(t64.abs().max()) > 0 else float(d)


def bar(b):
    return 4.0 * max(b, FLOOR)


QUANTITIES = ("param", "exp_avg", "exp_avg_sq", "update")


@functools.lru_cache(maxsize=None)
def truth(case):
    """(float64 results, b[quantity][tensor]) of a case of the table"""
    steps, max_norm, grad_scale = case
    p0, grads = inputs()
    lrs = [lr_at(s) for s in range(steps)]
    t64 = restate64(p0, grads, lrs, max_norm, grad_scale)
    t32 = torch32(p0, grads, lrs, max_norm, grad_scale)
    return t64, [[err(a, a64) for a, a64 in zip(q32, q64)] for q32, q64 in zip(t32, t64)]


def check(what, got, t64, b, names=NAMES):
    """got / t64: (param, exp_avg, exp_avg_sq, update) lists; every figure is printed before the assertion"""
    failures = []
    for qi, quantity in enumerate(QUANTITIES):
        for ti, name in enumerate(names):
            e = err(got[qi][ti], t64[qi][ti])
            line = f"{what} {quantity} {name}: e = {e:.3e}  b = {b[qi][ti]:.3e}  bar = {bar(b[qi][ti]):.3e}"
            print(line)
            if not bool(torch.isfinite(got[qi][ti]).all()) or e > bar(b[qi][ti]):
                failures.append(line)
    assert not failures, "beyond 4 max(b, 2^-20):\n" + "\n".join(failures)


def make_params(device):
    """fresh parameters holding inputs()' p0 on ``device`` -> (named parameters, the sentinel buffer "view" is carved from)"""
    p0, _ = inputs()
    named, buf = [], None
    for (name, shape, _, _), t in zip(TENSORS, p0):
        if name == "view":
            buf = torch.full((VIEW_OFFSET + t.numel() + VIEW_MARGIN,), SENTINEL, device=device)
            q = buf[VIEW_OFFSET:VIEW_OFFSET + t.numel()]
            q.copy_(t)
            assert q.data_ptr() % 16 == 4
        else:
            q = t.clone().to(device)
        named.append((name, q.requires_grad_(True)))
    return named, buf


def run_optimizer(case, device, chunk=None, poison=None):
    """ClipAdamW on the case -> ((param, exp_avg, exp_avg_sq, update) on the CPU, optimizer, sentinel buffer).  ``poison``: (tensor index, element, value)
    written into the gradient of the last step."""
    from rba_amd.solver import ClipAdamW
    steps, max_norm, grad_scale = case
    _, grads = inputs()
    named, buf = make_params(device)
    opt = ClipAdamW(named, LR_MULTS, WEIGHT_DECAYS, betas=BETAS, eps=EPS, max_norm=max_norm, chunk=chunk)
    opt.grad_scale = grad_scale
    before = None
    for s in range(steps):
        opt.zero_grad()
        for (_, q), g in zip(named, grads[s]):
            q.grad.copy_(g)
        if poison is not None and s == steps - 1:
            named[poison[0]][1].grad.view(-1)[poison[1]] = poison[2]
        before = [q.detach().clone() for _, q in named]
        opt.step(lr_at(s))
    got = ([q.detach().cpu() for _, q in named], [t.cpu() for t in opt._slices(opt.exp_avg)], [t.cpu() for t in opt._slices(opt.exp_avg_sq)],
           [(q.detach() - b).cpu() for (_, q), b in zip(named, before)])
    return got, opt, buf


# ---- the golden recipes and the tiny models (build_optimizer, Trainer)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES = {
    "coco_mix": ("k1_backward/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_coco_mix_finetune.yaml", "tiny1"),
    "densehybrid": ("dense_hybrid/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_densehybrid_cocomix_finetune.yaml", "tiny1_dh"),
    "pebal": ("pebal/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_pebal_finetune.yaml", "tiny1"),
}
PEBAL_OPTS = ["MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP", "True"]
def recipe_cfg(tmp_path, recipe, opts=None):
    """the recipe with its _BASE_ chain written into tmp_path: the keys the criterion reads and the base's SOLVER block (tests/golden/solver)"""
    from rba_amd.config import load_cfg
    d = tmp_path / "a" / "b"
    d.mkdir(parents=True, exist_ok=True)
    src = os.path.join(REPO, "tests", "golden", recipe)
    shutil.copy(src, d / os.path.basename(recipe))
    base = open(src).readline().split(":", 1)[1].strip()
    assert os.path.basename(base) == "maskformer2_R50_bs16_90k.yaml"
    solver = open(os.path.join(REPO, "tests", "golden", "solver", "base_solver.yaml")).read()
    (d / base).resolve().write_text("MODEL:\n  SEM_SEG_HEAD:\n    NUM_CLASSES: 19\n    IGNORE_VALUE: 255\n" + solver)
    return load_cfg(str(d / os.path.basename(recipe)), opts)


def tiny(name="tiny1", seed=0):
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS[name])
    return load_checkpoint(MaskFormer(a), A.seeded_weights(a, seed))
