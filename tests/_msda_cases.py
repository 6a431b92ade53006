"""Inputs, truth and error metric shared by tests/test_msda_backward_cpu.py, tests/test_msda_backward_gpu.py and
tools/k2_backward_probe.py --errors.  Test infrastructure, not product code.

Bilinear sampling is continuous in the location, its gradient is not: it jumps where a pixel coordinate crosses an integer, and the
in-window test flips at -1, H, W.  Two evaluations in different precision can only be compared away from those lines, so the generator
MOVES every pixel coordinate that lies within MARGIN of an integer to 4 MARGIN from it and `condition` verifies that all do -- in the
dtype the kernel will see (MARGIN = 1e-3 >> the fp32 spacing of a pixel coordinate <= 160, 1.5e-5).  Nothing is filtered out afterwards.
The fp64 truth is computed on `.double()` of the very same numbers."""
import torch

from oracle import ref_ops

MARGIN = 1e-3
FLOOR = 2.0 ** -20          # every output is a sum of >= 16 products of rounded factors: 16 units of 2^-24 of the tensor's largest entry
FP64_BAR = 1e-10            # <= ~2e5 adds into one element x 2^-53 ~ 2e-11, rounded up

MODEL_L3 = [(23, 40), (12, 20), (6, 10)]
TINY = [(6, 4), (3, 2)]
ODD = [(9, 7), (5, 3)]

# name -> N, M, D, Lq, shapes, P, kind ("rand" | "same" | "encoder" | "outside")
CASES = {
    "ref_tiny": (1, 2, 4, 2, TINY, 2, "rand"),
    "model_L3": (2, 8, 32, 300, MODEL_L3, 4, "rand"),
    "model_L1": (1, 8, 32, 512, [(16, 32)], 4, "rand"),
    "encoder_like": (1, 8, 32, 1610, MODEL_L3, 4, "encoder"),
    "D30": (1, 3, 30, 37, ODD, 3, "rand"),
    "D64": (1, 3, 64, 37, ODD, 3, "rand"),
    "D71": (1, 3, 71, 37, ODD, 3, "rand"),
    "same_loc_4096": (1, 1, 32, 4096, [(16, 32)], 4, "same"),
    "D1025": (1, 2, 1025, 2, TINY, 2, "rand"),
    "all_outside": (1, 8, 32, 64, MODEL_L3, 4, "outside"),
}
FP32_CASES = ["ref_tiny", "model_L3", "model_L1", "encoder_like", "D30", "D64", "D71", "same_loc_4096"]
FP64_CASES = ["ref_tiny", "D1025", "D30"]


def _wh(shapes, dtype):
    return torch.tensor(shapes, dtype=dtype).flip(-1).view(1, 1, 1, len(shapes), 1, 2)        # (W_l, H_l) per level


def pixel_coords(loc, shapes):
    """what the kernel computes from a location, in the location's dtype: (x W - 0.5, y H - 0.5)"""
    return loc * _wh(shapes, loc.dtype) - 0.5


def nudge(loc, shapes, margin=MARGIN):
    wh = _wh(shapes, loc.dtype)
    pix = loc * wh - 0.5
    frac = pix - pix.round()
    sign = torch.where(frac >= 0, 1.0, -1.0).to(loc.dtype)
    pix = torch.where(frac.abs() < margin, pix.round() + sign * 4 * margin, pix)
    return (pix + 0.5) / wh


def condition(loc, shapes, margin=MARGIN):
    pix = pixel_coords(loc, shapes)
    return bool(((pix - pix.round()).abs() >= margin).all())


def outside(loc, shapes):
    """bool [N,Lq,M,L,P]: the sample lies outside the window -1 < h < H, -1 < w < W"""
    pix = pixel_coords(loc, shapes)
    wh = _wh(shapes, loc.dtype)
    return ((pix <= -1) | (pix >= wh)).any(-1)


def make(name, dtype, seed=7):
    """-> dict(value, shapes [L,2] int64, lsi [L] int64, loc, w, go), CPU tensors of `dtype`"""
    return make_shape(*CASES[name], dtype, seed)


def make_shape(N, M, D, Lq, shapes, P, kind, dtype, seed):
    """`make` for any shape (the named cases and the random-shape sweep draw here)"""
    g = torch.Generator().manual_seed(seed)
    L = len(shapes)
    S = sum(h * w for h, w in shapes)
    value = torch.rand(N, S, M, D, generator=g, dtype=dtype) - 0.5
    if kind == "encoder":
        # self-attention of the encoder: queries on the pixels, reference point on the pixel's centre, offsets of about a pixel: many queries hit the same
        # pixels.  (The three maps hold S = 1 220 pixels; the case runs 1 610 queries, so query q sits on pixel q mod S.)
        assert N == 1
        ref = torch.cat([torch.stack(((torch.arange(w, dtype=dtype) + 0.5).repeat(h) / w,
                                      (torch.arange(h, dtype=dtype) + 0.5).repeat_interleave(w) / h), -1) for h, w in shapes], 0)
        off = torch.randn(N, Lq, M, L, P, 2, generator=g, dtype=dtype) * 1.2
        ref = ref[torch.arange(Lq) % S]
        loc = ref.view(1, Lq, 1, 1, 1, 2) + off / _wh(shapes, dtype)
    elif kind == "outside":
        loc = torch.rand(N, Lq, M, L, P, 2, generator=g, dtype=dtype) * 0.3 + 1.3
        loc = torch.where(torch.rand(N, Lq, M, L, P, 1, generator=g, dtype=dtype) < 0.5, loc, -loc)     # beyond either border
    else:
        loc = torch.rand(N, Lq, M, L, P, 2, generator=g, dtype=dtype) * 1.3 - 0.15
        if kind == "same":
            loc = loc[:, :1].expand(N, Lq, M, L, P, 2).contiguous()
    loc = nudge(loc, shapes)
    w = torch.rand(N, Lq, M, L, P, generator=g, dtype=dtype) + 1e-5
    w = w / w.sum((-1, -2), keepdim=True)
    go = torch.randn(N, Lq, M * D, generator=g, dtype=dtype)
    sh = torch.tensor(shapes, dtype=torch.int64)
    lsi = torch.cat((sh.new_zeros((1,)), sh.prod(1).cumsum(0)[:-1]))
    return dict(value=value, shapes=sh, lsi=lsi, loc=loc, w=w, go=go, shape_list=shapes)


def cpu_grads(inp, dtype=None, go=None):
    """(grad_value, grad_sampling_loc, grad_attn_weight) by CPU autograd through the oracle, in `dtype` (default: the inputs')"""
    dtype = dtype or inp["value"].dtype
    v, l, a = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("value", "loc", "w"))
    go = inp["go"] if go is None else go
    ref_ops.ms_deform_attn(v, inp["shapes"], l, a).backward(go.to(dtype))
    return v.grad, l.grad, a.grad


def err(t, t64):
    """e(T) = max|T - T64| / max|T64|"""
    return float((t.detach().cpu().double() - t64).abs().max() / t64.abs().max())


def bar(b):
    return 4.0 * max(b, FLOOR)


NAMES = ("grad_value", "grad_sampling_loc", "grad_attn_weight")
