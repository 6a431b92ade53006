"""GPU: the argument contracts of rba_amd.ops as one table of refusals.

Every row is a call with exactly ONE fault: it must raise RbaHipError before the wrapper allocates a device tensor and before anything is enqueued.  Per wrapper
there is also the well-formed call the rows are derived from, which must get as far as its launch -- so a row cannot be refused for a second, unintended fault.

Nothing runs on the device: the library handle is replaced by a stand-in that answers the size / support queries and fails the test when a kernel entry point
is reached.  The sizes K7 asks the library for (a 256 KiB weight image, 82 944 bias-fragment floats) are answered with small numbers, so that a well-formed
image / bias_frag stays tiny like every other tensor here (at most 128 x 64 elements).

Rows marked TIGHTENED are the sites whose bias was checked for rank only before the contracts were written once (token_linear, token_linear_multi,
bn_relu_conv1x1): the C side takes a bare pointer, so a short bias was read past its end.  Rows marked EARLIER were refused before too, but only after the
output had been allocated (resample_bilinear's `add`): the check moved in front of the allocation.

The second table (`_table2`, below the first test) holds every wrapper added since and the older ones that had no row, with the same mechanics; its own
TIGHTENED / EARLIER sites are listed in its docstring.  tests/_ops_surface.py names the wrappers of each table, tests/test_ops_surface_cpu.py fails for a
wrapper of rba_amd.ops that is in neither.
"""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

IMAGE_BYTES, FRAG_ELEMS = 256, 96
TIGHTENED = True
EARLIER = "earlier"


class _Reached(Exception):
    pass


class _NoLaunch:
    """stands in for the ctypes handle of the kernel library"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name == "rba_swin_attn_block_weight_bytes":
            return lambda C: IMAGE_BYTES
        if name == "rba_swin_bias_fragments_elems":
            return lambda nH, ws: FRAG_ELEMS
        if name.endswith(("_bytes", "_elems", "_supported", "_workspace_f32")):        # host-side size / support queries: nothing is enqueued
            return getattr(self._lib, name)

        def reached(*args):
            raise _Reached(name)
        return reached


def _table(ops):
    """[(id, call, kind)]: kind None = the well-formed call of a wrapper, False = a refusal, TIGHTENED = a refusal that is new, EARLIER = one that now precedes the allocation."""
    SA = ops.SplitActivations
    rows = []

    def z(*shape, dtype=torch.float32):
        t = torch.zeros(*shape, dtype=dtype, device="cuda")
        assert t.numel() <= 128 * 64
        return t

    def wrapper(fn, well_formed=True, **good):
        if well_formed:
            rows.append((f"{fn.__name__}: well-formed", lambda: fn(**good), None))

        def add(clause, kind=False, **bad):
            rows.append((f"{fn.__name__}: {clause}", lambda: fn(**{**good, **bad}), kind))
        return add

    def vector(add, arg, n, kind=False):
        """the clauses of `arg`, an fp32 vector of n elements"""
        add(f"{arg} too short", kind, **{arg: z(n - 1)})
        add(f"{arg} too long", kind, **{arg: z(n + 1)})
        add(f"{arg} of rank 2", **{arg: z(1, n)})
        add(f"{arg} of another dtype", **{arg: z(n, dtype=torch.float64)})
        add(f"{arg} on the CPU", **{arg: torch.zeros(n)})

    def packed(add, good, wrong_k, bf16=True, nk=2):
        """the clauses of `planes` = split_weight(W [128, 16 nk]); wrong_k: an override that changes the wrapper's K"""
        if bf16:
            add("planes: two bf16 planes", planes=z(1, nk, 2, 128, 2, 8, dtype=torch.bfloat16))
        else:
            add("planes: bf16 where only f16x3 is served", planes=z(1, nk, 2, 128, 2, 8, dtype=torch.bfloat16))
        add("planes: one f16 plane", planes=z(1, nk, 1, 128, 2, 8, dtype=torch.float16))
        add("planes: packed for another K", **wrong_k)
        add("planes: too few tiles for out_features", out_features=200)
        add("planes: fp32", planes=good.float())
        add("planes: rank 5", planes=good.view(nk, 2, 128, 2, 8))
        add("planes: on the CPU", planes=good.cpu())

    pl = z(1, 2, 2, 128, 2, 8, dtype=torch.float16)                      # split_weight(W [128, 32]), f16x3 form

    # ---- packed weights + bias
    add = wrapper(ops.split_linear, x=z(8, 32), planes=pl, bias=z(128))
    packed(add, pl, dict(x=z(8, 64)))
    vector(add, "bias", 128)
    add("x on the CPU", x=torch.zeros(8, 32))

    add = wrapper(ops.split_linear_nchw_out, x=z(8, 32), planes=pl, bias=z(128), rows_per_image=4)
    packed(add, pl, dict(x=z(8, 64)))
    vector(add, "bias", 128)
    add("x on the CPU", x=torch.zeros(8, 32))
    add("rows_per_image does not divide M", rows_per_image=3)

    add = wrapper(ops.split_linear_nchw_out_gn, x=z(128, 32), mr=z(1, 8, 2), weight=z(32), bias_gn=z(32), num_groups=8, relu=True, planes=pl, bias=z(128),
                  rows_per_image=128)
    packed(add, pl, dict(x=z(128, 64), weight=z(64), bias_gn=z(64)), bf16=False)
    vector(add, "bias", 128)
    vector(add, "weight", 32)
    vector(add, "bias_gn", 32)
    add("x on the CPU", x=torch.zeros(128, 32))
    add("mr of another batch", mr=z(2, 8, 2))

    plc = z(1, 0, 2, 128, 2, 8, dtype=torch.float16)                     # conv3x3_weight of a [128, 0, 3, 3] weight: every clause isolated, no element
    add = wrapper(ops.conv3x3_nhwc, x=z(1, 4, 4, 0), planes=plc, bias=z(128))
    packed(add, plc, dict(planes=pl), nk=0)
    vector(add, "bias", 128)
    add("x on the CPU", x=torch.zeros(1, 4, 4, 0))
    add("x of rank 3", x=z(4, 4, 0))
    add("x SplitActivations of rank 3", x=SA.empty((4, 4, 0), "cuda"))

    # no well-formed row here: the moment epilogue exists from 256 tiles of 128 x 128 on, so the call would allocate a 16 MiB output
    add = wrapper(ops.conv3x3_nhwc_gn_stats, False, x=SA.empty((1, 128, 256, 0), "cuda"), planes=plc, num_groups=8, eps=1e-5, bias=z(128))
    packed(add, plc, dict(planes=pl), bf16=False, nk=0)
    vector(add, "bias", 128)
    add("x not SplitActivations", x=z(1, 4, 4, 0))

    add = wrapper(ops.skinny_linear, x=z(8, 32), weight=z(128, 32), bias=z(128))
    vector(add, "bias", 128)
    add("x on the CPU", x=torch.zeros(8, 32))
    add("weight on the CPU", weight=torch.zeros(128, 32))
    add("x_add of another shape", x_add=z(4, 32))
    add("x_add of rank 1", x_add=z(256))
    add("x_add on the CPU", x_add=torch.zeros(8, 32))

    # ---- tensors of one given shape
    add = wrapper(ops.resample_bilinear, x=z(2, 4, 4), size=(8, 8), add=z(2, 8, 8))
    add("add of another shape", EARLIER, add=z(2, 8, 4))
    add("add of another rank", EARLIER, add=z(1, 2, 8, 8))
    add("add on the CPU", EARLIER, add=torch.zeros(2, 8, 8))
    add("x on the CPU", x=torch.zeros(2, 4, 4))

    add = wrapper(ops.masked_xattn, q=z(1, 4, 2, 32), k=z(1, 8, 2, 32), v=z(1, 8, 2, 32), mask_logits=z(1, 4, 8))
    add("mask_logits of another S", mask_logits=z(1, 4, 7))
    add("mask_logits of rank 2", mask_logits=z(4, 8))
    add("mask_logits on the CPU", mask_logits=torch.zeros(1, 4, 8))
    add("q on the CPU", q=torch.zeros(1, 4, 2, 32))

    # ---- norm weights, qkv bias, residual bias
    add = wrapper(ops.group_norm, x=z(1, 8, 2, 2), num_groups=2, weight=z(8), bias=z(8))
    vector(add, "weight", 8)
    vector(add, "bias", 8)
    add("x on the CPU", x=torch.zeros(1, 8, 2, 2))

    add = wrapper(ops.add_layer_norm, x=z(8, 32), weight=z(32), bias=z(32), residual=z(8, 32), residual_bias=z(32))
    vector(add, "weight", 32)
    vector(add, "bias", 32)
    vector(add, "residual_bias", 32)
    add("x on the CPU", x=torch.zeros(8, 32))
    add("residual on the CPU", residual=torch.zeros(8, 32))
    add("residual of another shape", residual=z(4, 32))

    add = wrapper(ops.merge_layer_norm, x=z(1, 4, 8), H=2, W=2, weight=z(32), bias=z(32))
    vector(add, "weight", 32)
    vector(add, "bias", 32)
    add("x on the CPU", x=torch.zeros(1, 4, 8))

    add = wrapper(ops.swin_window_attn, qkv=z(1, 4, 24), qkv_bias=z(24), rel_bias=z(2, 4, 4), H=2, W=2, num_heads=2, window_size=2, shift=0, bias_frag=z(FRAG_ELEMS))
    vector(add, "qkv_bias", 24)
    vector(add, "bias_frag", FRAG_ELEMS)
    add("qkv on the CPU", qkv=torch.zeros(1, 4, 24))
    add("rel_bias of another window", rel_bias=z(2, 9, 9))

    fc1, fc2 = torch.nn.Linear(128, 32).cuda(), torch.nn.Linear(32, 128).cuda()
    add = wrapper(ops.mlp_fused_ln, x=z(8, 128), norm=(z(128), z(128), 1e-5), fc1=fc1, fc2=fc2)
    for i, part in enumerate(("norm.weight", "norm.bias")):
        for what, bad in (("too short", z(127)), ("of rank 2", z(1, 128)), ("on the CPU", torch.zeros(128))):
            norm = [z(128), z(128), 1e-5]
            norm[i] = bad
            add(f"{part} {what}", norm=tuple(norm))
    add("x on the CPU", x=torch.zeros(8, 128))

    add = wrapper(ops.bn_relu_conv1x1, x=z(1, 8, 4), scale=z(8), shift=z(8), weight=z(2, 8), bias=z(2))
    vector(add, "scale", 8)
    vector(add, "shift", 8)
    vector(add, "bias", 2, TIGHTENED)
    add("x on the CPU", x=torch.zeros(1, 8, 4))

    lin = torch.nn.Linear(32, 16).cuda()

    def with_bias(b):
        return SimpleNamespace(weight=lin.weight, bias=b)
    add = wrapper(ops.token_linear, x=z(8, 32), lin=lin)
    add("bias too short", TIGHTENED, lin=with_bias(z(15)))
    add("bias too long", TIGHTENED, lin=with_bias(z(17)))
    add("bias of rank 2", lin=with_bias(z(1, 16)))
    add("bias on the CPU", lin=with_bias(torch.zeros(16)))
    add("x on the CPU", x=torch.zeros(8, 32))
    add("x_add of another shape", x_add=z(4, 32))

    out = z(8, 16)
    add = wrapper(ops.token_linear_multi, x=z(8, 32), specs=[(lin, None, out, 0, False)])
    add("bias too short", TIGHTENED, specs=[(with_bias(z(15)), None, out, 0, False)])
    add("bias too long", TIGHTENED, specs=[(with_bias(z(17)), None, out, 0, False)])
    add("bias of rank 2", specs=[(with_bias(z(1, 16)), None, out, 0, False)])
    add("bias on the CPU", specs=[(with_bias(torch.zeros(16)), None, out, 0, False)])
    add("x on the CPU", x=torch.zeros(8, 32))
    add("x_add of another shape", specs=[(lin, z(4, 32), out, 0, False)])

    # ---- multi-scale deformable attention, forward and backward
    i64 = torch.int64
    msda = dict(value=z(3, 6, 2, 4), spatial_shapes=z(2, 2, dtype=i64), level_start_index=z(2, dtype=i64), sampling_locations=z(3, 3, 2, 2, 2, 2),
                attention_weights=z(3, 3, 2, 2, 2))
    for fn, good in ((ops.ms_deform_attn_forward, msda), (ops.ms_deform_attn_backward, dict(msda, grad_output=z(3, 3, 8)))):
        add = wrapper(fn, **good)
        add("sampling_locations of another M", sampling_locations=z(3, 3, 3, 2, 2, 2))
        add("sampling_locations of another N", sampling_locations=z(2, 3, 2, 2, 2, 2))
        add("sampling_locations without the (x, y) pair", sampling_locations=z(3, 3, 2, 2, 2, 3))
        add("attention_weights of another M", attention_weights=z(3, 3, 3, 2, 2))
        add("attention_weights of another N", attention_weights=z(2, 3, 2, 2, 2))
        add("attention_weights of another L", attention_weights=z(3, 3, 2, 3, 2))
        add("spatial_shapes of another L", spatial_shapes=z(3, 2, dtype=i64))
        add("level_start_index of another L", level_start_index=z(3, dtype=i64))
        add("spatial_shapes int32", spatial_shapes=z(2, 2, dtype=torch.int32))
        add("mixed float / double", attention_weights=z(3, 3, 2, 2, 2, dtype=torch.float64))
        add("im2col_step does not divide the batch", im2col_step=2)
        for arg in good:
            add(f"{arg} on the CPU", **{arg: good[arg].cpu()})
    add("grad_output of another width", grad_output=z(3, 3, 4))
    add("grad_output of another Lq", grad_output=z(3, 2, 8))
    add("grad_output of rank 2", grad_output=z(9, 8))

    # ---- K7
    k7 = dict(x=z(1, 4, 128), norm1=(z(128), z(128), 1e-5), image=z(IMAGE_BYTES, dtype=torch.uint8), qkv_bias=z(384), bias_frag=z(FRAG_ELEMS), H=2, W=2,
              window_size=12, shift=0)
    for fn, good in ((ops.swin_attn_qkv, k7), (ops.swin_attn_block, dict(k7, proj_bias=z(128), norm2=(z(128), z(128), 1e-5)))):
        add = wrapper(fn, **good)
        add("image of another size", image=z(IMAGE_BYTES - 1, dtype=torch.uint8))
        add("image fp32", image=z(IMAGE_BYTES))
        add("image on the CPU", image=torch.zeros(IMAGE_BYTES, dtype=torch.uint8))
        vector(add, "bias_frag", FRAG_ELEMS)
        vector(add, "qkv_bias", 384)
        for norm in ("norm1", "norm2")[:1 if fn is ops.swin_attn_qkv else 2]:
            for i, part in enumerate(("weight", "bias")):
                for what, bad in (("too short", z(127)), ("of rank 2", z(1, 128)), ("on the CPU", torch.zeros(128))):
                    v = [z(128), z(128), 1e-5]
                    v[i] = bad
                    add(f"{norm}.{part} {what}", **{norm: tuple(v)})
        add("x on the CPU", x=torch.zeros(1, 4, 128))
        add("x of another H*W", H=3)
        add("x of a width without a kernel", x=z(1, 4, 96), norm1=(z(96), z(96), 1e-5), qkv_bias=z(288))
    vector(add, "proj_bias", 128)

    # ---- split_into, and the GroupNorm geometry of the channels-last kernels
    def split_into(add):
        add("split_into of another map", split_into=SA.empty((1, 4, 5, 32), "cuda"))
        add("split_into of rank 3", split_into=SA.empty((16, 1, 32), "cuda"))
        add("split_into a plain tensor", split_into=z(1, 4, 4, 32))
        add("image beyond the batch", image=1)
        add("image negative", image=-1)

    add = wrapper(ops.resample_bilinear_nhwc, x=z(2, 2, 32), size=(4, 4), add=z(4, 4, 32), split_into=SA.empty((1, 4, 4, 32), "cuda"), image=0)
    split_into(add)
    add("C % 32 with split_into", x=z(2, 2, 16), add=z(4, 4, 16), split_into=SA.empty((1, 4, 4, 16), "cuda"))
    add("x on the CPU", x=torch.zeros(2, 2, 32))
    add("add on the CPU", add=torch.zeros(4, 4, 32))
    add("add of another shape", add=z(4, 2, 32))

    add = wrapper(ops.resample_bilinear_nhwc_gn, x=z(2, 2, 32), size=(4, 4), add=z(4, 4, 32), num_groups=8, x_norm=(z(8, 2), z(32), z(32), True),
                  add_norm=(z(8, 2), z(32), z(32)), split_into=SA.empty((1, 4, 4, 32), "cuda"), image=0)
    split_into(add)
    add("C % 32 with split_into", x=z(2, 2, 16), add=z(4, 4, 16), num_groups=4, x_norm=None, add_norm=None, split_into=SA.empty((1, 4, 4, 16), "cuda"))
    add("x on the CPU", x=torch.zeros(2, 2, 32))
    add("add of another shape", add=z(4, 2, 32))
    for norm in ("x_norm", "add_norm"):
        for i, part in ((1, "weight"), (2, "bias")):
            for what, bad in (("too short", z(31)), ("of rank 2", z(1, 32)), ("on the CPU", torch.zeros(32))):
                v = [z(8, 2), z(32), z(32), True][:4 if norm == "x_norm" else 3]
                v[i] = bad
                add(f"{norm} {part} {what}", **{norm: tuple(v)})
        add(f"{norm} statistics of another G", **{norm: (z(4, 2), z(32), z(32))})
    add("C % G", num_groups=3, x_norm=None, add_norm=None)
    add("(C / G) % 4", num_groups=16, x_norm=None, add_norm=None)

    for fn, good in ((ops.group_norm_nhwc, dict(x=z(1, 4, 16), num_groups=4, weight=z(16), bias=z(16))), (ops.group_norm_nhwc_stats, dict(x=z(1, 4, 16), num_groups=4))):
        add = wrapper(fn, **good)
        wb = (lambda C: dict(weight=z(C), bias=z(C))) if fn is ops.group_norm_nhwc else (lambda C: {})
        add("C % G", num_groups=3)
        add("(C / G) % 4", num_groups=8)
        add("256 % (C / 4)", x=z(1, 4, 48), **wb(48))
        add("C > 1024", x=z(1, 2, 2048), num_groups=32, **wb(2048))
        add("x on the CPU", x=torch.zeros(1, 4, 16))
        add("x of rank 2", x=z(4, 16))
        if fn is ops.group_norm_nhwc:
            vector(add, "weight", 16)
            vector(add, "bias", 16)
    return rows


def test_one_fault_is_refused_before_anything_is_allocated_or_launched(monkeypatch):
    from rba_amd import _lib, ops
    from rba_amd._lib import RbaHipError
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    # the switches the geometry predicates read: with one of them off, rows behind such a predicate would be refused for that alone
    assert ops.SPLIT_MODE == "f16x3" and ops.SPLIT_ACTIVATIONS and ops.GN_MOMENTS and ops.TOKEN_LINEAR and ops.SWIN_ATTN_FUSED
    assert ops.conv3x3_emits_gn_moments(1, 128, 256, 128, 8)         # conv3x3_nhwc_gn_stats has no well-formed row (see the table)
    monkeypatch.setattr(_lib, "_lib", _NoLaunch(_lib.load()))
    rows = _table(ops)
    assert "allocation.all.allocated" in torch.cuda.memory_stats()

    def allocations():
        return torch.cuda.memory_stats()["allocation.all.allocated"]

    wrong, tightened = [], 0
    for name, call, kind in rows:
        before = allocations()
        try:
            call()
            outcome = "returned"
        except RbaHipError:
            outcome = "refused"
        except _Reached as e:
            outcome = f"reached {e}"
        except Exception as e:                                           # noqa: BLE001 -- the table reports every row, whatever it ran into
            outcome = f"{type(e).__name__}: {e}"
        grew = allocations() - before
        tightened += kind is TIGHTENED
        if kind is None:
            ok = outcome.startswith("reached")
        else:
            ok = outcome == "refused" and grew == 0
        if not ok:
            wrong.append(f"{'[TIGHTENED] ' if kind is TIGHTENED else '[EARLIER] ' if kind else ''}{name}: {outcome}, {grew} device allocations")
    print(f"{len(rows)} rows, {tightened} of them tightened sites, {len(wrong)} wrong")
    assert tightened == 6
    assert not wrong, "\n".join(wrong)


# ---------------------------------------------------------------------------------------------------------------- the wrappers added since
RETURNS = "returns"        # the well-formed call of a wrapper that has no kernel of its own (adamw_plan builds and uploads tables): it must return
ALLOCATES = "allocates"    # a refusal that follows a device read-back (match_cost's tgt_ids range): the comparison itself allocates


def _table2(ops):
    """The table of the wrappers the first one does not hold (K1, K3 / K4 backward, K8 - K15 and the older ones without a row), same mechanics:
    [(id, call, kind)] with kind None = well-formed (reaches a launch), RETURNS = well-formed without a launch, False = refused, TIGHTENED = refused only
    since the holes this table found were closed in ops.py, EARLIER = refused before too, but behind an allocation, ALLOCATES = refused behind a read-back.

    TIGHTENED sites, each a bare pointer read past its end before: rba_reduce_up4's cls_prob rows (the entry point gets Q and K only), swin_bias_fragments'
    rel_bias of another window, spatial_shapes without its two columns (K2 forward / backward, msda_prepare, msda_fused), the fc1 / fc2 bias lengths of
    mlp_fused and mlp_fused_ln, linear_gn_stats' bias.
    EARLIER: the score name of rba_reduce / rba_reduce_up4 (checked inside the launch line, behind the outputs) and train_view's crop / canvas check
    (behind the table uploads)."""
    from rba_amd.dataset_mappers import TrainViewParams
    rows, covered = [], []
    f32, i64, i32, u8 = torch.float32, torch.int64, torch.int32, torch.uint8

    def z(*shape, dtype=f32):
        t = torch.zeros(*shape, dtype=dtype, device="cuda")
        assert t.numel() <= 128 * 64
        return t

    def strided(t):
        """t's shape and values, not contiguous"""
        assert t.numel() > 1 and 2 * t.numel() <= 128 * 64
        v = torch.zeros(tuple(t.shape) + (2,), dtype=t.dtype, device=t.device)[..., 0]
        assert not v.is_contiguous() and v.shape == t.shape
        return v

    def wrapper(fn, well_formed=None, **good):
        if fn.__name__ not in covered:
            covered.append(fn.__name__)
        if well_formed is not False:
            rows.append((f"{fn.__name__}: well-formed", lambda: fn(**good), well_formed))

        def add(clause, kind=False, **bad):
            rows.append((f"{fn.__name__}: {clause}", lambda: fn(**{**good, **bad}), kind))
        add.good = good
        return add

    def tensor(add, arg, rank=True, other=None):
        """the clauses every tensor argument has: on the CPU, of another dtype, of another rank (where the wrapper takes one rank), not contiguous"""
        t = add.good[arg]
        other = other or {f32: torch.float64, i64: i32, i32: i64, u8: i32}[t.dtype]
        add(f"{arg} on the CPU", **{arg: t.cpu()})
        add(f"{arg} of dtype {other}", **{arg: t.to(other)})
        if rank:
            add(f"{arg} of rank {t.dim() + 1}", **{arg: t[None]})
        if t.numel() > 1:
            add(f"{arg} not contiguous", **{arg: strided(t)})

    def vector(add, arg, n, kind=False):
        add(f"{arg} too short", kind, **{arg: z(n - 1)})
        add(f"{arg} too long", kind, **{arg: z(n + 1)})
        add(f"{arg} of rank 2", **{arg: z(1, n)})
        add(f"{arg} of another dtype", **{arg: z(n, dtype=torch.float64)})
        add(f"{arg} on the CPU", **{arg: torch.zeros(n)})

    def one_element(add, arg):
        add(f"{arg} of two elements", **{arg: z(2)})
        add(f"{arg} on the CPU", **{arg: torch.zeros(1)})
        add(f"{arg} of another dtype", **{arg: z(1, dtype=torch.float64)})

    # ---- K1, forward and backward
    add = wrapper(ops.rba_reduce, mask_pred=z(5, 8, 8), cls_prob=z(5, 3))
    tensor(add, "mask_pred")
    tensor(add, "cls_prob")
    add("cls_prob of another Q", cls_prob=z(4, 3))
    add("unknown score", EARLIER, score="softmax")

    add = wrapper(ops.rba_reduce_up4, mask_lowres=z(5, 4, 4), cls_prob=z(5, 3), crop_hw=(16, 16))
    tensor(add, "mask_lowres")
    tensor(add, "cls_prob")
    add("cls_prob with fewer rows than Q", TIGHTENED, cls_prob=z(4, 3))
    add("cls_prob with more rows than Q", TIGHTENED, cls_prob=z(6, 3))
    add("unknown score", EARLIER, score="softmax")

    for fn, grad, g, wrong in ((ops.rba_reduce_backward, "grad_score", z(8, 8), z(8, 4)), (ops.sem_seg_backward, "grad_sem", z(3, 8, 8), z(2, 8, 8))):
        add = wrapper(fn, mask_pred=z(5, 8, 8), cls_prob=z(5, 3), **{grad: g})
        tensor(add, "mask_pred")
        tensor(add, "cls_prob")
        tensor(add, grad)
        add("cls_prob of another Q", cls_prob=z(4, 3))
        add(f"{grad} of another shape", **{grad: wrong})
        add("neither need_mask nor need_prob", need_mask=False, need_prob=False)
    wrapper(ops.rba_reduce_backward, False, mask_pred=z(5, 8, 8), cls_prob=z(5, 3), grad_score=z(8, 8))("unknown score", score="softmax")

    # ---- K3 backward, K4 forward and backward
    add = wrapper(ops.masked_xattn_backward, q=z(1, 4, 2, 32), k=z(1, 8, 2, 32), v=z(1, 8, 2, 32), mask_logits=z(1, 4, 8), grad_out=z(1, 4, 64))
    for arg in ("q", "k", "v"):
        tensor(add, arg)
    tensor(add, "mask_logits", rank=False)
    tensor(add, "grad_out", rank=False)
    add("v of another S", v=z(1, 7, 2, 32))
    add("k of another head count", k=z(1, 8, 1, 32))
    add("q of another B", q=z(2, 4, 2, 32))
    add("mask_logits of another S", mask_logits=z(1, 4, 7))
    add("mask_logits of rank 2", mask_logits=z(4, 8))
    add("grad_out of another width", grad_out=z(1, 4, 32))
    add("grad_out of another Q", grad_out=z(1, 3, 64))
    add("no gradient asked for", need_q=False, need_k=False, need_v=False)

    add = wrapper(ops.mask_logits, embed=z(1, 4, 8), feat=z(1, 8, 4, 4))
    tensor(add, "embed")
    tensor(add, "feat", rank=False)
    add("feat of rank 2", feat=z(8, 16))
    add("feat of rank 5", feat=z(1, 8, 2, 2, 4))
    add("feat of another B", feat=z(2, 8, 4, 4))
    add("feat of another C", feat=z(1, 4, 4, 4))

    add = wrapper(ops.mask_logits_backward, embed=z(1, 4, 8), feat=z(1, 8, 4, 4), grad_out=z(1, 4, 4, 4))
    tensor(add, "embed")
    tensor(add, "feat", rank=False)
    tensor(add, "grad_out", rank=False)
    add("grad_out of rank 2", grad_out=z(4, 16))
    add("embed of another Q", embed=z(1, 3, 8))
    add("feat of another C", feat=z(1, 4, 4, 4))
    add("feat of another map", feat=z(1, 8, 4, 2))
    add("feat of another B", feat=z(2, 8, 4, 4))
    add("embed None where grad_feat reads it", embed=None)
    add("feat None where grad_embed reads it", feat=None)
    add("neither need_embed nor need_feat", need_embed=False, need_feat=False)

    # ---- K8: point sampling, the mask losses, the matcher's cost
    add = wrapper(ops.point_sample, planes=z(2, 3, 4, 4), coords=z(6, 5, 2))
    tensor(add, "planes", rank=False)
    tensor(add, "coords", rank=False)
    add("planes of rank 2", planes=z(4, 4))
    add("planes with an empty row", planes=z(2, 3, 4, 0))
    add("coords of another N", coords=z(5, 5, 2))
    add("coords without the (x, y) pair", coords=z(6, 5, 3))
    add("coords of rank 4", coords=z(1, 6, 5, 2))
    add = wrapper(ops.point_sample, planes=z(2, 3, 4, 4), coords=z(5, 2), plane_index=z(4, dtype=i64))
    tensor(add, "plane_index")
    add("coords of another N", coords=z(3, 5, 2))

    mpl = dict(pred_masks=z(2, 3, 4, 4), plane_index=z(3, dtype=i64), point_coords=z(3, 5, 2), point_labels=z(3, 5), num_masks=2.0)
    for fn, good in ((ops.mask_point_loss, mpl), (ops.mask_point_loss_backward, dict(mpl, sums=z(3, 4), grad_loss_mask=z(1), grad_loss_dice=z(1)))):
        add = wrapper(fn, **good)
        tensor(add, "pred_masks", rank=False)
        tensor(add, "plane_index")
        tensor(add, "point_coords")
        tensor(add, "point_labels")
        add("pred_masks of rank 2", pred_masks=z(4, 4))
        add("point_coords of another N", point_coords=z(2, 5, 2))
        add("point_coords without the (x, y) pair", point_coords=z(3, 5, 3))
        add("point_labels of another P", point_labels=z(3, 4))
        add("point_labels of another N", point_labels=z(2, 5))
        add("num_masks = 0", num_masks=0.0)
        add("num_masks NaN", num_masks=float("nan"))
    tensor(add, "sums")
    add("sums of another N", sums=z(2, 4))
    add("sums of three columns", sums=z(3, 3))
    add("neither upstream gradient", grad_loss_mask=None, grad_loss_dice=None)
    one_element(add, "grad_loss_mask")
    one_element(add, "grad_loss_dice")

    add = wrapper(ops.match_cost, pred_masks=z(4, 4, 4), tgt_masks=z(2, 8, 8), coords=z(5, 2), cls_prob=z(4, 3), tgt_ids=z(2, dtype=i64))
    for arg in ("pred_masks", "tgt_masks", "cls_prob", "tgt_ids"):
        tensor(add, arg)
    tensor(add, "coords", rank=False)
    add("coords per query", coords=z(2, 5, 2))
    add("coords without the (x, y) pair", coords=z(5, 3))
    add("cls_prob of another Q", cls_prob=z(3, 3))
    add("tgt_ids of another T", tgt_ids=z(3, dtype=i64))
    add("no target", tgt_masks=z(0, 8, 8), tgt_ids=z(0, dtype=i64))
    add("an empty prediction plane", pred_masks=z(4, 0, 4))
    # last: the only fault a read-back finds; `(tgt_ids < 0) | (tgt_ids >= K1)` and its .any() allocate their results on the device
    add("tgt_ids beyond K", ALLOCATES, tgt_ids=torch.full((2,), 3, dtype=i64, device="cuda"))
    add("tgt_ids negative", ALLOCATES, tgt_ids=torch.full((2,), -1, dtype=i64, device="cuda"))

    # ---- K9 - K11: the loss tails.  labels: int64 or uint8 [B,H,W]
    def labels(add, B=2):
        t = add.good["labels"]
        add("labels on the CPU", labels=t.cpu())
        add("labels int32", labels=t.to(i32))
        add("labels of rank 2", labels=t[0])
        add("labels not contiguous", labels=strided(t))
        add("labels of another B", labels=z(B + 1, 8, 8, dtype=i64))
        add("labels with an empty axis", labels=z(B, 0, 8, dtype=i64))

    tail = dict(score=z(2, 4, 4), labels=z(2, 8, 8, dtype=i64), func="squared_hinge", thr_in=0.0, thr_out=1.0)
    for fn, good in ((ops.outlier_tail, tail), (ops.outlier_tail_backward, dict(tail, stats=z(4), grad_loss=z(1)))):
        add = wrapper(fn, **good)
        tensor(add, "score")
        labels(add)
        add("score with an empty axis", score=z(2, 0, 4))
        add("unknown func", func="huber")
    wrapper(ops.outlier_tail, **dict(tail, labels=z(2, 8, 8, dtype=u8)))
    vector(add, "stats", 4)
    one_element(add, "grad_loss")

    dh = dict(sem=z(2, 3, 4, 4), ood=z(2, 2, 4, 4), labels=z(2, 8, 8, dtype=i64), beta=0.5)
    for fn, good in ((ops.dense_hybrid_loss, dh), (ops.dense_hybrid_loss_backward, dict(dh, stats=z(8), lse=z(2, 8, 8), grad_loss=z(1)))):
        add = wrapper(fn, **good)
        tensor(add, "sem")
        tensor(add, "ood")
        labels(add)
        add("ood of one channel", ood=z(2, 1, 4, 4))
        add("ood of three channels", ood=z(2, 3, 4, 4))
        add("ood of another map", ood=z(2, 2, 4, 3))
        add("ood of another B", ood=z(1, 2, 4, 4))
        add("K = 33", sem=z(2, 33, 4, 4))
        add("K = 0", sem=z(2, 0, 4, 4))
    vector(add, "stats", 8)
    tensor(add, "lse")
    add("lse of another map", lse=z(2, 8, 4))
    one_element(add, "grad_loss")

    gam = dict(sem=z(2, 3, 4, 4), labels=z(2, 8, 8, dtype=i64))
    for fn, good in ((ops.gambler_loss, gam), (ops.gambler_loss_backward, dict(gam, stats=z(4), R=z(2, 8, 8), grad_loss=z(1)))):
        add = wrapper(fn, **good)
        tensor(add, "sem")
        labels(add)
        add("K + 1 = 1", sem=z(2, 1, 4, 4))
        add("K + 1 = 33", sem=z(2, 33, 4, 4))
        add("H = 3", labels=z(2, 3, 8, dtype=i64))
        add("W = 3", labels=z(2, 8, 3, dtype=i64))
        add("sem with an empty axis", sem=z(2, 3, 0, 4))
    vector(add, "stats", 4)
    tensor(add, "R")
    add("R of another map", R=z(2, 8, 4))
    one_element(add, "grad_loss")

    for fn, arg in ((ops.gaussian_blur_planes, "planes"), (ops.gaussian_blur_planes_adjoint, "grad_out")):
        add = wrapper(fn, **{arg: z(2, 8, 8)})
        tensor(add, arg)
        add("even kernel_size", kernel_size=6)
        add("kernel_size 17", kernel_size=17)
        add("kernel_size 0", kernel_size=0)
        add("sigma 0", sigma=0.0)
        add("H no larger than the padding", **{arg: z(2, 3, 8)})
        add("W no larger than the padding", **{arg: z(2, 8, 3)})
        add("no plane", **{arg: z(0, 8, 8)})

    reg = dict(score=z(2, 4, 4), labels=z(2, 8, 8, dtype=i64))
    for fn, good in ((ops.score_reg, reg), (ops.score_reg_backward, dict(reg, stats=z(2), grad_smoothness=z(1), grad_sparsity=z(1)))):
        add = wrapper(fn, **good)
        tensor(add, "score")
        labels(add)
        add("score with an empty axis", score=z(2, 0, 4))
    wrapper(ops.score_reg, score=z(2, 4, 4))
    vector(add, "stats", 2)
    add("neither upstream gradient", grad_smoothness=None, grad_sparsity=None)
    one_element(add, "grad_smoothness")
    one_element(add, "grad_sparsity")

    # ---- K12: test-time augmentation
    add = wrapper(ops.tta_merge, views=[z(3, 4, 4), z(3, 6, 6)], flips=[False, True], size=(8, 8))
    v0, v1 = add.good["views"]
    add("no view", views=[], flips=[])
    add("17 views", views=[z(3, 1, 1) for _ in range(17)], flips=[False] * 17)
    add("one flip flag for two views", flips=[False])
    add("a view on the CPU", views=[v0, v1.cpu()])
    add("a view float64", views=[v0, v1.double()])
    add("a view of rank 4", views=[v0, v1[None]])
    add("a view not contiguous", views=[v0, strided(v1)])
    add("a view of another K", views=[v0, z(2, 6, 6)])
    add("K = 33", views=[z(33, 1, 1), z(33, 2, 2)])
    add("K = 0", views=[z(0, 4, 4), z(0, 6, 6)])
    add("an empty view", views=[v0, z(3, 0, 6)])
    add("an empty output", size=(0, 8))
    add("unknown score", score="softmax")

    add = wrapper(ops.resize_u8_pil_bilinear, image=z(3, 4, 4, dtype=u8), size=(8, 8))
    tensor(add, "image", other=f32)
    add("an empty image", image=z(3, 0, 4, dtype=u8))
    add("an empty output", size=(8, 0))

    # ---- K13: the confusion matrix
    add = wrapper(ops.confusion_accumulate, pred=z(4, 4, dtype=i32), gt=z(4, 4, dtype=u8), num_classes=3, conf=z(4, 4, dtype=i64), bad=z(2, dtype=i64),
                  lut=z(256, dtype=u8))
    tensor(add, "pred", rank=False)
    tensor(add, "gt", rank=False)
    tensor(add, "conf")
    tensor(add, "bad")
    tensor(add, "lut")
    add("num_classes 0", num_classes=0, conf=z(1, 1, dtype=i64))
    add("num_classes 256 (conf cannot follow it within the table's size)", num_classes=256)
    add("pred and gt of different shapes", gt=z(4, 2, dtype=u8))
    add("empty maps", pred=z(0, 4, dtype=i32), gt=z(0, 4, dtype=u8))
    add("conf of another K", conf=z(3, 3, dtype=i64))
    add("conf not square", conf=z(4, 5, dtype=i64))
    add("bad of three elements", bad=z(3, dtype=i64))
    add("lut of 255 entries", lut=z(255, dtype=u8))
    wrapper(ops.confusion_accumulate, pred=z(4, 4, dtype=i32), gt=z(4, 4, dtype=i64), num_classes=3, conf=z(4, 4, dtype=i64), bad=z(2, dtype=i64))

    # ---- K14: the training view.  The well-formed call resizes, so its four tables are uploaded; every refusal precedes them
    add = wrapper(ops.train_view, img=z(3, 8, 8, dtype=u8), lab=z(8, 8, dtype=u8), params=TrainViewParams(new_h=12, new_w=10, crop=(1, 1, 8, 8)),
                  lut=z(256, dtype=u8))
    tensor(add, "img", other=f32)
    tensor(add, "lab", other=i64)
    tensor(add, "lut", other=i64)
    add("img of four channels", img=z(4, 8, 8, dtype=u8))
    add("lab of another size", lab=z(8, 6, dtype=u8))
    add("lut of 255 entries", lut=z(255, dtype=u8))
    add("an empty resize target", params=TrainViewParams(new_h=0, new_w=10, crop=(0, 0, 8, 8)))
    # sizes of their own: a table the well-formed call uploaded is cached, and would hide an upload in front of the refusal
    add("an empty crop", EARLIER, params=TrainViewParams(new_h=11, new_w=9, crop=(1, 1, 0, 8)))
    add("a canvas smaller than the crop", EARLIER, params=TrainViewParams(new_h=13, new_w=11, crop=(1, 1, 8, 8)), pad_size=(8, 4))
    paste = TrainViewParams(new_h=12, new_w=10, crop=(1, 1, 8, 8), paste=(1, 1))
    add = wrapper(ops.train_view, img=z(3, 8, 8, dtype=u8), lab=z(8, 8, dtype=u8), params=paste, obj=z(3, 2, 3, dtype=u8), objmask=z(2, 3, dtype=u8))
    tensor(add, "obj", other=f32)
    tensor(add, "objmask", other=f32)
    add("a paste without its object", obj=None)
    add("a paste without its mask", objmask=None)
    add("obj and objmask of different sizes", objmask=z(2, 2, dtype=u8))
    add("obj of one channel", obj=z(1, 2, 3, dtype=u8))
    add("an empty object", obj=z(3, 0, 3, dtype=u8), objmask=z(0, 3, dtype=u8))

    # ---- K15: the trainer's step
    p0, p1 = z(5), z(3, 3)
    add = wrapper(ops.adamw_plan, RETURNS, params=[p0, p1], lr_mults=[1.0, 1.0], weight_decays=[0.0, 0.0])
    add("no parameter", params=[], lr_mults=[], weight_decays=[])
    add("one multiplier for two parameters", lr_mults=[1.0])
    add("one weight decay for two parameters", weight_decays=[0.0])
    add("a parameter on the CPU", params=[p0, p1.cpu()])
    add("a parameter float64", params=[p0, p1.double()])
    add("a parameter not contiguous", params=[p0, strided(p1)])
    add("an empty parameter", params=[p0, z(0)])
    add("a parameter listed twice", params=[p0, p0])
    add("chunk 6", chunk=6)
    add("chunk 0", chunk=0)
    add("chunk -4", chunk=-4)
    plan = ops.adamw_plan([p0, p1], [1.0, 1.0], [0.0, 0.0])
    assert plan.total == 20
    resized = ops.adamw_plan([p0, p1], [1.0, 1.0], [0.0, 0.0])
    resized.sizes = [4, 9]                                      # what a plan looks like after `p0` was resized under it

    def flat(add, arg):
        add(f"{arg} too short", **{arg: z(19)})
        add(f"{arg} too long", **{arg: z(21)})
        add(f"{arg} of rank 2", **{arg: z(1, 20)})
        add(f"{arg} float64", **{arg: z(20, dtype=torch.float64)})
        add(f"{arg} on the CPU", **{arg: torch.zeros(20)})
        for off in (1, 2, 3):
            add(f"{arg} {4 * off} bytes off a 16-byte boundary", **{arg: z(24)[off:off + 20]})

    add = wrapper(ops.grad_sqnorm, plan=plan, grad=z(20))
    flat(add, "grad")
    add("plan not an AdamWPlan", plan=(p0, p1))
    add = wrapper(ops.clip_adamw_step, plan=plan, grad=z(20), exp_avg=z(20), exp_avg_sq=z(20), step=1, lr=1e-3)
    for arg in ("grad", "exp_avg", "exp_avg_sq"):
        flat(add, arg)
    add("plan not an AdamWPlan", plan=None)
    add("step 0", step=0)
    add("beta1 = 1", betas=(1.0, 0.999))
    add("beta2 = 1", betas=(0.9, 1.0))
    add("beta1 negative", betas=(-0.1, 0.999))
    add("eps negative", eps=-1e-8)
    add("a parameter resized since the plan", plan=resized)

    # ---- the older wrappers without a row
    add = wrapper(ops.swin_bias_fragments, rel_bias=z(2, 4, 4), window_size=2)
    tensor(add, "rel_bias")
    add("rel_bias of another window", TIGHTENED, rel_bias=z(2, 1, 1))
    add("rel_bias of a larger window", TIGHTENED, rel_bias=z(2, 9, 9))
    add("rel_bias not square", TIGHTENED, rel_bias=z(2, 4, 2))
    add("window_size 0", TIGHTENED, rel_bias=z(2, 0, 0), window_size=0)

    add = wrapper(ops.swin_attn_block_weights, qkv_weight=z(96, 32), proj_weight=z(32, 32))
    tensor(add, "qkv_weight")
    tensor(add, "proj_weight")
    add("qkv_weight of 2C rows", qkv_weight=z(64, 32))
    add("proj_weight not square", proj_weight=z(32, 16))
    add("C % 32", qkv_weight=z(48, 16), proj_weight=z(16, 16))

    add = wrapper(ops.msda_prepare, raw=z(3, 3, 24), reference_points=z(3, 3, 2, 2), spatial_shapes=z(2, 2, dtype=i64), M=2, L=2, P=2)
    tensor(add, "raw")
    tensor(add, "reference_points")
    tensor(add, "spatial_shapes")
    add("raw of another width", raw=z(3, 3, 16))
    add("reference_points of another L", reference_points=z(3, 3, 3, 2))
    add("reference_points of another Lq", reference_points=z(3, 2, 2, 2))
    add("spatial_shapes of another L", spatial_shapes=z(3, 2, dtype=i64))
    add("spatial_shapes [L,1]", TIGHTENED, spatial_shapes=z(2, 1, dtype=i64))
    add("spatial_shapes [L,3]", TIGHTENED, spatial_shapes=z(2, 3, dtype=i64))

    add = wrapper(ops.msda_fused, value=z(3, 6, 2, 32), spatial_shapes=z(1, 2, dtype=i64), level_start_index=z(1, dtype=i64), raw=z(3, 3, 24),
                  reference_points=z(3, 3, 1, 2), M=2, L=1, P=4)
    for arg in ("value", "spatial_shapes", "level_start_index", "raw", "reference_points"):
        tensor(add, arg)
    add("head_dim 16", value=z(3, 6, 2, 16))
    add("value of another M", value=z(3, 6, 1, 32))
    add("raw of another width", raw=z(3, 3, 12))
    add("raw of another N", raw=z(2, 3, 24))
    add("reference_points of another Lq", reference_points=z(3, 2, 1, 2))
    add("level_start_index of another L", level_start_index=z(2, dtype=i64))
    add("spatial_shapes of another L", spatial_shapes=z(2, 2, dtype=i64))
    add("spatial_shapes [L,1]", TIGHTENED, spatial_shapes=z(1, 1, dtype=i64))
    add("spatial_shapes [L,3]", TIGHTENED, spatial_shapes=z(1, 3, dtype=i64))

    msda = dict(value=z(3, 6, 2, 4), spatial_shapes=z(2, 2, dtype=i64), level_start_index=z(2, dtype=i64), sampling_locations=z(3, 3, 2, 2, 2, 2),
                attention_weights=z(3, 3, 2, 2, 2))
    for fn, good in ((ops.ms_deform_attn_forward, msda), (ops.ms_deform_attn_backward, dict(msda, grad_output=z(3, 3, 8)))):
        add = wrapper(fn, False, **good)                                     # their well-formed call and their other rows: the first table
        covered.remove(fn.__name__)
        add("spatial_shapes [L,1]", TIGHTENED, spatial_shapes=z(2, 1, dtype=i64))
        add("spatial_shapes [L,3]", TIGHTENED, spatial_shapes=z(2, 3, dtype=i64))

    fc1, fc2 = torch.nn.Linear(128, 32).cuda(), torch.nn.Linear(32, 128).cuda()

    def with_bias(lin, b):
        return SimpleNamespace(weight=lin.weight, bias=b)
    # reaches the weight split of fc1 (a launch of its own, once per weight load) -- every check of mlp_fused precedes it
    add = wrapper(ops.mlp_fused, x=z(8, 128), fc1=fc1, fc2=fc2, residual=z(8, 128))
    tensor(add, "x", rank=False)
    tensor(add, "residual", rank=False)
    add("residual of another shape", residual=z(4, 128))
    add("x of another width", x=z(8, 64), residual=z(8, 64))
    add("fc2 of another hidden width", fc2=torch.nn.Linear(64, 128).cuda())
    add("fc1.bias too short", TIGHTENED, fc1=with_bias(fc1, z(31)))
    add("fc1.bias too long", TIGHTENED, fc1=with_bias(fc1, z(33)))
    add("fc1.bias on the CPU", TIGHTENED, fc1=with_bias(fc1, torch.zeros(32)))
    add("fc2.bias too short", TIGHTENED, fc2=with_bias(fc2, z(127)))
    add("fc2.bias of rank 2", TIGHTENED, fc2=with_bias(fc2, z(1, 128)))

    # in place, like mlp_fused: its well-formed call and its other rows are in the first table
    add = wrapper(ops.mlp_fused_ln, False, x=z(8, 128), norm=(z(128), z(128), 1e-5), fc1=fc1, fc2=fc2)
    covered.remove("mlp_fused_ln")
    add("fc1.bias too short", TIGHTENED, fc1=with_bias(fc1, z(31)))
    add("fc2.bias too long", TIGHTENED, fc2=with_bias(fc2, z(129)))

    # the moment epilogue exists from 160 tiles of 128 x 128 on (20 480 rows): the test answers the geometry predicate itself (`linear_emits_gn_moments`,
    # replaced for this table), so that the well-formed call stays small; it reaches the weight split of the Linear
    lin = torch.nn.Linear(32, 128).cuda()
    add = wrapper(ops.linear_gn_stats, x=z(128, 32), lin=lin, num_groups=8, eps=1e-5, rows_per_image=128)
    tensor(add, "x", rank=False)
    add("x of another width", x=z(128, 64))
    add("bias too short", TIGHTENED, lin=with_bias(lin, z(127)))
    add("bias too long", TIGHTENED, lin=with_bias(lin, z(129)))
    add("bias on the CPU", TIGHTENED, lin=with_bias(lin, torch.zeros(128)))

    pl = z(1, 2, 2, 128, 2, 8, dtype=torch.float16)                      # split_weight(W [128, 32]), f16x3 form
    add = wrapper(ops.split_linear_nchw_out_gn_rows, x=z(128, 32), mr=z(1, 8, 2), weight=z(32), bias_gn=z(32), num_groups=8, relu=True, planes=pl, bias=z(128),
                  rows_per_image=128, rows=ops.RowIndex(z(1, 128, dtype=i32), 128))
    tensor(add, "x")
    tensor(add, "mr")
    vector(add, "weight", 32)
    vector(add, "bias_gn", 32)
    add("bias too short", bias=z(127))                                   # [1, 128] is a bias per image here, so no rank-2 clause
    add("bias too long", bias=z(129))
    add("bias of another dtype", bias=z(128, dtype=torch.float64))
    add("bias on the CPU", bias=torch.zeros(128))
    add("mr of another batch", mr=z(2, 8, 2))
    add("mr of another G", mr=z(1, 4, 2))
    add("bias per image of another B", bias=z(2, 128))
    add("planes bf16", planes=z(1, 2, 2, 128, 2, 8, dtype=torch.bfloat16))
    add("planes packed for another K", planes=z(1, 1, 2, 128, 2, 8, dtype=torch.float16))
    add("planes per image of another B", planes=z(0, 1, 2, 2, 128, 2, 8, dtype=torch.float16))
    add("planes on the CPU", planes=pl.cpu())
    add("rows_per_image does not divide M", rows_per_image=100, rows=None)
    add("rows_per_image % 128", x=z(64, 32), rows_per_image=64, rows=None)
    add("(K / G) % 4", num_groups=16, mr=z(1, 16, 2))
    add("rows a plain tensor", rows=z(1, 128, dtype=i32))
    add("rows of another rows_per_image", rows=ops.RowIndex(z(1, 128, dtype=i32), 256))
    add("rows of another B", rows=ops.RowIndex(z(2, 128, dtype=i32), 128))
    add("R % 128", rows=ops.RowIndex(z(1, 64, dtype=i32), 128))
    add("rows on the CPU", rows=ops.RowIndex(torch.zeros(1, 128, dtype=i32), 128))

    add = wrapper(ops.compose_query_operand, embed=z(1, 4, 8), weight=z(8, 32), bias=z(8))
    tensor(add, "embed")
    tensor(add, "weight")
    vector(add, "bias", 8)
    add("weight of another C", weight=z(4, 32))
    add("Q = 129", embed=z(1, 129, 8))
    add("C % 4", embed=z(1, 4, 6), weight=z(6, 32), bias=z(6))
    add("K % 32", weight=z(8, 16))
    add("no query", embed=z(1, 0, 8))

    add = wrapper(ops.patch_im2col, image=z(3, 8, 8, dtype=u8), mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), Hp=8, Wp=8)
    tensor(add, "image", other=i32)
    add("image of four channels", image=z(4, 8, 8, dtype=u8))
    add("Hp % 4", Hp=10)
    add("Wp % 4", Wp=10)
    add("Hp smaller than the image", Hp=4)
    add("Wp smaller than the image", Wp=4)
    add("mean of two values", mean=(0.0, 0.0))
    add("std of four values", std=(1.0, 1.0, 1.0, 1.0))
    wrapper(ops.patch_im2col, image=z(3, 8, 8), mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0), Hp=8, Wp=8)

    add = wrapper(ops.resample_bilinear_ac, x=z(2, 4, 4), size=(8, 8))
    tensor(add, "x", rank=False)
    add("x of rank 2", x=z(4, 4))
    add("x of rank 5", x=z(1, 1, 2, 4, 4))

    add = wrapper(ops.gaussian_blur, score=z(8, 8))
    tensor(add, "score")
    add("even kernel_size", kernel_size=6)
    add("kernel_size 17", kernel_size=17)
    add("sigma 0", sigma=0.0)
    add("H no larger than the padding", score=z(3, 8))
    add("W no larger than the padding", score=z(8, 3))

    add = wrapper(ops.quad_mean, v=z(2, 4, 8))
    tensor(add, "v", rank=False)
    add("three taps", v=z(2, 3, 8))
    add("v of rank 1", v=z(4))

    add = wrapper(ops.softmax_drop_last, logits=z(4, 5))
    tensor(add, "logits", rank=False)
    add("one class", logits=z(4, 1))
    add("65 classes", logits=z(4, 65))

    add = wrapper(ops.ood_components, score=z(8, 8), threshold=0.0)
    tensor(add, "score")

    # ---- the weight packers and the Linear front door (its well-formed call reaches the weight split, once per weight load)
    add = wrapper(ops.split_weight, weight=z(128, 32))
    tensor(add, "weight")
    add("K % 32", weight=z(128, 16))
    add("K = 0", weight=z(128, 0))
    add("unknown mode", mode="fp8")

    add = wrapper(ops.conv3x3_weight, weight=z(2, 32, 3, 3))
    tensor(add, "weight")
    add("a 5 x 5 kernel", weight=z(2, 32, 5, 5))
    add("C % 32", weight=z(2, 16, 3, 3))

    add = wrapper(ops.linear, x=z(8, 32), lin=lin)
    add("x on the CPU", x=torch.zeros(8, 32))
    add("x float64", x=z(8, 32, dtype=torch.float64))
    add("residual where the fused path does not apply", residual=z(8, 128))
    add("SplitActivations of another K", x=ops.SplitActivations.empty((8, 64), "cuda"))
    return rows, covered


def test_one_fault_is_refused_by_every_other_wrapper(monkeypatch):
    """The same statement for the second table; the rows TIGHTENED here fail on ops.py as it stood before them."""
    from rba_amd import _lib, ops
    from rba_amd._lib import RbaHipError
    from tests._ops_surface import REFUSAL_ROWS_SECOND_TABLE
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    assert ops.SPLIT_MODE == "f16x3" and ops.SPLIT_ACTIVATIONS and ops.GN_MOMENTS
    monkeypatch.setattr(_lib, "_lib", _NoLaunch(_lib.load()))
    monkeypatch.setattr(ops, "linear_emits_gn_moments", lambda M, N, K, rows_per_image, num_groups: True)        # see linear_gn_stats in the table
    rows, covered = _table2(ops)
    assert sorted(covered) == sorted(REFUSAL_ROWS_SECOND_TABLE), sorted(set(covered) ^ set(REFUSAL_ROWS_SECOND_TABLE))

    def allocations():
        return torch.cuda.memory_stats()["allocation.all.allocated"]

    wrong, tightened = [], 0
    for name, call, kind in rows:
        before = allocations()
        try:
            call()
            outcome = "returned"
        except RbaHipError:
            outcome = "refused"
        except _Reached as e:
            outcome = f"reached {e}"
        except Exception as e:                                           # noqa: BLE001 -- the table reports every row, whatever it ran into
            outcome = f"{type(e).__name__}: {e}"
        grew = allocations() - before
        tightened += kind is TIGHTENED
        if kind is None:
            ok = outcome.startswith("reached")
        elif kind == RETURNS:
            ok = outcome == "returned"
        elif kind == ALLOCATES:
            ok = outcome == "refused"
        else:
            ok = outcome == "refused" and grew == 0
        if not ok:
            tag = "[TIGHTENED] " if kind is TIGHTENED else f"[{kind.upper()}] " if kind else ""
            wrong.append(f"{tag}{name}: {outcome}, {grew} device allocations")
    print(f"{len(rows)} rows, {tightened} of them tightened sites, {len(wrong)} wrong")
    assert tightened == 24
    assert not wrong, "\n".join(wrong)
