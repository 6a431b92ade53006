"""GPU: the argument contracts of rba_amd.ops as one table of refusals.

Every row is a call with exactly ONE fault: it must raise RbaHipError before the wrapper allocates a device tensor and before anything is enqueued.  Per wrapper
there is also the well-formed call the rows are derived from, which must get as far as its launch -- so a row cannot be refused for a second, unintended fault.

Nothing runs on the device: the library handle is replaced by a stand-in that answers the size / support queries and fails the test when a kernel entry point
is reached.  The sizes K7 asks the library for (a 256 KiB weight image, 82 944 bias-fragment floats) are answered with small numbers, so that a well-formed
image / bias_frag stays tiny like every other tensor here (at most 128 x 64 elements).

Rows marked TIGHTENED are the sites whose bias was checked for rank only before the contracts were written once (token_linear, token_linear_multi,
bn_relu_conv1x1): the C side takes a bare pointer, so a short bias was read past its end.  Rows marked EARLIER were refused before too, but only after the
output had been allocated (resample_bilinear's `add`): the check moved in front of the allocation.
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
        if name.endswith(("_bytes", "_elems", "_supported")) or name == "rba_reduce_bwd_workspace_f32":
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
