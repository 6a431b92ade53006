"""CPU (no GPU): K9's entry points are declared, bound and built, refuse malformed calls without a launch, and criterion.outlier_loss no longer
carries the torch tail."""
import ctypes
import inspect
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_outlier_tail_workspace_f32", "rba_outlier_tail_fwd_f32", "rba_outlier_tail_bwd_f32")


def test_symbols_are_declared_bound_and_built():
    from rba_amd import _lib
    from rba_amd.csrc import build
    assert set(NEW) <= set(_lib.SIGNATURES)
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "rba_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(rf"\bint\s+{n}\s*\(", header), n
    assert "outlier_tail.hip" in build.SOURCES and "outlier_tail.hip" in build.UNPACKED_ALWAYS
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)


def test_entry_points_refuse_without_a_launch():
    """hipErrorInvalidValue (1) before anything is enqueued: no device is needed to get it"""
    from rba_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.rba_outlier_tail_workspace_f32(2, 512, 1024, ctypes.addressof(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert lib.rba_outlier_tail_workspace_f32(1, 1, 1, ctypes.addressof(n)) == 0 and n.value == 16
    assert lib.rba_outlier_tail_workspace_f32(0, 4, 4, ctypes.addressof(n)) == 1
    assert lib.rba_outlier_tail_workspace_f32(1, 4, 4, 0) == 1
    assert lib.rba_outlier_tail_workspace_f32(4, 1 << 15, 1 << 15, ctypes.addressof(n)) == 1            # B H W >= 2^31
    p = 16                                                          # a non-NULL, aligned stand-in: the refusals below come before any use of it
    good = dict(label_bytes=8, B=1, h=2, w=2, H=4, W=4, func=0)

    def fwd(score=p, labels=p, ws=p, loss=p, stats=p, **kw):
        a = {**good, **kw}
        return lib.rba_outlier_tail_fwd_f32(score, labels, a["label_bytes"], a["B"], a["h"], a["w"], a["H"], a["W"], a["func"], -1.0, -0.1, ws, loss, stats, 0)

    def bwd(score=p, labels=p, stats=p, grad_loss=p, grad=p, **kw):
        a = {**good, **kw}
        return lib.rba_outlier_tail_bwd_f32(score, labels, a["label_bytes"], a["B"], a["h"], a["w"], a["H"], a["W"], a["func"], -1.0, -0.1, stats, grad_loss,
                                            grad, 0)

    for bad in (dict(label_bytes=4), dict(func=4), dict(func=-1), dict(B=0), dict(h=0), dict(W=0), dict(B=2, H=1 << 15, W=1 << 15)):
        assert fwd(**bad) == 1 and bwd(**bad) == 1, bad
    for arg in ("score", "labels", "ws", "loss", "stats"):
        assert fwd(**{arg: 0}) == 1, arg
    assert fwd(ws=18) == 1                                          # not 4-byte aligned
    for arg in ("score", "labels", "stats", "grad_loss", "grad"):
        assert bwd(**{arg: 0}) == 1, arg


def test_wrappers_have_no_cpu_path():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError, match="no CPU path"):
        ops.outlier_tail(torch.zeros(1, 2, 2), torch.zeros(1, 4, 4, dtype=torch.int64), "squared_hinge", -1.0, -0.1)
    with pytest.raises(RbaHipError, match="no CPU path"):
        ops.outlier_tail_backward(torch.zeros(1, 2, 2), torch.zeros(1, 4, 4, dtype=torch.int64), torch.zeros(4), torch.ones(()), "squared_hinge", -1.0, -0.1)


def test_outlier_loss_has_no_torch_tail():
    from rba_amd.modeling import criterion
    src = inspect.getsource(criterion.outlier_loss)
    assert "F.interpolate" not in src and "interpolate(" not in src and "numel()" not in src
    assert "OutlierTailFunction" in src
    assert set(criterion.FUNCS) == set(criterion.ops.TAIL_FUNCS)


def test_deep_supervision_defaults_off():
    from rba_amd.modeling.transformer_decoder.mask2former_transformer_decoder import MultiScaleMaskedTransformerDecoder as D
    assert D.deep_supervision is False and D.differentiable_heads is False
