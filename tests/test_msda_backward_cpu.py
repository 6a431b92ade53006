"""CPU (no GPU): the backward half of the deformable-attention boundary exists at every layer (header, library, ctypes
signatures, autograd surface), the shared input generator meets its own condition for every case the GPU file uses, and
the oracle the GPU file compares against is itself a valid gradient oracle."""
import ctypes
import os
import re

import pytest
import torch

from oracle import ref_ops
from tests import _msda_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_ms_deform_attn_bwd_f32", "rba_ms_deform_attn_bwd_f64")


def test_backward_is_declared_exported_and_bound():
    from rba_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "rba_hip.h")).read(), flags=re.S)
    declared = re.findall(r"\bint\s+(rba_\w+)\s*\(", src)
    for n in NEW:
        assert n in declared, f"{n} not declared in include/rba_hip.h"
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        lib = ctypes.CDLL(path)
        for n in NEW:
            assert hasattr(lib, n), f"{path} does not export {n}"
    for n in NEW:
        assert n in _lib.SIGNATURES                                         # argument lists: test_host_cpu, against the header
    assert _lib.load().rba_hip_version() == _lib.EXPECTED_ABI == 191


def test_backward_knob_only_in_the_knobs_build():
    from rba_amd import _lib
    with pytest.raises(_lib.RbaHipError, match="compile-time constant"):
        _lib.knob("rba_k2_bwd_variant")
    with _lib.use_library(_lib.KNOBS_LIB_PATH):
        assert _lib.knob("rba_k2_bwd_variant").value == 0


def test_autograd_surface_and_no_cpu_path():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    from rba_amd.modeling.pixel_decoder.ops.ms_deform_attn import MSDeformAttn, MSDeformAttnFunction
    assert issubclass(MSDeformAttnFunction, torch.autograd.Function)
    assert MSDeformAttn(32, 1, 2, 2).differentiable is False
    inp = C.make("ref_tiny", torch.float32)
    with pytest.raises(RbaHipError, match="no CPU path"):
        ops.ms_deform_attn_backward(inp["value"], inp["shapes"], inp["lsi"], inp["loc"], inp["w"], inp["go"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("name", sorted(C.CASES))
def test_generator_meets_its_condition(name, dtype):
    """every pixel coordinate of every sample is at least MARGIN away from an integer, in the dtype the kernel sees"""
    inp = C.make(name, dtype)
    assert inp["loc"].dtype == dtype and C.condition(inp["loc"], inp["shape_list"])
    assert C.condition(inp["loc"].double(), inp["shape_list"])              # and so for the truth run on the same numbers
    out = C.outside(inp["loc"], inp["shape_list"])
    assert torch.equal(out, C.outside(inp["loc"].double(), inp["shape_list"]))
    kind = C.CASES[name][-1]
    if kind == "outside":
        assert bool(out.all())
    elif kind != "same":
        assert 0.05 < float(out.float().mean()) < 0.6 or kind == "encoder"  # both branches are exercised


def test_oracle_passes_gradcheck_on_generated_inputs():
    """the reference's own tiny set (ops/test.py:24-28) in double: the oracle's autograd gradient agrees with finite differences"""
    inp = C.make("ref_tiny", torch.float64)
    v, l, a = (inp[k].clone().requires_grad_(True) for k in ("value", "loc", "w"))
    assert torch.autograd.gradcheck(lambda v_, l_, a_: ref_ops.ms_deform_attn(v_, inp["shapes"], l_, a_), (v, l, a))
