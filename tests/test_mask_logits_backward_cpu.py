"""K4 backward and the trainable heads, everything that needs no GPU: the ABI surface (header, both libraries, bindings, version), the op's
refusal of CPU tensors, the opt-in's default, and the gradient check of the torch restatement the GPU tests use as truth."""
import os
import re
import subprocess

import pytest
import torch

from tests import _k4_bwd_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_mask_logits_bwd_workspace_f32", "rba_mask_logits_bwd_f32")


def test_header_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int rba_mask_logits_bwd_workspace_f32(int B, int Q, int C, int64_t N, int64_t* bytes);" in flat
    assert ("int rba_mask_logits_bwd_f32(const float* embed, const float* feat, const float* grad_out, float* grad_embed , float* grad_feat , "
            "int B, int Q, int C, int64_t N, void* workspace, int64_t workspace_bytes, void* stream);") in flat
    assert "decoder.py:479 under autograd" in text


@pytest.mark.parametrize("lib", ["librba_hip.so", "librba_hip_knobs.so"])
def test_libraries_export_the_entry_points(lib):
    path = os.path.join(REPO, "rba_amd", "csrc", lib)
    assert os.path.exists(path), f"{lib} is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    syms = {ln.split()[-1]: ln.split()[-2] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert syms.get(name) == "T", f"{lib} does not export {name}"
    if lib == "librba_hip.so":                                    # the product library has no writable symbol
        writable = [s for s, t in syms.items() if t in "BDGS" and not s.startswith(("_", "__"))]
        assert not writable, writable


def test_bindings_and_version():
    from rba_amd import _lib
    assert set(NEW) <= set(_lib.SIGNATURES)                       # argument lists: test_host_cpu, against the header
    assert _lib.EXPECTED_ABI == 191


def test_op_has_no_cpu_path():
    from rba_amd import ops
    with pytest.raises(ops.RbaHipError, match="no CPU path"):
        ops.mask_logits_backward(torch.zeros(1, 3, 4), torch.zeros(1, 4, 5), torch.zeros(1, 3, 5))
    with pytest.raises(ops.RbaHipError):
        ops.mask_logits_backward(torch.zeros(1, 3, 4), torch.zeros(1, 4, 5), torch.zeros(1, 3, 5), need_embed=False, need_feat=False)


def test_differentiable_heads_is_off_by_default():
    from rba_amd import arch as A
    from rba_amd.modeling.transformer_decoder.mask2former_transformer_decoder import MultiScaleMaskedTransformerDecoder
    dec = MultiScaleMaskedTransformerDecoder(A.complete(A.ARCHS["tiny1"]))
    assert dec.differentiable_heads is False and MultiScaleMaskedTransformerDecoder.differentiable_heads is False
    assert "differentiable_heads" not in dec.state_dict()


def test_restatement_gradcheck():
    """the truth of the fine-tune tests against finite differences, in double, at (B, Q, C, K, h, w) = (1, 5, 8, 3, 3, 4)"""
    gen = torch.Generator().manual_seed(11)
    B, Q, Cd, K, h, w = 1, 5, 8, 3, 3, 4
    shapes = {"decoder_norm.weight": (Cd,), "decoder_norm.bias": (Cd,), "class_embed.weight": (K + 1, Cd), "class_embed.bias": (K + 1,)}
    for i in range(3):
        shapes[f"mask_embed.layers.{i}.weight"], shapes[f"mask_embed.layers.{i}.bias"] = (Cd, Cd), (Cd,)
    assert set(shapes) == set(C.HEAD_TENSORS)
    p = {n: torch.randn(shapes[n], generator=gen).double().requires_grad_(True) for n in C.HEAD_TENSORS}
    output = torch.randn(B, Q, Cd, generator=gen).double()
    feat = torch.randn(B, Cd, h, w, generator=gen).double()
    w_cls, w_msk = torch.randn(B, Q, K + 1, generator=gen).double(), torch.randn(B, Q, h, w, generator=gen).double()

    def fn(*ts):
        cls, masks = C.ref_heads(output, feat, dict(zip(C.HEAD_TENSORS, ts)))
        return (cls * w_cls).sum() + (masks * w_msk).sum()

    assert torch.autograd.gradcheck(fn, tuple(p[n] for n in C.HEAD_TENSORS), eps=1e-6, atol=1e-6, rtol=1e-4)
