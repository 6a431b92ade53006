"""K1 backward and the outlier loss, everything that needs no GPU: the ABI surface (header, both libraries, bindings, version), the errors of
the op and of the loss, the config reader, and the gradient check of the torch restatement the GPU tests use as truth."""
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import _rba_bwd_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_reduce_bwd_workspace_f32", "rba_reduce_bwd_f32")
FINETUNE_YAML = os.path.join(REPO, "tests", "golden", "k1_backward", "maskformer2_swin_base_IN21k_384_bs16_90k_1dl_coco_mix_finetune.yaml")


def test_header_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    flat = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    flat = re.sub(r"\s+", " ", flat)
    assert "int rba_reduce_bwd_workspace_f32(int Q, int K, int64_t HW, int64_t* bytes);" in flat
    assert ("int rba_reduce_bwd_f32(const float* mask, const float* cls_prob, const float* grad_score, float* grad_mask , float* grad_prob , "
            "int Q, int K, int64_t HW, int score_mode, void* workspace, int64_t workspace_bytes, void* stream);") in flat
    assert "criterion.py:449-463" in text


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
    assert {"rba_reduce_bwd_workspace_f32", "rba_reduce_bwd_f32"} <= set(_lib.SIGNATURES)       # argument lists: test_host_cpu, against the header
    assert _lib.EXPECTED_ABI == 191


def test_stale_library_is_answered_with_rebuild(tmp_path):
    """a library that lacks the new symbols (any older build): RbaHipError that says to rebuild, not an AttributeError at the first call"""
    from rba_amd import _lib
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc is not None, "no C compiler for the stand-in library (the oracle's build needs one too)"
    src = tmp_path / "stale.c"
    names = [n for n in _lib.SIGNATURES if n not in NEW]
    src.write_text("".join(f"int {n}(void) {{ return {191 if n == 'rba_hip_version' else 0}; }}\n" for n in names))
    lib = tmp_path / "libstale.so"
    subprocess.run([cc, "-shared", "-fPIC", str(src), "-o", str(lib)], check=True)
    with pytest.raises(_lib.RbaHipError, match="rebuild"):
        _lib._open(str(lib))


def test_op_has_no_cpu_path():
    from rba_amd import ops
    with pytest.raises(ops.RbaHipError, match="no CPU path"):
        ops.rba_reduce_backward(torch.zeros(3, 4, 5), torch.zeros(3, 2), torch.zeros(4, 5))


@pytest.mark.parametrize("kw,word", [
    (dict(target="nls", score_norm="sigmoid"), "sigmoid"),
    (dict(target="softmax_entropy"), "softmax_entropy"),
    (dict(target="sum_entropy"), "sum_entropy"),
    (dict(func="kl"), "kl"),
    (dict(func="max"), "max"),
])
def test_outlier_loss_refuses_what_is_not_built(kw, word):
    from rba_amd.modeling.criterion import outlier_loss
    outputs = {"pred_logits": torch.zeros(1, 3, 3), "pred_masks": torch.zeros(1, 3, 2, 2)}
    targets = [{"outlier_masks": torch.zeros(4, 4, dtype=torch.int64)}]
    with pytest.raises(ValueError, match=word):
        outlier_loss(outputs, targets, **kw)


@pytest.mark.parametrize("combo", C.COMBOS)
@pytest.mark.parametrize("func", C.FUNCS)
@pytest.mark.parametrize("outliers", [True, False])
def test_restatement_gradcheck(combo, func, outliers):
    """the truth of the GPU tests against finite differences, in double, at (Q, K, h, w, H, W) = (5, 3, 4, 6, 8, 12)"""
    gen = torch.Generator().manual_seed(5)
    Q, K, h, w, H, W = 5, 3, 4, 6, 8, 12
    logits = (2.0 * torch.randn(1, Q, K + 1, generator=gen)).double().requires_grad_(True)
    masks = (2.0 * torch.randn(1, Q, h, w, generator=gen) - 1.0).double().requires_grad_(True)
    labels = torch.randint(0, 3, (1, H, W), generator=gen)
    labels[labels == 2] = 255
    if not outliers:
        labels[labels == 1] = 255
    # thresholds in the middle of this shape's score range, so that both hinge terms are active; pixels at a kink are ignored
    s = C.ref_score(masks.detach(), torch.softmax(logits.detach(), -1)[..., :-1], C.SCORE_OF[combo])
    thr_in, thr_out = float(s.median()) - 0.2, float(s.median()) + 0.2
    up = torch.nn.functional.interpolate(s[:, None], size=(H, W), mode="bilinear", align_corners=True)[:, 0]
    labels[((up - thr_in).abs() < 1e-3) | ((up - thr_out).abs() < 1e-3)] = 255
    fn = lambda lg, mk: C.ref_outlier_loss(lg, mk, labels, combo[0], combo[1], func, thr_in, thr_out)
    assert torch.autograd.gradcheck(fn, (logits, masks), eps=1e-6, atol=1e-6, rtol=1e-4)


def test_restatement_keeps_the_unhalved_inlier_term():
    """criterion.py:483-487: the 0.5 is applied only when there is an outlier pixel"""
    logits, masks = torch.zeros(1, 2, 3, dtype=torch.float64), torch.full((1, 2, 2, 2), 20.0, dtype=torch.float64)
    labels = torch.zeros(1, 2, 2, dtype=torch.int64)
    s = -2.0 * torch.tanh(torch.tensor(2.0 / 3.0, dtype=torch.float64))          # two classes, each sum_q 1/3 * sigmoid(20)
    got = C.ref_outlier_loss(logits, masks, labels, "nls", "tanh", "squared_hinge", -2.0, -0.1)
    assert abs(float(got) - float((s + 2.0) ** 2)) < 1e-8
    assert torch.isnan(C.ref_outlier_loss(logits, masks, labels + 1, "nls", "tanh", "squared_hinge"))   # no inlier: the mean of nothing


def test_outlier_loss_from_cfg_reads_the_finetune_recipe(tmp_path):
    """the reference's fine-tune YAML (a settings-only fixture; the two files of its _BASE_ chain set none of the five keys and are stood in
    for by an empty one)"""
    from rba_amd.config import load_cfg
    from rba_amd.modeling.criterion import outlier_loss, outlier_loss_from_cfg
    d = tmp_path / "swin" / "single_decoder_layer"
    d.mkdir(parents=True)
    shutil.copy(FINETUNE_YAML, d / os.path.basename(FINETUNE_YAML))
    (tmp_path / "maskformer2_R50_bs16_90k.yaml").write_text("{}\n")
    cfg = load_cfg(str(d / os.path.basename(FINETUNE_YAML)))
    assert cfg.MODEL.MASK_FORMER.DEC_LAYERS == 2 and cfg.MODEL.MASK_FORMER.NUM_OBJECT_QUERIES == 100      # load_cfg as before
    loss = outlier_loss_from_cfg(cfg)
    assert loss.func is outlier_loss
    assert loss.keywords == dict(target="nls", score_norm="tanh", func="squared_hinge", inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)


def test_outlier_loss_from_cfg_defaults_and_refusals():
    from rba_amd.modeling.criterion import outlier_loss_from_cfg
    mf = {"OUTLIER_LOSS_TARGET": "energy"}
    loss = outlier_loss_from_cfg({"MODEL": {"MASK_FORMER": mf}})
    assert loss.keywords == dict(target="energy", score_norm="none", func="squared_hinge", inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)
    with pytest.raises(ValueError, match="none"):
        outlier_loss_from_cfg({"MODEL": {"MASK_FORMER": {}}})     # OUTLIER_LOSS_TARGET defaults to "none": no outlier supervision configured
    with pytest.raises(ValueError, match="kl"):
        outlier_loss_from_cfg({"MODEL": {"MASK_FORMER": {"OUTLIER_LOSS_TARGET": "nls", "OUTLIER_LOSS_FUNC": "kl"}}})
