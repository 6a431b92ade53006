"""CPU (no GPU): K10's and the per-class K1 adjoint's entry points are declared, bound and built and refuse malformed calls without a launch; the
criterion's new names are exported; densehybrid_loss_from_cfg reads the reference's DenseHybrid fine-tune recipe (tests/golden/dense_hybrid/, a
settings-only file) while criterion_from_cfg keeps refusing it."""
import ctypes
import os
import re
import shutil

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_dense_hybrid_loss_workspace_f32", "rba_dense_hybrid_loss_fwd_f32", "rba_dense_hybrid_loss_bwd_f32", "rba_sem_seg_bwd_f32")
RECIPE_YAML = os.path.join(REPO, "tests", "golden", "dense_hybrid", "maskformer2_swin_base_IN21k_384_bs16_90k_1dl_densehybrid_cocomix_finetune.yaml")


def test_symbols_are_declared_bound_built_and_exported():
    from rba_amd import _lib, ops
    from rba_amd.csrc import build
    from rba_amd.modeling import criterion
    assert set(NEW) <= set(_lib.SIGNATURES) and _lib.EXPECTED_ABI == 191
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "rba_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(rf"\bint\s+{n}\s*\(", header), n
    assert "dense_hybrid_loss.hip" in build.SOURCES and "bilinear_ac.h" in build.HEADERS
    lib = _lib.load()
    assert all(hasattr(lib, n) for n in NEW)
    for name in ("dense_hybrid_loss", "dense_hybrid_loss_backward", "sem_seg_backward"):
        assert callable(getattr(ops, name)), name
    for name in ("SemSegFunction", "DenseHybridLossFunction", "densehybrid_loss", "densehybrid_loss_from_cfg"):
        assert callable(getattr(criterion, name)), name


def test_dense_hybrid_loss_entry_points_refuse_without_a_launch():
    """hipErrorInvalidValue (1) before anything is enqueued: no device is needed to get it"""
    from rba_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.rba_dense_hybrid_loss_workspace_f32(2, 512, 1024, ctypes.addressof(n)) == 0 and n.value > 0 and n.value % 32 == 0
    assert lib.rba_dense_hybrid_loss_workspace_f32(1, 1, 1, ctypes.addressof(n)) == 0 and n.value == 32
    assert lib.rba_dense_hybrid_loss_workspace_f32(0, 4, 4, ctypes.addressof(n)) == 1
    assert lib.rba_dense_hybrid_loss_workspace_f32(1, 4, 4, 0) == 1
    assert lib.rba_dense_hybrid_loss_workspace_f32(4, 1 << 15, 1 << 15, ctypes.addressof(n)) == 1       # B H W >= 2^31
    p = 16                                                          # a non-NULL, aligned stand-in: the refusals below come before any use of it
    good = dict(label_bytes=8, B=1, K=19, h=2, w=2, H=4, W=4)

    def fwd(sem=p, ood=p, labels=p, ws=p, losses=p, stats=p, lse=p, **kw):
        a = {**good, **kw}
        return lib.rba_dense_hybrid_loss_fwd_f32(sem, ood, labels, a["label_bytes"], a["B"], a["K"], a["h"], a["w"], a["H"], a["W"], 0.03, ws, losses,
                                                 stats, lse, 0)

    def bwd(sem=p, ood=p, labels=p, lse=p, stats=p, grad_loss=p, grad_sem=p, grad_ood=p, **kw):
        a = {**good, **kw}
        return lib.rba_dense_hybrid_loss_bwd_f32(sem, ood, labels, a["label_bytes"], lse, a["B"], a["K"], a["h"], a["w"], a["H"], a["W"], 0.03, stats,
                                                 grad_loss, grad_sem, grad_ood, 0)

    for bad in (dict(label_bytes=4), dict(K=0), dict(K=33), dict(B=0), dict(h=0), dict(W=0), dict(B=2, H=1 << 15, W=1 << 15),
                dict(K=32, h=1 << 13, w=1 << 13)):                  # B K h w >= 2^31
        assert fwd(**bad) == 1 and bwd(**bad) == 1, bad
    for arg in ("sem", "ood", "labels", "ws", "losses", "stats", "lse"):
        assert fwd(**{arg: 0}) == 1, arg
    assert fwd(ws=18) == 1                                          # not 4-byte aligned
    for arg in ("sem", "ood", "labels", "lse", "stats", "grad_loss", "grad_sem", "grad_ood"):
        assert bwd(**{arg: 0}) == 1, arg


def test_sem_seg_backward_entry_point_refuses_without_a_launch():
    from rba_amd import _lib
    lib = _lib.load()
    p = 16
    good = dict(Q=100, K=19, HW=4096)

    def call(mask=p, prob=p, grad_sem=p, grad_mask=p, grad_prob=p, ws=p, ws_bytes=1 << 40, **kw):
        a = {**good, **kw}
        return lib.rba_sem_seg_bwd_f32(mask, prob, grad_sem, grad_mask, grad_prob, a["Q"], a["K"], a["HW"], ws, ws_bytes, 0)

    for bad in (dict(Q=0), dict(K=0), dict(K=161), dict(HW=0)):
        assert call(**bad) == 1, bad
    for arg in ("mask", "prob", "grad_sem"):
        assert call(**{arg: 0}) == 1, arg
    assert call(grad_mask=0, grad_prob=0) == 1                      # at least one output
    assert call(ws=0) == 1 and call(ws=18) == 1 and call(ws_bytes=16) == 1         # grad_prob needs the workspace, aligned and large enough


def test_wrappers_have_no_cpu_path():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError):
        ops.dense_hybrid_loss(torch.zeros(1, 3, 2, 2), torch.zeros(1, 2, 2, 2), torch.zeros(1, 4, 4, dtype=torch.int64), 0.03)
    with pytest.raises(RbaHipError):
        ops.sem_seg_backward(torch.zeros(4, 2, 2), torch.zeros(4, 3), torch.zeros(3, 2, 2))


def _recipe_cfg(tmp_path):
    from rba_amd.config import load_cfg
    d = tmp_path / "densehybrid"
    d.mkdir(parents=True)
    shutil.copy(RECIPE_YAML, d / os.path.basename(RECIPE_YAML))
    # the recipe's _BASE_ chain, stood in for by the criterion keys it sets (as tests/test_point_loss_cpu.py does for the outlier recipe)
    (tmp_path / "maskformer2_R50_bs16_90k.yaml").write_text(
        "MODEL:\n  SEM_SEG_HEAD:\n    NUM_CLASSES: 19\n  MASK_FORMER:\n    DEEP_SUPERVISION: True\n    NO_OBJECT_WEIGHT: 0.1\n    CLASS_WEIGHT: 2.0\n"
        "    MASK_WEIGHT: 5.0\n    DICE_WEIGHT: 5.0\n    TRAIN_NUM_POINTS: 12544\n    OVERSAMPLE_RATIO: 3.0\n    IMPORTANCE_SAMPLE_RATIO: 0.75\n")
    return load_cfg(str(d / os.path.basename(RECIPE_YAML)))


def test_densehybrid_loss_from_cfg_reads_the_recipe_and_the_criterion_still_refuses_it(tmp_path):
    from rba_amd.modeling.criterion import criterion_from_cfg, densehybrid_loss, densehybrid_loss_from_cfg
    cfg = _recipe_cfg(tmp_path)
    assert cfg["MODEL"]["MASK_FORMER"]["DENSE_HYBRID_LOSS"] is True
    loss = densehybrid_loss_from_cfg(cfg)
    assert loss.func is densehybrid_loss and loss.keywords == {"num_classes": 19, "beta": 0.03}
    assert densehybrid_loss_from_cfg({"MODEL": {"MASK_FORMER": {"DENSE_HYBRID_BETA": 0.5}, "SEM_SEG_HEAD": {"NUM_CLASSES": 65}}}).keywords == {
        "num_classes": 65, "beta": 0.5}
    with pytest.raises(ValueError, match="densehybrid"):
        criterion_from_cfg(cfg)
