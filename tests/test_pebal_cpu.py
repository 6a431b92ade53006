"""CPU (no GPU): K11's entry points are declared, bound and built in both libraries and refuse malformed calls without a launch; the criterion's
new names are exported; pebal_criterion_from_cfg reads the reference's PEBAL fine-tune recipe (tests/golden/pebal/, a settings-only file) while
criterion_from_cfg keeps refusing its three loss names."""
import ctypes
import os
import re

import pytest
import torch

from tests import _pebal_cases as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_gambler_loss_workspace_f32", "rba_gambler_loss_fwd_f32", "rba_gambler_loss_bwd_f32", "rba_gaussian_blur_planes_f32",
       "rba_gaussian_blur_planes_adjoint_f32", "rba_score_reg_workspace_f32", "rba_score_reg_fwd_f32", "rba_score_reg_bwd_f32")


def test_symbols_are_declared_bound_built_and_exported_by_both_libraries():
    from rba_amd import _lib, ops
    from rba_amd.csrc import build
    from rba_amd.modeling import criterion
    assert set(NEW) <= set(_lib.SIGNATURES) and _lib.EXPECTED_ABI == 191
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "rba_hip.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(rf"\bint\s+{n}\s*\(", header), n
    assert "pebal_loss.hip" in build.SOURCES
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, n) for n in NEW), path
        assert lib.rba_hip_version() == 191
    for name in ("gambler_loss", "gambler_loss_backward", "gaussian_blur_planes", "gaussian_blur_planes_adjoint", "score_reg", "score_reg_backward"):
        assert callable(getattr(ops, name)), name
    for name in ("GamblerLossFunction", "ScoreRegFunction", "gambler_loss", "smoothness_loss", "sparsity_loss", "PebalCriterion",
                 "pebal_criterion_from_cfg"):
        assert callable(getattr(criterion, name)), name


def test_entry_points_refuse_without_a_launch():
    """hipErrorInvalidValue (1) before anything is enqueued: no device is needed to get it"""
    from rba_amd import _lib
    lib = _lib.load()
    n = ctypes.c_int64(-1)
    assert lib.rba_gambler_loss_workspace_f32(2, 512, 1024, ctypes.addressof(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert lib.rba_gambler_loss_workspace_f32(0, 4, 4, ctypes.addressof(n)) == 1 and lib.rba_gambler_loss_workspace_f32(1, 4, 4, 0) == 1
    assert lib.rba_score_reg_workspace_f32(2, 128, 256, 512, 1024, ctypes.addressof(n)) == 0 and n.value > 0 and n.value % 16 == 0
    assert lib.rba_score_reg_workspace_f32(1, 1, 1, 1, 1, ctypes.addressof(n)) == 0 and n.value == 16
    assert lib.rba_score_reg_workspace_f32(1, 0, 1, 1, 1, ctypes.addressof(n)) == 1 and lib.rba_score_reg_workspace_f32(1, 1, 1, 1, 1, 0) == 1
    p = 16                                                          # a non-NULL, aligned stand-in: the refusals below come before any use of it
    q = 32
    good = dict(label_bytes=8, B=1, K=19, h=2, w=2, H=4, W=4)

    def gfwd(sem=p, labels=p, ws=p, reward=p, losses=p, stats=p, R=q, **kw):
        a = {**good, **kw}
        return lib.rba_gambler_loss_fwd_f32(sem, labels, a["label_bytes"], a["B"], a["K"], a["h"], a["w"], a["H"], a["W"], 0.1, ws, reward, losses,
                                            stats, R, 0)

    def gbwd(sem=p, labels=p, R=p, stats=p, grad_loss=p, grad_R=p, grad_reward=q, grad_sem=p, **kw):
        a = {**good, **kw}
        return lib.rba_gambler_loss_bwd_f32(sem, labels, a["label_bytes"], R, a["B"], a["K"], a["h"], a["w"], a["H"], a["W"], 0.1, stats, grad_loss,
                                            grad_R, grad_reward, grad_sem, 0)

    for bad in (dict(label_bytes=4), dict(K=0), dict(K=32), dict(B=0), dict(h=0), dict(H=3), dict(W=3), dict(B=2, H=1 << 15, W=1 << 15),
                dict(K=31, h=1 << 13, w=1 << 13), dict(B=65536)):  # K + 1 = 33 channels; the blur's padding; B H W, B (K+1) h w >= 2^31; grid z
        assert gfwd(**bad) == 1 and gbwd(**bad) == 1, bad
    for arg in ("sem", "labels", "ws", "reward", "losses", "stats", "R"):
        assert gfwd(**{arg: 0}) == 1, arg
    assert gfwd(ws=18) == 1 and gfwd(reward=q) == 1                # not 4-byte aligned; the blur in place
    for arg in ("sem", "labels", "R", "stats", "grad_loss", "grad_R", "grad_reward", "grad_sem"):
        assert gbwd(**{arg: 0}) == 1, arg
    assert gbwd(grad_R=q) == 1

    def blur(fn, a=p, b=q, B=1, H=4, W=4, k=7, sigma=1.0):
        return fn(a, b, B, H, W, k, sigma, 0)

    for fn in (lib.rba_gaussian_blur_planes_f32, lib.rba_gaussian_blur_planes_adjoint_f32):
        for bad in (dict(a=0), dict(b=0), dict(b=p), dict(B=0), dict(B=65536), dict(H=3), dict(W=3), dict(k=6), dict(k=17), dict(sigma=0.0)):
            assert blur(fn, **bad) == 1, bad

    sgood = dict(label_bytes=8, B=1, h=2, w=2, H=4, W=4)

    def sfwd(score=p, labels=p, ws=p, losses=p, stats=p, **kw):
        a = {**sgood, **kw}
        return lib.rba_score_reg_fwd_f32(score, labels, a["label_bytes"], a["B"], a["h"], a["w"], a["H"], a["W"], ws, losses, stats, 0)

    def sbwd(score=p, labels=p, stats=p, gsm=p, gsp=p, grad=p, **kw):
        a = {**sgood, **kw}
        return lib.rba_score_reg_bwd_f32(score, labels, a["label_bytes"], a["B"], a["h"], a["w"], a["H"], a["W"], stats, gsm, gsp, grad, 0)

    for bad in (dict(label_bytes=4), dict(B=0), dict(h=0), dict(W=0), dict(B=2, H=1 << 15, W=1 << 15), dict(B=2, h=1 << 15, w=1 << 15)):
        assert sfwd(**bad) == 1 and sbwd(**bad) == 1, bad
    for arg in ("score", "ws", "losses", "stats"):
        assert sfwd(**{arg: 0}) == 1, arg
    assert sfwd(ws=18) == 1
    for arg in ("score", "stats", "grad"):
        assert sbwd(**{arg: 0}) == 1, arg
    assert sbwd(gsm=0, gsp=0) == 1                                  # at least one upstream gradient


def test_wrappers_have_no_cpu_path():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    from rba_amd.modeling.criterion import gambler_loss, smoothness_loss, sparsity_loss
    labels = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(RbaHipError):
        ops.gambler_loss(torch.zeros(1, 4, 2, 2), labels)
    with pytest.raises(RbaHipError):
        ops.gambler_loss_backward(torch.zeros(1, 4, 2, 2), labels, torch.zeros(4), torch.zeros(1, 4, 4), torch.ones(()))
    with pytest.raises(RbaHipError):
        ops.score_reg(torch.zeros(1, 2, 2), labels)
    with pytest.raises(RbaHipError):
        ops.score_reg_backward(torch.zeros(1, 2, 2), None, torch.zeros(2), torch.ones(()), None)
    with pytest.raises(RbaHipError):
        ops.gaussian_blur_planes(torch.zeros(1, 4, 4))
    with pytest.raises(RbaHipError):
        ops.gaussian_blur_planes_adjoint(torch.zeros(1, 4, 4))
    outputs = {"pred_logits": torch.zeros(1, 5, 4), "pred_masks": torch.zeros(1, 5, 2, 2)}
    targets = [{"outlier_masks": labels[0], "sem_seg": labels[0]}]
    with pytest.raises(RbaHipError):
        gambler_loss(outputs, targets, num_classes=3)
    with pytest.raises(ValueError, match="num_classes"):
        gambler_loss(outputs, targets, num_classes=4)
    for loss in (smoothness_loss, sparsity_loss):
        for score in ("softmax_entropy", "none"):
            with pytest.raises(ValueError, match="not built"):
                loss(outputs, targets, score=score)


def test_pebal_criterion_from_cfg_reads_the_recipe_and_the_criterion_still_refuses_its_losses(tmp_path):
    from rba_amd.modeling.criterion import PebalCriterion, SetCriterion, criterion_from_cfg, pebal_criterion_from_cfg
    cfg = G.recipe_cfg(tmp_path)
    mf = cfg["MODEL"]["MASK_FORMER"]
    assert mf["GAMBLER_LOSS"] is True and mf["SMOOTHNESS_LOSS"] is True and mf["SPARSITY_LOSS"] is True and mf["OUTLIER_SUPERVISION"] is True
    crit = pebal_criterion_from_cfg(cfg)
    assert isinstance(crit, PebalCriterion) and crit.losses == ["gambler", "smoothness", "sparsity", "outlier"]
    assert crit.num_classes == 19 and crit.ood_reg == 0.1 and crit.smoothness_score == "energy"
    assert crit.outlier == {"target": "energy", "score_norm": "none", "func": "squared_hinge", "inlier_upper_threshold": -1.0,
                            "outlier_lower_threshold": -0.1}
    want = {"gambler_loss": 1.0, "smoothness_loss": 3e-6, "sparsity_loss": 5e-4, "outlier_loss": 1.0}
    for k, w in want.items():
        assert crit.weight_dict[k] == w and crit.weight_dict[k + "_0"] == w, k
    assert not any(k.endswith("_1") for k in crit.weight_dict)      # DEC_LAYERS 2: one aux entry
    losses = {k: torch.tensor(2.0) for k in list(want) + [k + "_0" for k in want] + ["not_weighted"]}
    weighted = crit.weighted(losses)
    assert set(weighted) == set(losses) - {"not_weighted"} and float(weighted["sparsity_loss_0"]) == pytest.approx(1e-3)
    with pytest.raises(ValueError, match="gambler"):
        criterion_from_cfg(cfg)
    for name in ("gambler", "smoothness", "sparsity"):
        with pytest.raises(ValueError, match="not built"):
            SetCriterion(19, None, {}, 0.1, [name], 12544, 3.0, 0.75)

    def variant(**kw):
        v = {"MODEL": {"MASK_FORMER": dict(mf), "SEM_SEG_HEAD": dict(cfg["MODEL"]["SEM_SEG_HEAD"])}}
        v["MODEL"]["MASK_FORMER"].update(kw)
        return v

    with pytest.raises(ValueError, match="GAMBLER_LOSS"):
        pebal_criterion_from_cfg(variant(GAMBLER_LOSS=False))
    with pytest.raises(ValueError, match="DENSE_HYBRID_LOSS"):
        pebal_criterion_from_cfg(variant(DENSE_HYBRID_LOSS=True))
    for score in ("softmax_entropy", "none"):
        with pytest.raises(ValueError, match="not built"):
            pebal_criterion_from_cfg(variant(SMOOTHNESS_SCORE=score))
    nls = pebal_criterion_from_cfg(variant(SMOOTHNESS_SCORE="nls", SPARSITY_LOSS=False, OUTLIER_SUPERVISION=False, PEBAL_OOD_REG=0.25))
    assert nls.losses == ["gambler", "smoothness"] and nls.smoothness_score == "nls" and nls.ood_reg == 0.25 and nls.outlier == {}
