"""K8 (point-sampled mask losses and the matcher's cost), everything that needs no GPU: the ABI surface, the restatement the GPU tests use as truth
against the mathematics (grid_sample, gradcheck in double, the softplus identity, the planted assignment), and the criterion's host logic."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from tests import _point_loss_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FINETUNE_YAML = os.path.join(REPO, "tests", "golden", "k1_backward", "maskformer2_swin_base_IN21k_384_bs16_90k_1dl_coco_mix_finetune.yaml")
NEW = ("rba_point_sample_f32", "rba_mask_point_loss_fwd_f32", "rba_mask_point_loss_bwd_f32", "rba_match_cost_workspace_f32", "rba_match_cost_f32")


def test_header_declares_the_entry_points():
    text = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", flat), name
    assert "int rba_match_cost_workspace_f32(int Q, int T, int P, int64_t* bytes);" in flat
    assert "may differ from launch to launch" in text and "matcher.py:105-149" in text


@pytest.mark.parametrize("lib", ["librba_hip.so", "librba_hip_knobs.so"])
def test_libraries_export_the_entry_points(lib):
    path = os.path.join(REPO, "rba_amd", "csrc", lib)
    assert os.path.exists(path), f"{lib} is not built"
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    syms = {ln.split()[-1]: ln.split()[-2] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert syms.get(name) == "T", f"{lib} does not export {name}"


def test_bindings_and_refusals_without_a_device():
    from rba_amd import _lib, ops
    assert set(NEW) <= set(_lib.SIGNATURES) and _lib.EXPECTED_ABI == 191
    with pytest.raises(ops.RbaHipError, match="no CPU path"):
        ops.point_sample(torch.zeros(2, 3, 4), torch.zeros(2, 5, 2))
    with pytest.raises(ops.RbaHipError, match="no CPU path"):
        ops.match_cost(torch.zeros(2, 3, 4), torch.zeros(1, 6, 8), torch.zeros(5, 2), torch.zeros(2, 3), torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ops.RbaHipError, match="no CPU path"):
        ops.mask_point_loss(torch.zeros(1, 2, 3, 4), torch.zeros(1, dtype=torch.int64), torch.zeros(1, 5, 2), torch.zeros(1, 5), 1.0)
    lib = _lib.load()                                              # argument errors come back without a launch, so without a device too
    assert lib.rba_point_sample_f32(0, 0, 0, 0, 1, 1, 0, 4, 4, 0, 0) == 1 and lib.rba_match_cost_workspace_f32(0, 1, 1, 0) == 1
    assert lib.rba_mask_point_loss_fwd_f32(0, 0, 0, 0, 0, 0, 4, 1, 2, 2, 3, 1.0, 0) == 1
    assert lib.rba_mask_point_loss_bwd_f32(0, 0, 0, 0, 0, 0, 0, 0, 4, 1, 2, 2, 3, 1.0, 0) == 1
    assert lib.rba_match_cost_f32(0, 0, 0, 0, 0, 0, 3, 2, 5, 4, 4, 8, 8, 3, 1.0, 1.0, 1.0, 0, 0, 0) == 1


def test_restated_point_sample_is_grid_sample_and_returns_pixels_at_centres():
    for shape in C.SAMPLE_SHAPES[:4]:
        planes, coords, centres = C.sample_inputs(shape, False)
        N = shape[0]
        got = C.ref_point_sample(planes.double()[:N], coords.double())
        finite = coords.abs().amax(-1) < 1e6                     # grid_sample's own arithmetic overflows at 1e30; the restatement gives 0 there
        want = F.grid_sample(planes.double()[:N, None], (2.0 * coords.double() - 1.0)[:, :, None], mode="bilinear", padding_mode="zeros",
                             align_corners=False)[:, 0, :, 0]
        assert torch.allclose(got[finite], want[finite], rtol=0, atol=1e-12)
        assert bool((got[~finite] == 0).all())
        assert centres
        got32 = C.ref_point_sample(planes[:N], coords)
        for p, y, x in centres:
            assert torch.equal(got32[:, p], planes[:N, y, x])
    idx = torch.tensor([2, 0, 2])
    planes, coords, _ = C.sample_inputs(C.SAMPLE_SHAPES[0], True)
    assert torch.equal(C.ref_point_sample(planes, coords, idx), C.ref_point_sample(planes[idx], coords.expand(3, -1, -1)))


def test_restated_losses_gradcheck():
    gen = torch.Generator().manual_seed(5)
    pred = torch.randn(2, 3, 4, 5, generator=gen).double().requires_grad_(True)
    index, coords = torch.tensor([4, 1, 3]), torch.rand(3, 6, 2, generator=gen).double() * 1.1 - 0.05
    labels = torch.rand(3, 6, generator=gen).double()
    for k in (0, 1):
        assert torch.autograd.gradcheck(lambda p: C.ref_mask_losses(p, index, coords, labels, 2.0)[k], (pred,), eps=1e-6, atol=1e-7, rtol=1e-5)
    # against the reference's formulas on sampled logits, written the short way
    x = C.ref_point_sample(pred.detach().flatten(0, 1), coords, index)
    lm, ld = C.ref_mask_losses(pred.detach(), index, coords, labels, 2.0)
    bce = (x.clamp(min=0) - x * labels + torch.log1p(torch.exp(-x.abs()))).mean(1).sum() / 2.0
    assert abs(float(lm - bce)) < 1e-14


def test_softplus_identity_of_the_matcher_cost():
    """pos t + neg (1 - t) = softplus(x) - x t: the kernel's form against the un-rewritten one, in double"""
    pred, tgt, coords, logits, ids = C.cost_inputs((100, 7, 333))
    c64, _ = C.cost_truth((100, 7, 333))
    x = C.ref_point_sample(pred.double(), coords.double()[None])
    t = C.ref_point_sample(tgt.double(), coords.double()[None])
    wm, wc, wd = C.COST_WEIGHTS
    s = x.sigmoid()
    mine = (wm * (F.softplus(x).sum(-1)[:, None] - x @ t.T) / x.shape[1] - wc * logits.double().softmax(-1)[:, ids]
            + wd * (1 - (2 * s @ t.T + 1) / (s.sum(-1)[:, None] + t.sum(-1)[None] + 1)))
    assert float((mine - c64).abs().max()) < 1e-13 * float(c64.abs().max())


def test_restated_matcher_returns_the_planted_assignment():
    from scipy.optimize import linear_sum_assignment
    logits, pred, targets, coords = C.planted()
    c64, rows, margin, bound = C.planted_assignment(logits[0], pred[0], targets[0], coords)
    print(f"margin {margin:.3e} against {bound:.3e}")
    i, j = linear_sum_assignment(c64.numpy())
    assert sorted(zip(i.tolist(), j.tolist())) == sorted(zip(rows.tolist(), range(len(rows))))
    assert rows.tolist() == targets[0]["rows"].tolist()


def test_restated_selection_is_topk_of_uncertainty():
    pred, index, _, _, _ = C.loss_inputs((9, 32, 64, 448))
    cand = torch.rand(9, 40, 2, generator=torch.Generator().manual_seed(3))
    idx, mag = C.ref_select(pred.double(), index, cand.double(), 10)
    for n in range(9):
        assert float(mag[n, idx[n]].max()) <= float(mag[n][[k for k in range(40) if k not in idx[n].tolist()]].min())


def _finetune_cfg(tmp_path):
    from rba_amd.config import load_cfg
    d = tmp_path / "swin" / "single_decoder_layer"
    d.mkdir(parents=True)
    shutil.copy(FINETUNE_YAML, d / os.path.basename(FINETUNE_YAML))
    # the recipe's _BASE_ chain, stood in for by the criterion keys it sets (maskformer2_R50_bs16_90k.yaml of the reference)
    (tmp_path / "maskformer2_R50_bs16_90k.yaml").write_text(
        "MODEL:\n  SEM_SEG_HEAD:\n    NUM_CLASSES: 19\n  MASK_FORMER:\n    DEEP_SUPERVISION: True\n    NO_OBJECT_WEIGHT: 0.1\n    CLASS_WEIGHT: 2.0\n"
        "    MASK_WEIGHT: 5.0\n    DICE_WEIGHT: 5.0\n    TRAIN_NUM_POINTS: 12544\n    OVERSAMPLE_RATIO: 3.0\n    IMPORTANCE_SAMPLE_RATIO: 0.75\n")
    return load_cfg(str(d / os.path.basename(FINETUNE_YAML)))


def test_criterion_from_cfg_reads_the_finetune_recipe(tmp_path):
    from rba_amd.modeling.criterion import SetCriterion, criterion_from_cfg
    from rba_amd.modeling.matcher import HungarianMatcher
    crit = criterion_from_cfg(_finetune_cfg(tmp_path))
    assert isinstance(crit, SetCriterion) and crit.losses == ["labels", "masks", "outlier"]
    assert (crit.num_classes, crit.eos_coef, crit.num_points, crit.oversample_ratio, crit.importance_sample_ratio) == (19, 0.1, 12544, 3.0, 0.75)
    m = crit.matcher
    assert isinstance(m, HungarianMatcher) and (m.cost_class, m.cost_mask, m.cost_dice, m.num_points) == (2.0, 5.0, 5.0, 12544)
    base = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "smoothness_loss": 3e-6, "sparsity_loss": 5e-4, "outlier_loss": 1.0, "gambler_loss": 1.0,
            "densehybrid_loss": 1.0}
    assert crit.weight_dict == {**base, **{f"{k}_0": v for k, v in base.items()}}            # DEC_LAYERS: 2 -> one aux entry
    assert crit.outlier == dict(target="nls", score_norm="tanh", func="squared_hinge", inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)
    one = torch.ones(())
    assert crit.weighted({"loss_ce": one, "loss_mask_0": one, "accuracy": one}) == {"loss_ce": 2.0 * one, "loss_mask_0": 5.0 * one}


def test_criterion_defaults_and_refusals():
    from rba_amd.modeling.criterion import SetCriterion, criterion_from_cfg
    from rba_amd.modeling.matcher import FixedMatcher, HungarianMatcher
    crit = criterion_from_cfg({"MODEL": {"MASK_FORMER": {}}})
    assert crit.losses == ["labels", "masks"] and crit.weight_dict["loss_mask"] == 20.0 and "loss_ce_4" in crit.weight_dict and crit.outlier == {}
    for key, name in (("SMOOTHNESS_LOSS", "smoothness"), ("SPARSITY_LOSS", "sparsity"), ("GAMBLER_LOSS", "gambler"), ("DENSE_HYBRID_LOSS", "densehybrid")):
        with pytest.raises(ValueError, match=name):
            criterion_from_cfg({"MODEL": {"MASK_FORMER": {key: True}}})
        with pytest.raises(ValueError, match=name):
            SetCriterion(19, FixedMatcher(), {}, 0.1, ["labels", name], 16, 3.0, 0.75)
    with pytest.raises(ValueError, match="not defined"):
        criterion_from_cfg({"MODEL": {"MASK_FORMER": {"MATCHER": "Greedy"}}})
    with pytest.raises(ValueError, match="object queries"):
        criterion_from_cfg({"MODEL": {"MASK_FORMER": {"MATCHER": "FixedMatcher"}}})
    with pytest.raises(ValueError):
        HungarianMatcher(0, 0, 0, 4)
    crit = SetCriterion(3, FixedMatcher(), {"loss_ce": 1.0}, 0.1, ["labels", "masks"], 16, 3.0, 0.75)
    outputs = {"pred_logits": torch.zeros(1, 3, 4), "pred_masks": torch.zeros(1, 3, 2, 2), "aux_outputs": [{"pred_logits": torch.zeros(1, 3, 4)}]}
    with pytest.raises(ValueError, match="pred_masks"):
        crit(outputs, [{"labels": torch.tensor([1]), "masks": torch.zeros(1, 4, 4)}])


def test_fixed_matcher_and_empty_targets():
    from rba_amd.modeling.matcher import FixedMatcher, HungarianMatcher
    out = FixedMatcher()({}, [{"labels": torch.tensor([2, 0])}])
    assert out[0][0].tolist() == [2, 0] and out[0][1].tolist() == [0, 1] and out[0][0].dtype == torch.int64
    empty = {"labels": torch.zeros(0, dtype=torch.int64), "masks": torch.zeros(0, 4, 4)}
    (i, j), = HungarianMatcher(1, 1, 1, 4)({"pred_logits": torch.zeros(1, 3, 4), "pred_masks": torch.zeros(1, 3, 2, 2)}, [empty])   # no launch: CPU tensors pass
    assert i.numel() == 0 and j.numel() == 0 and i.dtype == torch.int64


def test_loss_labels_is_the_restatement_and_empty_loss_masks_is_zero():
    from rba_amd.modeling.criterion import loss_labels, loss_masks
    gen = torch.Generator().manual_seed(9)
    logits = torch.randn(2, 6, 5, generator=gen)
    targets = [{"labels": torch.tensor([1, 3]), "masks": torch.zeros(2, 4, 4)}, {"labels": torch.tensor([0]), "masks": torch.zeros(1, 4, 4)}]
    indices = [(torch.tensor([4, 2]), torch.tensor([1, 0])), (torch.tensor([5]), torch.tensor([0]))]
    got = loss_labels({"pred_logits": logits}, targets, indices, num_classes=4, eos_coef=0.1)["loss_ce"]
    assert torch.allclose(got, C.ref_loss_labels(logits, targets, indices, 4, 0.1), rtol=1e-6, atol=0)
    pred = torch.randn(2, 6, 3, 3, generator=gen).requires_grad_(True)                       # no matched mask: zeros, differentiable, no launch (CPU tensors pass)
    none = [(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))] * 2
    losses = loss_masks({"pred_masks": pred}, targets, none, 1.0, num_points=8, oversample_ratio=3.0, importance_sample_ratio=0.75)
    assert float(losses["loss_mask"].detach()) == 0.0 and float(losses["loss_dice"].detach()) == 0.0
    (losses["loss_mask"] + losses["loss_dice"]).backward()
    assert pred.grad is not None and float(pred.grad.abs().max()) == 0.0
