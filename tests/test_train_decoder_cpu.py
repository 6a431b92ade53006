"""CPU (no GPU): K3 backward's entry points are declared, bound, built and exported; build_optimizer's opt-in to the whole-decoder fine-tune
names every predictor parameter with the reference's weight-decay classes and sets the predictor's switches; without the keyword the refusal is
today's, and a trainable backbone stays refused with it."""
import ctypes
import os
import re

import pytest

from tests._solver_cases import RECIPES, recipe_cfg, tiny

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rba_masked_xattn_bwd_workspace_bytes", "rba_masked_xattn_bwd_f32")
PEBAL = RECIPES["pebal"][0]
DECAYS = ["SOLVER.WEIGHT_DECAY_NORM", "0.01", "SOLVER.WEIGHT_DECAY_EMBED", "0.02"]


def test_symbols_are_declared_bound_built_and_exported():
    from rba_amd import _lib, ops
    from rba_amd.csrc import build
    from rba_amd.modeling.transformer_decoder import mask2former_transformer_decoder as M
    assert set(NEW) <= set(_lib.SIGNATURES) and _lib.EXPECTED_ABI == 191
    assert len(_lib.SIGNATURES["rba_masked_xattn_bwd_f32"]) == 15 and len(_lib.SIGNATURES["rba_masked_xattn_bwd_workspace_bytes"]) == 4
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(REPO, "include", "rba_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint64_t\s+rba_masked_xattn_bwd_workspace_bytes\s*\(", header) and re.search(r"\bint\s+rba_masked_xattn_bwd_f32\s*\(", header)
    assert "masked_xattn_bwd.hip" in build.SOURCES
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert all(hasattr(lib, n) for n in NEW), path
        assert lib.rba_hip_version() == 191
    assert callable(ops.masked_xattn_backward) and callable(M.MaskedXattnFunction.apply)
    assert M.MultiScaleMaskedTransformerDecoder.differentiable_decoder is False


def test_entry_points_answer_without_a_launch():
    from rba_amd import _lib
    lib = _lib.load()
    assert lib.rba_masked_xattn_bwd_workspace_bytes(2, 100, 512, 8) == 2 * 8 * 100 * 16
    assert lib.rba_masked_xattn_bwd_workspace_bytes(0, 100, 512, 8) == 0 and lib.rba_masked_xattn_bwd_workspace_bytes(1, 0, 512, 8) == 0
    bad = lambda *dims: lib.rba_masked_xattn_bwd_f32(0, 0, 0, 0, 0, 0, 0, 0, 0, *dims, 0)     # noqa: E731
    assert bad(1, 4, 8, 2, 16) == 1                     # head_dim other than 32
    assert bad(1, 4, 0, 2, 32) == 1                     # no key
    assert bad(-1, 4, 8, 2, 32) == 1 and bad(1, 4, 8, 0, 32) == 1
    assert bad(1, 4, 8, 2, 32) == 0                     # no gradient asked for: a no-op
    assert bad(0, 4, 8, 2, 32) == 0


def test_build_optimizer_accepts_the_released_pebal_recipe(tmp_path):
    from rba_amd.solver import build_optimizer
    model = tiny()
    cfg = recipe_cfg(tmp_path, PEBAL, DECAYS)
    opt = build_optimizer(cfg, model, differentiable_decoder=True)
    predictor = model.sem_seg_head.predictor
    # every predictor parameter, in named_modules order (train_net.py:276-300), and nothing else
    want = [f"sem_seg_head.predictor.{m}.{n}" if m else f"sem_seg_head.predictor.{n}"
            for m, mod in predictor.named_modules() for n, _ in mod.named_parameters(recurse=False)]
    assert opt.names == want and len(want) == len(list(predictor.parameters())) > 8
    assert all(p.requires_grad for p in predictor.parameters())
    assert not any(p.requires_grad for p in model.backbone.parameters()) and not any(p.requires_grad for p in model.sem_seg_head.pixel_decoder.parameters())
    for name, wd, mult in zip(opt.names, opt.weight_decays, opt.lr_mults):
        part = name.split("predictor.")[1]
        if part.split(".")[0] in ("query_feat", "query_embed", "level_embed"):
            assert wd == 0.02, name                      # WEIGHT_DECAY_EMBED
        elif ".norm." in part or part.startswith("decoder_norm."):
            assert wd == 0.01, name                      # WEIGHT_DECAY_NORM
        else:
            assert wd == 0.05, name
        assert mult == 1.0
    assert predictor.differentiable_heads is True and predictor.deep_supervision is True and predictor.differentiable_decoder is True
    assert predictor.differentiable_ood_head is False


def test_object_queries_and_heads_only_sets(tmp_path):
    from rba_amd.solver import build_optimizer
    model = tiny()
    opt = build_optimizer(recipe_cfg(tmp_path, PEBAL, ["MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES", "True"]), model, differentiable_decoder=True)
    assert opt.names == ["sem_seg_head.predictor.query_feat.weight", "sem_seg_head.predictor.query_embed.weight"]
    assert model.sem_seg_head.predictor.differentiable_decoder is True
    model = tiny()                                        # the keyword with a heads-only cfg: the switch stays off
    opt = build_optimizer(recipe_cfg(tmp_path, PEBAL, ["MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP", "True"]), model, differentiable_decoder=True)
    assert len(opt.names) == 8 and model.sem_seg_head.predictor.differentiable_decoder is False
    assert model.sem_seg_head.predictor.differentiable_heads is True


def test_refusals_stay(tmp_path):
    from rba_amd import train_net
    from rba_amd.solver import build_optimizer
    with pytest.raises(ValueError, match=r"predictor\.\S+ would be trained.*MODEL\.FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP.*differentiable_decoder"):
        build_optimizer(recipe_cfg(tmp_path, PEBAL), tiny())
    model = tiny()
    with pytest.raises(ValueError, match=r"predictor\.query_feat\.weight would be trained.*EXCEPT_OBJECT_QUERIES"):
        build_optimizer(recipe_cfg(tmp_path, PEBAL, ["MODEL.FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES", "True"]), model)
    assert model.sem_seg_head.predictor.differentiable_decoder is False
    for opts, match in ((["MODEL.FREEZE_BACKBONE", "False"], r"backbone\.\S+ would be trained.*MODEL\.FREEZE_BACKBONE: True \(the COCO-mix and DenseHybrid recipes set such flags\)$"),
                        (["MODEL.FREEZE_PIXEL_DECODER", "False"], r"sem_seg_head\.pixel_decoder\.\S+ would be trained.*MODEL\.FREEZE_PIXEL_DECODER")):
        with pytest.raises(ValueError, match=match):
            build_optimizer(recipe_cfg(tmp_path, PEBAL, opts), tiny(), differentiable_decoder=True)
    args = train_net.build_parser().parse_args(["--config-file", "c", "--cityscapes_root", "r"])
    assert args.differentiable_decoder is False
    assert train_net.build_parser().parse_args(["--config-file", "c", "--cityscapes_root", "r", "--differentiable_decoder"]).differentiable_decoder is True
