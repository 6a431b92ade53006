"""CPU: the MiT (SegFormer) backbone's architecture layer -- config parsing with the stage-name mapping, the state-dict contract, the registry, the
torch restatement of tests/_mit_cases.py against the fixtures the reference's own module wrote (tests/golden/make_golden_mit.py), the optimizer of
the outlier-supervised recipe with the backbone frozen, and the refusals that need no device."""
import os

import pytest
import torch

from rba_amd import arch as A
from rba_amd.seeded_weights import seeded_tensor
from tests import _mit_cases as C

T = torch.from_numpy
SWIN_ONLY = ("embed_dim", "depths", "num_heads", "window_size", "patch_size", "mlp_ratio", "object_mask_threshold", "overlap_threshold")


def _cfg(tmp_path, backbone, dec_layers=None, enc_in=("stage4",), more="", opts=None):
    """a config of this test's own: the keys a MiT recipe sets (BACKBONE.NAME, the stage names, DEC_LAYERS) over a `_BASE_` file that names a ResNet
    backbone and its res2..res5 features, so that the child's names have to replace the base's"""
    from rba_amd.config import load_cfg
    (tmp_path / "base.yaml").write_text("MODEL:\n  BACKBONE:\n    NAME: build_resnet_backbone\n  SEM_SEG_HEAD:\n    IN_FEATURES: [res2, res3, res4, res5]\n"
                                        "    DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES: [res3, res4, res5]\n  MASK_FORMER:\n    DEC_LAYERS: 10\n")
    path = tmp_path / f"{backbone}.yaml"
    text = (f"_BASE_: base.yaml\nMODEL:\n  BACKBONE:\n    NAME: {backbone}\n  SEM_SEG_HEAD:\n    IN_FEATURES: [stage1, stage2, stage3, stage4]\n"
            f"    DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES: [{', '.join(enc_in)}]\n")
    if dec_layers is not None:
        text += f"  MASK_FORMER:\n    DEC_LAYERS: {dec_layers}\n"
    path.write_text(text + more)
    return load_cfg(str(path), opts)


def _same_but_swin(a, b):
    return {k: v for k, v in a.items() if k not in SWIN_ONLY} == {k: v for k, v in b.items() if k not in SWIN_ONLY}


def test_mit_configs_parse_with_the_stage_names_mapped(tmp_path):
    for name, variant in A.MIT_VARIANTS.items():
        a = A.arch_from_cfg(_cfg(tmp_path, name, dec_layers=2))
        assert a["mit"] == variant and A.backbone_name(a) == name and a["resnet"] is None
        assert a["dec_layers"] == 1 and a["enc_in"] == ["res5"] and a["size_divisibility"] == 32
        assert A.feature_channels(a) == dict(zip(A.FEATURE_NAMES, variant["embed_dims"]))
    assert _same_but_swin(A.arch_from_cfg(_cfg(tmp_path, "mit_b5", dec_layers=2)), A.complete(A.ARCHS["mit_b5_1dl"]))
    a = A.arch_from_cfg(_cfg(tmp_path, "mit_b5", enc_in=("stage3", "stage2", "stage4")))
    assert a["enc_in"] == ["res3", "res4", "res5"] and a["dec_layers"] == 9
    # the SWIN.* checks do not apply to MiT ...
    A.arch_from_cfg(_cfg(tmp_path, "mit_b2", opts=["MODEL.SWIN.APE", "True"]))
    # ... every other refusal stays, and the names must be the backbone's own
    for bad in (dict(opts=["MODEL.MASK_FORMER.PRE_NORM", "True"]), dict(enc_in=("res5",)),
                dict(opts=["MODEL.SEM_SEG_HEAD.IN_FEATURES", "[res2, res3, res4, res5]"])):
        with pytest.raises(NotImplementedError):
            A.arch_from_cfg(_cfg(tmp_path, "mit_b2", **bad))
    with pytest.raises(NotImplementedError, match="mit_b6"):
        A.arch_from_cfg(_cfg(tmp_path, "mit_b6"))


def test_registry_holds_the_six_names():
    import rba_amd.maskformer_model  # noqa: F401  (imports the backbones)
    from rba_amd.registry import BACKBONE_REGISTRY
    for name, variant in A.MIT_VARIANTS.items():
        cls = BACKBONE_REGISTRY.get(name)
        assert cls.__name__ == name
    assert A.MIT_VARIANTS["mit_b0"]["embed_dims"] == [32, 64, 160, 256] and A.MIT_VARIANTS["mit_b5"]["depths"] == [3, 6, 40, 3]
    assert all(v["num_heads"] == [1, 2, 5, 8] and v["sr_ratios"] == [8, 4, 2, 1] and v["mlp_ratio"] == 4 for v in A.MIT_VARIANTS.values())
    assert [A.MIT_VARIANTS[f"mit_b{i}"]["depths"] for i in range(1, 5)] == [[2, 2, 2, 2], [3, 4, 6, 3], [3, 4, 18, 3], [3, 8, 27, 3]]


@pytest.mark.parametrize("name", ["tiny1_mit_b0", "tiny1_mit_b1"])
def test_state_dict_contract_equals_the_references(golden, name):
    from rba_amd.maskformer_model import MaskFormer
    g = golden(f"g10_{name}_60x90")
    want = dict(zip(g["sd_keys"].tolist(), g["sd_shapes"].tolist()))
    shapes = A.state_dict_shapes(A.ARCHS[name])
    assert {k: ",".join(map(str, s)) for k, (s, _) in shapes.items()} == want
    sd = MaskFormer(A.ARCHS[name]).state_dict()
    assert {k: ",".join(map(str, v.shape)) for k, v in sd.items()} == want
    stage1 = [k for k in want if k.startswith("backbone.block4.0.attn.")]
    assert not any(".sr." in k or ".attn.norm." in k for k in stage1), "sr_ratio 1 has neither attn.sr nor attn.norm"


def _close(got, g, key, where, key64=None):
    """double: 1e-12 relative to the fixture's float64 output; float: within the reference's own fp32-vs-float64 distance on that tensor"""
    want32, want64 = T(g[key]), T(g[key64 or key + "64"])
    own = (want32.double() - want64).abs().max().item()
    err64 = (got[1] - want64).abs().max().item()
    err32 = (got[0].double() - want32.double()).abs().max().item()
    print(f"{where}: restatement fp64 err {err64:.3g}, fp32 err {err32:.3g}, the reference's own fp32 distance {own:.3g}")
    assert err64 <= 1e-12 * max(1.0, want64.abs().max().item()), where
    assert err32 <= own, where


def _seeded(keys, prefix, shapes, dtype):
    return {prefix + k: seeded_tensor(prefix + k, torch.empty(shapes[k]), 0).to(dtype) for k in keys}


def test_restatement_equals_the_parts_fixture(golden):
    g = golden("g10_mit_parts")
    for stage in (1, 2, 3, 4):
        Cn, nH, sr, H, W = g[f"block{stage}_cfg"].tolist()
        p = f"backbone.block{stage}.0"
        mit = dict(embed_dims=[Cn] * 4, num_heads=[nH] * 4, depths=[1] * 4, sr_ratios=[sr] * 4, mlp_ratio=4)
        shapes = {k[len("backbone.block1.0."):]: s for k, (s, _) in A.state_dict_shapes(dict(A.ARCHS["tiny1_mit_b0"], mit=mit)).items()
                  if k.startswith("backbone.block1.0.")}
        assert sorted(shapes) == g[f"block{stage}_keys"].tolist()
        x = T(g[f"block{stage}_x"])
        for tag, xs in (("unit", x), ("small", x * 0.01)):
            got = [C.block(xs.to(dt), H, W, _seeded(shapes, p + ".", shapes, dt), p, nH, sr) for dt in (torch.float32, torch.float64)]
            _close(got, g, f"block{stage}_{tag}_out", f"block sr={sr} {tag}")
    for tag, p in (("pe7", "backbone.patch_embed1"), ("pe3", "backbone.patch_embed2")):
        k, s, cin, cout, H, W = g[f"{tag}_cfg"].tolist()
        shapes = {"proj.weight": (cout, cin, k, k), "proj.bias": (cout,), "norm.weight": (cout,), "norm.bias": (cout,)}
        got = [C.patch_embed(T(g[f"{tag}_x"]).to(dt), _seeded(shapes, p + ".", shapes, dt), p, k, s)[0] for dt in (torch.float32, torch.float64)]
        _close(got, g, f"{tag}_out", tag)
    Cn, hidden, H, W = g["mlp_cfg"].tolist()
    p = "backbone.block1.1.mlp"
    shapes = {"fc1.weight": (hidden, Cn), "fc1.bias": (hidden,), "dwconv.dwconv.weight": (hidden, 1, 3, 3), "dwconv.dwconv.bias": (hidden,),
              "fc2.weight": (Cn, hidden), "fc2.bias": (Cn,)}
    got = [C.mlp(T(g["mlp_x"]).to(dt), H, W, _seeded(shapes, p + ".", shapes, dt), p) for dt in (torch.float32, torch.float64)]
    _close(got, g, "mlp_out", "mlp")


def test_low_variance_input_tells_the_eps_apart(golden):
    """on the tokens scaled by 0.01 a block norm with eps 1e-5 instead of 1e-6 is off by percents; at unit scale it is not"""
    g = golden("g10_mit_parts")
    Cn, nH, sr, H, W = g["block1_cfg"].tolist()
    p = "backbone.block1.0"
    shapes = {k[len(p) + 1:]: s for k, (s, _) in A.state_dict_shapes(A.ARCHS["tiny1_mit_b0"]).items() if k.startswith(p + ".")}
    sd = _seeded(shapes, p + ".", shapes, torch.float64)
    x = T(g["block1_x"]).double() * 0.01
    y6 = torch.nn.functional.layer_norm(x, (Cn,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-6)
    y5 = torch.nn.functional.layer_norm(x, (Cn,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5)
    assert ((y6 - y5).abs().max() / y6.abs().max()).item() > 0.02


@pytest.mark.parametrize("name", ["tiny1_mit_b0", "tiny1_mit_b1"])
def test_restatement_equals_the_end_to_end_fixtures_features(golden, name):
    g = golden(f"g10_{name}_60x90")
    a = A.complete(A.ARCHS[name])
    assert str(g["arch"]) == name and len(g["neartie_idx"]) <= 0.01 * 60 * 90
    sd = A.seeded_weights(a, int(g["seed"]))
    image = T(g["image"]).float()
    x = (image - torch.tensor(a["pixel_mean"]).view(-1, 1, 1)) / torch.tensor(a["pixel_std"]).view(-1, 1, 1)
    x = torch.nn.functional.pad(x, (0, 96 - 90, 0, 64 - 60))[None]
    f32, f64 = C.backbone(x, sd, a["mit"]), C.backbone(x.double(), C.cast(sd, torch.float64), a["mit"])
    for k in ("res4", "res5"):                 # the float64 forward is stored for the two last stages: every earlier stage feeds them
        _close((f32[k][0], f64[k][0]), g, "feat_" + k, f"{name} {k}", key64="feat64_" + k)
    for k in ("res2", "res3"):                 # fp32 only: within the reference's fp32 distance from the float64 restatement pinned above
        want32 = T(g["feat_" + k]).double()
        assert (f32[k][0].double() - want32).abs().max().item() <= (want32 - f64[k][0]).abs().max().item(), k


def test_coco_mix_recipe_builds_its_optimizer_with_the_backbone_frozen(tmp_path):
    """the outlier-supervised MiT recipe freezes the backbone and the pixel decoder and nothing else: the whole transformer decoder trains, which
    build_optimizer takes with differentiable_decoder (as the released PEBAL recipe); no backbone parameter is trainable afterwards"""
    from rba_amd.maskformer_model import MaskFormer
    from rba_amd.solver import build_optimizer
    solver = open(os.path.join(os.path.dirname(__file__), "golden", "solver", "base_solver.yaml")).read()
    more = ("    OUTLIER_SUPERVISION: True\n    OUTLIER_LOSS_TARGET: nls\n  FREEZE_PIXEL_DECODER: True\n  FREEZE_BACKBONE: True\n" + solver)
    cfg = _cfg(tmp_path, "mit_b0", dec_layers=2, more=more)
    assert A.arch_from_cfg(cfg)["mit"] == A.MIT_VARIANTS["mit_b0"]
    model = MaskFormer(A.ARCHS["tiny1_mit_b0"])
    with pytest.raises(ValueError, match="sem_seg_head.predictor"):
        build_optimizer(cfg, model)
    build_optimizer(cfg, model, differentiable_decoder=True)
    assert not any(p.requires_grad for p in model.backbone.parameters())
    assert not any(p.requires_grad for p in model.sem_seg_head.pixel_decoder.parameters())
    assert all(p.requires_grad for p in model.sem_seg_head.predictor.parameters())


def test_refusals_by_name():
    from rba_amd import mit_ops
    from rba_amd._lib import RbaHipError
    from rba_amd.maskformer_model import MaskFormer
    backbone = MaskFormer(A.ARCHS["tiny1_mit_b0"]).backbone
    assert backbone.size_divisibility == 32
    for hw in ((60, 96), (64, 90), (48, 64)):
        with pytest.raises(RbaHipError, match="multiple of 32"):
            backbone(torch.zeros(1, 3, *hw))
    with pytest.raises(RbaHipError, match="C % 4 == 0"):
        mit_ops._channels4(130, "dwconv3x3_gelu")
    for Cn, nH in ((96, 2), (128, 8), (128, 1), (64, 0), (100, 3)):
        with pytest.raises(RbaHipError, match="head_dim"):
            mit_ops._heads(Cn, nH, "sr_attention")
    with pytest.raises(RbaHipError, match="head_dim"):
        MaskFormer(dict(A.ARCHS["tiny1_mit_b0"], mit=dict(A.MIT_VARIANTS["mit_b0"], num_heads=[2, 2, 5, 8])))
    assert mit_ops._heads(160, 5, "x") == 32 and mit_ops._heads(512, 8, "x") == 64 and mit_ops.padded_columns(7, 3) == 160
