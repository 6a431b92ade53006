"""Test-time augmentation without a GPU: the Pillow restatements against Pillow, Detectron2's shortest-edge rule, DatasetMapperTTA on the host, the
TEST.AUG config keys, the two new entry points in both libraries, the --tta flag, and the merge fixture's own conditions."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import _tta_cases as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_id = lambda s: "{}x{}to{}x{}".format(*s[0], *s[1])


@pytest.mark.parametrize("i", range(len(G.RESIZE_SHAPES)), ids=[_id(s) for s in G.RESIZE_SHAPES])
def test_numpy_restatements_equal_pillow_in_every_byte(i):
    Image = pytest.importorskip("PIL.Image")
    from rba_amd.test_time_augmentation import pil_bilinear_resize_numpy
    (h, w), (H, W) = G.RESIZE_SHAPES[i]
    img, want = G.resize_case(i)
    pil = np.asarray(Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).resize((W, H), Image.BILINEAR)).transpose(2, 0, 1)
    assert want.shape == (3, H, W) and np.array_equal(want, pil)                              # the tests' loops
    assert np.array_equal(pil_bilinear_resize_numpy(img, (H, W)), pil)                        # the product's tables (what K12b is handed)


def test_product_tables_equal_the_loops():
    """ops.pil_bilinear_coeffs (vectorised, what the device kernel reads) against the plain loops, also at the recipe's sizes"""
    from rba_amd.ops import pil_bilinear_coeffs
    for n_in, n_out in ((9, 20), (64, 32), (70, 25), (5, 1), (1, 5), (1024, 1792), (2048, 3584), (2048, 1024), (1024, 768), (1000, 7)):
        kk, bounds, ksize = pil_bilinear_coeffs(n_in, n_out)
        ks, rows = G.pil_axis_table(n_in, n_out)
        assert ksize == ks and kk.shape == (n_out, ks) and bounds.shape == (n_out, 2) and kk.dtype == np.int32 and bounds.dtype == np.int32
        for xx, (xmin, k) in enumerate(rows):
            assert tuple(bounds[xx]) == (xmin, len(k)) and list(kk[xx, : len(k)]) == k and not kk[xx, len(k):].any(), (n_in, n_out, xx)
        assert (bounds[:, 0] >= 0).all() and (bounds[:, 1] <= ks).all() and (bounds.sum(1) <= n_in).all()     # what the kernel relies on


def test_resize_shortest_edge_shape():
    from rba_amd.test_time_augmentation import resize_shortest_edge_shape as f
    assert f(1024, 2048, 512, 4096) == (512, 1024)
    assert f(1024, 2048, 1792, 4096) == (1792, 3584)
    assert f(2048, 1024, 768, 4096) == (1536, 768)                    # portrait: the width is the short edge
    assert f(1024, 2048, 1792, 3000) == (1500, 3000)                  # max_size binds: 1792 x 3584 scaled by 3000 / 3584
    assert f(100, 333, 50, 160) == (48, 160)                          # binds, 50 * 160 / 166.5 = 48.048 -> 48
    assert f(48, 96, 32, 4096) == (32, 64)
    assert f(10, 25, 3, 4096) == (3, 8)                               # 7.5 rounds up
    assert f(20, 50, 5, 4096) == (5, 13)                              # 12.5 rounds up
    assert f(10, 23, 5, 4096) == (5, 12)                              # 11.5 rounds up: int(v + 0.5), not round-half-even
    assert f(8, 17, 4, 4096) == (4, 9)                                # 8.5 rounds up (round-half-even would give 8)
    assert f(7, 7, 9, 4096) == (9, 9)


def test_test_aug_is_read_from_the_settings_fixture_and_defaults_are_detectron2s(tmp_path):
    from rba_amd.config import load_cfg
    from rba_amd.test_time_augmentation import tta_enabled
    cfg = load_cfg(os.path.join(REPO, "tests", "golden", "tta", "test_aug.yaml"))
    aug = cfg.TEST.AUG
    assert list(aug.MIN_SIZES) == [512, 768, 1024, 1280, 1536, 1792] and aug.MAX_SIZE == 4096 and aug.FLIP is True and aug.ENABLED is False
    assert not tta_enabled(cfg)
    assert tta_enabled(load_cfg(os.path.join(REPO, "tests", "golden", "tta", "test_aug.yaml"), ["TEST.AUG.ENABLED", "True"]))
    # a config without the keys: Detectron2's defaults
    (tmp_path / "bare.yaml").write_text("MODEL:\n  META_ARCHITECTURE: MaskFormer\n")
    aug = load_cfg(str(tmp_path / "bare.yaml")).TEST.AUG
    assert dict(aug) == {"ENABLED": False, "MIN_SIZES": list(range(400, 1201, 100)), "MAX_SIZE": 4000, "FLIP": True}
    assert not tta_enabled(load_cfg(str(tmp_path / "bare.yaml")))


def test_dataset_mapper_tta_on_the_recipe():
    pytest.importorskip("PIL.Image")
    from rba_amd.config import load_cfg
    from rba_amd.test_time_augmentation import DatasetMapperTTA
    cfg = load_cfg(os.path.join(REPO, "tests", "golden", "tta", "test_aug.yaml"))
    mapper = DatasetMapperTTA(cfg)
    assert mapper.view_shapes(1024, 2048) == [(s, 2 * s, f) for s in (512, 768, 1024, 1280, 1536, 1792) for f in (False, True)]
    # the same rule on a small image, through the pixels: 16 x 32 asked at 1024 x 2048
    small = load_cfg(os.path.join(REPO, "tests", "golden", "tta", "test_aug.yaml"), ["TEST.AUG.MIN_SIZES", "[8, 12, 16, 20, 24, 28]"])
    image = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (3, 16, 32), dtype=np.uint8))
    views = DatasetMapperTTA(small)({"image": image, "height": 1024, "width": 2048, "file_name": "x.png"})
    assert len(views) == 12
    for i, v in enumerate(views):
        s, flipped = (8, 12, 16, 20, 24, 28)[i // 2], bool(i % 2)
        assert v["height"] == 1024 and v["width"] == 2048 and v["file_name"] == "x.png"
        assert v["image"].dtype == torch.uint8 and tuple(v["image"].shape) == (3, s, 2 * s) and v["image"].is_contiguous()
        want = G.pil_bilinear_resize(image.numpy(), (s, 2 * s))
        assert np.array_equal(v["image"].numpy(), want[:, :, ::-1] if flipped else want), i
        assert v["transforms"] == [("resize", 16, 32, 1024, 2048), ("resize", 16, 32, s, 2 * s)] + ([("hflip", 2 * s)] if flipped else [])
    # no flip: one view per size; float images go through F.interpolate
    nof = DatasetMapperTTA(G.aug_cfg((8, 16), 4096, False))({"image": image.float()})
    assert [tuple(v["image"].shape) for v in nof] == [(3, 8, 16), (3, 16, 32)] and nof[1]["image"].dtype == torch.float32
    assert torch.equal(nof[1]["image"], image.float()) and "height" not in nof[0]


def test_new_entry_points_are_exported_by_both_libraries_and_bound():
    from rba_amd import _lib
    for name in ("rba_tta_merge_f32", "rba_resize_u8_pil_bilinear"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rba_tta_merge_f32"]) == 10 and len(_lib.SIGNATURES["rba_resize_u8_pil_bilinear"]) == 16
    assert _lib.EXPECTED_ABI == 191
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        syms = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout.split()
        assert "rba_tta_merge_f32" in syms and "rba_resize_u8_pil_bilinear" in syms, path
    import ctypes
    assert ctypes.sizeof(_lib.TtaViews) == 16 * 8 + 3 * 16 * 4                    # rba_tta_views of include/rba_hip.h
    hdr = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    assert "#define RBA_TTA_MAX_VIEWS 16" in hdr and "int rba_tta_merge_f32(" in hdr and "int rba_resize_u8_pil_bilinear(" in hdr


def test_tta_flag_parses_and_defaults_to_off():
    import argparse
    from rba_amd import evaluate_ood as E
    p = E.build_parser()
    assert p.parse_args([]).tta is False and p.parse_args(["--tta"]).tta is True
    # off and not enabled in the config: the model and the arguments pass through untouched
    args = p.parse_args(["--streams", "3"])
    sentinel = object()
    assert E.with_tta(sentinel, G.aug_cfg((32,), 4096, True), args) == (sentinel, args)
    # on (by the flag, or by the config): wrapped, and the loop is the serial one without graph capture
    class Model(torch.nn.Module):
        device = torch.device("cpu")
    for a, cfg in ((p.parse_args(["--tta"]), G.aug_cfg((32,), 4096, True)), (p.parse_args([]), G.aug_cfg((32,), 4096, True, enabled=True))):
        wrapped, run_args = E.with_tta(Model(), cfg, a)
        from rba_amd.test_time_augmentation import SemanticSegmentorWithTTA
        assert isinstance(wrapped, SemanticSegmentorWithTTA) and isinstance(run_args, argparse.Namespace)
        assert (run_args.streams, run_args.graph) == (1, 0) and a.streams == 3 and a.graph == 1
        assert not hasattr(wrapped, "graph_replay") and not hasattr(wrapped, "_graphed_scores") and wrapped.device == torch.device("cpu")


@pytest.mark.parametrize("name", sorted(G.MERGE_CASES))
def test_merge_fixture_conditions_hold(name):
    """merge_truth asserts them: undecided argmax pixels <= 1 % of the map, no fp32 flip on a decided one"""
    t = G.merge_truth(name)
    K, size, spec = G.MERGE_CASES[name]
    assert t["sem64"].shape == (K,) + size and t["sem64"].dtype == torch.float64
    print(name, "undecided", int((~t["decided"]).sum()), "of", t["decided"].numel(), "b_sem", t["b_sem"], "b_score", t["b_score"])


def test_unfused_wrapper_arithmetic_on_the_cpu():
    """the reference's sequence as the wrapper states it for K > 32 / more than 16 views, against the restatement -- identity-size views only (the
    resize of other sizes is a HIP kernel)"""
    from rba_amd.test_time_augmentation import SemanticSegmentorWithTTA as W
    views = [torch.rand(3, 5, 7, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    keep = [v.clone() for v in views]
    flips = [False, True, False]
    assert torch.equal(W._unfused_mean(views, flips, (5, 7)), G.ref_merge(views, flips, (5, 7)))
    assert all(torch.equal(a, b) for a, b in zip(views, keep))                     # the first view's own map is not the accumulator
