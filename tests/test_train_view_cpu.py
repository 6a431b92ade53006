"""CPU (no GPU): the COCO-mix mapper's host logic.  The host composition of rba_amd.dataset_mappers against the plain restatement of
tests/_train_view_cases.py, the label rule against F.interpolate, the HSV restatement's own properties (and cv2 where cv2 imports), the draw order of
sample_train_view_params on recorded generators, the three paste cases, the refusals, the INPUT defaults and the three recipes, CocoOodObjects on a temp
tree, prepare_targets, and K14's entry point declared, bound, built and refusing malformed calls without a launch."""
import ctypes
import os
import random
import shutil

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _train_view_cases as C

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECIPES = ("k1_backward/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_coco_mix_finetune.yaml",
           "dense_hybrid/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_densehybrid_cocomix_finetune.yaml",
           "pebal/maskformer2_swin_base_IN21k_384_bs16_90k_1dl_pebal_finetune.yaml")
# the INPUT block of the recipes' _BASE_ chain (Base-Cityscapes-SemanticSegmentation.yaml of the reference), as settings
BASE_INPUT = ("INPUT:\n  MIN_SIZE_TRAIN: !!python/object/apply:eval [\"[int(x * 0.1 * 1024) for x in range(5, 21)]\"]\n"
              "  MIN_SIZE_TRAIN_SAMPLING: \"choice\"\n  MIN_SIZE_TEST: 1024\n  MAX_SIZE_TRAIN: 4096\n  MAX_SIZE_TEST: 2048\n"
              "  CROP:\n    ENABLED: True\n    TYPE: \"absolute\"\n    SIZE: (512, 1024)\n    SINGLE_CATEGORY_MAX_AREA: 1.0\n"
              "  COLOR_AUG_SSD: True\n  SIZE_DIVISIBILITY: -1\n  FORMAT: \"RGB\"\n  DATASET_MAPPER_NAME: \"mask_former_semantic\"\n")


def _recipe_cfg(tmp_path, recipe):
    from rba_amd.config import load_cfg
    d = tmp_path / "a" / "b"
    d.mkdir(parents=True, exist_ok=True)
    shutil.copy(os.path.join(REPO, "tests", "golden", recipe), d / os.path.basename(recipe))
    base = open(os.path.join(REPO, "tests", "golden", recipe)).readline().split(":", 1)[1].strip()          # _BASE_: ../(../)maskformer2_R50_bs16_90k.yaml
    assert os.path.basename(base) == "maskformer2_R50_bs16_90k.yaml"
    # the recipe's _BASE_ chain, stood in for by the keys the mapper reads (as tests/test_point_loss_cpu.py does for the criterion's)
    (d / base).resolve().write_text("MODEL:\n  SEM_SEG_HEAD:\n    NUM_CLASSES: 19\n    IGNORE_VALUE: 255\n" + BASE_INPUT)
    return load_cfg(str(d / os.path.basename(recipe)))


def _settings(**kw):
    from rba_amd.dataset_mappers import MapperSettings
    base = dict(min_sizes=(12, 17, 24, 31, 48), max_size=4096, crop_enabled=True, crop_type="absolute", crop_size=(12, 24), color_aug=True)
    base.update(kw)
    return MapperSettings(**base)


# ---------------------------------------------------------------------------------------------------------------- the host composition
@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("name", sorted(C.GEOMETRY))
def test_host_composition_equals_the_restatement(name, flip):
    from rba_amd.dataset_mappers import train_view_host
    src = C.GEOMETRY[name][0]
    img, lab = C.frame(*src)
    color = C.color_cases()["all_order1" if flip else "all_order0"] if name.startswith("e") else None
    p = C.params_of(name, flip=flip, color=color)
    C.check_equal(train_view_host(img, lab, p), C.ref_view(img, lab, p), name)


@pytest.mark.parametrize("paste", sorted(C.PASTES))
def test_host_composition_with_a_paste_a_table_and_a_canvas(paste):
    from rba_amd.dataset_mappers import train_view_host
    from rba_amd.sem_seg_datasets import cityscapes_lut
    (bh, bw), holes, pos, geometry = C.PASTES[paste]
    img, lab = C.frame(24, 48, raw_ids=True)
    obj, objmask = C.ood_object(bh, bw, holes)
    p = C.params_of(geometry, flip=paste == "holes", color=C.color_cases()["all_order0"], paste=pos)
    got = train_view_host(img, lab, p, obj, objmask, cityscapes_lut(), pad_size=(32, 32))
    want = C.ref_view(img, lab, p, obj, objmask, cityscapes_lut(), pad_size=(32, 32))
    C.check_equal(got, want, paste)
    assert int(want[3][C.OOD]) > 0 and tuple(want[0].shape) == (3, 32, 32) and tuple(want[2].shape) == (12, 24)
    assert bool((want[0][:, 12:] == 128).all()) and bool((want[1][:, 24:] == C.IGNORE).all())


@pytest.mark.parametrize("name", sorted(C.color_cases()))
def test_host_colour_legs_equal_the_restatement(name):
    from rba_amd.dataset_mappers import color_aug_ssd
    c = C.color_cases()[name]
    for img, _ in (C.lattice(), C.primaries(), C.frame(24, 48)):
        hwc = np.ascontiguousarray(img.numpy().transpose(1, 2, 0))
        assert np.array_equal(color_aug_ssd(hwc, c), C.color_legs(hwc, c)), name


# ---------------------------------------------------------------------------------------------------------------- the label rule
LABEL_SHAPES = sorted({(s, n) for s, n, _ in C.GEOMETRY.values()}) + [
    ((3, 7), (123, 11)), ((2, 5), (82, 5)), ((7, 3), (11, 123)), ((3, 123), (123, 3)),      # where ATen's index depends on the other axis' shape
    ((60, 90), (72, 108)), ((1024, 2048), (1228, 2456)), ((1024, 2048), (512, 1024)), ((1024, 2048), (2048, 4096))]


@pytest.mark.parametrize("shape", LABEL_SHAPES)
def test_label_tables_equal_f_interpolate(shape):
    """K14 reads the labels at (ny[Y], nx[X]) (include/rba_hip.h) with the tables of ops.nearest_index_tables: held here against F.interpolate itself on
    random float64 labels as the reference hands them to ResizeTransform -- [1,1,h,w] -- at every shape the other tests use and at the recipe's"""
    from rba_amd import ops
    (h, w), (nh, nw) = shape
    lab = torch.randint(0, 256, (h, w), generator=torch.Generator().manual_seed(h * w + nh)).double()
    want = F.interpolate(lab[None, None], size=(nh, nw), mode="nearest")[0, 0]
    ny, nx = ops.nearest_index_tables(h, w, nh, nw)
    assert (ny is None) == (nh == h) and (nx is None) == (nw == w)
    ny = torch.arange(h) if ny is None else ny
    nx = torch.arange(w) if nx is None else nx
    assert (ny.numel(), nx.numel()) == (nh, nw) and 0 <= int(ny.min()) and int(ny.max()) < h and 0 <= int(nx.min()) and int(nx.max()) < w
    assert torch.equal(lab[ny.long()][:, nx.long()], want)
    if nh == 2 * h:
        assert ny.tolist() == [d >> 1 for d in range(nh)]


# ---------------------------------------------------------------------------------------------------------------- the HSV restatement
def test_hsv_round_trip_leaves_gray_unchanged_and_hue_stays_below_180():
    from rba_amd.dataset_mappers import bgr_to_hsv_u8, hsv_to_bgr_u8
    gray = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)[None]
    for to_hsv, to_bgr in ((bgr_to_hsv_u8, hsv_to_bgr_u8), (C.bgr2hsv, C.hsv2bgr)):
        hsv = to_hsv(gray)
        assert not hsv[..., 0].any() and not hsv[..., 1].any()
        assert np.array_equal(to_bgr(hsv), gray)
        lat = np.ascontiguousarray(C.lattice()[0].numpy().transpose(1, 2, 0))
        hsv = to_hsv(lat)
        assert int(hsv[..., 0].max()) <= 179 and int(hsv[..., 0].max()) >= 170
        back = to_bgr(hsv).astype(int) - lat.astype(int)
        assert np.abs(back).max() <= 6                                  # an 8-bit HSV triple does not hold every colour; it stays close
    assert np.array_equal(bgr_to_hsv_u8(lat), C.bgr2hsv(lat)) and np.array_equal(hsv_to_bgr_u8(hsv), C.hsv2bgr(hsv))
    prim = np.ascontiguousarray(C.primaries()[0].numpy().transpose(1, 2, 0))[..., ::-1]
    assert np.array_equal(C.hsv2bgr(C.bgr2hsv(prim)), prim)
    assert C.bgr2hsv(prim).reshape(-1, 3).tolist() == [[0, 0, 0], [0, 0, 255], [0, 255, 255], [60, 255, 255], [120, 255, 255], [30, 255, 255],
                                                       [90, 255, 255], [150, 255, 255]]


def test_hsv_restatement_against_cv2_where_it_is_installed():
    cv2 = pytest.importorskip("cv2")
    lat = np.ascontiguousarray(C.lattice()[0].numpy().transpose(1, 2, 0))
    hsv = cv2.cvtColor(lat, cv2.COLOR_BGR2HSV)
    assert np.array_equal(hsv, C.bgr2hsv(lat))
    assert np.array_equal(cv2.cvtColor(hsv, cv2.COLOR_HSV2BGR), C.hsv2bgr(hsv))


# ---------------------------------------------------------------------------------------------------------------- the sampler
class _Recorder:
    """a generator that answers from a script and records what it was asked"""

    def __init__(self, answers):
        self.answers, self.calls = list(answers), []

    def _next(self, *call):
        self.calls.append(call)
        return self.answers.pop(0)

    def rand(self):
        return self._next("rand")

    def randint(self, *a):
        return self._next("randint", *a)

    def choice(self, a):
        return self._next("choice", tuple(a))

    def uniform(self, *a):
        return self._next("uniform", *a)

    def randrange(self, n):
        return self._next("randrange", n)


def test_draw_order_with_a_paste_and_every_leg():
    from rba_amd.dataset_mappers import sample_train_view_params
    npr = _Recorder([0.1, 2, 31, 7, 13, 0.25])
    pyr = _Recorder([5, 9, 1, -3.5, 0, 1, 0.75, 1, -4, 1, 1.25])
    p = sample_train_view_params(_settings(), 24, 48, [(0, 0), (30, 5), (6, 9)], npr, pyr)
    assert npr.calls == [("rand",), ("randint", 0, 3), ("choice", (12, 17, 24, 31, 48)), ("randint", 31 - 12 + 1), ("randint", 62 - 24 + 1), ("uniform", 0, 1)]
    assert pyr.calls == [("randint", 0, 24 - 6), ("randint", 0, 48 - 9), ("randrange", 2), ("uniform", -32, 32), ("randrange", 2),
                         ("randrange", 2), ("uniform", 0.5, 1.5), ("randrange", 2), ("randint", -18, 18), ("randrange", 2), ("uniform", 0.5, 1.5)]
    c = p.color
    assert (p.ood_index, p.paste, p.new_h, p.new_w, p.crop, p.flip) == (2, (5, 9), 31, 62, (7, 13, 12, 24), True)
    assert (c.brightness, c.beta, c.order, c.saturation, c.saturation_alpha, c.hue, c.hue_delta, c.contrast, c.contrast_alpha) == (
        True, -3.5, False, True, 0.75, True, -4, True, 1.25)


def test_draw_order_without_a_paste_and_with_legs_off():
    from rba_amd.dataset_mappers import sample_train_view_params
    npr = _Recorder([0.2, 12, 0, 0, 0.5])                          # ood_p == OOD_PROB: `<` fails, no object
    pyr = _Recorder([0, 1, 0, 1, 1.5, 0])
    p = sample_train_view_params(_settings(), 24, 48, [(6, 9)], npr, pyr)
    assert npr.calls == [("rand",), ("choice", (12, 17, 24, 31, 48)), ("randint", 1), ("randint", 1), ("uniform", 0, 1)]
    assert pyr.calls == [("randrange", 2), ("randrange", 2), ("randrange", 2), ("randrange", 2), ("uniform", 0.5, 1.5), ("randrange", 2)]
    c = p.color
    assert (p.ood_index, p.paste, p.crop, p.flip) == (None, None, (0, 0, 12, 24), False)
    assert (c.brightness, c.order, c.contrast, c.saturation, c.saturation_alpha, c.hue) == (False, True, False, True, 1.5, False)
    # no colour augmentation, no crop: no draw from the second generator at all
    npr, pyr = _Recorder([0.9, 17, 0.1]), _Recorder([])
    p = sample_train_view_params(_settings(color_aug=False, crop_enabled=False), 24, 48, None, npr, pyr)
    assert [c[0] for c in npr.calls] == ["rand", "choice", "uniform"] and pyr.calls == [] and p.color is None and p.crop == (0, 0, 17, 34) and p.flip


def test_sampler_on_real_generators_is_a_function_of_their_states():
    from rba_amd.dataset_mappers import sample_train_view_params
    a = sample_train_view_params(_settings(), 24, 48, [(6, 9)], np.random.RandomState(5), random.Random(6))
    b = sample_train_view_params(_settings(), 24, 48, [(6, 9)], np.random.RandomState(5), random.Random(6))
    assert a == b
    np.random.seed(5)
    random.seed(6)
    assert sample_train_view_params(_settings(), 24, 48, [(6, 9)]) == a              # the defaults are the two global generators


def test_the_three_paste_cases():
    """mix_object: no ood pixel -> no paste and no draw; a box larger than the frame -> unchanged and no draw; a box that fits -> the drawn position"""
    from rba_amd.dataset_mappers import sample_train_view_params
    tail = [0, 0, 0, 0, 0]                                           # colour legs all off
    for box, draws, paste in (((0, 0), [], None), ((25, 9), [], None), ((6, 49), [], None), ((24, 48), [0, 0], (0, 0)), ((6, 9), [18, 39], (18, 39))):
        npr, pyr = _Recorder([0.0, 0, 24, 3, 4, 0.9]), _Recorder(draws + tail)
        p = sample_train_view_params(_settings(), 24, 48, [box], npr, pyr)
        assert p.ood_index == 0 and p.paste == paste and [c[0] for c in pyr.calls[:len(draws)]] == ["randint"] * len(draws), box
        assert len(pyr.calls) == len(draws) + 5


def test_refusals():
    from rba_amd.config import CfgNode
    from rba_amd.dataset_mappers import MaskFormerSemanticCocoMixDatasetMapper, sample_train_view_params
    for kw, match in ((dict(single_category_max_area=0.5), "SINGLE_CATEGORY_MAX_AREA"), (dict(crop_type="relative_range"), "CROP.TYPE"),
                      (dict(sampling="range"), "SAMPLING"), (dict(size_divisibility=16), "SIZE_DIVISIBILITY"), (dict(image_format="BGR"), "FORMAT")):
        with pytest.raises(NotImplementedError, match=match):
            sample_train_view_params(_settings(**kw), 24, 48, None, np.random.RandomState(0), random.Random(0))
    with pytest.raises(ValueError, match="between"):
        sample_train_view_params(_settings(ood_prob=1.5), 24, 48, None, np.random.RandomState(0), random.Random(0))
    cfg = CfgNode(INPUT=CfgNode(FORMAT="RGB"))
    with pytest.raises(NotImplementedError, match="labels_mapping"):
        MaskFormerSemanticCocoMixDatasetMapper(cfg, coco=[], labels_mapping=[0, 1])
    mapper = MaskFormerSemanticCocoMixDatasetMapper(cfg, coco=[])
    img, lab = C.frame(24, 48)
    with pytest.raises(ValueError, match="annotations"):
        mapper({"image": img, "sem_seg_gt": lab, "annotations": []})
    with pytest.raises(ValueError, match="sem_seg_file_name"):
        mapper({"image": img})
    with pytest.raises(ValueError, match="uint8"):
        mapper({"image": img, "sem_seg_gt": lab.long()})


# ---------------------------------------------------------------------------------------------------------------- the settings
def test_input_defaults():
    from rba_amd.config import CfgNode, _DEFAULTS
    from rba_amd.dataset_mappers import mapper_settings
    inp = _DEFAULTS["INPUT"]
    assert (inp["OOD_LABEL"], inp["OOD_PROB"], inp["COCO_ROOT"], inp["COCO_PROXY_SIZE"], inp["REPEAT_INSTANCE_MASKS"]) == (254, 0.2, "coco/", 300, 1)
    assert (inp["DATASET_MAPPER_NAME"], inp["COLOR_AUG_SSD"], inp["SIZE_DIVISIBILITY"], inp["CROP"]["SINGLE_CATEGORY_MAX_AREA"]) == (
        "mask_former_semantic", False, -1, 1.0)
    assert (inp["MIN_SIZE_TRAIN"], inp["MAX_SIZE_TRAIN"], inp["MIN_SIZE_TRAIN_SAMPLING"], inp["CROP"]["ENABLED"], inp["CROP"]["TYPE"], inp["FORMAT"],
            inp["RANDOM_FLIP"]) == ([800], 1333, "choice", False, "relative_range", "BGR", "horizontal")
    s = mapper_settings(CfgNode())
    assert (s.min_sizes, s.max_size, s.crop_enabled, s.ood_label, s.ood_prob, s.ignore_label, s.size_divisibility) == ((800,), 1333, False, 254, 0.2, 255, -1)


@pytest.mark.parametrize("recipe", RECIPES)
def test_the_recipes_resolve_to_this_mapper(tmp_path, recipe):
    from rba_amd.dataset_mappers import mapper_settings, sample_train_view_params
    cfg = _recipe_cfg(tmp_path, recipe)
    assert cfg.INPUT.DATASET_MAPPER_NAME == "mask_former_semantic_coco_mix"
    s = mapper_settings(cfg)
    assert s.min_sizes == tuple(int(x * 0.1 * 1024) for x in range(5, 21)) and s.min_sizes[0] == 512 and s.min_sizes[-1] == 2048
    assert (s.max_size, s.sampling, s.crop_enabled, s.crop_type, tuple(s.crop_size), s.single_category_max_area) == (4096, "choice", True, "absolute",
                                                                                                                  (512, 1024), 1.0)
    assert (s.color_aug, s.image_format, s.size_divisibility, s.ignore_label, s.ood_label, s.ood_prob, s.coco_root, s.coco_proxy_size,
            s.repeat_instance_masks) == (True, "RGB", -1, 255, 254, 0.2, "coco/", 300, 1)
    p = sample_train_view_params(s, 1024, 2048, None, np.random.RandomState(1), random.Random(2))
    assert p.new_h in s.min_sizes and p.new_w == 2 * p.new_h and p.crop[2:] == (512, 1024) and p.color is not None


# ---------------------------------------------------------------------------------------------------------------- the COCO objects
def _write_coco(root):
    from PIL import Image
    rng = np.random.default_rng(3)
    os.makedirs(root / "annotations" / "ood_seg_train2017")
    os.makedirs(root / "train2017")
    boxes = {}
    for i, box in enumerate(((3, 5, 17, 21), None)):
        m = np.zeros((30, 40), dtype=np.uint8)
        m[0, 0] = 7                                                   # another value: not part of the box
        if box is not None:
            y1, x1, y2, x2 = box
            m[y1:y2, x1:x2] = 254
            m[y1 + 2, x1 + 1:x2 - 1] = 0                              # a hole
        Image.fromarray(m).save(root / "annotations" / "ood_seg_train2017" / f"{i:012d}.png")
        Image.fromarray(rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)).save(root / "train2017" / f"{i:012d}.jpg", quality=95)
        boxes[f"{i:012d}"] = box
    return boxes


def test_coco_ood_objects_on_a_four_file_tree(tmp_path):
    from PIL import Image
    from rba_amd.dataset_mappers import CocoOodObjects, extract_bbox
    boxes = _write_coco(tmp_path)
    coco = CocoOodObjects(str(tmp_path), proxy_size=300, shuffle=False)
    assert len(coco) == 2 and len(coco.box_hw) == 2 and "2" in repr(coco)
    for i in range(2):
        stem = os.path.basename(coco.targets[i])[:-4]
        assert coco.images[i] == os.path.join(str(tmp_path), "train2017", stem + ".jpg")
        obj, mask = coco[i]
        box = boxes[stem]
        if box is None:
            assert obj.shape == (0, 0, 3) and mask.shape == (0, 0) and tuple(coco.box_hw[i]) == (0, 0)
            continue
        y1, x1, y2, x2 = box
        full = np.array(Image.open(coco.images[i]).convert("RGB"))
        assert tuple(coco.box_hw[i]) == (y2 - y1, x2 - x1) and np.array_equal(obj, full[y1:y2, x1:x2])
        assert mask.dtype == np.uint8 and int((mask == 254).sum()) == (y2 - y1) * (x2 - x1) - (x2 - x1 - 2) and not mask[2, 1:-1].any()
    assert extract_bbox(np.zeros((4, 4), dtype=bool)) == (0, 0, 0, 0)
    # the shuffle is random.shuffle of the (image, target) pairs; the proxy subset is its head
    a = CocoOodObjects(str(tmp_path), proxy_size=1, py_rng=random.Random(1))
    pairs = list(zip(coco.images, coco.targets))
    random.Random(1).shuffle(pairs)
    assert len(a) == 1 and (a.images[0], a.targets[0]) == pairs[0]


def test_mapper_on_the_host_returns_the_reference_dict(tmp_path):
    from rba_amd.config import CfgNode
    from rba_amd.dataset_mappers import CocoOodObjects, MaskFormerSemanticCocoMixDatasetMapper
    _write_coco(tmp_path)
    cfg = CfgNode(INPUT=CfgNode(MIN_SIZE_TRAIN=[24, 31], MAX_SIZE_TRAIN=4096, CROP=CfgNode(ENABLED=True, TYPE="absolute", SIZE=[12, 24]),
                                COLOR_AUG_SSD=True, FORMAT="RGB", OOD_PROB=1.0, REPEAT_INSTANCE_MASKS=2, SIZE_DIVISIBILITY=32))
    coco = CocoOodObjects(str(tmp_path), 300, shuffle=False)
    mapper = MaskFormerSemanticCocoMixDatasetMapper(cfg, coco=coco, np_rng=np.random.RandomState(11), py_rng=random.Random(12))
    img, lab = C.frame(48, 96)
    seen_paste = False
    for _ in range(30):
        d = mapper({"image": img, "sem_seg_gt": lab, "file_name": "x.png"})
        assert set(d) == {"image", "sem_seg", "outlier_mask", "instances", "file_name"}
        assert d["image"].dtype == torch.uint8 and tuple(d["image"].shape) == (3, 32, 32) and tuple(d["sem_seg"].shape) == (32, 32)
        assert d["sem_seg"].dtype == torch.int64 and d["outlier_mask"].dtype == torch.int64 and tuple(d["outlier_mask"].shape) == (12, 24)
        classes = np.unique(d["sem_seg"].numpy())
        classes = classes[(classes != 255) & (classes != 254)]
        inst = d["instances"]
        assert inst.gt_classes.dtype == torch.int64 and inst.gt_classes.tolist() == classes.repeat(2).tolist() and inst.image_size == (32, 32)
        assert inst.gt_masks.dtype == torch.bool and tuple(inst.gt_masks.shape) == (2 * len(classes), 32, 32)
        for k, cls in enumerate(inst.gt_classes.tolist()):
            assert torch.equal(inst.gt_masks[k], d["sem_seg"] == cls)
        seen_paste |= bool((d["sem_seg"] == 254).any())
        assert torch.equal(d["outlier_mask"] == 1, d["sem_seg"][:12, :24] == 254) and torch.equal(d["outlier_mask"] == 255, d["sem_seg"][:12, :24] == 255)
    assert seen_paste
    assert torch.equal(img, C.frame(48, 96)[0])                       # the input is left as it was


def test_mapper_reads_the_files_a_dataset_dict_names(tmp_path):
    from PIL import Image
    from rba_amd.config import CfgNode
    from rba_amd.dataset_mappers import MaskFormerSemanticCocoMixDatasetMapper
    img, lab = C.frame(24, 48)
    Image.fromarray(np.ascontiguousarray(img.numpy().transpose(1, 2, 0))).save(tmp_path / "a_leftImg8bit.png")
    Image.fromarray(lab.numpy()).save(tmp_path / "a_gtFine_labelTrainIds.png")
    mapper = MaskFormerSemanticCocoMixDatasetMapper(CfgNode(INPUT=CfgNode(FORMAT="RGB")), coco=[])
    p = C.params_of("e31_inside", flip=True, color=C.color_cases()["all_order1"])
    names = {"file_name": str(tmp_path / "a_leftImg8bit.png"), "sem_seg_file_name": str(tmp_path / "a_gtFine_labelTrainIds.png")}
    a, b = mapper(names, params=p), mapper({"image": img, "sem_seg_gt": lab}, params=p)
    assert "sem_seg_file_name" not in a and a["file_name"] == names["file_name"] and "sem_seg_file_name" in names
    for k in ("image", "sem_seg", "outlier_mask"):
        assert torch.equal(a[k], b[k])
    C.check_equal((a["image"], a["sem_seg"], a["outlier_mask"]), C.ref_view(img, lab, p)[:3], "from files")


# ---------------------------------------------------------------------------------------------------------------- prepare_targets
def test_prepare_targets_keys_and_padding():
    from rba_amd.dataset_mappers import Instances
    from rba_amd.maskformer_model import MaskFormer
    model = MaskFormer.__new__(MaskFormer)
    torch.nn.Module.__init__(model)
    model.register_buffer("pixel_mean", torch.zeros(3, 1, 1))
    sem = torch.randint(0, 3, (12, 24))
    inst = Instances((12, 24), torch.tensor([0, 2]), torch.stack([sem == 0, sem == 2]))
    out = model.prepare_targets([{"instances": inst, "outlier_mask": sem * 0, "sem_seg": sem}, {"instances": inst}], (32, 64))
    assert len(out) == 2 and set(out[0]) == {"labels", "masks", "outlier_masks", "sem_seg"} and set(out[1]) == {"labels", "masks"}
    m = out[0]["masks"]
    assert tuple(m.shape) == (2, 32, 64) and m.dtype == torch.bool and torch.equal(m[:, :12, :24], inst.gt_masks)
    assert not m[:, 12:].any() and not m[:, :, 24:].any() and torch.equal(out[0]["labels"], inst.gt_classes)
    assert out[0]["outlier_masks"] is not None and torch.equal(out[0]["sem_seg"], sem)
    with pytest.raises(ValueError, match="do not fit"):
        model.prepare_targets([{"instances": inst}], (8, 64))


# ---------------------------------------------------------------------------------------------------------------- the entry point
def _view(**kw):
    """a well-formed call's struct on fake (never dereferenced: every case below is refused before the launch) pointers"""
    from rba_amd import _lib
    v = _lib.TrainView()
    for n in ("img", "lab", "image", "sem_seg", "outlier_mask", "hist"):
        setattr(v, n, 0x1000)
    v.h, v.w, v.new_h, v.new_w, v.y0, v.x0, v.ch, v.cw, v.pad_h, v.pad_w, v.ignore_label, v.ood_label = 24, 48, 24, 48, 0, 0, 12, 24, 12, 24, 255, 254
    for k, val in kw.items():
        setattr(v, k, val)
    return v


def test_entry_point_is_declared_bound_and_built_and_refuses_without_a_launch():
    from rba_amd import _lib
    assert _lib.SIGNATURES["rba_train_view_u8"] == [ctypes.c_void_p, ctypes.c_void_p] and _lib.EXPECTED_ABI == 191
    hdr = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    assert "int rba_train_view_u8(const rba_train_view* view" in hdr and "} rba_train_view_color;" in hdr
    assert ctypes.sizeof(_lib.TrainViewColor) == 40 and ctypes.sizeof(_lib.TrainView) == 15 * 8 + 19 * 4 + 40 + 4      # padded to 8 bytes
    lib = _lib.load()
    assert hasattr(lib, "rba_train_view_u8") and hasattr(ctypes.CDLL(_lib.KNOBS_LIB_PATH), "rba_train_view_u8")
    invalid = 1                                                       # hipErrorInvalidValue
    bad = [dict(ch=0), dict(h=0), dict(new_w=0), dict(y0=-1), dict(y0=13), dict(x0=25), dict(pad_h=11), dict(pad_w=23), dict(img=None),
           dict(hist=None), dict(ood_label=256), dict(bh=3, bw=0), dict(bh=3, bw=4, obj=0x1000, objmask=0x1000, py=22, px=0),
           dict(bh=3, bw=4, obj=0x1000, objmask=0x1000, py=0, px=45), dict(bh=3, bw=4, py=0, px=0), dict(new_w=40), dict(new_h=30),
           dict(sem_seg=0x1004)]
    for kw in bad:
        assert lib.rba_train_view_u8(ctypes.addressof(_view(**kw)), None) == invalid, kw
    assert lib.rba_train_view_u8(None, None) == invalid
