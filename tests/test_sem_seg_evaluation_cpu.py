"""CPU: the closed-set evaluation's host side -- the metric formulas, the Cityscapes reader and its id -> trainId table, the published mIoU table of
tools/model_zoo_check.py, and the cross-rank sum of the confusion matrix on gloo."""
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _confusion_cases as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def v06_metrics(C):
    """Detectron2 v0.6 SemSegEvaluator.evaluate, transcribed class by class with Python floats (no vector code shared with the product)"""
    K = len(C) - 1
    tp = [float(C[k][k]) for k in range(K)]
    pos_gt = [float(sum(C[r][k] for r in range(K))) for k in range(K)]            # column sums of C[:-1, :-1]
    pos_pred = [float(sum(C[k][c] for c in range(K))) for k in range(K)]           # row sums
    acc = [tp[k] / pos_gt[k] if pos_gt[k] > 0 else math.nan for k in range(K)]
    iou = [tp[k] / (pos_gt[k] + pos_pred[k] - tp[k]) if pos_gt[k] > 0 else math.nan for k in range(K)]
    acc_valid = [k for k in range(K) if pos_gt[k] > 0]
    iou_valid = [k for k in range(K) if pos_gt[k] + pos_pred[k] > 0]
    total = sum(pos_gt)
    return {"mIoU": 100 * sum(iou[k] for k in acc_valid) / len(iou_valid),
            "fwIoU": 100 * sum(iou[k] * pos_gt[k] / total for k in acc_valid),
            "mACC": 100 * sum(acc[k] for k in acc_valid) / len(acc_valid),
            "pACC": 100 * sum(tp) / total,
            "iou": [100 * v for v in iou], "acc": [100 * v for v in acc]}


def _matrices():
    rng = np.random.RandomState(0)
    full = rng.randint(1, 1000, (5, 5)).astype(np.int64)
    full[:, -1] = 0
    full[-1, :] = 0
    absent = full.copy()                        # class 2 neither labelled nor predicted: NaN entries, outside both means
    absent[2, :] = 0
    absent[:, 2] = 0
    quirk = full.copy()                         # class 1 predicted, never labelled: in mIoU's denominator, not in its numerator
    quirk[:, 1] = 0
    ignored = full.copy()                       # ignored pixels (last column) change nothing
    ignored[:-1, -1] = rng.randint(1, 1000, 4)
    big = rng.randint(0, 1 << 40, (20, 20)).astype(np.int64)
    big[-1, :] = 0
    return {"full": full, "absent": absent, "quirk": quirk, "ignored": ignored, "big": big}


@pytest.mark.parametrize("name", sorted(_matrices()))
def test_sem_seg_metrics_equal_the_v06_definitions(name):
    from rba_amd.sem_seg_evaluation import sem_seg_metrics
    C = _matrices()[name]
    K = C.shape[0] - 1
    names = [f"c{k}" for k in range(K)]
    want = v06_metrics(C.tolist())
    for conf in (C, torch.from_numpy(C)):
        got = sem_seg_metrics(conf, names)
        assert list(got)[:4] == ["mIoU", "fwIoU", "mACC", "pACC"] and len(got) == 4 + 2 * K and all(type(v) is float for v in got.values())
        for k in ("mIoU", "fwIoU", "mACC", "pACC"):
            assert abs(got[k] - want[k]) <= 1e-12 * max(1.0, abs(want[k])), (k, got[k], want[k])
        for i, n in enumerate(names):
            for key, ref in ((f"IoU-{n}", want["iou"][i]), (f"ACC-{n}", want["acc"][i])):
                assert (math.isnan(got[key]) and math.isnan(ref)) or abs(got[key] - ref) <= 1e-12 * max(1.0, abs(ref)), key
    assert list(sem_seg_metrics(C))[4] == "IoU-0"                                  # default names


def test_sem_seg_metrics_special_cases():
    from rba_amd.sem_seg_evaluation import sem_seg_metrics
    m = _matrices()
    full, absent, quirk, ignored = (sem_seg_metrics(m[k]) for k in ("full", "absent", "quirk", "ignored"))
    assert math.isnan(absent["IoU-2"]) and math.isnan(absent["ACC-2"]) and not math.isnan(absent["mIoU"])
    ious = [absent[f"IoU-{k}"] for k in (0, 1, 3)]
    assert abs(absent["mIoU"] - sum(ious) / 3) < 1e-12                             # 3 valid classes in numerator and denominator
    # the v0.6 quirk: class 1 is NaN, yet mIoU divides by all 4 classes; mACC by the 3 labelled ones
    assert math.isnan(quirk["IoU-1"])
    assert abs(quirk["mIoU"] - sum(quirk[f"IoU-{k}"] for k in (0, 2, 3)) / 4) < 1e-12
    assert abs(quirk["mACC"] - sum(quirk[f"ACC-{k}"] for k in (0, 2, 3)) / 3) < 1e-12
    assert ignored == full
    # every class labelled: mIoU is the plain mean of the per-class IoUs
    assert abs(full["mIoU"] - sum(full[f"IoU-{k}"] for k in range(4)) / 4) < 1e-12
    with pytest.raises(ValueError):
        sem_seg_metrics(np.zeros((3, 4), dtype=np.int64))


def test_cityscapes_reader(tmp_path):
    from rba_amd import datasets as DS
    from rba_amd.sem_seg_datasets import CITYSCAPES_CLASSES, CityscapesSemSeg, cityscapes_lut
    both = G.make_cityscapes(str(tmp_path / "both"))
    only_ids = G.make_cityscapes(str(tmp_path / "ids"), train_ids=False, seed=1)
    assert len(CITYSCAPES_CLASSES) == 19 and CITYSCAPES_CLASSES[0] == "road" and CITYSCAPES_CLASSES[13] == "car" and CITYSCAPES_CLASSES[18] == "bicycle"
    auto = CityscapesSemSeg(str(tmp_path / "both"))
    assert len(auto) == 5 and auto.label_source == "trainIds" and auto.lut is None            # auto prefers trainIds
    assert auto.images == [t[0] for t in both] and auto.images == sorted(auto.images)
    assert [os.path.basename(os.path.dirname(p)) for p in auto.images] == ["aachen"] * 3 + ["bonn"] * 2
    for p, lab in zip(auto.images, auto.labels):                                               # pairing: same city, same stem
        assert lab == p.replace("leftImg8bit", "gtFine", 1).replace("_leftImg8bit.png", "_gtFine_labelTrainIds.png")
    raw = CityscapesSemSeg(str(tmp_path / "both"), split="val", labels="labelIds")
    assert raw.label_source == "labelIds" and torch.equal(raw.lut, cityscapes_lut()) and raw.lut.dtype == torch.uint8 and raw.lut.shape == (256,)
    assert all(p.endswith("_gtFine_labelIds.png") for p in raw.labels)
    for i, (_, img, ids, tids) in enumerate(both):
        x, y = auto[i]
        assert x.dtype == torch.uint8 and x.shape == (3, 24, 40) and y.dtype == torch.int64 and y.shape == (24, 40)
        assert np.array_equal(x.numpy().transpose(1, 2, 0), img) and np.array_equal(y.numpy(), tids.astype(np.int64))
        xr, yr = auto.raw_item(i)                                                              # both item forms agree
        assert xr.dtype == torch.uint8 and xr.shape == (24, 40, 3) and yr.dtype == torch.uint8 and xr.is_contiguous()
        assert torch.equal(xr.permute(2, 0, 1), x) and torch.equal(yr.to(torch.int64), y)
        xi, yi = raw[i]
        assert torch.equal(xi, x) and np.array_equal(yi.numpy(), ids.astype(np.int64))
        assert np.array_equal(raw.lut.numpy()[raw.raw_item(i)[1].numpy()], tids)               # both label sources say the same
    fallback = CityscapesSemSeg(str(tmp_path / "ids"), labels="auto")                          # no trainId PNGs: auto falls back to the raw ids
    assert fallback.label_source == "labelIds" and fallback.lut is not None and len(fallback) == len(only_ids)
    got = list(DS.prefetch(auto, range(len(auto)), 2, raw=True))                               # the OoD loader drives it
    assert all(torch.equal(a[0], auto.raw_item(i)[0]) and torch.equal(a[1], auto.raw_item(i)[1]) for i, a in enumerate(got))
    with pytest.raises(KeyError):
        DS.get_dataset("cityscapes", str(tmp_path / "both"))
    assert "cityscapes" not in DS.available_datasets()
    with pytest.raises(RuntimeError):
        CityscapesSemSeg(str(tmp_path / "both"), split="test")
    with pytest.raises(ValueError):
        CityscapesSemSeg(str(tmp_path / "both"), labels="colors")


def test_id_to_trainid_table():
    from rba_amd.sem_seg_datasets import CITYSCAPES_ID_TO_TRAINID, cityscapes_lut
    lut = cityscapes_lut().numpy()
    ref = "/root/reference/datasets/cityscapes.py"
    if os.path.exists(ref):
        rows = re.findall(r"CityscapesClass\('([^']+)',\s*(-?\d+),\s*(-?\d+),", open(ref).read())
        table = {int(i): int(t) for _, i, t in rows if int(i) >= 0}
        assert sorted(table) == list(range(34))
        assert [table[i] for i in range(34)] == list(CITYSCAPES_ID_TO_TRAINID) == lut[:34].tolist()
    assert (lut[7], lut[26], lut[33], lut[0]) == (0, 13, 18, 255)
    assert len(CITYSCAPES_ID_TO_TRAINID) == 34 and (lut[34:] == 255).all() and lut.dtype == np.uint8
    assert sorted(v for v in CITYSCAPES_ID_TO_TRAINID if v != 255) == list(range(19))
    assert list(CITYSCAPES_ID_TO_TRAINID) == G.CITYSCAPES_ID_TO_TRAINID                         # the tests' own copy (the kernel tests' table)


def _zoo():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import model_zoo_check as Z
    return Z


def test_model_zoo_miou_table():
    Z = _zoo()
    zoo = "/root/reference/MODEL_ZOO.md"
    if os.path.exists(zoo):
        got = {}
        for table in re.findall(r"<table>.*?</table>", open(zoo).read(), flags=re.S):
            if "Cityscapes mIoU" not in table:                   # the fine-tuned models' tables have "Finetuned Component" in that place: no mIoU is published
                continue
            for r in re.findall(r'<tr><td align="left">.*?</tr>', table, flags=re.S):
                cfg = re.search(r"ckpts/([a-z0-9_]+)/config.yaml", r).group(1)
                got[cfg] = float(re.findall(r'<td align="center">([0-9.]+)</td>', r)[0])         # the first numeric column
        assert got == Z.MODEL_ZOO_MIOU
    assert Z.MODEL_ZOO_MIOU["swin_b_1dl"] == 82.25 and set(Z.MODEL_ZOO_MIOU) <= set(Z.MODEL_ZOO)


def test_model_zoo_check_prints_what_it_printed_without_the_new_flag(tmp_path):
    """the tool as a command (its report writes to the stdout it was imported under): stdout and exit status, byte for byte, without --cityscapes_root"""
    import pickle
    Z = _zoo()

    def tool(argv):
        r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "model_zoo_check.py")] + argv, capture_output=True, text=True, timeout=300)
        return r.returncode, r.stdout

    models, out = tmp_path / "ckpts", tmp_path / "results"
    (models / "swin_b_1dl").mkdir(parents=True)
    (models / "swin_b_1dl" / "config.yaml").write_text("MODEL: {}\n")
    (models / "swin_b_1dl" / "model_final.pth").write_bytes(b"")
    (out / "swin_b_1dl").mkdir(parents=True)
    with open(out / "swin_b_1dl" / "results.pkl", "wb") as f:
        pickle.dump({ds: {k: v / 100.0 for k, v in Z.MODEL_ZOO["swin_b_1dl"][ds].items()} for ds in Z.DATASETS}, f)
    base = ["--models_folder", str(models), "--out_path", str(out), "--results-only"]
    code, txt = tool(base)
    assert code == 0
    ck = models / "swin_b_1dl" / "model_final.pth"
    assert txt == (
        f"[model_zoo_check] swin_b_1dl: config.yaml found, checkpoint {ck}\n"
        "model                              dataset          metric published   measured      diff  verdict (tolerance 0.005 pp)\n"
        "swin_b_1dl                         road_anomaly     AP         78.45    78.4500   +0.0000  ok\n"
        "swin_b_1dl                         road_anomaly     FPR95      11.83    11.8300   +0.0000  ok\n"
        "swin_b_1dl                         fishyscapes_laf  AP         60.96    60.9600   +0.0000  ok\n"
        "swin_b_1dl                         fishyscapes_laf  FPR95      10.63    10.6300   +0.0000  ok\n"
        "[model_zoo_check] 4 of 4 published numbers reproduced within 0.005 percentage points; largest |difference| 0.0000\n")
    # opt-in: one mIoU line per model, the protocol named; a missing sem_seg.json is a MISSING row
    code, txt = tool(base + ["--cityscapes_root", str(tmp_path / "cityscapes")])
    assert code == 1
    assert "mIoU" in txt and "MISSING (no sem_seg.json)" in txt and "results.pkl entry" not in txt and "4 of 5 published numbers" in txt
    with open(out / "swin_b_1dl" / "sem_seg.json", "w") as f:
        json.dump({"sem_seg": {"mIoU": 82.2531}, "tta": False, "images": 500}, f)
    code, txt = tool(base + ["--cityscapes_root", str(tmp_path / "cityscapes")])
    assert code == 0
    assert "Cityscapes mIoU measured with: single scale" in txt and "5 of 5 published numbers" in txt
    assert re.search(r"swin_b_1dl\s+cityscapes\s+mIoU\s+82\.25\s+82\.2531\s+\+0\.0031\s+ok", txt)


_WORKER = r'''
import sys, json
import torch
sys.path.insert(0, sys.argv[1])
from rba_amd import distributed as D
rank, world, local = D.init_from_env("gloo")
K = 19
g = torch.Generator().manual_seed(0)
parts = [torch.randint(0, 1 << 40, (K + 1, K + 1), generator=g, dtype=torch.int64) for _ in range(world)]
bads = [torch.tensor([r + 1, 10 * r], dtype=torch.int64) for r in range(world)]
mine, mine_bad = parts[rank].clone(), bads[rank].clone()
conf, bad = D.pooled_confusion(mine, mine_bad)
ok = torch.equal(conf, sum(parts)) and torch.equal(bad, sum(bads)) and conf.dtype == torch.int64 and conf.shape == (K + 1, K + 1) and bad.shape == (2,)
ok = ok and torch.equal(mine, parts[rank]) and torch.equal(mine_bad, bads[rank])          # the inputs are left as they are
print(json.dumps({"rank": rank, "ok": bool(ok)}), flush=True)
torch.distributed.destroy_process_group()
sys.exit(0 if ok else 1)
'''


def test_pooled_confusion_gloo(tmp_path):
    """distributed.pooled_confusion under torch.distributed.run with 2 ranks (gloo, CPU tensors): both ranks end with the sum"""
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", OMP_NUM_THREADS="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1", "--master-port",
                        "29643", str(script), REPO], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.count('"ok": true') == 2


def test_pooled_confusion_single_process():
    from rba_amd import distributed as D
    conf, bad = torch.arange(9, dtype=torch.int64).reshape(3, 3), torch.tensor([2, 0])
    c, b = D.pooled_confusion(conf, bad)
    assert torch.equal(c, conf) and torch.equal(b, bad)


def test_launch_rule_constants_match_the_kernel_source():
    """ops.CONFUSION_* (what the GPU tests size their maps and pick their class counts from) are the constants of csrc/confusion.hip; the symbol is declared,
    bound and exported by both libraries"""
    import ctypes
    from rba_amd import _lib, ops
    src = open(os.path.join(REPO, "rba_amd", "csrc", "confusion.hip")).read()
    const = {n: int(v) for n, v in re.findall(r"constexpr int (K13_[A-Z_]+) = (\d+);", src)}
    assert (const["K13_THREADS"], const["K13_TILE"], const["K13_GRID_CAP"], const["K13_LDS_MAX_K"]) == \
        (ops.CONFUSION_THREADS, ops.CONFUSION_TILE, ops.CONFUSION_GRID_CAP, ops.CONFUSION_LDS_MAX_K)
    words = const["K13_LDS_WORDS"] - const["K13_LUT_WORDS"]                          # the threshold is the LDS budget's
    assert (ops.CONFUSION_LDS_MAX_K + 1) ** 2 + 2 <= words < (ops.CONFUSION_LDS_MAX_K + 2) ** 2 + 2 and const["K13_LDS_WORDS"] * 4 == 65536
    assert len(_lib.SIGNATURES["rba_confusion_accum"]) == 10 and _lib.SIGNATURES["rba_confusion_accum"][3] is ctypes.c_int64
    assert "int rba_confusion_accum(" in open(os.path.join(REPO, "include", "rba_hip.h")).read()
    for path in (_lib.LIB_PATH, _lib.KNOBS_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "rba_confusion_accum"), path
    assert "confusion.hip" in __import__("rba_amd.csrc.build", fromlist=["SOURCES"]).SOURCES


def test_confusion_accumulate_has_no_cpu_path():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    with pytest.raises(RbaHipError, match="no CPU path"):
        ops.confusion_accumulate(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8), 19, torch.zeros(20, 20, dtype=torch.int64),
                                 torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RbaHipError, match="num_classes"):
        ops.confusion_accumulate(torch.zeros(4, 4, dtype=torch.int32), torch.zeros(4, 4, dtype=torch.uint8), 256, torch.zeros(257, 257, dtype=torch.int64),
                                 torch.zeros(2, dtype=torch.int64))


def test_element_access_kernels_hold_no_merged_label_load():
    """Where predictions and labels cannot both be 16-byte aligned, the labels are read element by element -- in the BINARY, not only in the source: the
    compiler's load-store vectoriser merges sixteen adjacent byte reads into one unaligned 16-byte load unless it is kept from it, and the GPU tolerates
    such a load, so no result shows it.  Every K13 kernel of the built code is disassembled: the element-access instantiations (GA = sizeof(GT)) hold exactly
    the four 16-byte prediction loads and sixteen label loads of the element's size (plus workgroup 0's single head / tail pixel); the aligned ones hold
    four + one (uint8) or four + eight (int64) 16-byte loads."""
    from rba_amd import _lib
    from rba_amd.csrc import isa_hazards
    obj = os.path.join(REPO, "rba_amd", "csrc", "build", "confusion.o")
    kernels = {}
    for _, ins in isa_hazards.disassemble(obj if os.path.exists(obj) else _lib.LIB_PATH):
        for text, kernel in ins:
            m = re.search(r"confusion_(lds|global)_kernelI([hl])Li(\d+)ELb([01])E", kernel)
            if m and text != "label":
                kernels.setdefault(m.groups(), []).append(text.split()[0])
    assert len(kernels) == 16, sorted(kernels)
    for (form, gt, ga, lut), mnems in kernels.items():
        wide = mnems.count("global_load_dwordx4")
        assert not any(m.startswith(("flat_load", "scratch_", "buffer_load")) for m in mnems), (form, gt, ga, lut)
        if int(ga) == 16:
            assert wide == (5 if gt == "h" else 12), (form, gt, ga, lut, wide)
        else:
            assert int(ga) == (1 if gt == "h" else 8) and wide == 4, (form, gt, ga, lut, wide)
            assert mnems.count("global_load_ubyte" if gt == "h" else "global_load_dwordx2") == 17, (form, gt, ga, lut)
