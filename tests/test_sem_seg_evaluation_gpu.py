"""SemSegEvaluator and `python -m rba_amd.evaluate_semseg` on the GPU with the tiny seeded model and a synthetic Cityscapes tree (60 x 90 images, trainId
labels 0..18 and 255): the evaluator's matrix is the numpy oracle's on the model's own argmax maps -- integer counts, compared exactly."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from rba_amd import arch as A
from tests import _confusion_cases as G
from tests import _tta_cases as T

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 19
CFG = {"MODEL": {"SWIN": {"EMBED_DIM": 32, "DEPTHS": [2, 2, 2, 2], "NUM_HEADS": [1, 2, 4, 8], "WINDOW_SIZE": 6},
                 "SEM_SEG_HEAD": {"CONVS_DIM": 64, "MASK_DIM": 64, "TRANSFORMER_ENC_LAYERS": 2, "DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["res5"]},
                 "MASK_FORMER": {"HIDDEN_DIM": 64, "NHEADS": 2, "NUM_OBJECT_QUERIES": 16, "DIM_FEEDFORWARD": 128, "DEC_LAYERS": 2}},
       "TEST": {"AUG": {"ENABLED": False, "MIN_SIZES": [32, 48], "MAX_SIZE": 4096, "FLIP": True}}}


@pytest.fixture(scope="module")
def model():
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS["tiny1"])
    return load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """(root, dataset with trainId labels, dataset with raw ids + table)"""
    from rba_amd.sem_seg_datasets import CityscapesSemSeg
    root = str(tmp_path_factory.mktemp("cityscapes"))
    G.make_cityscapes(root, per_city=(2, 2), h=60, w=90, seed=3)
    return root, CityscapesSemSeg(root, labels="trainIds"), CityscapesSemSeg(root, labels="labelIds")


def _evaluator(ds, **kw):
    from rba_amd.sem_seg_evaluation import SemSegEvaluator
    return SemSegEvaluator(ds.num_classes, ds.ignore_label, ds.class_names, lut=ds.lut, **kw)


def _same(a, b):
    return all((np.isnan(a[k]) and np.isnan(b[k])) or a[k] == b[k] for k in a) and list(a) == list(b)


def _check_forms(ds, ds_raw, outputs):
    """outputs: per image (sem_seg [K,H,W], argmax int32 [H,W]) of one model -> the summed matrix, after checking both input forms, both label sources,
    host and device labels, against the oracle on sem_seg.argmax(0)"""
    from rba_amd.sem_seg_evaluation import sem_seg_metrics
    want = np.zeros((K + 1, K + 1), dtype=np.int64)
    ev_sem, ev_arg, ev_raw = _evaluator(ds), _evaluator(ds), _evaluator(ds_raw)
    for i, (sem, arg) in enumerate(outputs):
        label = ds.raw_item(i)[1]                                                   # uint8, host
        conf, bad = G.oracle(sem.argmax(0).cpu().numpy(), label.numpy(), K, 255)
        assert not bad.any() and conf[:, K].sum() == (label == 255).sum()
        want += conf
        ev_sem.process([{"sem_seg": label}], [{"sem_seg": sem}])
        ev_arg.process([{"sem_seg": ds[i][1].cuda()}], [{"argmax": arg}])          # int64, on the device
        ev_raw.process([{"sem_seg": ds_raw.raw_item(i)[1]}], [{"argmax": arg}])    # raw ids through the table inside the kernel
    res = [e.evaluate() for e in (ev_sem, ev_arg, ev_raw)]
    for e, r in zip((ev_sem, ev_arg, ev_raw), res):
        assert e.images == len(outputs) and np.array_equal(e.matrix, want) and e.matrix.dtype == np.int64
        assert list(r) == ["sem_seg"] and _same(r["sem_seg"], sem_seg_metrics(want, ds.class_names))
    assert want.sum() == len(outputs) * 60 * 90 and "IoU-road" in res[0]["sem_seg"] and 0.0 <= res[0]["sem_seg"]["pACC"] <= 100.0
    ev_sem.reset()
    assert int(ev_sem.confusion.sum()) == 0 and ev_sem.images == 0
    return want


def test_evaluator_through_the_model(model, tree):
    root, ds, ds_raw = tree
    outputs = []
    for i in range(len(ds)):
        out = model([{"image": ds[i][0]}], return_argmax=True)[0]
        assert out["sem_seg"].shape == (K, 60, 90) and out["argmax"].dtype == torch.int32
        outputs.append((out["sem_seg"], out["argmax"]))
    _check_forms(ds, ds_raw, outputs)


def test_evaluator_through_the_tta_wrapper(model, tree):
    from rba_amd.test_time_augmentation import SemanticSegmentorWithTTA
    root, ds, ds_raw = tree
    w = SemanticSegmentorWithTTA(T.aug_cfg(min_sizes=(32, 48), max_size=4096, flip=True), model)
    outputs = []
    for i in range(len(ds)):
        sem = w([{"image": ds[i][0]}])[0]["sem_seg"]
        _, arg = w.rba_scores([{"image": ds[i][0]}], return_argmax=True)[0]
        assert sem.shape == (K, 60, 90) and arg.shape == (60, 90)
        outputs.append((sem, arg))
    _check_forms(ds, ds_raw, outputs)


def _models_folder(tmp_path):
    import yaml
    mdir = tmp_path / "ckpts" / "m"
    mdir.mkdir(parents=True)
    (mdir / "config.yaml").write_text(yaml.safe_dump(CFG))
    torch.save({"model": A.seeded_weights(A.complete(A.ARCHS["tiny1"]), 0)}, mdir / "model_final.pth")
    return str(tmp_path / "ckpts")


def test_cli_end_to_end(model, tree, tmp_path):
    """the command in a fresh child process: sem_seg.json holds the matrix of the oracle on the model's argmax maps (the fast path the command scores
    through, MaskFormer.rba_scores), its metrics, the image count and the protocol; in-process with --tta: the wrapper's"""
    from rba_amd import evaluate_semseg as E
    from rba_amd.sem_seg_evaluation import sem_seg_metrics
    from rba_amd.test_time_augmentation import SemanticSegmentorWithTTA
    root, ds, ds_raw = tree
    models = _models_folder(tmp_path)
    w = SemanticSegmentorWithTTA(T.aug_cfg(min_sizes=(32, 48), max_size=4096, flip=True), model)
    want = {False: np.zeros((K + 1, K + 1), dtype=np.int64), True: np.zeros((K + 1, K + 1), dtype=np.int64)}
    for i in range(len(ds)):
        x, label = ds[i][0].cuda(), ds.raw_item(i)[1].numpy()
        for tta, m in ((False, model), (True, w)):
            want[tta] += G.oracle(m.rba_scores([{"image": x}], return_argmax=True)[0][1].cpu().numpy(), label, K, 255)[0]
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "rba_amd.evaluate_semseg", "--models_folder", models, "--cityscapes_root", root, "--out_path",
                        str(tmp_path / "res"), "--num_workers", "2", "--labels", "labelIds"], env=env, capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "single scale" in r.stdout and "mIoU" in r.stdout and "bicycle" in r.stdout
    with open(tmp_path / "res" / "m" / "sem_seg.json") as f:
        got = json.load(f)
    assert np.array_equal(np.array(got["confusion_matrix"], dtype=np.int64), want[False])
    assert got["images"] == len(ds) and got["tta"] is False and got["labels"] == "labelIds" and got["split"] == "val"
    assert _same(got["sem_seg"], sem_seg_metrics(want[False], ds.class_names))
    E.main(["--models_folder", models, "--cityscapes_root", root, "--out_path", str(tmp_path / "res_tta"), "--num_workers", "0", "--tta", "--upper_limit", "3"])
    with open(tmp_path / "res_tta" / "m" / "sem_seg.json") as f:
        got = json.load(f)
    assert got["tta"] is True and got["images"] == 3 and got["labels"] == "trainIds"
    sub = np.zeros_like(want[True])
    for i in range(3):
        sub += G.oracle(w.rba_scores([{"image": ds[i][0].cuda()}], return_argmax=True)[0][1].cpu().numpy(), ds.raw_item(i)[1].numpy(), K, 255)[0]
    assert np.array_equal(np.array(got["confusion_matrix"], dtype=np.int64), sub)


def test_a_labelled_class_out_of_range_is_an_error(model, tree):
    """a label >= K that is not the ignore label: evaluate() raises and names the count; out-of-range predictions likewise"""
    from rba_amd.sem_seg_evaluation import SemSegEvaluator
    root, ds, _ = tree
    label = ds.raw_item(0)[1].clone()
    label[5, 7:18] = 100
    arg = torch.zeros((60, 90), dtype=torch.int32, device="cuda")
    ev = SemSegEvaluator(K, 255)
    ev.process([{"sem_seg": label}], [{"argmax": arg}])
    with pytest.raises(ValueError, match=r"11 pixel\(s\) with a label outside 0\.\.18.*0 pixel\(s\) with a prediction"):
        ev.evaluate()
    ev.reset()
    arg[0, :4] = K
    ev.process([{"sem_seg": ds.raw_item(0)[1]}], [{"argmax": arg}])
    with pytest.raises(ValueError, match=r"0 pixel\(s\) with a label.*4 pixel\(s\) with a prediction outside 0\.\.18"):
        ev.evaluate()
    ev.reset()
    ev.process([{"sem_seg": ds.raw_item(0)[1]}], [{"argmax": torch.zeros((60, 90), dtype=torch.int32, device="cuda")}])
    assert ev.evaluate()["sem_seg"]["pACC"] >= 0.0
    with pytest.raises(Exception):                          # evaluated at the label's size: a mismatch is the caller's error
        ev.process([{"sem_seg": ds.raw_item(0)[1]}], [{"argmax": torch.zeros((30, 45), dtype=torch.int32, device="cuda")}])
