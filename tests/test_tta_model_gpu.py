"""SemanticSegmentorWithTTA on the GPU with the tiny seeded model: against the same protocol composed from the public API that exists without it --
the host mapper's views, MaskFormer.forward with ``height`` / ``width`` per view, torch's flip, ``+=`` and ``/ n`` (the reference's loop,
mask2former/test_time_augmentation.py:83-97).  One uint8 48 x 96 image, MIN_SIZES (32, 48, 64), FLIP: six views."""
import sys

import pytest
import torch

from rba_amd import arch as A
from tests import _tta_cases as G

pytestmark = pytest.mark.gpu
BAR = 4.0 * G.FLOOR
H, W = G.MODEL_IMAGE_HW


@pytest.fixture(scope="module")
def model():
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS["tiny1"])
    return load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()


@pytest.fixture(scope="module")
def truth(model):
    """the composition, computed once: (mean sem_seg [K,H,W] on the GPU, the host views)"""
    from rba_amd.test_time_augmentation import DatasetMapperTTA
    views = DatasetMapperTTA(G.aug_cfg(**{k.lower(): v for k, v in G.MODEL_AUG.items()}))({"image": G.model_image(), "height": H, "width": W})
    assert [tuple(v["image"].shape[1:]) for v in views] == [(32, 64), (32, 64), (48, 96), (48, 96), (64, 128), (64, 128)]
    total = None
    for i, v in enumerate(views):
        sem = model([{"image": v["image"], "height": H, "width": W}])[0]["sem_seg"]
        assert sem.shape[1:] == (H, W)
        if i % 2:
            sem = sem.flip(dims=[2])
        if total is None:
            total = sem.clone()
        else:
            total += sem
    return total / len(views), views


def _wrapper(model, **aug):
    from rba_amd.test_time_augmentation import SemanticSegmentorWithTTA
    s = {**{k.lower(): v for k, v in G.MODEL_AUG.items()}, **aug}
    return SemanticSegmentorWithTTA(G.aug_cfg(**s), model)


def _rel(t, want):
    e = float((t.double() - want.double()).abs().max() / want.double().abs().max())
    print(f"e = {e:.3e}  bar = {BAR:.3e}")
    return e


def test_sem_seg_equals_the_composition(model, truth):
    out = _wrapper(model)([{"image": G.model_image()}])
    assert len(out) == 1 and set(out[0]) == {"sem_seg"} and out[0]["sem_seg"].shape == truth[0].shape
    assert _rel(out[0]["sem_seg"], truth[0]) <= BAR
    # height / width given: the size the result is asked at
    out = _wrapper(model)([{"image": G.model_image(), "height": H, "width": W}])
    assert _rel(out[0]["sem_seg"], truth[0]) <= BAR


@pytest.mark.parametrize("mode", G.MODES)
def test_rba_scores_equal_the_score_of_the_compositions_average(model, truth, mode):
    w = _wrapper(model)
    want = G.ref_score(truth[0], mode)
    s = w.rba_scores([{"image": G.model_image()}], score=mode)
    assert len(s) == 1 and s[0].shape == (H, W)
    assert _rel(s[0], want) <= BAR
    s2, arg = w.rba_scores([{"image": G.model_image()}], return_argmax=True, score=mode)[0]
    assert torch.equal(s2, s[0]) and arg.dtype == torch.int32
    top2 = truth[0].topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > 8.0 * G.FLOOR * float(truth[0].abs().max())
    assert not ((arg.long() != truth[0].argmax(0)) & decided).any()


def test_device_views_equal_the_host_views_in_every_byte(model, truth):
    from rba_amd.test_time_augmentation import DatasetMapperTTA
    cfg = G.aug_cfg(**{k.lower(): v for k, v in G.MODEL_AUG.items()})
    dev = DatasetMapperTTA(cfg, device=model.device)({"image": G.model_image(), "height": H, "width": W})
    assert len(dev) == len(truth[1])
    for d, c in zip(dev, truth[1]):
        assert d["image"].is_cuda and d["image"].dtype == torch.uint8 and torch.equal(d["image"].cpu(), c["image"])
        assert d["transforms"] == c["transforms"] and d["height"] == H and d["width"] == W


def test_the_fused_path_is_the_one_in_use(model, truth, monkeypatch):
    """ops.resample_bilinear, torch.flip and Tensor.flip raise when the TTA module calls them (the network's own calls of ops.resample_bilinear -- FPN
    top-down, attention-mask downsample -- are not the wrapper's and pass): the wrapper still runs, so views and merge are K12b and K12a."""
    from rba_amd import ops
    tta = "rba_amd.test_time_augmentation"

    def guarded(fn, name):
        def wrapper(*a, **k):
            if sys._getframe(1).f_globals.get("__name__") == tta:
                raise AssertionError(f"{name} called by the TTA wrapper: the unfused path")
            return fn(*a, **k)
        return wrapper

    w = _wrapper(model)
    monkeypatch.setattr(ops, "resample_bilinear", guarded(ops.resample_bilinear, "ops.resample_bilinear"))
    monkeypatch.setattr(torch, "flip", guarded(torch.flip, "torch.flip"))
    monkeypatch.setattr(torch.Tensor, "flip", guarded(torch.Tensor.flip, "Tensor.flip"))
    assert _rel(w([{"image": G.model_image()}])[0]["sem_seg"], truth[0]) <= BAR
    assert _rel(w.rba_scores([{"image": G.model_image()}])[0], G.ref_score(truth[0], "rba")) <= BAR
    # the guard itself works: the unfused fallback trips it
    with pytest.raises(AssertionError):
        type(w)._unfused_mean([truth[0]], [True], (H, W))


def test_one_unflipped_view_of_the_images_size_returns_model_forwards_bits(model):
    w = _wrapper(model, min_sizes=(48,), flip=False)
    image = G.model_image()
    want = model([{"image": image}], return_argmax=True)[0]
    assert torch.equal(w([{"image": image}])[0]["sem_seg"], want["sem_seg"])
    s, arg = w.rba_scores([{"image": image}], return_argmax=True)[0]
    assert torch.equal(arg, want["argmax"])
    assert _rel(s, want["rba"]) <= BAR                       # (K = 19 rows of 96: the model's K1 runs its matrix-pipe form, another order of the same sum)


def test_more_than_sixteen_views_take_the_unfused_path_with_the_same_result(model):
    """nine sizes with their flipped twins = 18 views: ops.resample_bilinear and torch, within the bar of the fused arithmetic on the same class maps"""
    from rba_amd import ops
    w = _wrapper(model, min_sizes=(32,) * 9)
    inp = w._complete({"image": G.model_image()})
    sems, flips = w._view_class_maps(inp)
    assert len(sems) == 18 and not w._fused(sems) and w._fused(sems[:16])
    got = w([{"image": G.model_image()}])[0]["sem_seg"]
    half = ops.tta_merge(sems[:2], flips[:2], (H, W), want_sem_seg=True)[1]       # every pair is the same pair: the mean of 18 is the mean of 2
    assert _rel(got, half) <= BAR
    s, arg = w.rba_scores([{"image": G.model_image()}], return_argmax=True, score="energy")[0]
    assert _rel(s, G.ref_score(got, "energy")) <= BAR and arg.dtype == torch.int32


def test_ood_evaluator_accepts_the_wrapper(model, truth):
    from rba_amd import evaluate_ood as E
    from rba_amd.support import OODEvaluator
    w = _wrapper(model)
    x = G.model_image()[None]
    logits = E.get_logits(w, x)
    assert logits.shape == (1,) + tuple(truth[0].shape) and _rel(logits[0], truth[0]) <= BAR
    want, want_arg = w.rba_scores([{"image": x[0]}], return_argmax=True)[0]
    assert torch.equal(E.get_RbA(w, x), want)
    assert _rel(E.get_energy(w, x), G.ref_score(truth[0], "energy")) <= BAR
    ev = OODEvaluator(w, E.get_logits, E.get_RbA)
    gt = torch.zeros(1, H, W, dtype=torch.long)
    gt[:, 10:20, 10:30] = 1
    gt[:, :2] = 255
    scores, gts, preds = ev.compute_anomaly_scores([(x, gt)], device=torch.device("cuda"), return_preds=True)
    assert scores.shape == (1, H, W) and gts.shape == (1, 1, H, W) and preds.shape == (1, 1, H, W)
    assert torch.equal(torch.from_numpy(scores[0]), want.cpu()) and torch.equal(torch.from_numpy(preds[0, 0]), want_arg.cpu().long())
    r = ev.evaluate_ood(scores, gts, verbose=False)
    assert set(r) >= {"auroc", "aupr", "fpr95"}


def test_evaluate_ood_cli_with_tta(tmp_path, monkeypatch):
    """`python -m rba_amd.evaluate_ood --tta`, and a checkpoint config with TEST.AUG.ENABLED without the flag: every image is scored through the wrapper,
    on the serial loop (one stream, no graph capture -- the defaults ask for three streams and graphs), and both give the same metrics; without
    either the wrapper is not built."""
    import pickle
    import yaml
    from rba_amd import evaluate_ood as E
    from rba_amd import test_time_augmentation as T
    from tests.test_datasets_cpu import make_road_anomaly
    a = A.complete(A.ARCHS["tiny1"])
    cfg = {"MODEL": {"SWIN": {"EMBED_DIM": 32, "DEPTHS": [2, 2, 2, 2], "NUM_HEADS": [1, 2, 4, 8], "WINDOW_SIZE": 6},
                     "SEM_SEG_HEAD": {"CONVS_DIM": 64, "MASK_DIM": 64, "TRANSFORMER_ENC_LAYERS": 2,
                                      "DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["res5"]},
                     "MASK_FORMER": {"HIDDEN_DIM": 64, "NHEADS": 2, "NUM_OBJECT_QUERIES": 16, "DIM_FEEDFORWARD": 128, "DEC_LAYERS": 2}},
           "TEST": {"AUG": {"ENABLED": False, "MIN_SIZES": [32, 48], "MAX_SIZE": 4096, "FLIP": True}}}
    data = tmp_path / "data"
    make_road_anomaly(str(data), n=3, h=48, w=80)
    calls, timings = [], []
    real_scores, real_run = T.SemanticSegmentorWithTTA.rba_scores, E._run_evaluations
    monkeypatch.setattr(T.SemanticSegmentorWithTTA, "rba_scores", lambda self, *a_, **k: calls.append(1) or real_scores(self, *a_, **k))

    def run(model, dataset, model_name, dataset_name, args, rank=0, world=1, timing=None):
        r = real_run(model, dataset, model_name, dataset_name, args, rank, world, timing)
        timings.append((type(model).__name__, args.streams, args.graph, dict(timing)))
        return r

    monkeypatch.setattr(E, "_run_evaluations", run)
    res = {}
    for tag, enabled, flags in (("flag", False, ["--tta"]), ("config", True, []), ("off", False, [])):
        cfg["TEST"]["AUG"]["ENABLED"] = enabled
        mdir = tmp_path / f"ckpts_{tag}" / "m"
        mdir.mkdir(parents=True)
        (mdir / "config.yaml").write_text(yaml.safe_dump(cfg))
        torch.save({"model": A.seeded_weights(a, 0)}, mdir / "model_final.pth")
        n0 = len(calls)
        E.main(["--models_folder", str(tmp_path / f"ckpts_{tag}"), "--datasets_folder", str(data), "--out_path", str(tmp_path / f"res_{tag}"), "--verbose", "0",
                "--dataset_mode", "selective", "--selected_datasets", "road_anomaly", "--num_workers", "2"] + flags)
        with open(tmp_path / f"res_{tag}" / "m" / "results.pkl", "rb") as f:
            res[tag] = pickle.load(f)["road_anomaly"]
        name, streams, graph, timing = timings[-1]
        if tag == "off":
            assert len(calls) == n0 and name == "MaskFormer" and (streams, graph) == (3, 1)
        else:
            assert len(calls) - n0 == 3 and name == "SemanticSegmentorWithTTA" and (streams, graph) == (1, 0)
            assert timing["images"] == 3 and timing["streams"] == 1 and timing["hip_graphs"] == 0
    assert res["flag"] == res["config"] and set(res["flag"]) >= {"auroc", "aupr", "fpr95"}
