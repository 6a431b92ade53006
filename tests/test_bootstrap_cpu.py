"""CPU: the bootstrap's definition (rba_amd.metrics.bootstrap_ood_metrics = the loop of ood_metrics over the trials' pixels) against scikit-learn, the
cases of tests/_bootstrap_cases.py, OODEvaluator.evaluate_ood_bootstrapped(one_pass=True) against the re-scoring loop under the same draws, and the
command line's results.pkl with and without --bootstrap."""
import pickle

import numpy as np
import pytest
import torch

from rba_amd import metrics
from tests import _bootstrap_cases as C


def test_the_cases_are_what_they_are_for():
    with_empty_trial = []
    for name in C.CASES:
        score, lab, members = C.case(name)
        s, y, ids = C.pooled(name)
        t = C.truth(name)                                           # (asserts that the integers reproduce ood_metrics' floats)
        assert 6 <= score.shape[0] <= 9 and score.shape[1:] == (24, 40) and 2000 <= s.numel() <= 10000, name
        assert np.all(lab[:, :2] == 255) and np.all(lab[:, :, -2:] == 255) and set(np.unique(lab)) == {0, 1, 255}, name
        share = float((lab == 1).sum()) / float((lab != 255).sum())
        assert 0.03 <= share <= 0.10, (name, share)
        assert np.array_equal(t["P"] + t["N"], np.array([int(np.isin(ids.numpy(), np.nonzero(row)[0]).sum()) for row in members])), name
        if (t["P"] == 0).any():
            with_empty_trial.append(name)
    assert with_empty_trial == ["no_positive"]
    t = C.truth("no_positive")
    assert t["P"][2] == 0 and np.isnan(t["auroc"][2]) and np.isnan(t["aupr"][2]) and t["fpr95"][2] == 0.0
    assert np.unique(C.case("constant")[0]).size == 1
    assert np.unique(C.case("ties")[0]).size < 100 < np.unique(C.case("continuous")[0]).size
    # (d): the first point above 0.95 is dropped as collinear, with fp moving: the answers with and without drop_intermediate differ in EVERY trial
    t = C.truth("collinear")
    k = C.case("collinear")[2].sum(1)
    assert np.array_equal(t["fp95"], 14 * k) and np.array_equal(t["fp95_all"], 8 * k) and np.array_equal(t["tp95"], 50 * k)
    for name in C.TRIAL_CASES:                                       # (e)
        members = C.case(name)[2]
        assert members.shape[0] == int(name.split("_")[1]) and members[-1].all()
        assert members[0].sum() == (9 if name.endswith("_100") or members.shape[0] == 1 else 4)


@pytest.mark.parametrize("name", ["continuous", "ties", "collinear"])
def test_the_cpu_loop_equals_scikit_learn_per_trial(name):
    from sklearn.metrics import auc, average_precision_score, roc_curve
    s, y, ids = C.pooled(name)
    members = C.case(name)[2]
    got = metrics.bootstrap_ood_metrics(s, y, ids, members)
    assert all(got[k].dtype == np.float64 and got[k].shape == (members.shape[0],) for k in ("auroc", "aupr", "fpr95"))
    for t, row in enumerate(members):
        sel = row[ids.numpy()]
        st, yt = s.numpy()[sel], y.numpy()[sel]
        fpr, tpr, _ = roc_curve(yt, st)
        want = {"auroc": auc(fpr, tpr), "aupr": average_precision_score(yt, st), "fpr95": next(f for f, r in zip(fpr, tpr) if r > 0.95)}
        for k in want:
            assert abs(got[k][t] - want[k]) < 1e-12, (name, t, k, got[k][t], want[k])


def _stand_in_data(n=8):
    rng = np.random.RandomState(0)
    data = []
    for _ in range(n):
        gt = torch.from_numpy(rng.choice([0, 1, 255], size=(12, 16), p=[0.8, 0.1, 0.1]))
        data.append((torch.from_numpy(np.round(rng.randn(3, 12, 16) * 4).astype(np.float32) / 4) + (gt == 1) * 2.0, gt))
    return data


@pytest.mark.parametrize("trials,ratio", [(3, 0.5), (9, 0.75), (4, 1.0)])
def test_one_pass_and_the_rescoring_loop_give_the_same_means_and_stds(trials, ratio):
    """the same np.random.choice calls in the same order: the same subsets, and (means, stds) equal to 1e-12 (this test fails without the feature: the keyword
    does not exist)"""
    from rba_amd.support import OODEvaluator
    ev = OODEvaluator(None, None, lambda model, x: x[0].mean(0))
    data = _stand_in_data()
    np.random.seed(7)
    want = ev.evaluate_ood_bootstrapped(data, ratio=ratio, trials=trials, num_workers=0)
    after_loop = np.random.rand()
    np.random.seed(7)
    got = ev.evaluate_ood_bootstrapped(data, ratio=ratio, trials=trials, num_workers=0, one_pass=True)
    assert np.random.rand() == after_loop, "the two paths consume the generator alike"
    for a, b in zip(got, want):
        assert set(a) == set(b) == {"auroc", "aupr", "fpr95"}
        for k in a:
            assert abs(a[k] - b[k]) <= 1e-12, (k, a[k], b[k])
    np.random.seed(7)
    assert ev.evaluate_ood_bootstrapped(data, ratio=ratio, trials=trials, num_workers=0, one_pass=False) == want      # the default is the loop


def test_member_words_pack_bit_t_of_word_i():
    from rba_amd import bootstrap_ops as B
    rng = np.random.RandomState(4)
    m = rng.rand(64, 11) < 0.5
    m[63, 3] = True
    w = B.member_words(m, "cpu")
    assert w.dtype == torch.int64 and w.shape == (11,)
    words = [int(v) & 0xFFFFFFFFFFFFFFFF for v in w.tolist()]
    assert all(bool((words[i] >> t) & 1) == bool(m[t, i]) for t in range(64) for i in range(11))
    with pytest.raises(RuntimeError):
        B.member_words(np.ones((65, 3), dtype=bool), "cpu")


def test_the_library_exports_the_entry_points_the_header_declares():
    import os
    import re
    from rba_amd import _lib
    names = ["rba_subset_curves_totals", "rba_subset_curves_walk", "rba_subset_curves_finish", "rba_labelled_tags_i32"]
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rba_hip.h")) as f:
        header = f.read()
    lib = _lib.load()
    for n in names:
        decl = re.search(r"\bint " + n + r"\(([^;]*)\);", header)
        assert decl is not None and hasattr(lib, n), n
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[n]), n            # the stream is the header's last parameter and the bindings' last argtype


class _TinyCpuModel(torch.nn.Module):
    """a stand-in with MaskFormer's calling convention, on the CPU: sem_seg [K,H,W] from a fixed 1x1 projection of the image"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.weight = torch.nn.Parameter(torch.randn(4, 3, generator=g))
        self.device = torch.device("cpu")

    def forward(self, batched):
        x = batched[0]["image"].float() / 64.0 - 2.0
        return [{"sem_seg": torch.einsum("kc,chw->khw", self.weight, torch.round(x * 2) / 2)}]


def _run_cli(tmp_path, monkeypatch, out, extra=()):
    from rba_amd import evaluate_ood as E
    mdir = tmp_path / "ckpts" / "tiny"
    mdir.mkdir(parents=True, exist_ok=True)
    (mdir / "config.yaml").write_text("MODEL: {}\n")
    (mdir / "model_final.pth").write_bytes(b"")
    model = _TinyCpuModel().eval()
    monkeypatch.setattr(E, "get_model", lambda config_path, model_path, device=None: model)
    monkeypatch.chdir(tmp_path)
    E.main(["--models_folder", str(tmp_path / "ckpts"), "--datasets_folder", str(tmp_path / "data"), "--out_path", str(tmp_path / out), "--verbose", "false",
            "--device", "cpu", "--num_workers", "0", "--dataset_mode", "selective", "--selected_datasets", "fishyscapes_laf"] + list(extra))
    with open(tmp_path / out / "tiny" / "results.pkl", "rb") as f:
        return model, f.read()


def test_results_pkl_with_and_without_the_bootstrap_flag(tmp_path, monkeypatch):
    """without --bootstrap the file is byte for byte the `value`-only structure {dataset: {metric: float}}; with it {dataset: {metric: {value, mean, std}}}
    where value is the same float and mean / std are the CPU loop's over the flag's draws"""
    from rba_amd import evaluate_ood as E
    from rba_amd.datasets import get_dataset
    from tests.test_datasets_cpu import make_fs_laf
    make_fs_laf(str(tmp_path / "data"), n=6, h=20, w=36)
    model, plain = _run_cli(tmp_path, monkeypatch, "plain")
    ds = get_dataset("fishyscapes_laf", str(tmp_path / "data"))
    s, y, ids = [], [], []
    for i in range(len(ds)):
        x, g = ds[i]
        si, yi = metrics.select_labelled(E.get_RbA(model, x[None]), g)
        s.append(si), y.append(yi), ids.append(torch.full((si.numel(),), i, dtype=torch.int64))
    s, y, ids = torch.cat(s), torch.cat(y), torch.cat(ids)
    value = metrics.ood_metrics(s, y)
    assert plain == pickle.dumps({"fishyscapes_laf": value}), pickle.loads(plain)
    _, boot = _run_cli(tmp_path, monkeypatch, "boot", ["--bootstrap", "70", "--bootstrap_ratio", "0.5", "--bootstrap_seed", "3"])
    boot = pickle.loads(boot)
    assert list(boot) == ["fishyscapes_laf"] and set(boot["fishyscapes_laf"]) == set(value)
    members = E.bootstrap_members(6, 70, 0.5, 3)
    assert members.shape == (70, 6) and members.sum(1).tolist() == [3] * 70 and len({tuple(r) for r in members.tolist()}) > 10
    loop = metrics.bootstrap_ood_metrics(s, y, ids, members)
    for k, v in boot["fishyscapes_laf"].items():
        assert set(v) == {"value", "mean", "std"} and v["value"] == value[k]
        assert abs(v["mean"] - float(np.mean(loop[k]))) <= 1e-12 and abs(v["std"] - float(np.std(loop[k]))) <= 1e-12, (k, v)
    _, again = _run_cli(tmp_path, monkeypatch, "plain2")
    assert again == plain
