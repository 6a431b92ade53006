"""GPU: K18 (rba_amd.bootstrap_ops, csrc/bootstrap_curve.hip) -- the curves of every trial from one sorted pixel list against the CPU truth of
tests/_bootstrap_cases.py (rba_amd.metrics.ood_metrics on every trial's pixels), reproducibility, the (score, tag) producer against select_labelled, its
capacity flag, the wrappers' refusals, and `--bootstrap` through the command line.

Bars.  P, N, auroc2, fp95 and tp95 are integers: equal.  fpr95 is the float64 quotient of two of them: bitwise equal.  auroc and aupr: 1e-12 absolute --
float64 sums of at most 10^4 terms of magnitude at most 1 (10^4 * 2^-53 = 1.1e-12 is the worst case of a sum whose every term rounds the same way; these
are a few thousand terms), not a measured bar."""
import numpy as np
import pytest
import torch

from tests import _bootstrap_cases as C

pytestmark = pytest.mark.gpu

CHUNKS = (64, None)            # 64: dozens of chunks per case (runs and the walk from the crossing span them); None: the product's rule


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run rba_amd.bootstrap_ops' allocations under the guard bands too"""
    import rba_amd.bootstrap_ops as B
    if canary is None:
        yield
        return
    real, B.torch = B.torch, canary._PROXY
    try:
        yield
    finally:
        B.torch = real


def _curves(name, chunk):
    from rba_amd import bootstrap_ops as B
    s, tag = C.sorted_list(name)
    members = C.case(name)[2]
    r = B.subset_curves(s.cuda(), tag.cuda(), B.member_words(members, "cuda"), int(members.shape[0]), chunk=chunk)
    return {k: v.cpu().numpy() for k, v in r.items()}


@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", C.CASES)
def test_k18_equals_the_truth_of_every_trial(name, chunk):
    want = C.truth(name)
    got = _curves(name, chunk)
    assert got["ap"].dtype == np.float64 and all(got[k].dtype == np.int64 for k in ("P", "N", "auroc2", "fp95", "tp95"))
    for k in ("P", "N", "auroc2", "fp95", "tp95"):
        assert np.array_equal(got[k], want[k]), f"{name} chunk {chunk} {k}: {got[k].tolist()} != {want[k].tolist()}"
    with np.errstate(divide="ignore", invalid="ignore"):
        P, N = got["P"].astype(np.float64), got["N"].astype(np.float64)
        fpr95, auroc, aupr = got["fp95"].astype(np.float64) / N, got["auroc2"].astype(np.float64) / (2.0 * P * N), got["ap"] / P
    assert np.array_equal(np.isnan(fpr95), np.isnan(want["fpr95"]))
    ok = ~np.isnan(fpr95)
    assert np.array_equal(fpr95[ok].view(np.int64), want["fpr95"][ok].view(np.int64)), f"{name}: fpr95 {fpr95.tolist()} != {want['fpr95'].tolist()}"
    for k, v in (("auroc", auroc), ("aupr", aupr)):
        assert np.array_equal(np.isnan(v), np.isnan(want[k])), f"{name} {k}: {v.tolist()} != {want[k].tolist()}"
        err = np.nanmax(np.abs(v - want[k]), initial=0.0)
        print(f"{name} chunk {chunk}: max |d {k}| = {err:.3g}")
        assert err <= 1e-12, f"{name} chunk {chunk} {k}: off by {err:.3g}"
    if name == "no_positive":
        assert int(got["P"][2]) == 0 and np.isnan(auroc[2]) and np.isnan(aupr[2]) and fpr95[2] == 0.0
    if name == "collinear":
        assert np.all(got["fp95"] != want["fp95_all"]), "the walk past the dropped points is what this case is for"


@pytest.mark.parametrize("name", C.CASES)
def test_bootstrap_ood_metrics_on_the_device_equals_the_cpu_loop(name):
    """the public function end to end (tags, the sort on the device, the membership words, the read-back)"""
    from rba_amd import metrics
    s, y, ids = C.pooled(name)
    want = C.truth(name)
    got = metrics.bootstrap_ood_metrics(s.cuda(), y.cuda(), ids.cuda(), C.case(name)[2])
    for k in ("auroc", "aupr", "fpr95"):
        assert got[k].dtype == np.float64 and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (name, k)
        assert np.nanmax(np.abs(got[k] - want[k]), initial=0.0) <= (0.0 if k == "fpr95" else 1e-12), (name, k, got[k].tolist(), want[k].tolist())


def test_more_than_64_trials_run_as_several_calls():
    from rba_amd import metrics
    s, y, ids = C.pooled("ties")
    members = C.draws(9, 8, 70, 0.5)
    got = metrics.bootstrap_ood_metrics(s.cuda(), y.cuda(), ids.cuda(), members)
    want = metrics.bootstrap_ood_metrics(s, y, ids, members)
    for k in want:
        assert got[k].shape == (70,) and np.max(np.abs(got[k] - want[k])) <= (0.0 if k == "fpr95" else 1e-12), k


@pytest.mark.parametrize("name", ["ties", "constant", "trials_64_50"])
def test_two_runs_are_bitwise_equal(name):
    a, b = _curves(name, 64), _curves(name, 64)
    for k in a:
        assert np.array_equal(a[k].view(np.int64), b[k].view(np.int64)), (name, k)


def _pairs(scores, tags):
    return sorted(zip(scores.cpu().numpy().view(np.int32).tolist(), tags.cpu().numpy().tolist()))


@pytest.mark.parametrize("label_dtype", [torch.uint8, torch.int64])
def test_labelled_tags_equal_select_labelled(label_dtype, canary):
    from rba_amd import bootstrap_ops as B
    from rba_amd import metrics
    score, lab, _ = C.case("ties")
    n = score.shape[0]
    capacity = score.size
    out_s, out_t = canary.empty(capacity, dtype=torch.float32), canary.empty(capacity, dtype=torch.int32)
    cursor = torch.zeros(2, dtype=torch.int64, device="cuda")
    want = []
    for i in range(n):
        s, g = torch.from_numpy(score[i]).cuda(), torch.from_numpy(lab[i]).to(label_dtype).cuda()
        B.labelled_tags(s, g, 1000 + i, out_s, out_t, cursor)
        ss, yy = metrics.select_labelled(torch.from_numpy(score[i]), torch.from_numpy(lab[i]))
        want += list(zip(ss.numpy().view(np.int32).tolist(), (((1000 + i) << 1) | yy.to(torch.int64)).tolist()))
    count, overflow = cursor.tolist()
    assert overflow == 0 and count == len(want)
    assert _pairs(out_s[:count], out_t[:count]) == sorted(want)


def test_labelled_tags_raise_the_flag_and_write_nothing_past_the_buffer(canary):
    from rba_amd import bootstrap_ops as B
    score, lab, _ = C.case("continuous")
    labelled = int((lab[0] != 255).sum()) + int((lab[1] != 255).sum())
    capacity = labelled - 37                                         # the second image does not fit
    out_s, out_t = canary.empty(capacity, dtype=torch.float32), canary.empty(capacity, dtype=torch.int32)
    cursor = torch.zeros(2, dtype=torch.int64, device="cuda")
    for i in range(2):
        B.labelled_tags(torch.from_numpy(score[i]).cuda(), torch.from_numpy(lab[i]).cuda(), i, out_s, out_t, cursor)
    assert cursor.tolist() == [labelled, 1]
    canary.check()                                                   # the guard bands behind both buffers are intact
    tags = out_t.cpu().numpy()
    assert np.all((tags >> 1 == 0) | (tags >> 1 == 1)), "every slot inside the buffer was written with a pair"


class _Reached(Exception):
    pass


def test_one_fault_is_refused_before_anything_is_allocated_or_launched(monkeypatch):
    from rba_amd import bootstrap_ops as B
    from rba_amd._lib import RbaHipError

    def reached(name, *args, **kw):
        raise _Reached(name)
    monkeypatch.setattr(B, "_launch", reached)
    n, n_images = 500, 5
    score = torch.rand(n, device="cuda")
    tag = torch.zeros(n, dtype=torch.int32, device="cuda")
    member = torch.ones(n_images, dtype=torch.int64, device="cuda")
    smap = torch.rand(10, 50, device="cuda")
    lmap = torch.zeros(10, 50, dtype=torch.uint8, device="cuda")
    out_s, out_t = torch.empty(n, device="cuda"), torch.empty(n, dtype=torch.int32, device="cuda")
    cursor = torch.zeros(2, dtype=torch.int64, device="cuda")
    curves = lambda **kw: lambda: B.subset_curves(**{**dict(score=score, tag=tag, member=member, T=7), **kw})                      # noqa: E731
    tags = lambda **kw: lambda: B.labelled_tags(**{**dict(score=smap, labels=lmap, image_index=3, out_score=out_s, out_tag=out_t, cursor=cursor), **kw})   # noqa: E731
    rows = [
        ("subset_curves", curves(), True),
        ("subset_curves T = 1", curves(T=1), True),
        ("subset_curves T = 64", curves(T=64), True),
        ("subset_curves: score on the CPU", curves(score=score.cpu()), False),
        ("subset_curves: tag on the CPU", curves(tag=tag.cpu()), False),
        ("subset_curves: member on the CPU", curves(member=member.cpu()), False),
        ("subset_curves: score float64", curves(score=score.double()), False),
        ("subset_curves: tag int64", curves(tag=tag.long()), False),
        ("subset_curves: member int32", curves(member=member.int()), False),
        ("subset_curves: score strided", curves(score=torch.rand(2 * n, device="cuda")[::2]), False),
        ("subset_curves: tag strided", curves(tag=torch.zeros(2 * n, dtype=torch.int32, device="cuda")[::2]), False),
        ("subset_curves: member strided", curves(member=torch.ones(2 * n_images, dtype=torch.int64, device="cuda")[::2]), False),
        ("subset_curves: T = 0", curves(T=0), False),
        ("subset_curves: T = 65", curves(T=65), False),
        ("subset_curves: T = 7.0", curves(T=7.0), False),
        ("subset_curves: score and tag of different length", curves(tag=tag[:-1]), False),
        ("subset_curves: no pixel", curves(score=score[:0], tag=tag[:0]), False),
        ("subset_curves: score 2-d", curves(score=score.reshape(5, 100)), False),
        ("subset_curves: chunk 100", curves(chunk=100), False),
        ("subset_curves: chunk 0", curves(chunk=0), False),
        ("labelled_tags", tags(), True),
        ("labelled_tags int64 labels", tags(labels=lmap.long()), True),
        ("labelled_tags: score on the CPU", tags(score=smap.cpu()), False),
        ("labelled_tags: labels on the CPU", tags(labels=lmap.cpu()), False),
        ("labelled_tags: out_score on the CPU", tags(out_score=out_s.cpu()), False),
        ("labelled_tags: cursor on the CPU", tags(cursor=cursor.cpu()), False),
        ("labelled_tags: score float64", tags(score=smap.double()), False),
        ("labelled_tags: labels int32", tags(labels=lmap.int()), False),
        ("labelled_tags: out_tag int64", tags(out_tag=out_t.long()), False),
        ("labelled_tags: cursor int32", tags(cursor=cursor.int()), False),
        ("labelled_tags: score strided", tags(score=torch.rand(10, 100, device="cuda")[:, ::2]), False),
        ("labelled_tags: labels strided", tags(labels=torch.zeros(10, 100, dtype=torch.uint8, device="cuda")[:, ::2]), False),
        ("labelled_tags: out_score strided", tags(out_score=torch.empty(2 * n, device="cuda")[::2]), False),
        ("labelled_tags: image_index 2^30", tags(image_index=1 << 30), False),
        ("labelled_tags: image_index -1", tags(image_index=-1), False),
        ("labelled_tags: labels of another size", tags(labels=lmap[:-1]), False),
        ("labelled_tags: out_score and out_tag of different capacity", tags(out_tag=out_t[:-1]), False),
        ("labelled_tags: cursor of three elements", tags(cursor=torch.zeros(3, dtype=torch.int64, device="cuda")), False),
    ]
    wrong = []
    for name, call, well_formed in rows:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        try:
            call()
            outcome = "returned"
        except RbaHipError:
            outcome = "refused"
        except _Reached as e:
            outcome = f"reached {e}"
        except Exception as e:                                           # noqa: BLE001 -- the table reports every row, whatever it ran into
            outcome = f"{type(e).__name__}: {e}"
        grew = torch.cuda.memory_allocated() - before
        if not (outcome.startswith("reached") if well_formed else (outcome == "refused" and grew == 0)):
            wrong.append(f"{name}: {outcome}, {grew} bytes allocated")
    assert not wrong, "\n".join(wrong)


def test_one_pass_equals_the_rescoring_loop_on_the_device():
    """OODEvaluator.evaluate_ood_bootstrapped(one_pass=True) with a model on the device: labelled_tags, the sort and K18 behind a stand-in score function"""
    from rba_amd.support import OODEvaluator

    class OnDevice:
        device = torch.device("cuda")

    score, lab, _ = C.case("ties")
    data = [(torch.from_numpy(np.repeat(score[i][None], 3, 0)), torch.from_numpy(lab[i].astype(np.int64))) for i in range(score.shape[0])]
    ev = OODEvaluator(OnDevice(), None, lambda model, x: x[0].mean(0))
    np.random.seed(3)
    want = ev.evaluate_ood_bootstrapped(data, ratio=0.5, trials=5, num_workers=0)
    np.random.seed(3)
    got = ev.evaluate_ood_bootstrapped(data, ratio=0.5, trials=5, num_workers=0, one_pass=True)
    for a, b in zip(got, want):
        assert set(a) == set(b) == {"auroc", "aupr", "fpr95"} and all(abs(a[k] - b[k]) < 1e-10 for k in a), (got, want)     # percent: 100 x 1e-12


def test_bootstrap_flag_through_the_command_line(tmp_path, monkeypatch):
    """`python -m rba_amd.evaluate_ood --bootstrap 5` on the tiny model: value = the file without the flag, mean / std = the CPU loop over the same pooled
    pixels and the same draws"""
    import pickle
    import yaml
    from rba_amd import arch as A
    from rba_amd import evaluate_ood as E
    from rba_amd import metrics
    from tests.test_datasets_cpu import make_fs_laf
    a = A.complete(A.ARCHS["tiny1"])
    mdir = tmp_path / "ckpts" / "tiny"
    mdir.mkdir(parents=True)
    cfg = {"MODEL": {"SWIN": {"EMBED_DIM": 32, "DEPTHS": [2, 2, 2, 2], "NUM_HEADS": [1, 2, 4, 8], "WINDOW_SIZE": 6},
                     "SEM_SEG_HEAD": {"CONVS_DIM": 64, "MASK_DIM": 64, "TRANSFORMER_ENC_LAYERS": 2,
                                      "DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["res5"]},
                     "MASK_FORMER": {"HIDDEN_DIM": 64, "NHEADS": 2, "NUM_OBJECT_QUERIES": 16, "DIM_FEEDFORWARD": 128, "DEC_LAYERS": 2}}}
    (mdir / "config.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model": A.seeded_weights(a, 0)}, mdir / "model_final.pth")
    data = tmp_path / "data"
    make_fs_laf(str(data), n=6, h=40, w=72)
    monkeypatch.chdir(tmp_path)
    argv = ["--models_folder", str(tmp_path / "ckpts"), "--datasets_folder", str(data), "--verbose", "false", "--dataset_mode", "selective",
            "--selected_datasets", "fishyscapes_laf", "--num_workers", "0", "--streams", "1", "--graph", "0"]
    seen = {}
    from rba_amd import distributed as D
    pooled = D.pooled_bootstrap_metrics

    def spy(scores, tags, members):
        seen.update(scores=scores.cpu(), tags=tags.cpu(), members=np.array(members))
        return pooled(scores, tags, members)
    monkeypatch.setattr(D, "pooled_bootstrap_metrics", spy)
    E.main(argv + ["--out_path", str(tmp_path / "plain")])
    E.main(argv + ["--out_path", str(tmp_path / "boot"), "--bootstrap", "5", "--bootstrap_seed", "11"])
    with open(tmp_path / "plain" / "tiny" / "results.pkl", "rb") as f:
        plain = pickle.load(f)["fishyscapes_laf"]
    with open(tmp_path / "boot" / "tiny" / "results.pkl", "rb") as f:
        boot = pickle.load(f)["fishyscapes_laf"]
    assert set(plain) == set(boot) == {"auroc", "aupr", "fpr95"}
    n_images = seen["members"].shape[1]
    assert np.array_equal(seen["members"], E.bootstrap_members(n_images, 5, 0.5, 11)) and seen["members"].sum(1).tolist() == [n_images // 2] * 5
    loop = metrics.bootstrap_ood_metrics(seen["scores"], seen["tags"] & 1, seen["tags"] >> 1, seen["members"])
    for k in plain:
        assert set(boot[k]) == {"value", "mean", "std"}
        assert boot[k]["value"] == plain[k], k
        assert abs(boot[k]["mean"] - float(np.mean(loop[k]))) <= 1e-12 and abs(boot[k]["std"] - float(np.std(loop[k]))) <= 1e-12, (k, boot[k], loop[k])
