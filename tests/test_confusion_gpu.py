"""K13 (ops.confusion_accumulate, csrc/confusion.hip) against the numpy oracle of its per-pixel rule (tests/_confusion_cases.py).  Integer counts: every
comparison is exact."""
import numpy as np
import pytest
import torch

from tests import _confusion_cases as G

pytestmark = pytest.mark.gpu


def _ks():
    from rba_amd import ops
    return sorted({1, 2, 19, 20, 150, 255, ops.CONFUSION_LDS_MAX_K, ops.CONFUSION_LDS_MAX_K + 1})


KS = (1, 2, 19, 20, 126, 127, 150, 255)          # test_the_class_counts_cover_the_threshold pins this list to ops.CONFUSION_LDS_MAX_K


def test_the_class_counts_cover_the_threshold():
    """the last K of the LDS form and the first K of the global form are in KS, whatever the threshold is"""
    assert list(KS) == _ks()


def run(pred, gt, K, ignore_label=255, lut=None, conf=None, bad=None, launches=1):
    """numpy or device maps -> (conf, bad) as numpy after `launches` calls on zeroed (or the given) outputs"""
    from rba_amd import ops
    dev = torch.device("cuda")
    p = pred if torch.is_tensor(pred) else torch.from_numpy(np.ascontiguousarray(pred)).to(dev)
    g = gt if torch.is_tensor(gt) else torch.from_numpy(np.ascontiguousarray(gt)).to(dev)
    conf = torch.zeros((K + 1, K + 1), dtype=torch.int64, device=dev) if conf is None else conf
    bad = torch.zeros(2, dtype=torch.int64, device=dev) if bad is None else bad
    lut_d = None if lut is None else torch.from_numpy(np.asarray(lut, dtype=np.uint8)).to(dev)
    for _ in range(launches):
        ops.confusion_accumulate(p, g, K, conf, bad, ignore_label, lut_d)
    return conf.cpu().numpy(), bad.cpu().numpy()


def check(pred, gt, K, ignore_label=255, lut=None, what=""):
    conf, bad = run(pred, gt, K, ignore_label, lut)
    want_conf, want_bad = G.oracle(pred.cpu().numpy() if torch.is_tensor(pred) else pred, gt.cpu().numpy() if torch.is_tensor(gt) else gt, K, ignore_label, lut)
    assert np.array_equal(bad, want_bad), f"{what}: bad {bad} != {want_bad}"
    assert np.array_equal(conf, want_conf), f"{what}: {int((conf != want_conf).sum())} counters differ"
    return conf, bad


@pytest.mark.parametrize("content", G.CONTENTS)
@pytest.mark.parametrize("K", KS)
def test_every_size_and_content_equals_the_oracle(K, content):
    """heads, tails, one and several workgroups, two sweeps of the capped grid; contention (one counter takes the map), no run to merge (alternating), runs that
    end beside every tile boundary"""
    sizes = G.confusion_sizes()
    pred, gt = G.make_maps(content, max(sizes), K)
    pd, gd = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    for n in sizes:
        conf, bad = run(pd[:n], gd[:n], K)
        want_conf, want_bad = G.oracle(pred[:n], gt[:n], K)
        assert not want_bad.any() and np.array_equal(bad, want_bad), (n, bad)
        assert np.array_equal(conf, want_conf), f"n = {n}: {int((conf != want_conf).sum())} counters differ"
        assert conf.sum() == n


@pytest.mark.parametrize("K", (19, 150))
def test_int64_labels_equal_uint8_labels(K):
    for content in ("blocks", "uniform"):
        pred, gt = G.make_maps(content, 4097 + 65, K, seed=3)
        a = run(pred, gt, K)
        b = run(pred, gt.astype(np.int64), K)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].sum() == pred.size


def _sprinkle(gt, value, every, seed=0):
    rng = np.random.default_rng(seed)
    gt = gt.copy()
    gt[rng.random(gt.size) < 1.0 / every] = value
    gt[:40:3] = value                                         # some in the scalar head and the first tiles whatever the seed
    return gt


def test_ignore_label():
    n = 4097 + 1024
    for K in (19, 126, 127, 255):
        pred, gt = G.make_maps("blocks", n, K, seed=1)
        gt = _sprinkle(gt, 255, 9)
        # 255 = the ignore label: column K
        conf, bad = check(pred, gt, K, 255, what=f"K={K} ignore 255")
        assert conf[:, K].sum() >= (gt == 255).sum() and not bad.any()
        # ignore_label = K: a label K is the ignored column either way; 255 is out of range unless K = 255
        check(pred, _sprinkle(gt, K, 11, seed=2), K, K, what=f"K={K} ignore K")
    # no ignore label, 255s present.  K = 19: 255 is out of range, a bad label.  K = 255: the rule's range 0..K holds 255, which IS column K -- the rule as
    # include/rba_hip.h states it; the oracle decides, and these two asserts say what it decided
    for ignore in (-1, None):
        pred, gt = G.make_maps("blocks", n, 19, seed=1)
        gt = _sprinkle(gt, 255, 9)
        conf, bad = check(pred, gt, 19, ignore, what="K=19 no ignore")
        assert bad[0] == (gt == 255).sum() and bad[1] == 0 and conf.sum() == n - bad[0]
        pred, gt = G.make_maps("blocks", n, 255, seed=1)
        gt = _sprinkle(gt, 255, 9)
        conf, bad = check(pred, gt, 255, ignore, what="K=255 no ignore")
        assert not bad.any() and conf[:, 255].sum() == (gt == 255).sum()


@pytest.mark.parametrize("K", (19, 127))
def test_label_table(K):
    """Cityscapes raw ids through the id -> trainId table, ids 34..255 sprinkled in (they map to 255 = ignored); uint8 and int64 labels, the int64 ones with
    -1 and 256, which no table entry exists for: bad labels"""
    lut = G.cityscapes_lut()
    rng = np.random.default_rng(5)
    n = 4097 + 300
    runs = rng.integers(1, 200, n)
    ids = np.repeat(rng.integers(0, 34, n), runs)[:n].astype(np.uint8)
    far = rng.random(n) < 0.05
    ids[far] = rng.integers(34, 256, int(far.sum())).astype(np.uint8)
    pred = np.repeat(rng.integers(0, min(K, 19), n, dtype=np.int32), runs)[:n].copy()
    conf8, bad8 = check(pred, ids, K, 255, lut, what="uint8 ids")
    assert not bad8.any() and conf8[:, K].sum() == (lut[ids] == 255).sum() and conf8.sum() == n
    conf64, bad64 = check(pred, ids.astype(np.int64), K, 255, lut, what="int64 ids")
    assert np.array_equal(conf64, conf8) and not bad64.any()
    wide = ids.astype(np.int64)
    wide[5::97] = -1
    wide[6::89] = 256
    wide[7::1001] = 1 << 40
    conf, bad = check(pred, wide, K, 255, lut, what="int64 ids with -1 and 256")
    assert bad[0] == ((wide < 0) | (wide > 255)).sum() and bad[1] == 0 and conf.sum() == n - bad[0]


@pytest.mark.parametrize("K", (19, 127))
def test_bad_predictions_are_counted_and_left_out(K):
    n = 4097 + 200
    pred, gt = G.make_maps("blocks", n, K, seed=2)
    pred[3::101] = -1
    pred[4::103] = K
    pred[5::107] = 1 << 30
    gt = _sprinkle(gt, 255, 13)
    gt[3::202] = K + 1 if K + 1 < 255 else 254                # both out of range on some pixels: counts as a label
    conf, bad = check(pred, gt, K, 255, what="bad predictions")
    out = (pred < 0) | (pred >= K)
    lab = (gt > K) & (gt != 255)
    assert bad[0] == lab.sum() and bad[1] == (out & ~lab).sum() and bad[1] > 0 and bad[0] > 0 and conf.sum() == n - bad.sum()


@pytest.mark.parametrize("K", (19, 127))
def test_accumulates_with_64_bit_carry(K):
    """conf pre-filled with 2^40 + i, one counter at 2^32 - 1; two launches -> the prefill plus twice the oracle"""
    n = 4097
    pred, gt = G.make_maps("blocks", n, K, seed=4)
    want, _ = G.oracle(pred, gt, K)
    pre = (1 << 40) + np.arange((K + 1) ** 2, dtype=np.int64).reshape(K + 1, K + 1)
    hot = np.unravel_index(int(want.argmax()), want.shape)
    pre[hot] = (1 << 32) - 1
    conf = torch.from_numpy(pre.copy()).cuda()
    bad = torch.tensor([1 << 33, 7], dtype=torch.int64, device="cuda")
    got, got_bad = run(pred, gt, K, conf=conf, bad=bad, launches=2)
    assert np.array_equal(got, pre + 2 * want) and got[hot] > 1 << 32
    assert got_bad.tolist() == [1 << 33, 7]


def test_same_bits_every_launch():
    for K, content in ((19, "uniform"), (150, "uniform"), (19, "blocks")):
        pred, gt = G.make_maps(content, 1 << 18, K, seed=6)
        gt = _sprinkle(gt, 255, 17)
        a, b = run(pred, gt, K), run(pred, gt, K)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("K", (19, 127))
def test_misaligned_views_equal_aligned_copies(K):
    """pred = big[1:1+n], gt = bigu8[3:3+n] (no pixel offset aligns both to 16 bytes: the labels go by element accesses) and other offsets, among them ones
    where both align after a head of 1..15 pixels; int64 labels at an odd element offset"""
    n = 4097 + 47
    pred, gt = G.make_maps("boundary16", n + 32, K, seed=7)
    gt = _sprinkle(gt, 255, 19)
    big, bigu8, big64 = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), torch.from_numpy(gt.astype(np.int64)).cuda()
    for po, go in ((1, 3), (0, 0), (1, 12), (3, 4), (2, 5), (0, 1), (3, 15), (2, 8)):
        for m in (n, 29, 5):
            p, g = big[po:po + m], bigu8[go:go + m]
            assert p.data_ptr() % 16 == 4 * po and g.data_ptr() % 16 == go
            got = run(p, g, K)
            ref = run(p.clone(), g.clone(), K)
            want = G.oracle(pred[po:po + m], gt[go:go + m], K)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[0], want[0]), (po, go, m)
    for po, go in ((1, 1), (2, 1), (0, 1), (3, 2)):
        got = run(big[po:po + n], big64[go:go + n], K)
        want = G.oracle(pred[po:po + n], gt[go:go + n], K)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (po, go)


@pytest.mark.parametrize("K", (19, 127))
def test_graph_capture(K):
    """one call captured on one stream (no parallel branches), replayed three times: the warm-up call plus three replays"""
    from rba_amd import ops
    n = 4097
    pred, gt = G.make_maps("blocks", n, K, seed=8)
    want, _ = G.oracle(pred, gt, K)
    p, g = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    conf = torch.zeros((K + 1, K + 1), dtype=torch.int64, device="cuda")
    bad = torch.zeros(2, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.confusion_accumulate(p, g, K, conf, bad)         # warm-up: counts once
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ops.confusion_accumulate(p, g, K, conf, bad)         # captured, not run
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(conf.cpu().numpy(), 4 * want) and bad.tolist() == [0, 0]


def test_refusals(monkeypatch):
    """every error of the wrapper is raised before any launch"""
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    K = 19
    dev = "cuda"
    pred = torch.zeros((8, 12), dtype=torch.int32, device=dev)
    gt = torch.zeros((8, 12), dtype=torch.uint8, device=dev)
    conf = torch.zeros((K + 1, K + 1), dtype=torch.int64, device=dev)
    bad = torch.zeros(2, dtype=torch.int64, device=dev)
    lut = torch.zeros(256, dtype=torch.uint8, device=dev)

    def no_launch(*a, **k):
        raise AssertionError("launched")

    monkeypatch.setattr(ops, "_launch", no_launch)
    cases = {
        "pred dtype": dict(pred=pred.long()),
        "pred on the host": dict(pred=pred.cpu()),
        "pred not contiguous": dict(pred=torch.zeros((12, 8), dtype=torch.int32, device=dev).t()),
        "gt dtype": dict(gt=gt.to(torch.int32)),
        "gt float": dict(gt=gt.float()),
        "gt on the host": dict(gt=gt.cpu()),
        "shapes": dict(gt=torch.zeros((8, 13), dtype=torch.uint8, device=dev)),
        "same numel, other shape": dict(gt=torch.zeros((12, 8), dtype=torch.uint8, device=dev)),
        "conf shape": dict(conf=torch.zeros((K, K), dtype=torch.int64, device=dev)),
        "conf dtype": dict(conf=conf.to(torch.int32)),
        "conf on the host": dict(conf=conf.cpu()),
        "bad shape": dict(bad=torch.zeros(3, dtype=torch.int64, device=dev)),
        "bad dtype": dict(bad=bad.to(torch.int32)),
        "bad on the host": dict(bad=bad.cpu()),
        "lut size": dict(lut=lut[:255]),
        "lut dtype": dict(lut=lut.to(torch.int64)),
        "lut on the host": dict(lut=lut.cpu()),
        "K = 0": dict(num_classes=0),
        "K = 256": dict(num_classes=256, conf=torch.zeros((257, 257), dtype=torch.int64, device=dev)),
    }
    for what, change in cases.items():
        kw = dict(pred=pred, gt=gt, num_classes=K, conf=conf, bad=bad, ignore_label=255, lut=None)
        kw.update(change)
        with pytest.raises(RbaHipError):
            ops.confusion_accumulate(**kw)
            pytest.fail(what)
    monkeypatch.undo()
    ops.confusion_accumulate(pred, gt, K, conf, bad, 255, lut)          # the unchanged arguments are accepted
    assert int(conf.sum()) == pred.numel() and int(conf[0, 0]) == pred.numel()


def test_pixel_indices_past_two_to_the_31():
    """2^31 + 4114 pixels (8.6 GB of predictions): one pair everywhere except four marked pixels around index 2^31 and at the very end -- a 32-bit pixel or
    tile index would miss or double them.  The expectation is arithmetic, not a 2^31-element bincount.  One K: both forms share the index arithmetic
    (`accumulate`)."""
    from rba_amd import ops
    K = 19
    n = (1 << 31) + 4097 + 17
    pred = torch.zeros(n, dtype=torch.int32, device="cuda")
    gt = torch.zeros(n, dtype=torch.uint8, device="cuda")
    marks = torch.tensor([(1 << 31) - 1, 1 << 31, (1 << 31) + 1, n - 1], device="cuda")
    pred[marks] = 3 % K
    gt[marks] = 5
    conf = torch.zeros((K + 1, K + 1), dtype=torch.int64, device="cuda")
    bad = torch.zeros(2, dtype=torch.int64, device="cuda")
    ops.confusion_accumulate(pred, gt, K, conf, bad)
    got, got_bad = conf.cpu().numpy(), bad.tolist()
    del pred, gt
    torch.cuda.empty_cache()
    want = np.zeros((K + 1, K + 1), dtype=np.int64)
    want[0, 0] = n - 4
    want[3 % K, 5] = 4
    assert got_bad == [0, 0] and np.array_equal(got, want)
