"""The two homes of state that outlives one forward, driven on the CPU: lru.derived (images of the weights) and graph_replay.GraphReplay
(which key is eager, measured, captured).  Both are plain Python: CPU tensors, a fake capture and fake events stand in for the GPU."""
import copy
import pickle
from types import SimpleNamespace

import torch

from rba_amd import graph_replay as GR
from rba_amd import lru


class _View:                       # a plain object owner, as msdeformattn._LinearView
    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


def _owners():
    lin = torch.nn.Linear(8, 4)
    return [lin, _View(lin.weight, lin.bias), SimpleNamespace(weight=lin.weight, bias=lin.bias)]


def test_derived_hits_and_rebuilds_on_every_source_change():
    for owner in _owners():
        built = []

        def get(extra=()):
            def build():
                built.append(extra)
                return [len(built)]                              # a fresh object per build
            return lru.derived(owner, "image", (owner.weight, owner.bias), build, extra=extra)

        first = get()
        assert get() is first and get() is first and len(built) == 1, type(owner)          # a hit returns the same object
        with torch.no_grad():
            owner.weight.mul_(2.0)                               # in-place edit of the first source
        second = get()
        assert second is not first and get() is second and len(built) == 2
        with torch.no_grad():
            owner.bias.add_(1.0)                                 # ... and of the second (the bias VERSION is part of every key)
        third = get()
        assert third is not second and len(built) == 3
        owner.weight.data = owner.weight.data.clone()            # re-point: no version moves, the data pointer does
        fourth = get()
        assert fourth is not third and get() is fourth and len(built) == 4
        assert get(extra=64) is not fourth and len(built) == 5   # another `extra` is another value ...
        assert get(extra=64) is get(extra=64) and len(built) == 5
        assert get() is not fourth and len(built) == 6           # ... in the same slot: one entry per slot


def test_derived_bias_none_to_tensor_rebuilds():
    for owner in _owners():
        owner.bias = None
        n = []

        def get():
            return lru.derived(owner, "view", (owner.weight, owner.bias), lambda: n.append(0) or (owner.weight, owner.bias))

        assert get()[1] is None and get() is get() and len(n) == 1
        owner.bias = torch.nn.Parameter(torch.zeros(4))
        assert get()[1] is owner.bias and len(n) == 2
        owner.bias = torch.nn.Parameter(torch.ones(4))           # a replaced bias: the old one is still alive in the old value, so the pointer differs
        assert get()[1] is owner.bias and len(n) == 3


def test_derived_slots_coexist_and_peek_never_builds():
    for owner in _owners():
        assert lru.peek(owner, ("planes", "f16x3")) is None
        a = lru.derived(owner, ("planes", "f16x3"), (owner.weight,), lambda: ["h", "l"])
        b = lru.derived(owner, ("planes", "bf16x6"), (owner.weight,), lambda: ["b0", "b1", "b2"])
        assert lru.derived(owner, ("planes", "f16x3"), (owner.weight,), lambda: 1 / 0) is a        # the bf16x6 entry did not evict it
        assert lru.derived(owner, ("planes", "bf16x6"), (owner.weight,), lambda: 1 / 0) is b
        assert lru.peek(owner, ("planes", "f16x3")) is a and lru.peek(owner, ("planes", "bf16x6")) is b
        with torch.no_grad():
            owner.weight.mul_(2.0)
        assert lru.peek(owner, ("planes", "f16x3")) is a         # peek reports what is stored, stale or not; the next derived() replaces it
        assert lru.derived(owner, ("planes", "f16x3"), (owner.weight,), lambda: ["h2", "l2"]) is not a
        assert lru.peek(owner, ("planes", "bf16x6")) is b


def test_source_key_is_hashable_and_sees_device_and_extra():
    w, b = torch.zeros(3), torch.zeros(3)
    k = lru.source_key(w, None, b, extra=("pad", 64))
    assert hash(k) == hash(lru.source_key(w, None, b, extra=("pad", 64))) and k == lru.source_key(w, None, b, extra=("pad", 64))
    assert k != lru.source_key(w, b, None, extra=("pad", 64)) and k != lru.source_key(w, None, b) and k != lru.source_key(w, None, b.clone(), extra=("pad", 64))
    assert w.device in k and None in k


def test_copies_and_pickles_of_an_owner_start_with_an_empty_store():
    for owner in _owners():
        image = lru.derived(owner, "image", (owner.weight,), lambda: owner.weight.detach().clone())
        for twin in (copy.deepcopy(owner), pickle.loads(pickle.dumps(owner))):
            assert vars(twin).get(lru._STORE) is not None and len(vars(twin)[lru._STORE]) == 0, type(owner)
            assert lru.peek(twin, "image") is None
            rebuilt = lru.derived(twin, "image", (twin.weight,), lambda: twin.weight.detach().clone())        # built from the TWIN's weight on first use
            assert rebuilt is not image and torch.equal(rebuilt, image)
        assert lru.peek(owner, "image") is image                 # the original keeps its own
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    for m in model:
        lru.derived(m, "image", (m.weight,), lambda: object())
    assert not any(vars(m).get(lru._STORE) for m in copy.deepcopy(model).modules())


# ---------------------------------------------------------------------------------------------------------------- GraphReplay
class _Event:
    """stands in for a HIP event pair: e0.elapsed_time(e1) is the GPU span in milliseconds"""
    synchronised = 0

    def __init__(self, span_ms=None):
        self.span_ms = span_ms

    def synchronize(self):
        _Event.synchronised += 1

    def elapsed_time(self, other):
        return other.span_ms


def _key(h, weights=(1, 0), stream=7, score="rba"):
    return GR.GraphKey((3, h, 64), torch.uint8, "dev", stream, False, score, True, True, "f16x3", True, 0, 0, 1, True, None, weights)


class _Driver:
    """what MaskFormer.rba_scores / _graphed_scores do around GraphReplay.step, with a fake capture and fake timings"""

    def __init__(self, auto, issue_s=1.0, span_ms=1000.0, **limits):
        self.limits = SimpleNamespace(**dict(dict(GRAPH_MAX=8, GRAPH_THRASH_MAX=4, LAUNCH_BOUND_RATIO=0.95, GRAPH_REMEASURE_EVERY=32), **limits))
        self.state, self.auto, self.issue_s, self.span_ms = GR.GraphReplay(), auto, issue_s, span_ms
        self.captures, self.fail = [], False

    def call(self, key):
        """-> "eager" | "eager fast" | "measured" | "captured" | "replayed" | "failed" """
        fk = (key.shape, key.dtype, key.return_argmax, key.score, key.split_mode, key.stream)       # what rba_scores builds without the weights
        if self.auto and self.state.eager_left.get(fk, 0) > 0:
            self.state.eager_left[fk] -= 1
            return "eager fast"
        what = self.state.step(key, self.auto, self.limits)
        if what == "measure":
            self.state.measured(key, self.issue_s, _Event(), _Event(self.span_ms))
            return "measured"
        if what == "capture":
            self.captures.append(key)
            if self.fail:
                self.state.captured(key)
                return "failed"
            self.state.captured(key, "graph", "in", "out", stream="stream")
            rec = self.state.graphs[key]
            assert (rec.state, rec.graph, rec.static_in, rec.static_out, rec.stream, rec.uses) == ("captured", "graph", "in", "out", "stream", 1)
            return "captured"
        if what == "replay":
            assert self.state.graphs[key].state == "captured" and self.state.graphs[key].uses >= 2
            return "replayed"
        assert what == "eager"
        return "eager"


def test_graph_key_names_its_fields():
    k = _key(32)
    assert len(k) == 16 and k[0] == k.shape and k[3] == k.stream == 7 and k[8] == k.split_mode and k[15] == k.weights
    assert (k.shape, k.dtype, k.return_argmax, k.score) == ((3, 32, 64), torch.uint8, False, "rba")             # bench.py reads [0] of it: the image shape
    assert k == tuple(k) and hash(k) == hash(tuple(k)) and k != _key(32, weights=(1, 1))


def test_explicit_mode_captures_on_the_second_call_and_evicts_oldest_first():
    d = _Driver(auto=False, GRAPH_MAX=2)
    a, b, c = _key(32), _key(36), _key(40)
    assert [d.call(a) for _ in range(4)] == ["eager", "captured", "replayed", "replayed"]
    assert d.state.live() == 1 and d.captures == [a]
    assert [d.call(b) for _ in range(3)] == ["eager", "captured", "replayed"]
    assert d.call(a) == "replayed"                                                  # a is now the most recently used: b goes first
    assert [d.call(c), d.call(c)] == ["eager", "captured"]
    assert list(d.state.graphs) == [a, c] and d.state.live() == 2 and d.state.thrash == 0    # b had been replayed: its eviction is no thrash
    assert [d.call(b), d.call(b)] == ["eager", "captured"]                          # evicts a (oldest use), which had paid
    assert list(d.state.graphs) == [c, b] and d.state.thrash == 0
    assert d.call(_key(32, weights=(1, 1))) == "eager"                              # other weights: another key, from the start
    assert d.call(_key(32, stream=9)) == "eager"


def test_keys_met_once_never_evict_a_graph_and_are_bounded():
    d = _Driver(auto=False, GRAPH_MAX=2)
    a = _key(32)
    d.call(a), d.call(a)
    for h in range(100, 100 + 40):
        assert d.call(_key(h)) == "eager"
    assert d.state.live() == 1 and len(d.state.pending) == 4 * 2
    assert d.call(a) == "replayed"
    assert d.call(_key(100)) == "eager"                                             # forgotten meanwhile: met "for the first time" again
    assert d.call(_key(139)) == "captured"                                          # still remembered


def test_thrash_stops_new_captures_until_drop():
    d = _Driver(auto=False, GRAPH_MAX=2, GRAPH_THRASH_MAX=3)
    shapes = [_key(32 + 4 * i) for i in range(2 + 3)]
    for k in shapes:                                                                # every shape comes exactly twice: captured, never replayed again
        assert [d.call(k), d.call(k)] == ["eager", "captured"]
    assert d.state.thrash == 3 and d.state.live() == 2 and len(d.captures) == 5
    late = _key(200)
    assert [d.call(late) for _ in range(3)] == ["eager"] * 3 and len(d.captures) == 5        # gave up capturing new keys
    assert d.call(shapes[-1]) == "replayed"                                         # the graphs it has still replay
    d.state.drop()
    assert d.state.thrash == 0 and d.state.live() == 0
    assert [d.call(late) for _ in range(3)] == ["eager", "captured", "replayed"]


def test_a_failed_capture_is_remembered_and_counts_as_no_thrash():
    d = _Driver(auto=False, GRAPH_MAX=1)
    a, b = _key(32), _key(36)
    d.fail = True
    assert [d.call(a) for _ in range(4)] == ["eager", "failed", "eager", "eager"] and len(d.captures) == 1
    assert d.state.live() == 0 and len(d.state.graphs) == 1
    d.fail = False
    assert [d.call(b), d.call(b)] == ["eager", "captured"] and d.state.thrash == 0  # the failed entry was evicted: not a graph that did not pay
    assert [d.call(a), d.call(a)] == ["eager", "captured"] and d.state.thrash == 1  # b was: captured, never replayed again


def test_auto_mode_measures_then_decides_and_remeasures_gpu_bound_shapes():
    a = _key(32)
    dk = (a.shape, a.dtype, a.return_argmax, a.score)                                # the public key of MaskFormer.graph_decisions()
    # launch-bound: 1.0 s of host issue for 1.0 s of GPU span -> eager, measured eager, then the capture
    d = _Driver(auto=True, issue_s=1.0, span_ms=1000.0)
    before = _Event.synchronised
    assert [d.call(a) for _ in range(5)] == ["eager", "measured", "captured", "replayed", "replayed"]
    assert _Event.synchronised == before + 1                                        # the events are read once, by the call that decides
    assert d.state.decisions == {dk: {"decision": "replay", "host_issue_ms": 1000.0, "gpu_span_ms": 1000.0}}
    # GPU-bound: 0.5 s of issue for 1.0 s of span -> stays eager; GRAPH_REMEASURE_EVERY calls without the key, then measured again
    d = _Driver(auto=True, issue_s=0.5, span_ms=1000.0, GRAPH_REMEASURE_EVERY=3)
    assert [d.call(a) for _ in range(3)] == ["eager", "measured", "eager"]
    assert d.state.decisions[dk]["decision"] == "eager" and d.state.pending[a].state == "gpu_bound"
    assert [d.call(a) for _ in range(5)] == ["eager fast"] * 3 + ["measured", "eager"]
    assert [d.call(_key(32, weights=(2, 0))) for _ in range(3)] == ["eager fast"] * 3      # the fast key has no weights in it: stale costs speed only
    d.issue_s = 2.0                                                                  # the host got busier: the next measurement captures
    assert [d.call(a) for _ in range(3)] == ["measured", "captured", "replayed"]
    assert d.state.decisions[dk] == {"decision": "replay", "host_issue_ms": 2000.0, "gpu_span_ms": 1000.0}
    assert d.limits.LAUNCH_BOUND_RATIO == 0.95
    edge = _Driver(auto=True, issue_s=0.95, span_ms=1000.0)                         # exactly at the ratio: launch-bound (>=)
    assert [edge.call(a) for _ in range(3)] == ["eager", "measured", "captured"]
    # a measured call that raised left no timing: measured again
    d = _Driver(auto=True)
    assert d.call(a) == "eager" and d.state.step(a, True, d.limits) == "measure" and d.state.step(a, True, d.limits) == "measure"
    # explicit mode ignores a pending measurement
    d.state.measured(a, 0.1, _Event(), _Event(1000.0))
    assert d.state.step(a, False, d.limits) == "capture"


def test_decisions_survive_a_drop_everything_else_does_not():
    d = _Driver(auto=True, issue_s=0.5, span_ms=1000.0)
    a, b = _key(32), _key(36)
    [d.call(a) for _ in range(3)]
    d.issue_s = 1.0
    [d.call(b) for _ in range(3)]
    assert d.state.live() == 1 and d.state.eager_left and d.state.pending
    decisions = dict(d.state.decisions)
    assert sorted(v["decision"] for v in decisions.values()) == ["eager", "replay"]
    d.state.drop()
    assert d.state.decisions == decisions
    assert d.state.live() == 0 and not d.state.graphs and not d.state.pending and not d.state.eager_left and d.state.thrash == 0
    assert [d.call(b) for _ in range(3)] == ["eager", "measured", "captured"]       # from the start again
