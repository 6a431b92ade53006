"""hipGraph replay of a forward: the key of a graph, the one capture sequence, and the per-key policy of MaskFormer.rba_scores.
What a captured graph reads must outlive it: the lifetime rule is in lru.py."""
from collections import namedtuple
from types import SimpleNamespace

import torch

# everything a captured forward of MaskFormer depends on beside the pixels (MaskFormer._graph_key); `sparse_intermediate_heads` is the pair of switches the mask
# heads run by: (predictor.sparse_intermediate_heads, ops.COMPOSED_MASK_HEAD)
GraphKey = namedtuple("GraphKey", "shape dtype device stream return_argmax score fused_upsample fused_front_end split_mode split_activations tiles_min "
                                  "mlp_fused_min_rows concurrent_streams swin_attn_fused sparse_intermediate_heads weights")


def capture(fn, x, stream):
    """Capture ``fn(static_in)`` for a clone of `x` on `stream` -> (graph, static_in, static_out), or raise what the capture raised (the caller
    falls back to eager launches).  thread_local: other threads (decode threads pinning memory) may call the runtime meanwhile."""
    static_in = x.clone()
    stream.wait_stream(torch.cuda.current_stream(x.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream, capture_error_mode="thread_local"):
        static_out = fn(static_in)
    torch.cuda.current_stream(x.device).wait_stream(stream)
    return g, static_in, static_out


class GraphReplay:
    """The replay state of one model: the caller runs, measures and captures, this object decides.  Every key has ONE record with a `state`:
    "seen" (met once, ran eagerly: lazy per-shape state, weight planes), "measured" (auto mode: an eager call ran between two events, `timing`),
    "gpu_bound" (measured not to be launch-bound: eager), "captured" (`graph`, `static_in`, `static_out`, `stream`, `uses`) or "failed".
    `limits` carries GRAPH_MAX, GRAPH_THRASH_MAX, LAUNCH_BOUND_RATIO and GRAPH_REMEASURE_EVERY (the model: settable per instance)."""

    def __init__(self):
        self.graphs = {}        # key -> "captured" / "failed" records, least recently used first, at most GRAPH_MAX
        self.pending = {}       # key -> "seen" / "measured" / "gpu_bound" records, oldest first; bounded on its own, never evicts a graph
        self.eager_left = {}    # (shape, dtype, return_argmax, score, split mode, stream) -> eager calls left before a gpu_bound shape is measured again
        self.decisions = {}     # (shape, dtype, return_argmax, score) -> the last measurement (MaskFormer.graph_decisions); survives drop()
        self.thrash = 0         # graphs evicted before they were replayed a second time

    def drop(self):
        self.graphs, self.pending, self.eager_left, self.thrash = {}, {}, {}, 0

    def live(self):
        return sum(1 for rec in self.graphs.values() if rec.state == "captured")

    def step(self, key, auto, limits):
        """What this call of `key` is to be: "replay" (of self.graphs[key]), "capture" (then `captured`), "measure" (auto mode: run eagerly between two
        events, then `measured`) or "eager".  Explicit mode: eager, capture, replay ...  Auto mode: eager, measure, then the call that decides WAITS for
        the second event and reads the pair: launch-bound -> capture; else eager for GRAPH_REMEASURE_EVERY calls (served by the caller from `eager_left`,
        without building a key), then measure again (the host may get busier: decode threads, other ranks)."""
        rec = self.graphs.get(key)
        if rec is not None:
            if rec.state == "failed":
                return "eager"
            self.graphs[key] = self.graphs.pop(key)                 # most recently used last
            rec.uses += 1
            return "replay"
        if self.thrash >= limits.GRAPH_THRASH_MAX:
            return "eager"                                          # image shapes churn faster than graphs are replayed (see below)
        rec = self.pending.get(key)
        if rec is None:
            self.pending[key] = SimpleNamespace(state="seen")
            while len(self.pending) > 4 * limits.GRAPH_MAX:
                self.pending.pop(next(iter(self.pending)))
            return "eager"
        if auto:
            if rec.state != "measured":                             # seen, or gpu_bound with its eager calls used up
                return "measure"
            # LAUNCH-BOUND: the Python thread needed at least LAUNCH_BOUND_RATIO of the GPU's own span to issue the forward (a launch-bound GPU span
            # stretches to the issue time, so the ratio saturates near 1) -- then, and only then, the shape is captured
            t_issue, e0, e1 = rec.timing
            e1.synchronize()
            t_gpu = e0.elapsed_time(e1) * 1e-3
            bound = t_issue >= limits.LAUNCH_BOUND_RATIO * t_gpu
            self.decisions[key.shape, key.dtype, key.return_argmax, key.score] = {
                "decision": "replay" if bound else "eager", "host_issue_ms": t_issue * 1e3, "gpu_span_ms": t_gpu * 1e3}
            if not bound:
                rec.state = "gpu_bound"
                while len(self.eager_left) > 4 * limits.GRAPH_MAX:
                    self.eager_left.pop(next(iter(self.eager_left)))
                self.eager_left[key.shape, key.dtype, key.return_argmax, key.score, key.split_mode, key.stream] = limits.GRAPH_REMEASURE_EVERY
                return "eager"
        del self.pending[key]
        while len(self.graphs) >= limits.GRAPH_MAX:                 # oldest first; a graph owns its pool, dropping it frees the memory
            old = self.graphs.pop(next(iter(self.graphs)))          # (on ROCm destroying a graph synchronises the device)
            if old.state == "captured" and old.uses <= 1:           # 1 = only the replay that followed its capture
                # a graph that never paid is being evicted: with more live shapes than GRAPH_MAX every capture costs more than it saves; after
                # GRAPH_THRASH_MAX of these the model stops capturing new keys (drop() resets)
                self.thrash += 1
        return "capture"

    def measured(self, key, seconds, e0, e1):
        """the eager call step() answered "measure" for took the host `seconds` to issue, between the events e0 and e1 on its stream"""
        rec = self.pending.get(key)
        if rec is not None:
            rec.state, rec.timing = "measured", (seconds, e0, e1)

    def captured(self, key, graph=None, static_in=None, static_out=None, stream=None):
        """what capture() returned for the key step() answered "capture" for, and the stream to keep with it; no graph = the capture failed, which is
        remembered: the key stays eager.  The first replay follows at once: uses = 1."""
        self.graphs[key] = SimpleNamespace(state="failed" if graph is None else "captured", graph=graph, static_in=static_in, static_out=static_out,
                                           stream=stream, uses=1)
