"""The two caches of state that outlives one forward: ``ShapeCache`` (per-image-size constants) and ``derived`` (images of the weights)."""
from collections import OrderedDict

import torch


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class ShapeCache:
    """A tiny bounded cache for per-image-size constants (position embeddings, reference points, gather plans): the values depend only
    on shapes, so sharing them between calls and threads is safe; the bound keeps a long evaluation over many image sizes from growing
    the cache without limit.

    hipGraph safety: a captured graph bakes in the ADDRESSES of the constants it read, and a replay never calls ``get`` -- so to the
    cache, the entries of a captured shape look idle and would be the first to be evicted (and their memory reused under the graph's
    feet).  Every entry that is looked up while the current stream is being captured is therefore PINNED: it is never evicted and does
    not count against ``maxsize`` (the number of live graphs is bounded by their owners).  An entry that would have to be BUILT during
    a capture is returned without being inserted: its tensors live in that graph's private pool and hold garbage until the first
    replay, so no other caller may ever see them."""

    def __init__(self, maxsize=8):
        self.maxsize = maxsize
        self._d = OrderedDict()
        self._pinned = {}

    def get(self, key, build):
        cap = _capturing()
        v = self._pinned.get(key)
        if v is not None:
            return v
        d = self._d
        v = d.get(key)
        if v is None:
            v = build()
            if cap:
                return v                     # graph-private constants: rebuilt inside the graph, never shared
            d[key] = v
            while len(d) > self.maxsize:
                d.popitem(last=False)
        elif cap:
            self._pinned[key] = d.pop(key)   # a graph now holds its addresses
        else:
            d.move_to_end(key)
        return v

    def __contains__(self, key):
        return key in self._pinned or key in self._d

    def pinned(self):
        return len(self._pinned)

    def unpin(self):
        """Hand the pinned entries back to the bounded LRU part.  ONLY when every graph that read them is gone (MaskFormer.drop_graphs
        (release_constants=True), i.e. after a device move, which invalidates every captured graph of the model anyway)."""
        for k, v in self._pinned.items():
            self._d[k] = v
        self._pinned = {}
        while len(self._d) > self.maxsize:
            self._d.popitem(last=False)

    def __len__(self):
        return len(self._d) + len(self._pinned)


# ---------------------------------------------------------------------------------------------------------------- images of the weights
# The pinning rule above is wider than ShapeCache: EVERY tensor a capture reads must stay alive, unchanged, for as long as the graph can be
# replayed.  Per-shape constants and per-batch-size constants of the weights (the decoder's initial prediction heads) live in ShapeCaches for
# that reason.  The images of the weights (split planes, token planes, K7 block images, bias fragments, Linear views, folded BatchNorm) live
# in `derived` below: an image is replaced only after one of its sources changed (data pointer or version), and a source change changes
# MaskFormer's graph key, so no graph of the model replays the old image afterwards.  A graph captured OUTSIDE the model (bench.py,
# evaluate_ood.GraphedScore) keys on the image shape only: its owner must drop it after a weight change.
_STORE = "_rba_derived"


class _Store(dict):
    """{slot: (source key, value)} of one owner.  A copy or a pickle of the owner starts empty: the keys hold the ADDRESSES of the owner's
    tensors, so a copied image could never be hit -- the copy builds its own on first use."""
    __slots__ = ()

    def __deepcopy__(self, memo):
        return _Store()

    def __reduce_ex__(self, protocol):
        return _Store, ()


def source_key(*tensors, extra=()):
    """What a value derived from `tensors` depends on, hashable: data pointer and version of each (None for a missing one, e.g. no bias), the
    device of the first, then `extra`.  Moves with an in-place edit, a `p.data = ...` re-point and a replaced tensor; NOT with an in-place
    edit through `p.data`, which bypasses the version counter."""
    return tuple([None if t is None else (t.data_ptr(), t._version) for t in tensors]) + (tensors[0].device, extra)


def derived(owner, slot, sources, build, extra=()):
    """The value `build()` made for (owner, slot) from the tensors `sources`, rebuilt when what source_key(*sources, extra=extra) looks at moved.
    One entry per slot (any hashable: per-mode images are ("planes", "f16x3") and ("planes", "bf16x6"), side by side), kept in one attribute of
    the owner -- an nn.Module, a Linear view or a SimpleNamespace."""
    key = []                        # source_key's contents, flat, in a plain loop: this runs in front of every Linear and convolution launch
    for t in sources:
        if t is None:
            key.append(None)
        else:
            key.append(t.data_ptr())
            key.append(t._version)
    key.append(sources[0].device)
    key.append(extra)
    store = owner.__dict__.get(_STORE)
    if store is None:
        store = owner.__dict__[_STORE] = _Store()
    hit = store.get(slot)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = build()
    store[slot] = (key, value)
    return value


def peek(owner, slot):
    """The value cached for (owner, slot), or None: for tests and tools, never builds."""
    hit = owner.__dict__.get(_STORE, {}).get(slot)
    return None if hit is None else hit[1]
