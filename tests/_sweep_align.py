"""Test infrastructure of the shape sweep: align the oracle's `sigmoid(logit) < 0.5` decisions to the product's, deterministically.

The reference's decoder thresholds its interpolated mask logits (mask2former_transformer_decoder.py:483-487).  A logit within rounding noise of zero may fall on
either side in two correct implementations, and the masked attention downstream then differs by far more than any parity bound: the reference's own discontinuity.
Instead of searching for an inversion that explains a failing output, every run is treated alike:

* `tap_attn_logits` records the attention-mask logits P_c the product hands to K3 (K3 thresholds them itself; tests/test_kernels_gpu.py pins that it decides exactly
  like torch's fp32 `sigmoid(x) < 0.5`, so the product's decisions are `blocked(P_c)`);
* `align` walks the oracle's head calls in order and inverts exactly the decisions that differ from the product's (`ref_model.forward(toggles=...)`): at most one
  oracle re-run per head call, no search;
* `logit_parity` then holds the product's logits to the ALIGNED oracle's at every entry: |P - R32| <= k * own, own = max |R32 - R64| of the fp32 and the float64
  oracle aligned to the same decisions -- the reference's own distance from exact arithmetic at this case, free of threshold cascades.  A decision that had to be
  inverted is therefore at a logit within k * own of zero on both sides, and nothing else can be inverted without failing.
"""
import contextlib

import torch

MAX_TOGGLES = 12          # inverted decisions per run (the cap of the search this replaces; the reference alone has <= 4 entries within 2e-5 of zero at any default size)
K_PARITY = {"bf16x6": 3.0, "f16x3": 5.0}
# bf16x6 is fp32-class arithmetic: |P - truth| <~ own, so |P - R32| <= 2 own; x 1.5 because `own` is a maximum over a finite sample (the factor the sweep's output
# bound already grants: tol = max(1e-4, 3 own)).  f16x3 operands carry 22 bits and the op-level tests allow it twice the fp32 GEMM's error: |P - R32| <= 3 own,
# x 1.5, rounded up.  Derived, not measured.
OLD_BAND = 2e-5           # the band of the search this replaces: no inverted decision may lie outside it (scaled with the output tolerance as before)


class AlignmentError(AssertionError):
    pass


def blocked(logits):
    """the threshold decision exactly as the oracle takes it (in the logits' own dtype).  In fp32 that is x <= -1.7881392e-07 (bits 0xb43fffff): false for
    0xb43ffffe and everything above, -2^-23, -0.0, denormals and NaN included; tests/test_kernels_gpu.py re-derives both bit patterns from torch by bisection."""
    return logits.sigmoid() < 0.5


@contextlib.contextmanager
def tap_attn_logits(decoder):
    """Wrap the bound `forward_prediction_heads` of this decoder INSTANCE; yields the list that receives the third return -- attention-mask logits [B, Q, h*w] --
    of every call that has one (the last head call of a forward has none: its mask is never used).  Inside the block the list holds the product's own device
    tensors (each a fresh allocation that nothing writes again): no copy, no synchronisation, the forward runs as free as an untapped one.  They are copied to the
    CPU when the block ends."""
    got = []
    inner = decoder.forward_prediction_heads

    def tapped(*args, **kwargs):
        ret = inner(*args, **kwargs)
        if ret[2] is not None:
            got.append(ret[2].detach())
        return ret

    decoder.__dict__["forward_prediction_heads"] = tapped
    try:
        yield got
    finally:
        del decoder.__dict__["forward_prediction_heads"]
        got[:] = [t.float().cpu() for t in got]


def toggle_key(toggles):
    return tuple(sorted((int(c), tuple(int(j) for j in idx.tolist())) for c, idx in toggles.items() if len(idx)))


def memoised(run):
    """`run(toggles)` cached per toggle set: the configurations of one case mostly ask for the same alignments"""
    cache = {}

    def cached(toggles):
        key = toggle_key(toggles)
        if key not in cache:
            cache[key] = run(toggles)
        return cache[key]

    cached.cache = cache
    return cached


def align(run, want_blocked, cap=MAX_TOGGLES):
    """run(toggles) -> (per-head-call logits of the oracle under `toggles` {call: flat indices}, anything else the caller wants back).
    want_blocked: one bool tensor per head call whose mask is used.  Head calls in order: the oracle's natural decision at call c (under the toggles of the calls
    before it) is compared with want_blocked[c]; the entries that differ become toggles[c]; the oracle is re-run only if there are any.
    -> (toggles, result of the final run).  More than `cap` inverted entries: AlignmentError at once, without running further."""
    toggles = {}
    result = run(toggles)
    for c, want in enumerate(want_blocked):
        logits = result[0][c]
        if logits.shape != want.shape:
            raise AlignmentError(f"head call {c}: oracle logits {tuple(logits.shape)}, product decisions {tuple(want.shape)}")
        differ = (blocked(logits) != want).reshape(-1).nonzero().flatten()
        if len(differ):
            n = len(differ) + sum(len(v) for v in toggles.values())
            if n > cap:
                raise AlignmentError(f"head call {c}: {n} threshold decisions differ from the product's so far (cap {cap}); "
                                     f"|oracle logit| there up to {float(logits.reshape(-1)[differ].abs().max()):.3e}")
            toggles[c] = differ
            result = run(toggles)
    for c, want in enumerate(want_blocked):                  # what was decided upstream of a toggle does not move: a re-run only changes later calls
        dec = blocked(result[0][c]).reshape(-1).clone()
        if c in toggles:
            dec[toggles[c]] ^= True
        if not torch.equal(dec, want.reshape(-1)):
            raise AlignmentError(f"head call {c}: the aligned oracle does not reproduce the wanted decisions")
    return toggles, result


def n_toggles(toggles):
    return sum(len(v) for v in toggles.values())


def logit_parity(P, R32, R64, toggles, mode, band=OLD_BAND):
    """The conditions on the logits of one run.  P / R32 / R64: per used head call, the product's, the aligned fp32 oracle's and the aligned float64 oracle's
    logits.  -> (list of failure strings, dict(own, max_diff, ratio, near_zero)); near_zero counts the aligned fp32 oracle's entries within k * own of zero."""
    k = K_PARITY[mode]
    own = max(float((r32.double() - r64.double()).abs().max()) for r32, r64 in zip(R32, R64))
    bad, max_diff, near = [], 0.0, 0
    for c, (p, r32) in enumerate(zip(P, R32)):
        d = (p.double() - r32.double()).abs()
        max_diff = max(max_diff, float(d.max()))
        near += int((r32.abs() <= k * own).sum())
        if not bool((d <= k * own).all()):                   # NaN compares False
            j = int(torch.nan_to_num(d, nan=float("inf")).reshape(-1).argmax())
            bad.append(f"head call {c}: |P - R32| = {float(d.reshape(-1)[j]):.3e} at entry {j} (oracle logit {float(r32.reshape(-1)[j]):.3e}) > {k:g} x own = {k * own:.3e}")
        if c in toggles:
            far = r32.reshape(-1)[toggles[c]].abs()
            if not bool((far < band).all()):
                bad.append(f"head call {c}: inverted decision at |oracle logit| {float(far.max()):.3e}, outside the {band:.1e} band")
    return bad, dict(own=own, max_diff=max_diff, ratio=max_diff / own if own > 0 else float("inf" if max_diff > 0 else 0), near_zero=near)


def oracle_runs(image, sd, a):
    """-> (run32, run64): memoised `run(toggles)` of the fp32 oracle and of the same oracle in float64 on the same weights (how far the reference's own fp32
    forward is from exact arithmetic at this size).  Each returns (logits of the head calls whose mask is used, the oracle's output dict)."""
    from oracle import ref_model

    def run32(toggles):
        taps = {}
        out = ref_model.forward(image, sd, a, taps=taps, toggles=toggles)
        return taps["am_logits"][:-1], out

    sd64 = {}

    def run64(toggles):
        if not sd64:
            sd64.update({k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()})
        taps = {}
        torch.set_default_dtype(torch.float64)
        try:
            out = ref_model.forward(image.double(), sd64, a, taps=taps, toggles=toggles)
        finally:
            torch.set_default_dtype(torch.float32)
        return taps["am_logits"][:-1], out

    return memoised(run32), memoised(run64)
