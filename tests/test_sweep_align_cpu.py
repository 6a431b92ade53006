"""CPU: the aligner of the shape sweep (tests/_sweep_align.py) on the oracle alone.  The float64 oracle plays the product: its logits (rounded to fp32, as a
product hands them to K3) decide `sigmoid < 0.5` the way torch's fp32 sigmoid decides, and the fp32 oracle is aligned to those decisions."""
import pytest
import torch

from rba_amd import arch as A
from tests import _sweep_align as SA
from tests.test_shape_sweep_gpu import _check, _image

_CASES = {}


def _case(name, h, w):
    """-> (run32, run64, P, want, outputs of the stand-in): shared by the tests below and left unchanged"""
    if (name, h, w) not in _CASES:
        a = A.complete(A.ARCHS[name])
        run32, run64 = SA.oracle_runs(_image(h, w), A.seeded_weights(a, 0), a)
        # the stand-in takes its decisions from its own fp32-rounded logits; call c's logits are fixed once the decisions of the calls before it are
        want = [SA.blocked(l.float()) for l in run64({})[0]]
        for _ in range(a["dec_layers"] + 1):
            _, (logits, out) = SA.align(run64, want)
            again = [SA.blocked(l.float()) for l in logits]
            if all(torch.equal(x, y) for x, y in zip(again, want)):
                break
            want = again
        else:
            raise AssertionError("the stand-in's decisions did not settle")
        _CASES[name, h, w] = (run32, run64, [l.float() for l in logits], want, out)
    return _CASES[name, h, w]


@pytest.mark.parametrize("name,h,w", [("tiny3", 2000, 48), ("tiny3", 375, 1242), ("tiny3", 333, 777), ("tiny1", 190, 650)])
def test_aligner_converges_on_a_float64_stand_in(name, h, w):
    """sizes at which the fp32 oracle has entries within 2e-5 of zero (2000 x 48: one at 1.5e-7): <= 12 inverted decisions, at most one oracle re-run per head call,
    the aligned fp32 oracle reproduces the stand-in's outputs within 1e-4 and its logits within the sweep's own bound"""
    run32, run64, P, want, out = _case(name, h, w)
    before = len(run32.cache)
    toggles, (R32, ref) = SA.align(run32, want)
    assert SA.n_toggles(toggles) <= SA.MAX_TOGGLES
    if (name, h, w) == ("tiny3", 2000, 48):                  # the fp32 oracle's entry at |logit| 1.5e-7 is on the other side in float64: the test must invert something
        assert SA.n_toggles(toggles) >= 1
    assert len(run32.cache) - before <= len(want) + 1
    _, (R64, _) = SA.align(run64, want)
    bad, stats = SA.logit_parity(P, R32, R64, toggles, "bf16x6")
    print(f"[align] {name} {h}x{w}: {SA.n_toggles(toggles)} inverted decisions, max|P - R32| / own = {stats['ratio']:.3f}, own {stats['own']:.2e}, "
          f"{stats['near_zero']} entries within 3 own of zero")
    assert not bad, bad
    ok, nums = _check({k: (v.float() if v.is_floating_point() else v) for k, v in out.items()}, ref, h, w, "")
    assert ok, nums


def test_aligner_rejects_a_decision_flipped_away_from_zero():
    """negative control: a stand-in whose logit at one entry with |logit| > 1e-3 (the nearest such to zero) has the other sign, hence the other decision.  The aligner
    follows it -- it aligns to whatever it is told -- and the logit-parity condition rejects the run, as does the band of the search it replaces."""
    run32, run64, P, want, _ = _case("tiny1", 190, 650)
    mag = P[0].abs().reshape(-1)
    j = int(torch.where(mag > 1e-3, mag, torch.full_like(mag, float("inf"))).argmin())
    P2 = [p.clone() for p in P]
    P2[0].view(-1)[j] = -P2[0].view(-1)[j]
    want2 = [SA.blocked(p) for p in P2]
    assert int((want2[0] != want[0]).sum()) == 1
    toggles, (R32, _) = SA.align(run32, want2)
    assert j in toggles[0].tolist()
    _, (R64, _) = SA.align(run64, want2)
    bad, stats = SA.logit_parity(P2, R32, R64, toggles, "f16x3")                # the laxer of the two k
    assert any("|P - R32|" in b for b in bad) and any("band" in b for b in bad), bad
    assert stats["max_diff"] > 2e-3 > SA.K_PARITY["f16x3"] * stats["own"]


def test_aligner_leaves_a_case_without_near_zero_entries_alone():
    """no entry near zero: no inverted decision, and the oracle is not run a second time"""
    run32, run64, P, want, _ = _case("tiny1", 60, 90)
    assert min(float(p.abs().min()) for p in P) > 1e-4
    calls = []

    def counted(toggles):
        calls.append(dict(toggles))
        return run32(toggles)

    toggles, (R32, _) = SA.align(counted, want)
    assert toggles == {} and calls == [{}]
    bad, stats = SA.logit_parity(P, R32, [l for l in run64({})[0]], toggles, "bf16x6")
    assert not bad and stats["max_diff"] <= stats["own"] + max(float(p.abs().max()) for p in P) * 2.0 ** -24    # P is R64 rounded to fp32


def test_aligner_stops_at_the_cap_without_running_further():
    run32, _, P, want, _ = _case("tiny1", 60, 90)
    want2 = [w.clone() for w in want]
    want2[0].view(-1)[: SA.MAX_TOGGLES + 1] ^= True
    calls = []

    def counted(toggles):
        calls.append(dict(toggles))
        return run32(toggles)

    with pytest.raises(SA.AlignmentError, match="cap"):
        SA.align(counted, want2)
    assert calls == [{}]
