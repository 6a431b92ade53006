"""K12a on the GPU: ops.tta_merge against the fp64 CPU restatement of the reference's multi-view merge (tests/_tta_cases.py; reference
mask2former/test_time_augmentation.py:83-97).  Bar (tests/_rba_bwd_cases.py): e = max|T - T64| / max|T64| <= 4 max(b, 2^-20), b = the fp32 CPU
restatement's own error.  Every run is preceded by NaN-poisoned allocations: no output word may depend on what it held before."""
import pytest
import torch

from tests import _tta_cases as G

pytestmark = pytest.mark.gpu


def _poison():
    for n in (1 << 10, 1 << 16, 1 << 20):
        torch.full((n,), float("nan"), device="cuda")
    torch.cuda.synchronize()


def _run(name, mode="rba", want_sem_seg=True, want_argmax=True):
    from rba_amd import ops
    K, size, spec = G.MERGE_CASES[name]
    views = [v.cuda() for v in G.merge_inputs(name)]
    _poison()
    return ops.tta_merge(views, [bool(f) for _, _, f in spec], size, want_sem_seg, want_argmax, mode)


@pytest.mark.parametrize("name", sorted(G.MERGE_CASES))
def test_kernel_against_fp64(name):
    K, size, spec = G.MERGE_CASES[name]
    t = G.merge_truth(name)
    for mode in G.MODES:
        score, sem, arg = _run(name, mode)
        assert score.shape == size and sem.shape == (K,) + size and arg.shape == size and arg.dtype == torch.int32
        if mode == "rba":
            G.check(f"{name} sem_seg", sem.cpu(), t["sem64"], t["b_sem"])
        G.check(f"{name} score ({mode})", score.cpu(), t["score64"][mode], t["b_score"][mode])
        flips = (arg.cpu().long() != t["argmax64"]) & t["decided"]
        assert not flips.any(), f"{name}: {int(flips.sum())} argmax flips where the fp64 top-two gap exceeds 8 2^-20 max|sem64|"
        assert int(arg.min()) >= 0 and int(arg.max()) < K


@pytest.mark.parametrize("K,q,hw,crop", [(7, 5, (3, 5), (11, 18)), (32, 6, (2, 4), (8, 16)), (19, 9, (4, 6), (14, 23)), (20, 9, (4, 6), (16, 24)),
                                         (19, 9, (4, 6), (16, 24))])
def test_one_unflipped_view_of_the_outputs_size_returns_k1s_bits(K, q, hw, crop, knobs):
    """One unflipped view of the output's own size: the view's sem_seg comes back bit for bit, and score and argmax are the bits ops.rba_reduce_up4
    returned beside that sem_seg, for all three score modes.  K1 here is its VALU forms (rba_k1_up4_variant = 2 on the knobs build: K = 19 / 20 rows
    that are a multiple of four wide otherwise run the matrix-pipe form, which adds the score's class terms in two halves -- another order of the
    same sum; for that form the last block checks sem_seg and argmax bits and the score to the fp32 floor)."""
    from rba_amd import _lib, ops
    gen = torch.Generator().manual_seed(77 + K)
    low = (4.0 * torch.randn(q, *hw, generator=gen)).cuda()
    prob = torch.softmax(2.0 * torch.randn(q, K + 1, generator=gen), -1)[:, :-1].contiguous().cuda()
    _lib.knob("rba_k1_up4_variant").value = 2
    try:
        for mode in G.MODES:
            score1, sem1, arg1 = ops.rba_reduce_up4(low, prob, crop, True, True, mode)
            _poison()
            score, sem, arg = ops.tta_merge([sem1], [False], crop, True, True, mode)
            assert torch.equal(sem, sem1) and torch.equal(score, score1) and torch.equal(arg, arg1), (K, mode)
    finally:
        _lib.knob("rba_k1_up4_variant").value = 0
    for mode in G.MODES:                                                 # the product's choice of K1 form
        score1, sem1, arg1 = ops.rba_reduce_up4(low, prob, crop, True, True, mode)
        score, sem, arg = ops.tta_merge([sem1], [False], crop, True, True, mode)
        assert torch.equal(sem, sem1) and torch.equal(arg, arg1), (K, mode)
        assert float((score - score1).abs().max()) <= 4 * G.FLOOR * float(score1.abs().max()), (K, mode)


@pytest.mark.parametrize("name", ["identity_flip_ragged", "k20", "wide", "one_view"])
def test_a_flipped_source_with_the_flag_equals_the_source_without(name):
    """tta_merge([x.flip(-1)], [True]) == tta_merge([x], [False]) at equal size: the flag reads column W - 1 - x of the resized map"""
    from rba_amd import ops
    x = G.merge_inputs(name)[0].cuda()
    size = tuple(x.shape[1:])
    _poison()
    a = ops.tta_merge([x.flip(-1).contiguous()], [True], size, True, True)
    b = ops.tta_merge([x], [False], size, True, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert torch.equal(b[1], x)


def test_two_runs_give_equal_bits_and_the_score_does_not_depend_on_the_optional_outputs():
    for name in sorted(G.MERGE_CASES):
        for mode in G.MODES:
            first = _run(name, mode)
            again = _run(name, mode)
            for u, v in zip(first, again):
                assert torch.equal(u, v), (name, mode)
            for want_sem, want_arg in ((False, False), (True, False), (False, True)):
                score, sem, arg = _run(name, mode, want_sem, want_arg)
                assert (sem is None) == (not want_sem) and (arg is None) == (not want_arg)
                assert torch.equal(score, first[0]), (name, mode, want_sem, want_arg)
                assert sem is None or torch.equal(sem, first[1])
                assert arg is None or torch.equal(arg, first[2])


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    z = lambda *s: torch.zeros(*s, device="cuda")
    ok = z(3, 4, 5)
    for views, flips in (([z(33, 2, 2)], [False]),                                  # K = 33
                         ([ok] * 17, [False] * 17),                                 # 17 views
                         ([ok, z(4, 4, 5)], [False, True]),                         # mismatched K
                         ([ok.cpu()], [False]),                                     # a CPU tensor
                         ([z(3, 4, 10)[..., ::2]], [False]),                        # a non-contiguous view
                         ([], []), ([ok], [False, True]), ([ok.double()], [False]), ([ok[0]], [False]), ([z(3, 0, 5)], [False])):
        with pytest.raises(RbaHipError):
            ops.tta_merge(views, flips, (4, 5))
    for size in ((0, 5), (4, 0)):
        with pytest.raises(RbaHipError):
            ops.tta_merge([ok], [False], size)
    with pytest.raises(RbaHipError):
        ops.tta_merge([ok], [False], (4, 5), score="max_logit")
    assert ops.tta_merge([ok] * 16, [False] * 16, (4, 5))[0].shape == (4, 5)          # 16 views and K = 32 are inside the contract
    assert ops.tta_merge([z(32, 2, 2)], [True], (3, 3), True)[1].shape == (32, 3, 3)
