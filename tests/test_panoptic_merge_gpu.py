"""GPU: K16a / K16b (rba_amd.panoptic_ops, csrc/panoptic_merge.hip) -- the closed-set panoptic merge against its numpy restatement, operand placement,
the wrappers' refusals, the up4 form against the materialised planes, the id gather, graph capture.

Every parity fixture comes from tests/_panoptic_cases.py, which asserts the two decision margins in fp64 on the CPU before anything is launched (the
fixtures are also built by tests/test_panoptic_evaluation_cpu.py without a device): with the margins held, `winner` and `counts` are compared exactly."""
import numpy as np
import pytest
import torch

from tests import _panoptic_cases as C
from tests import _placement

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run this module's allocations under the guard bands too"""
    import rba_amd.panoptic_ops as pops
    if canary is None:
        yield
        return
    real, pops.torch = pops.torch, canary._PROXY
    try:
        yield
    finally:
        pops.torch = real


def _dev(mask, score, keep):
    return mask.cuda(), score.cuda(), keep.to(torch.uint8).cuda()


def _check(winner, counts, mask, score, keep):
    w_ref, c_ref = C.merge_reference(mask.numpy(), score.numpy(), keep.numpy())
    assert winner.dtype == torch.uint8 and counts.dtype == torch.int32
    assert np.array_equal(winner.cpu().numpy(), w_ref), f"{int((winner.cpu().numpy() != w_ref).sum())} winners differ"
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), c_ref)


@pytest.mark.parametrize("mode", C.KEEP_MODES)
@pytest.mark.parametrize("Q,H,W", C.MERGE_SHAPES)
def test_merge_equals_the_numpy_restatement(Q, H, W, mode):
    from rba_amd import panoptic_ops as pops
    mask, score, keep = C.merge_case(Q, H, W, mode)
    _check(*pops.panoptic_merge(*_dev(mask, score, keep)), mask, score, keep)


def test_a_winner_that_is_nowhere_solid_and_a_tie_between_equal_queries():
    from rba_amd import panoptic_ops as pops
    mask, score, keep = C.never_solid_case()
    winner, counts = pops.panoptic_merge(*_dev(mask, score, keep))
    _check(winner, counts, mask, score, keep)
    assert bool((winner == pops.NOBODY).all()) and counts[:, 2].tolist() == [99, 0, 0]
    mask, score, keep = C.tie_case()
    winner, counts = pops.panoptic_merge(*_dev(mask, score, keep))
    _check(winner, counts, mask, score, keep)
    assert int(counts[0, 1]) > 0 and int(counts[0, 3]) == 0, "of two queries with equal score and equal logits the lower q wins"


def test_placement_of_mask_and_winner():
    """mask 4, 8 and 12 bytes off a 16-byte boundary (through the wrapper) and winner 1 - 3 bytes off (through the entry point, which takes the
    output's address): the same results, the bytes beside the operands untouched."""
    from rba_amd import ops, panoptic_ops as pops
    mask, score, keep = C.merge_case(*C.PLACED_SHAPE, "alternating")
    Q, H, W = C.PLACED_SHAPE
    m, s, k = _dev(mask, score, keep)
    base_w, base_c = pops.panoptic_merge(m, s, k)
    _check(base_w, base_c, mask, score, keep)
    for shift in _placement.SHIFTS[torch.float32]:
        placed = _placement.place(m, shift)
        assert placed.tensor.data_ptr() % 16 == shift
        winner, counts = pops.panoptic_merge(placed.tensor, s, k)
        assert torch.equal(winner, base_w) and torch.equal(counts, base_c) and placed.untouched(), f"mask {shift} bytes off"
    for shift in (1, 2, 3):
        out = _placement.place(torch.zeros((H, W), dtype=torch.uint8, device="cuda"), shift)
        counts = torch.zeros((3, Q), dtype=torch.int32, device="cuda")
        ops._launch("rba_panoptic_merge_f32", m.data_ptr(), s.data_ptr(), k.data_ptr(), out.tensor.data_ptr(), counts.data_ptr(), Q, H * W)
        assert torch.equal(out.tensor, base_w) and torch.equal(counts, base_c) and out.untouched(), f"winner {shift} bytes off"
        # both off at once, and the up4 form's winner
        placed = _placement.place(m, 4 * shift)
        counts.zero_()
        ops._launch("rba_panoptic_merge_f32", placed.tensor.data_ptr(), s.data_ptr(), k.data_ptr(), out.tensor.data_ptr(), counts.data_ptr(), Q, H * W)
        assert torch.equal(out.tensor, base_w) and torch.equal(counts, base_c) and out.untouched() and placed.untouched()
    h, w, crop = C.UP4_CASES[2]
    low, score, keep = C.up4_case(h, w, crop)
    lo, s, k = _dev(low, score, keep)
    base_w, base_c = pops.panoptic_merge_up4(lo, s, k, crop)
    for shift in (1, 2, 3):
        out = _placement.place(torch.zeros(crop, dtype=torch.uint8, device="cuda"), shift)
        placed = _placement.place(lo, 4 * shift)
        counts = torch.zeros((3, C.UP4_Q), dtype=torch.int32, device="cuda")
        ops._launch("rba_panoptic_merge_up4_f32", placed.tensor.data_ptr(), s.data_ptr(), k.data_ptr(), out.tensor.data_ptr(), counts.data_ptr(), C.UP4_Q,
                    h, w, crop[0], crop[1])
        assert torch.equal(out.tensor, base_w) and torch.equal(counts, base_c) and out.untouched() and placed.untouched()


class _Reached(Exception):
    pass


def test_one_fault_is_refused_before_anything_is_allocated_or_launched(monkeypatch):
    from rba_amd import panoptic_ops as pops
    from rba_amd._lib import RbaHipError

    def reached(name, *args, **kw):
        raise _Reached(name)
    monkeypatch.setattr(pops, "_launch", reached)

    def z(*shape, dtype=torch.float32):
        return torch.zeros(*shape, dtype=dtype, device="cuda")

    def ones(n):
        return torch.ones(n, dtype=torch.uint8, device="cuda")
    rows = []

    def wrapper(fn, **good):
        rows.append((f"{fn.__name__}: well-formed", lambda: fn(**good), True))

        def add(clause, **bad):
            rows.append((f"{fn.__name__}: {clause}", lambda: fn(**{**good, **bad}), False))
        return add

    for fn, name, more in ((pops.panoptic_merge, "mask", {}), (pops.panoptic_merge_up4, "mask_lowres", {"crop": (16, 20)})):
        add = wrapper(fn, **{name: z(3, 4, 5)}, score=z(3), keep=ones(3), **more)
        add("Q = 0", **{name: z(0, 4, 5)}, score=z(0), keep=ones(0))
        add("Q = 256", **{name: z(256, 2, 2)}, score=z(256), keep=ones(256), **({"crop": (8, 8)} if more else {}))
        add(f"{name} of another dtype", **{name: z(3, 4, 5, dtype=torch.float64)})
        add(f"{name} not contiguous", **{name: z(3, 4, 10)[:, :, ::2]})
        add(f"{name} of rank 2", **{name: z(3, 20)})
        add(f"{name} on the CPU", **{name: torch.zeros(3, 4, 5)})
        add("score of another dtype", score=z(3, dtype=torch.float64))
        add("score too short", score=z(2))
        add("score too long", score=z(4))
        add("score on the CPU", score=torch.zeros(3))
        add("keep of another dtype", keep=z(3, dtype=torch.bool))
        add("keep too short", keep=ones(2))
        add("keep too long", keep=ones(4))
        add("keep on the CPU", keep=torch.ones(3, dtype=torch.uint8))
        add("no kept query", keep=z(3, dtype=torch.uint8))
        add("no kept query, as the caller counted", kept=0)
        if more:
            add("crop higher than 4h", crop=(17, 20))
            add("crop wider than 4w", crop=(16, 21))
            add("empty crop", crop=(0, 20))
        else:
            add("H * W = 0", mask=z(3, 0, 5))
    add = wrapper(pops.panoptic_assign, winner=z(4, 5, dtype=torch.uint8), seg_of_query=z(3, dtype=torch.int32))
    add("winner of another dtype", winner=z(4, 5, dtype=torch.int32))
    add("winner on the CPU", winner=torch.zeros(4, 5, dtype=torch.uint8))
    add("no pixels", winner=z(0, 5, dtype=torch.uint8))
    add("seg_of_query of another dtype", seg_of_query=z(3, dtype=torch.int64))
    add("seg_of_query of 256 entries", seg_of_query=z(256, dtype=torch.int32))
    add("seg_of_query empty", seg_of_query=z(0, dtype=torch.int32))
    add("seg_of_query on the CPU", seg_of_query=torch.zeros(3, dtype=torch.int32))
    i32, i64 = torch.int32, torch.int64
    add = wrapper(pops.segment_pairs, gt=z(4, 5, dtype=i32), pred=z(4, 5, dtype=i32), G=3, P=4, counts=z(3, 4, dtype=i64), bad=z(1, dtype=i64))
    add("G * P > 2^24", G=4097, P=4096)
    add("G = 0", G=0)
    add("gt and pred of different shapes", pred=z(5, 4, dtype=i32))
    add("gt of another dtype", gt=z(4, 5, dtype=i64))
    add("pred of another dtype", pred=z(4, 5, dtype=i64))
    add("pred on the CPU", pred=torch.zeros(4, 5, dtype=i32))
    add("empty maps", gt=z(0, 5, dtype=i32), pred=z(0, 5, dtype=i32))
    add("counts of the wrong size", counts=z(4, 3, dtype=i64))
    add("counts of another dtype", counts=z(3, 4, dtype=i32))
    add("bad of two elements", bad=z(2, dtype=i64))
    add("bad on the CPU", bad=torch.zeros(1, dtype=i64))

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
    assert len(rows) >= 50 and not wrong, "\n".join(wrong)


@pytest.mark.parametrize("h,w,crop", C.UP4_CASES)
def test_up4_equals_the_merge_of_the_materialised_planes(h, w, crop):
    from rba_amd import ops, panoptic_ops as pops
    low, score, keep = C.up4_case(h, w, crop)
    lo, s, k = _dev(low, score, keep)
    winner, counts = pops.panoptic_merge_up4(lo, s, k, crop)
    full = ops.resample_bilinear(lo, (4 * h, 4 * w))[:, :crop[0], :crop[1]].contiguous()
    w_full, c_full = pops.panoptic_merge(full, s, k)
    assert torch.equal(winner, w_full) and torch.equal(counts, c_full)
    _check(winner, counts, C.upsample4_fp64(low)[:, :crop[0], :crop[1]], score, keep)       # and both equal the fp64 restatement
    assert int(counts[0].sum()) == crop[0] * crop[1]


def test_assign_equals_numpy_indexing():
    from rba_amd import panoptic_ops as pops
    g = torch.Generator().manual_seed(3)
    for Q, shape in ((1, (1, 1)), (9, (37, 53)), (255, (64, 100))):
        winner = torch.randint(0, Q, shape, generator=g, dtype=torch.uint8)
        winner[torch.rand(shape, generator=g) < 0.3] = pops.NOBODY
        table = torch.randint(0, 6, (Q,), generator=g, dtype=torch.int32)              # entries of 0: dropped queries
        table[Q // 2] = 0
        out = pops.panoptic_assign(winner.cuda(), table.cuda())
        w = winner.numpy()
        ref = np.where(w == pops.NOBODY, 0, table.numpy()[np.minimum(w, Q - 1)]).astype(np.int32)
        assert out.dtype == torch.int32 and np.array_equal(out.cpu().numpy(), ref)


def test_merge_and_assign_are_capturable_in_one_graph():
    """K16a then K16b with the table given and no read-back in between, captured once and replayed twice on new inputs"""
    from rba_amd import panoptic_ops as pops
    cases = [C.merge_case(16, 37, 53, "alternating"), C.merge_case(16, 37, 53, "all"), C.merge_case(16, 37, 53, "one")]
    g = torch.Generator().manual_seed(8)
    tables = [torch.randint(0, 9, (16,), generator=g, dtype=torch.int32) for _ in cases]
    eager = []
    for (mask, score, keep), table in zip(cases, tables):
        winner, counts = pops.panoptic_merge(*_dev(mask, score, keep))
        eager.append((winner, counts, pops.panoptic_assign(winner, table.cuda())))
    m, s, k = _dev(*cases[0])
    t = tables[0].cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        winner, counts = pops.panoptic_merge(m, s, k, kept=1)             # the kept count is the caller's under capture: reading it is a read-back
        pan = pops.panoptic_assign(winner, t)
    for i in (1, 2, 0):
        mask, score, keep = _dev(*cases[i])
        m.copy_(mask), s.copy_(score), k.copy_(keep), t.copy_(tables[i].cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(winner, eager[i][0]) and torch.equal(counts, eager[i][1]) and torch.equal(pan, eager[i][2]), f"replay on case {i}"
