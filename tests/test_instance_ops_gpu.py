"""GPU: K17a / K17b (rba_amd.instance_ops, csrc/instance_masks.hip) -- the per-query mask statistics and the result planes of instance inference against
their numpy restatement, operand placement, the up4 forms against the materialised planes, reproducibility, the wrappers' refusals, graph capture.

Every fixture comes from tests/_instance_cases.py, which asserts the logit margin on the CPU (tests/test_instance_cases_cpu.py builds them without a
device): `count`, `box` and the planes are compared exactly.  `ssum` is the kernel's exact sum of ITS fp32 sigmoids; no elementwise launch exposes those
sigmoids, so it is held to the fp64 sum within count * 2^32 * SIGMOID_ERR (rba_sigmoid's bound, csrc/common.h)."""
import numpy as np
import pytest
import torch

from tests import _instance_cases as C
from tests import _placement

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run rba_amd.instance_ops' allocations under the guard bands too"""
    import rba_amd.instance_ops as iops
    if canary is None:
        yield
        return
    real, iops.torch = iops.torch, canary._PROXY
    try:
        yield
    finally:
        iops.torch = real


def _check_stats(count, ssum, box, mask64, keep, where=""):
    """K17a's outputs against the restatement on `mask64` (numpy [Q,H,W])"""
    c_ref, s_ref, b_ref = C.stats_reference(mask64, keep.numpy())
    assert count.dtype == torch.int32 and ssum.dtype == torch.int64 and box.dtype == torch.int32
    c, s, b = count.cpu().numpy().astype(np.int64), ssum.cpu().numpy(), box.cpu().numpy().astype(np.int64)
    assert np.array_equal(c, c_ref), f"{where}count: {c.tolist()} != {c_ref.tolist()}"
    assert np.array_equal(b, b_ref), f"{where}box"
    err = np.abs(s.astype(np.float64) - s_ref * C.SSUM_ONE)
    bound = c_ref * C.SSUM_ONE * C.SIGMOID_ERR
    worst = (err / np.maximum(c_ref, 1) / C.SSUM_ONE).max()
    print(f"{where}ssum: worst mean sigmoid error {worst:.3g} (bound {C.SIGMOID_ERR})")
    assert np.all(err <= bound), f"{where}ssum off by {worst:.3g} per pixel"
    assert np.all(s[c_ref == 0] == 0) and np.all(s >= 0)


@pytest.mark.parametrize("mode", C.KEEP_MODES)
@pytest.mark.parametrize("H,W", C.STATS_SHAPES)
@pytest.mark.parametrize("Q", C.STATS_QUERIES)
def test_stats_equal_the_numpy_restatement(Q, H, W, mode):
    from rba_amd import instance_ops as iops
    mask, keep = C.stats_case(Q, H, W, mode)
    _check_stats(*iops.instance_stats(mask.cuda(), keep.to(torch.uint8).cuda()), mask.numpy(), keep)


def test_empty_full_nan_single_pixel_and_saturated_planes():
    from rba_amd import instance_ops as iops
    mask, keep = C.special_case()
    count, ssum, box = iops.instance_stats(mask.cuda(), keep.to(torch.uint8).cuda())
    _check_stats(count, ssum, box, mask.numpy(), keep)
    assert int(count[0]) == 0 and int(ssum[0]) == 0 and box[0].tolist() == [22, 13, -1, -1]
    assert float(iops.mask_scores(count, ssum)[0]) == 0.0 and iops.boxes_xyxy(count, box)[0].tolist() == [0, 0, 0, 0]
    assert int(count[1]) == 13 * 22 and iops.boxes_xyxy(count, box)[1].tolist() == [0, 0, 22, 13]
    assert box[3].tolist() == [21, 12, 21, 12]
    assert int(ssum[4]) == int(count[4]) * C.SSUM_ONE, "a saturated sigmoid is 1 exactly"
    for dtype in (torch.float32, torch.uint8):
        planes = iops.instance_masks(mask.cuda(), torch.arange(5, dtype=torch.int32, device="cuda"), dtype)
        assert np.array_equal(planes.cpu().numpy(), (mask.numpy() > 0).astype(planes.cpu().numpy().dtype)), "a NaN logit gives 0"


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8])
def test_masks_with_a_duplicated_and_an_out_of_range_query(dtype):
    from rba_amd import instance_ops as iops
    for Q, H, W in ((5, 7, 9), (5, 8, 12), (100, 61, 93), (5, 128, 256)):
        mask, _ = C.stats_case(Q, H, W, "all")
        qidx = torch.tensor([Q - 1, 0, Q // 2, Q - 1, Q, -1, 0], dtype=torch.int32)
        out = iops.instance_masks(mask.cuda(), qidx.cuda(), dtype)
        assert out.dtype == dtype and tuple(out.shape) == (7, H, W)
        want = np.stack([(mask[q].numpy() > 0) if 0 <= q < Q else np.zeros((H, W), bool) for q in qidx.tolist()])
        assert np.array_equal(out.cpu().numpy() != 0, want) and set(np.unique(out.cpu().numpy()).tolist()) <= {0, 1}


def test_placement_of_mask_and_out():
    """mask 4, 8 and 12 bytes off a 16-byte boundary (through the wrappers) and out 1 - 3 elements off (through the entry points, which take the output's
    address): the same results, the bytes beside the operands untouched."""
    from rba_amd import instance_ops as iops, ops
    Q, H, W = C.PLACED_SHAPE
    mask, keep = C.stats_case(Q, H, W, "all")
    m, k = mask.cuda(), keep.to(torch.uint8).cuda()
    qidx = torch.tensor([4, 0, 4, 2], dtype=torch.int32, device="cuda")
    base = iops.instance_stats(m, k)
    _check_stats(*base, mask.numpy(), keep)
    base_planes = {dt: iops.instance_masks(m, qidx, dt) for dt in (torch.float32, torch.uint8)}
    for shift in _placement.SHIFTS[torch.float32]:
        placed = _placement.place(m, shift)
        assert placed.tensor.data_ptr() % 16 == shift
        got = iops.instance_stats(placed.tensor, k)
        assert all(torch.equal(a, b) for a, b in zip(got, base)) and placed.untouched(), f"mask {shift} bytes off"
        for dt, want in base_planes.items():
            assert torch.equal(iops.instance_masks(placed.tensor, qidx, dt), want) and placed.untouched(), f"mask {shift} bytes off, {dt}"
    for dt, name in ((torch.float32, "rba_instance_masks_f32"), (torch.uint8, "rba_instance_masks_u8")):
        for elems in (1, 2, 3):
            out = _placement.place(torch.zeros((4, H, W), dtype=dt, device="cuda"), elems * base_planes[dt].element_size())
            for src in (m, _placement.place(m, 4 * elems)):
                tensor = src if torch.is_tensor(src) else src.tensor
                out.tensor.fill_(7)
                ops._launch(name, tensor.data_ptr(), qidx.data_ptr(), out.tensor.data_ptr(), Q, 4, H * W)
                assert torch.equal(out.tensor, base_planes[dt]) and out.untouched(), f"out {elems} elements off, {dt}"
                assert torch.is_tensor(src) or src.untouched()
    # the up4 forms: odd crop width (element stores) and out off its alignment
    h, w, crop = C.UP4_CASES[0]
    low, keep, _ = C.up4_case(h, w, crop)
    lo, k = low.cuda(), keep.to(torch.uint8).cuda()
    q12 = torch.tensor([0, 11, 6], dtype=torch.int32, device="cuda")
    base = iops.instance_stats_up4(lo, k, crop)
    for shift in _placement.SHIFTS[torch.float32]:
        placed = _placement.place(lo, shift)
        got = iops.instance_stats_up4(placed.tensor, k, crop)
        assert all(torch.equal(a, b) for a, b in zip(got, base)) and placed.untouched()
    for dt, name in ((torch.float32, "rba_instance_masks_up4_f32"), (torch.uint8, "rba_instance_masks_up4_u8")):
        want = iops.instance_masks_up4(lo, q12, (16, 24), dt)                      # crop_w % 4 == 0: the wide store where `out` allows it
        for elems in (1, 2, 3):
            out = _placement.place(torch.zeros((3, 16, 24), dtype=dt, device="cuda"), elems * want.element_size())
            ops._launch(name, lo.data_ptr(), q12.data_ptr(), out.tensor.data_ptr(), C.UP4_Q, 3, h, w, 16, 24)
            assert torch.equal(out.tensor, want) and out.untouched(), f"up4 out {elems} elements off, {dt}"


@pytest.mark.parametrize("h,w,crop", C.UP4_CASES)
def test_up4_forms_equal_the_full_resolution_forms_on_the_materialised_planes(h, w, crop):
    from rba_amd import instance_ops as iops, ops
    low, keep, up64 = C.up4_case(h, w, crop)
    lo, k = low.cuda(), keep.to(torch.uint8).cuda()
    full = ops.resample_bilinear(lo, (4 * h, 4 * w))[:, :crop[0], :crop[1]].contiguous()
    assert torch.equal(full.cpu().double(), up64), "the materialised planes are the dyadic values the fixture promises"
    got, want = iops.instance_stats_up4(lo, k, crop), iops.instance_stats(full, k)
    assert all(torch.equal(a, b) for a, b in zip(got, want)), "count, ssum and box bit for bit"
    _check_stats(*got, up64.numpy(), keep)
    qidx = torch.tensor([11, 0, 5, 0, C.UP4_Q], dtype=torch.int32, device="cuda")
    for dt in (torch.float32, torch.uint8):
        planes = iops.instance_masks_up4(lo, qidx, crop, dt)
        assert planes.dtype == dt and torch.equal(planes, iops.instance_masks(full, qidx, dt))
        assert np.array_equal(planes[:4].cpu().numpy() != 0, up64.numpy()[[11, 0, 5, 0]] > 0) and not bool(planes[4].any())
        kept = keep.nonzero().flatten().tolist()
        assert (iops.instance_masks_up4(lo, torch.tensor(kept, dtype=torch.int32, device="cuda"), crop, dt) != 0).flatten(1).sum(1).tolist() == \
            got[0][kept].tolist(), "the planes and the counts agree pixel by pixel"


def test_two_launches_give_the_same_bits():
    from rba_amd import instance_ops as iops
    mask, keep = C.stats_case(100, 128, 256, "all")
    m, k = (mask * 1.37).cuda(), keep.to(torch.uint8).cuda()               # off the grid: sigmoids with every mantissa bit in play
    a, b = iops.instance_stats(m, k), iops.instance_stats(m, k)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and int(a[1].min()) > 0
    low, keep, _ = C.up4_case(16, 24, (61, 93))
    lo, k = (low * 1.37).cuda(), torch.ones(C.UP4_Q, dtype=torch.uint8, device="cuda")
    a, b = iops.instance_stats_up4(lo, k, (61, 93)), iops.instance_stats_up4(lo, k, (61, 93))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


class _Reached(Exception):
    pass


def test_one_fault_is_refused_before_anything_is_allocated_or_launched(monkeypatch):
    from rba_amd import instance_ops as iops
    from rba_amd._lib import RbaHipError

    def reached(name, *args, **kw):
        raise _Reached(name)
    monkeypatch.setattr(iops, "_launch", reached)
    monkeypatch.setattr(iops.ops, "_launch", reached)                      # instance_segments' first launch is ops.softmax_drop_last's

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

    for fn, name, more in ((iops.instance_stats, "mask", {}), (iops.instance_stats_up4, "mask_lowres", {"crop": (16, 20)})):
        add = wrapper(fn, **{name: z(3, 4, 5)}, keep=ones(3), **more)
        add("Q = 0", **{name: z(0, 4, 5)}, keep=ones(0))
        add("Q = 256", **{name: z(256, 2, 2)}, keep=ones(256), **({"crop": (8, 8)} if more else {}))
        add(f"{name} of another dtype", **{name: z(3, 4, 5, dtype=torch.float64)})
        add(f"{name} not contiguous", **{name: z(3, 4, 10)[:, :, ::2]})
        add(f"{name} of rank 2", **{name: z(3, 20)})
        add(f"{name} on the CPU", **{name: torch.zeros(3, 4, 5)})
        add("keep of another dtype", keep=z(3, dtype=torch.bool))
        add("keep too short", keep=ones(2))
        add("keep too long", keep=ones(4))
        add("keep on the CPU", keep=torch.ones(3, dtype=torch.uint8))
        if more:
            add("crop higher than 4h", crop=(17, 20))
            add("crop wider than 4w", crop=(16, 21))
            add("empty crop", crop=(0, 20))
        else:
            add("H * W = 0", mask=z(3, 0, 5))
    i32 = torch.int32
    for fn, name, more in ((iops.instance_masks, "mask", {}), (iops.instance_masks_up4, "mask_lowres", {"crop": (16, 20)})):
        add = wrapper(fn, **{name: z(3, 4, 5)}, qidx=z(2, dtype=i32), **more)
        add("Q = 0", **{name: z(0, 4, 5)})
        add(f"{name} of another dtype", **{name: z(3, 4, 5, dtype=torch.float16)})
        add(f"{name} not contiguous", **{name: z(3, 4, 10)[:, :, ::2]})
        add(f"{name} of rank 4", **{name: z(1, 3, 4, 5)})
        add(f"{name} on the CPU", **{name: torch.zeros(3, 4, 5)})
        add("qidx of another dtype", qidx=z(2, dtype=torch.int64))
        add("qidx empty", qidx=z(0, dtype=i32))
        add("qidx of 65536 entries", qidx=z(65536, dtype=i32))
        add("qidx of rank 2", qidx=z(2, 1, dtype=i32))
        add("qidx on the CPU", qidx=torch.zeros(2, dtype=i32))
        add("planes of another dtype", dtype=torch.int32)
        if more:
            add("crop higher than 4h", crop=(17, 20))
            add("crop wider than 4w", crop=(16, 21))
            add("empty crop", crop=(16, 0))
        else:
            add("H * W = 0", mask=z(3, 4, 0))
    add = wrapper(iops.instance_segments, mask_cls=z(3, 5), mask=z(3, 4, 5), topk=12, num_classes=4)
    add("topk > Q * K", topk=13)
    add("topk = 0", topk=0)
    add("num_classes that is not mask_cls' width - 1", num_classes=5)
    add("mask of another query count", mask=z(2, 4, 5))
    add("mask_cls of another dtype", mask_cls=z(3, 5, dtype=torch.float64))
    add("mask_cls on the CPU", mask_cls=torch.zeros(3, 5))
    add("mask of rank 2", mask=z(3, 20))
    add("mask on the CPU", mask=torch.zeros(3, 4, 5))
    add("Q = 256", mask_cls=z(256, 5), mask=z(256, 2, 2))
    add("K = 64", mask_cls=z(3, 65), num_classes=64)
    add("a crop outside the x4 map", crop=(17, 20))
    add("no pixels", mask=z(3, 0, 5))
    add("planes of another dtype", mask_dtype=torch.float16)

    wrong = []
    for name, call, well_formed in rows:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        try:
            call()
            outcome = "returned"
        except RbaHipError as e:
            outcome = "refused"
            if "topk > Q * K" in name:
                assert "topk" in str(e)
        except _Reached as e:
            outcome = f"reached {e}"
        except Exception as e:                                           # noqa: BLE001 -- the table reports every row, whatever it ran into
            outcome = f"{type(e).__name__}: {e}"
        grew = torch.cuda.memory_allocated() - before
        if not (outcome.startswith("reached") if well_formed else (outcome == "refused" and grew == 0)):
            wrong.append(f"{name}: {outcome}, {grew} bytes allocated")
    assert len(rows) >= 60 and not wrong, "\n".join(wrong)


def test_stats_and_masks_are_capturable_in_one_graph():
    """K17a then K17b with nothing read back in between, captured once and replayed on new inputs"""
    from rba_amd import instance_ops as iops
    cases = [C.stats_case(5, 61, 93, mode) for mode in C.KEEP_MODES]
    cases[1] = (cases[1][0].flip(0).contiguous(), cases[1][1])
    cases[2] = (-cases[2][0], cases[2][1])
    tables = [torch.tensor(t, dtype=torch.int32) for t in ([0, 4, 4], [2, 0, 9], [1, 1, 3])]
    eager = []
    for (mask, keep), qidx in zip(cases, tables):
        m, k = mask.cuda(), keep.to(torch.uint8).cuda()
        eager.append(iops.instance_stats(m, k) + (iops.instance_masks(m, qidx.cuda(), torch.uint8),))
    m, k, q = cases[0][0].cuda(), cases[0][1].to(torch.uint8).cuda(), tables[0].cuda()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        count, ssum, box = iops.instance_stats(m, k)
        planes = iops.instance_masks(m, q, torch.uint8)
        score = iops.mask_scores(count, ssum)
    for i in (1, 2, 0):
        m.copy_(cases[i][0].cuda()), k.copy_(cases[i][1].to(torch.uint8).cuda()), q.copy_(tables[i].cuda())
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip((count, ssum, box, planes), eager[i])), f"replay on case {i}"
        assert torch.equal(score, iops.mask_scores(eager[i][0], eager[i][1]))
