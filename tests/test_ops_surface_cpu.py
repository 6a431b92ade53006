"""CPU: every launch wrapper of rba_amd.ops has its rows.

A wrapper is a function of rba_amd.ops that `_hip_op` wrapped (functools.wraps leaves `__wrapped__`).  Each must be named in one of the refusal tables of
tests/test_ops_refusals_gpu.py AND in the placement table of tests/test_operand_placement_gpu.py, or be exempt with a reason (pure-host helpers only).  The lists live in tests/_ops_surface.py, which imports without a
device; the GPU tests check that their tables hold exactly the listed names, this test checks the lists against the module -- so a new wrapper fails here
until it has rows."""
import inspect
import os
import re

from tests import _ops_surface as S


def _wrappers():
    from rba_amd import ops
    return sorted(n for n, f in vars(ops).items() if inspect.isfunction(f) and hasattr(f, "__wrapped__") and f.__module__ == ops.__name__)


def test_every_wrapper_has_refusal_rows_or_a_reason():
    names = _wrappers()
    assert len(names) > 60, names                                        # the walk itself: it finds the surface
    listed = S.REFUSAL_ROWS_FIRST_TABLE + S.REFUSAL_ROWS_SECOND_TABLE
    assert len(set(listed)) == len(listed), sorted(n for n in set(listed) if listed.count(n) > 1)
    missing = [n for n in names if n not in listed and n not in S.EXEMPT]
    assert not missing, f"wrappers without refusal rows (tests/test_ops_refusals_gpu.py, tests/_ops_surface.py): {missing}"
    stale = [n for n in listed + list(S.EXEMPT) if n not in names]
    assert not stale, f"listed, but no wrapper of rba_amd.ops: {stale}"
    assert not set(listed) & set(S.EXEMPT)
    # ... and a case in the placement table (tests/test_operand_placement_gpu.py checks that its cases are exactly these names)
    assert len(set(S.PLACEMENT_ROWS)) == len(S.PLACEMENT_ROWS)
    unplaced = [n for n in names if n not in S.PLACEMENT_ROWS and n not in S.EXEMPT]
    assert not unplaced, f"wrappers without a placement case (tests/test_operand_placement_gpu.py, docs/kernels/placement.md, tests/_ops_surface.py): {unplaced}"
    assert not [n for n in S.PLACEMENT_ROWS if n not in names] and not set(S.PLACEMENT_ROWS) & set(S.EXEMPT)
    assert all(isinstance(r, str) and len(r) > 20 for r in S.EXEMPT.values())


def test_exempt_names_reach_no_entry_point():
    """an exemption is for a pure-host helper: its source names neither the launch line nor a library query"""
    from rba_amd import ops
    for name in S.EXEMPT:
        src = inspect.getsource(getattr(ops, name))
        assert "_launch(" not in src and "_query(" not in src, name


def test_the_first_table_holds_the_names_listed_for_it():
    """the first table predates the lists: its source is read instead (the second one reports its own names to its GPU test)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_ops_refusals_gpu.py")) as f:
        src = f.read()
    first = src[src.index("def _table(ops)"):src.index("def test_one_fault_is_refused_before_anything_is_allocated_or_launched")]
    named = set(re.findall(r"ops\.([a-z_0-9]+)", first))
    assert sorted(S.REFUSAL_ROWS_FIRST_TABLE) == sorted(n for n in named if n in _wrappers())


def test_the_placement_seeds_leave_out_at_most_one_percent_of_the_argmax_pixels():
    """the argmax maps of tests/test_operand_placement_gpu.py are compared where the fp64 reference's top-two gap exceeds the sem_seg bar: the seeds are
    chosen so that the reference alone leaves out at most 1 % of the pixels"""
    from oracle import ref_ops
    from tests import _placement as P
    from tests import _tta_cases as G
    for name in P.K1_CASES:
        mp, prob = P.k1_inputs(name)
        sem64, _, _ = ref_ops.rba_reduce_ordered(mp.double(), prob.double())
        _, left_out = P.decided_pixels(sem64, P.K1_SEM_SEG_BAR)
        print(f"{name}: {100 * left_out:.2f} % of the pixels left out")
        assert left_out <= P.ARGMAX_LEFT_OUT_CAP, name
    low, prob = P.up4_inputs()
    up = ref_ops.upsample_bilinear(low.double()[None], (4 * low.shape[1], 4 * low.shape[2]))[0]
    sem64, _, _ = ref_ops.rba_reduce_ordered(up, prob.double())
    assert P.decided_pixels(sem64, P.UP4_SEM_SEG_BAR)[1] <= P.ARGMAX_LEFT_OUT_CAP, "rba_reduce_up4"
    assert 1.0 - G.merge_truth("wide")["decided"].double().mean().item() <= P.ARGMAX_LEFT_OUT_CAP
