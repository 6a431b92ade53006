"""Host logic of the composed mask head (docs/kernels/K4.md): the shape half of the selection rule on the released shapes, the bindings."""
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gathered_rows(H, W, strides=(32, 16, 8)):
    """(map rows P, [4 h w per level]) of an image padded to a multiple of 32: the map is 1/4 resolution, the attention masks live at 1/32, 1/16, 1/8"""
    Hp, Wp = -(-H // 32) * 32, -(-W // 32) * 32
    return (Hp // 4) * (Wp // 4), [4 * (Hp // s) * (Wp // s) for s in strides]


def test_selection_rule_on_the_released_shapes():
    from rba_amd import ops
    # C2 / Swin-L: 1024 x 2048, one decoder layer, one level (res5): 8 192 gathered rows of 131 072
    P, rows = _gathered_rows(1024, 2048)
    assert (P, rows) == (131072, [8192, 32768, 131072])
    assert ops.composed_mask_head_pays(P, rows[0])
    # C5: nine layers over three levels at 720 x 1280 (padded 736 x 1280): the three levels' rows exceed the whole map
    P, rows = _gathered_rows(720, 1280)
    assert sum(rows) > P and not ops.composed_mask_head_pays(P, sum(rows))
    # two levels (1/32 + 1/16) of a 1024 x 2048 image would still pay; the boundary is half the map, inclusive
    assert ops.composed_mask_head_pays(131072, 8192 + 32768)
    assert ops.composed_mask_head_pays(2048, 1024) and not ops.composed_mask_head_pays(2048, 1025)
    assert ops.composed_mask_head_pays(2048, 0)


def test_bindings_match_the_header():
    from rba_amd import _lib
    hdr = open(os.path.join(REPO, "include", "rba_hip.h")).read()
    for name in ("rba_split_linear_nchw_out_gn_rows_f16x3_f32", "rba_compose_query_operand_f16x2"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
        assert m, name
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        assert len(params) == len(_lib.SIGNATURES[name]), (name, params)
        for p, t in zip(params, _lib.SIGNATURES[name]):
            want = "ptr" if "*" in p else ("i64" if p.startswith("int64_t") else "i")
            got = "ptr" if t is _lib._vp else ("i64" if t is _lib._i64 else "i")
            assert want == got, (name, p)
