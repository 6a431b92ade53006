"""GPU: the argument contracts of the composed mask head's wrappers (ops.row_index, split_linear_nchw_out_gn_rows, compose_query_operand) as a table of
refusals, in the manner of tests/test_ops_refusals_gpu.py: every row is a call with ONE fault and must raise RbaHipError before anything is enqueued; the
well-formed call each is derived from must reach its launch.  Nothing runs on the device: the library handle is a stand-in."""
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Reached(Exception):
    pass


class _NoLaunch:
    def __getattr__(self, name):
        def reached(*args):
            raise _Reached(name)
        return reached


def _z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device="cuda")


def test_refusals(monkeypatch):
    from rba_amd import _lib, ops
    from rba_amd._lib import RbaHipError
    B, P, K, G, Q, C = 2, 256, 128, 32, 100, 64
    rows_ok = ops.row_index(torch.arange(128, device="cuda").repeat(B, 1), P)
    monkeypatch.setattr(_lib, "_lib", _NoLaunch())
    good = dict(x=_z(B * P, K), mr=_z(B, G, 2), weight=_z(K), bias_gn=_z(K), num_groups=G, relu=True, planes=_z(1, K // 16, 2, 128, 2, 8, dtype=torch.float16),
                bias=_z(C), rows_per_image=P, out_features=C, rows=rows_ok)
    per_image = dict(good, planes=_z(B, 1, K // 16, 2, 128, 2, 8, dtype=torch.float16), bias=_z(B, Q), out_features=Q, rows=None)
    comp = dict(embed=_z(B, Q, C), weight=_z(C, K), bias=_z(C))
    for fn, kw in ((ops.split_linear_nchw_out_gn_rows, good), (ops.split_linear_nchw_out_gn_rows, per_image), (ops.compose_query_operand, comp)):
        with pytest.raises(_Reached):
            fn(**kw)
    table = [
        ("rows: a bare tensor", ops.split_linear_nchw_out_gn_rows, dict(good, rows=rows_ok.data)),
        ("rows: validated for another image size", ops.split_linear_nchw_out_gn_rows, dict(good, rows=ops.RowIndex(rows_ok.data, 512))),
        ("rows: R % 128 != 0", ops.split_linear_nchw_out_gn_rows, dict(good, rows=ops.RowIndex(rows_ok.data[:, :100].contiguous(), P))),
        ("rows: another batch size", ops.split_linear_nchw_out_gn_rows, dict(good, rows=ops.RowIndex(rows_ok.data[:1].contiguous(), P))),
        ("planes: bf16", ops.split_linear_nchw_out_gn_rows, dict(good, planes=_z(1, K // 16, 3, 128, 2, 8, dtype=torch.bfloat16))),
        ("planes: per-image, for another batch size", ops.split_linear_nchw_out_gn_rows, dict(per_image, planes=_z(3, 1, K // 16, 2, 128, 2, 8, dtype=torch.float16))),
        ("planes: too few tiles for out_features", ops.split_linear_nchw_out_gn_rows, dict(good, out_features=200)),
        ("bias: per-image, wrong shape", ops.split_linear_nchw_out_gn_rows, dict(per_image, bias=_z(B, Q + 1))),
        ("P % 128 != 0", ops.split_linear_nchw_out_gn_rows, dict(good, x=_z(2 * 192, K), rows_per_image=192, rows=None)),
        ("mr of another batch size", ops.split_linear_nchw_out_gn_rows, dict(good, mr=_z(1, G, 2))),
        ("(K / G) % 4 != 0", ops.split_linear_nchw_out_gn_rows, dict(good, num_groups=64, mr=_z(B, 64, 2))),
        ("compose: Q > 128", ops.compose_query_operand, dict(comp, embed=_z(B, 129, C))),
        ("compose: C > 256", ops.compose_query_operand, dict(embed=_z(1, 4, 260), weight=_z(260, K), bias=None)),
        ("compose: K % 32 != 0", ops.compose_query_operand, dict(comp, weight=_z(C, 48))),
        ("compose: weight for another C", ops.compose_query_operand, dict(comp, weight=_z(C + 4, K))),
        ("compose: bias too short", ops.compose_query_operand, dict(comp, bias=_z(C - 1))),
        ("compose: embed float64", ops.compose_query_operand, dict(comp, embed=_z(B, Q, C, dtype=torch.float64))),
    ]
    wrong = []
    for name, fn, kw in table:
        try:
            fn(**kw)
            wrong.append(f"{name}: returned")
        except RbaHipError:
            pass
        except _Reached as e:
            wrong.append(f"{name}: reached {e}")
    assert not wrong, wrong


def test_row_index_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    ok = torch.arange(128, device="cuda").repeat(2, 1)
    assert ops.row_index(ok, 128).data.dtype == torch.int32 and ops.row_index(ok.int(), 128).data.shape == (2, 128)
    for bad, P in ((ok, 127), (ok - 1, 128), (ok.float(), 128), (ok[0], 128), (ok.cpu(), 128), (ok.short(), 128), (ok[:, :0], 128)):
        with pytest.raises(RbaHipError):
            ops.row_index(bad, P)
