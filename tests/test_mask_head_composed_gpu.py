"""GPU: the mask heads of the masked decoder without the mask-feature map (docs/kernels/K4.md) -- the gathered / per-image forms of the GroupNorm-folded
projection, the composed query operand, the final logits against float64, and the model with the switch on and off."""
import pytest
import torch

from rba_amd import arch as A
from tests._mask_head_ref import EPS, G, logits64, operands

pytestmark = pytest.mark.gpu


def _full(o, relu=True):
    from rba_amd import ops
    return ops.split_linear_nchw_out_gn(o["y"], o["mr"], o["gamma"], o["beta"], G, relu, o["planes"], o["bias"], o["P"], out_features=o["C"])


def _rows(o, planes, bias, N, rows=None, relu=True):
    from rba_amd import ops
    return ops.split_linear_nchw_out_gn_rows(o["y"], o["mr"], o["gamma"], o["beta"], G, relu, planes, bias, o["P"], out_features=N, rows=rows)


def _index(B, P, R, seed):
    """row 0, row P - 1, repeats, and different rows per image"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, P, (B, R), generator=g)
    idx[:, 0], idx[:, 1], idx[:, 2], idx[:, 3] = 0, P - 1, 0, P - 1
    idx[:, 64:72] = idx[:, 5:6]
    return idx.cuda()


# ---- 1. the gathered projection is exact
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("B,P,K,C,R", [(1, 256, 128, 64, 128), (2, 384, 256, 256, 384), (2, 256, 256, 64, 128), (1, 384, 128, 256, 384)])
def test_gathered_projection_is_exact(B, P, K, C, R, relu):
    from rba_amd import ops
    o = operands(B, P, K, C, 5, seed=B * 1000 + P + K + C)
    idx = _index(B, P, R, 7)
    assert B == 1 or not torch.equal(idx[0], idx[1])
    want = torch.stack([_full(o, relu)[b][:, idx[b]] for b in range(B)])
    got = _rows(o, o["planes"], o["bias"], C, ops.row_index(idx, P), relu)
    assert got.shape == (B, C, R) and torch.equal(got, want)
    assert torch.equal(_rows(o, o["planes"], o["bias"], C, None, relu), _full(o, relu))          # no index: the entry it extends


# ---- 2. per-image planes are exact, and N < 128 writes N planes only (the guard bands of tests/_guard.py around `out` are checked by the canary fixture)
@pytest.mark.parametrize("Q", [5, 100, 128])
@pytest.mark.parametrize("P,K", [(256, 128), (384, 256)])
def test_per_image_operands_equal_single_image_calls(Q, P, K, canary):
    from rba_amd import ops
    o = operands(2, P, K, 64, Q, seed=Q + P)
    planes, bias_q = ops.compose_query_operand(o["E"], o["W"], o["bias"])
    assert not torch.equal(planes[0], planes[1]) and not torch.equal(bias_q[0], bias_q[1])
    both = _rows(o, planes, bias_q, Q)
    assert both.shape == (2, Q, P) and bool(torch.isfinite(both).all())                           # (a plane the kernel skipped would still hold the NaN poison)
    idx = _index(2, P, 128, 3)
    both_g = _rows(o, planes, bias_q, Q, ops.row_index(idx, P))
    for b in range(2):
        one = dict(o, y=o["y"][b * P:(b + 1) * P].contiguous(), mr=o["mr"][b:b + 1].contiguous())
        assert torch.equal(_rows(one, planes[b:b + 1].contiguous(), bias_q[b:b + 1].contiguous(), Q)[0], both[b])
        assert torch.equal(_rows(one, planes[b].contiguous(), bias_q[b].contiguous(), Q)[0], both[b])              # ... and as SHARED operands of a B = 1 call
        assert torch.equal(both_g[b], both[b][:, idx[b]])
    if canary is not None:
        canary.check()


# ---- 3. the composed operand
@pytest.mark.parametrize("B,Q,C,K", [(1, 5, 64, 128), (2, 100, 256, 256), (1, 128, 256, 128), (2, 100, 64, 256)])
def test_composed_operand(B, Q, C, K):
    from rba_amd import ops
    o = operands(B, 256, K, C, Q, seed=Q * C + K)
    planes, bias_q = ops.compose_query_operand(o["E"], o["W"], o["bias"])
    planes2, bias_q2 = ops.compose_query_operand(o["E"], o["W"], o["bias"])
    assert torch.equal(planes.view(torch.int16), planes2.view(torch.int16)) and torch.equal(bias_q, bias_q2)      # deterministic
    E, W, bias = o["E"].double().cpu(), o["W"].double().cpu(), o["bias"].double().cpu()
    u = 2.0 ** -24
    for b in range(B):
        hl = ops.unpack_split_weight(planes[b]).double().cpu()                                     # [2, 128, K]
        got = hl[0] + hl[1] * 2.0 ** -11
        assert bool((got[Q:] == 0).all()) and bool((hl[:, Q:] == 0).all())                        # padding rows
        ref, mag = E[b] @ W, E[b].abs() @ W.abs()
        bound = (C + 2) * u * mag + 2.0 ** -22 * ref.abs()
        err = (got[:Q] - ref).abs()
        print(f"E W: B {b} max err {err.max():.3e}, max err / bound {(err / bound).max():.3f}")
        assert bool((err <= bound).all())
        rb, mb = E[b] @ bias, E[b].abs() @ bias.abs()
        errb = (bias_q[b].double().cpu() - rb).abs()
        print(f"E bias: max err {errb.max():.3e}, max err / bound {(errb / ((C + 2) * u * mb)).max():.3f}")
        assert bool((errb <= (C + 2) * u * mb).all())
    _, bq0 = ops.compose_query_operand(o["E"], o["W"], None)
    assert bool((bq0 == 0).all())


def test_composed_operand_overflow_is_loud():
    """a product beyond f16's range packs to +-inf: the final logits of that query are NaN, never finite wrong numbers"""
    from rba_amd import ops
    o = operands(1, 256, 128, 64, 5, seed=11)
    W = o["W"].clone()
    W[7] = torch.where(W[7].abs() < 0.25, torch.full_like(W[7], 0.25), W[7])                     # |1e6 W[7, k]| >= 2.5e5 > 65504 for every k
    E = o["E"].clone()
    E[0, 3, 7] = 1e6
    planes, bias_q = ops.compose_query_operand(E, W, o["bias"])
    out = _rows(o, planes, bias_q, 5)
    assert bool(torch.isnan(out[0, 3]).all())
    assert bool(torch.isfinite(out[0, [0, 1, 2, 4]]).all())


# ---- 4. final logits: composed form and two-launch form against float64
def test_final_logits_against_float64():
    """Measured on MI355X (see docs/kernels/K4.md): composed / two-launch max error ratio printed below; the bound is 1.5 (one longer rounding chain)."""
    from rba_amd import ops
    o = operands(2, 384, 256, 256, 100, seed=4)
    ref = logits64(o["y"], o["mr"], o["gamma"], o["beta"], o["W"], o["bias"], o["E"], 2)
    two = ops.mask_logits(o["E"], _full(o), mode="f16x3")
    planes, bias_q = ops.compose_query_operand(o["E"], o["W"], o["bias"])
    one = _rows(o, planes, bias_q, 100)
    e_two, e_one = (two.double().cpu() - ref).abs().max().item(), (one.double().cpu() - ref).abs().max().item()
    print(f"final logits: max |ref| {ref.abs().max():.1f}; two-launch max err {e_two:.3e}, composed max err {e_one:.3e}, ratio {e_one / e_two:.3f}")
    assert e_one <= 1.5 * e_two


# ---- 5. / 6. the model
ARCH128 = dict(A.ARCHS["tiny1"], conv_dim=128, mask_dim=64, nheads=4)           # (K3 serves head_dim 32)


def _build(arch, seed=0):
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(dict(arch))
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, seed)).cuda().eval()
    model.graph_replay = False
    return model


def _images(n, h=128, w=256, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8).cuda() for _ in range(n)]


class _Trace:
    """records the mask-head ops of a forward: (name, first tensor argument's shape) and the outputs of quad_mean (the attention-mask logits)"""
    NAMES = ("mask_logits", "quad_mean", "split_linear_nchw_out_gn", "split_linear_nchw_out_gn_rows", "compose_query_operand", "split_linear_nchw_out")

    def __init__(self, monkeypatch):
        from rba_amd import ops
        self.calls, self.attn, self.contract, self.gathers = [], [], [], 0
        for nm in self.NAMES:
            f = getattr(ops, nm)

            def w(*args, _f=f, _nm=nm, **kw):
                out = _f(*args, **kw)
                self.calls.append((_nm, tuple(args[1].shape if _nm == "mask_logits" else args[0].shape)))
                if _nm == "quad_mean":
                    self.attn.append(out.clone())
                return out
            monkeypatch.setattr(ops, nm, w)
        real = torch.Tensor.index_select

        def counted(t, *a, **k):
            self.gathers += 1
            return real(t, *a, **k)
        monkeypatch.setattr(torch.Tensor, "index_select", counted)

    def names(self):
        return [c[0] for c in self.calls]


def _run(model, images, on, monkeypatch, grad=False):
    from rba_amd import ops
    with monkeypatch.context() as m:
        m.setattr(ops, "COMPOSED_MASK_HEAD", on)
        tr = _Trace(m)
        batch = [{"image": im} for im in images]
        if grad:                                                         # the head called in grad mode: the predictor is handed the deferred operand
            with torch.no_grad():
                d = model.size_divisibility
                H, W = [(v + d - 1) // d * d for v in images[0].shape[-2:]]
                features = model.backbone.forward_images([im.contiguous() for im in images], model._mean3, model._std3, H, W)
            got = []
            hook = model.sem_seg_head.predictor.register_forward_pre_hook(lambda mod, args: got.append(type(args[1]).__name__))
            try:
                with torch.enable_grad():
                    out = model.sem_seg_head(features)
            finally:
                hook.remove()
            tr.handed = got
            assert out["pred_masks"].requires_grad and out["pred_logits"].requires_grad
            cls, masks = out["pred_logits"], out["pred_masks"]
        else:
            with torch.no_grad():
                cls, masks, _, _ = model.predict(batch)
        torch.cuda.synchronize()
    return cls.detach().clone(), masks.detach().clone(), tr


@pytest.mark.parametrize("B", [1, 2])
def test_model_switch_on_and_off(B, monkeypatch):
    from rba_amd.modeling.pixel_decoder.msdeformattn import DeferredMaskFeatures
    model = _build(ARCH128)
    images = _images(B)
    seen = []
    real = DeferredMaskFeatures.contract
    monkeypatch.setattr(DeferredMaskFeatures, "contract", lambda self, embed: (seen.append((self, embed.clone())), real(self, embed))[1])
    cls1, m1, t1 = _run(model, images, True, monkeypatch)
    cls0, m0, t0 = _run(model, images, False, monkeypatch)
    P = 32 * 64
    assert torch.equal(cls1, cls0)
    assert len(t1.attn) == len(t0.attn) == 1 and torch.equal(t1.attn[0], t0.attn[0])              # the attention-mask logits: the very bits
    # switch off: today's launches; switch on: no P-column mask_logits, no ATen gather, no full projection
    assert [s for n, s in t0.calls if n == "mask_logits"] == [(B, 64, 128), (B, 64, 32, 64)] and t0.gathers == 1 and P == 2048
    assert "split_linear_nchw_out_gn" in t0.names() and "compose_query_operand" not in t0.names() and "split_linear_nchw_out_gn_rows" not in t0.names()
    assert t1.gathers == 0 and "split_linear_nchw_out_gn" not in t1.names() and "split_linear_nchw_out" not in t1.names()
    assert t1.names().count("split_linear_nchw_out_gn_rows") == 2 and t1.names().count("compose_query_operand") == 1
    assert [s for n, s in t1.calls if n == "mask_logits"] == [(B, 64, 128)]                         # only the 4 h w = 128 gathered columns
    # pred_masks: both forms against float64 on the operands the model handed over (test 4's bound)
    (d, E), = seen
    ref = logits64(d.prev, d.mr, d.norm.weight, d.norm.bias, d.conv.weight.view(64, 128), d.conv.bias, E, B).view(B, -1, 32, 64)
    e1, e0 = (m1.double().cpu() - ref).abs().max().item(), (m0.double().cpu() - ref).abs().max().item()
    print(f"model pred_masks: max |ref| {ref.abs().max():.2f}; map + einsum max err {e0:.3e}, composed max err {e1:.3e}, ratio {e1 / e0:.3f}; "
          f"max |on - off| {(m1 - m0).abs().max().item():.3e}")
    assert m1.shape == m0.shape and e1 <= 1.5 * e0


def test_model_composed_under_graph_capture(monkeypatch):
    """capture + replay with two different images: what the eager composed forward gives; nothing is built inside the capture"""
    from rba_amd import ops
    assert ops.COMPOSED_MASK_HEAD
    model = _build(ARCH128)
    a, b = _images(2, seed=9)
    with torch.no_grad():
        want = [tuple(t.clone() for t in model.predict([{"image": im}])[:2]) for im in (a, b)]
        static = a.clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            model.predict([{"image": static}])
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        tr = _Trace(monkeypatch)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            out = model.predict([{"image": static}])[:2]
        torch.cuda.synchronize()
    assert "compose_query_operand" in tr.names() and "split_linear_nchw_out_gn" not in tr.names()  # the capture took the composed path
    for im, w in ((b, want[1]), (a, want[0]), (b, want[1])):
        static.copy_(im)
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], w[0]) and torch.equal(out[1], w[1])


def _same_either_way(model, images, monkeypatch, grad=False):
    cls1, m1, t1 = _run(model, images, True, monkeypatch, grad)
    cls0, m0, t0 = _run(model, images, False, monkeypatch, grad)
    assert torch.equal(cls1, cls0) and torch.equal(m1, m0)
    assert t1.calls == t0.calls and t1.gathers == t0.gathers
    assert "compose_query_operand" not in t1.names() and "split_linear_nchw_out_gn_rows" not in t1.names()
    return t1


def test_fallback_tiny1_as_shipped(monkeypatch):
    """conv_dim = 64: K / G = 2, the GroupNorm-folded projection does not apply"""
    _same_either_way(_build(A.ARCHS["tiny1"]), _images(1), monkeypatch)


def test_fallback_bf16x6(monkeypatch):
    from rba_amd import ops
    model = _build(ARCH128)
    with ops.split_mode("bf16x6"):
        _same_either_way(model, _images(1), monkeypatch)


def test_fallback_ood_prediction(monkeypatch):
    t = _same_either_way(_build(dict(A.ARCHS["tiny1_dh"], conv_dim=128, mask_dim=128, nheads=4)), _images(1), monkeypatch)
    assert "split_linear_nchw_out_gn" in t.names()                                                 # (the folded projection ran: the map is needed by ood_pred)


def test_fallback_differentiable_heads(monkeypatch):
    """grad mode with differentiable heads, through the head (the predictor IS handed the deferred operand with the switch on): the map is materialised, the
    outputs are the switch-off run's bits and carry a graph"""
    model = _build(ARCH128)
    model.sem_seg_head.predictor.differentiable_heads = True
    cls1, m1, t1 = _run(model, _images(1), True, monkeypatch, grad=True)
    cls0, m0, t0 = _run(model, _images(1), False, monkeypatch, grad=True)
    assert t1.handed == t0.handed == ["DeferredMaskFeatures"]        # (the head always asks for the operand; the switch is read by the predictor's rule)
    assert torch.equal(cls1, cls0) and torch.equal(m1, m0)
    assert t1.calls == t0.calls and t1.names().count("split_linear_nchw_out_gn") == 1 and "compose_query_operand" not in t1.names()
    # ... and the same model with grad mode off takes the composed path: the clause is about grad mode, not about the attribute
    _, _, t = _run(model, _images(1), True, monkeypatch)
    assert "compose_query_operand" in t.names()


def test_switch_is_part_of_the_graph_key(monkeypatch):
    """a graph captured with the switch on is not replayed with it off"""
    from rba_amd import ops
    model = _build(ARCH128)
    im = _images(1)[0]
    k1 = model._graph_key(im, False, "rba")
    monkeypatch.setattr(ops, "COMPOSED_MASK_HEAD", not ops.COMPOSED_MASK_HEAD)
    k0 = model._graph_key(im, False, "rba")
    assert k1 != k0 and k1 == k1._replace() and k0[:14] == k1[:14]


def test_fallback_nine_layers_three_levels(monkeypatch):
    """Three levels: the 1/8 level's 4 h w samples are the whole 1/4 map, so it has no sparse plan and the rule keeps the map at its plan clause.  With the
    released strides (levels at 1/8, 1/16, 1/32 under a 1/4 map) the P / 2 clause cannot be the one that decides in the model: without the 1/8 level the rows
    are at most 5/16 of the map, with it there is no plan (docs/kernels/K4.md).  Its arithmetic is tested as a pure function in
    tests/test_mask_head_composed_cpu.py."""
    arch = dict(A.ARCHS["tiny3"], conv_dim=128, mask_dim=64, nheads=4, dec_layers=9)
    t = _same_either_way(_build(arch), _images(1), monkeypatch)
    assert "split_linear_nchw_out_gn" in t.names()
