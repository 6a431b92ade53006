"""GPU: the differentiable decoder layers (MultiScaleMaskedTransformerDecoder.differentiable_decoder) against fp64 CPU autograd through the
oracle -- each layer type at the released widths, then the whole decoder of tiny3 / tiny1 / a three-level one-layer decoder.

Metric and bar as tests/test_msda_backward_gpu.py: e(T) = max|T_gpu - T64| / max|T64| per gradient tensor, e <= 4 max(b, 2^-20) with b the same
metric for the oracle's fp32 CPU autograd on the same inputs, computed per case and printed; nothing is left out.  Library GEMMs run with
allow_tf32 = False.  Forward values are compared for equality with the inference path."""
import pytest
import torch

from oracle import ref_model, ref_ops
from tests import _decoder_bwd_cases as C

pytestmark = pytest.mark.gpu

D, NH, Q, S, FFN, B = 256, 8, 100, 512, 2048, 2


@pytest.fixture(autouse=True)
def no_tf32():
    old = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = old


def dev(t):
    return t.cuda().contiguous()


def compare(what, got, t64, t32):
    assert sorted(got) == sorted(t64), (sorted(got), sorted(t64))
    failures = []
    for k in sorted(t64):
        assert got[k] is not None and got[k].shape == t64[k].shape, k
        e, b = C.err(got[k], t64[k]), C.err(t32[k], t64[k])
        line = f"{what} {k}: e = {e:.3e} b = {b:.3e} bar = {C.bar(b):.3e}"
        print(line)
        if not e <= C.bar(b):
            failures.append(line)
    assert not failures, "beyond 4 max(b, 2^-20):\n" + "\n".join(failures)


# ---------------------------------------------------------------------------------------------- each layer type at the released widths
def _layer(kind, B=B, S=S):
    from rba_amd.modeling.transformer_decoder import mask2former_transformer_decoder as M
    layer = {"cross": lambda: M.CrossAttentionLayer(D, NH), "self": lambda: M.SelfAttentionLayer(D, NH), "ffn": lambda: M.FFNLayer(D, FFN)}[kind]()
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.05 + (1.0 if n.endswith("norm.weight") else 0.0))
    inp = {"tgt": torch.randn(B, Q, D, generator=g), "qpos": torch.randn(B, Q, D, generator=g), "go": torch.randn(B, Q, D, generator=g)}
    if kind == "cross":
        inp["mem"], inp["pos"] = torch.randn(B, S, D, generator=g), torch.randn(B, S, D, generator=g)
        ml = torch.randn(B, Q, S, generator=g) * 3
        ml[:, 0] = -5.0                                      # a fully blocked row attends everywhere
        ml[:, 1] = 5.0
        ml[:, 2, : S - 150] = -5.0
        inp["ml"] = ml
    return layer, inp


def _oracle_layer(kind, layer, inp, dtype):
    sd = {"L." + k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in layer.state_dict().items()}
    tgt = inp["tgt"].to(dtype).clone().requires_grad_(True)
    t, qp = tgt.transpose(0, 1), inp["qpos"].to(dtype).transpose(0, 1)                    # the oracle is sequence-first
    if kind == "ffn":
        t2 = ref_model._lin(torch.relu(ref_model._lin(t, sd, "L.linear1")), sd, "L.linear2")
    else:
        m = "L.multihead_attn" if kind == "cross" else "L.self_attn"
        w = [sd[m + ".in_proj_weight"], sd[m + ".in_proj_bias"], sd[m + ".out_proj.weight"], sd[m + ".out_proj.bias"]]
        if kind == "cross":
            mem, pos = inp["mem"].to(dtype).transpose(0, 1), inp["pos"].to(dtype).transpose(0, 1)
            blocked = ref_ops.attn_mask_from_logits(inp["ml"].clone())                    # fp32: the kernel's own logits
            t2 = ref_ops.multihead_attention(t + qp, mem + pos, mem, *w, NH, blocked.unsqueeze(1).repeat(1, NH, 1, 1).flatten(0, 1))
        else:
            t2 = ref_ops.multihead_attention(t + qp, t + qp, t, *w, NH, None)
    out = ref_model._ln(t + t2, sd, "L.norm").transpose(0, 1)
    out.backward(inp["go"].to(dtype))
    grads = {k[2:]: v.grad for k, v in sd.items()}
    grads["tgt"] = tgt.grad
    return grads


def _layer_args(kind, inp):
    return {"cross": lambda: (dev(inp["mem"]), dev(inp["ml"]), dev(inp["pos"]), dev(inp["qpos"])), "self": lambda: (dev(inp["qpos"]),), "ffn": lambda: ()}[kind]()


# self at B = 1 is the stacked in_proj in one launch (B Q <= 128); at B = 2 the split projections
@pytest.mark.parametrize("kind, batch", [pytest.param("cross", 2, id="cross"), pytest.param("self", 2, id="self"), pytest.param("ffn", 2, id="ffn"),
                                         pytest.param("self", 1, id="self-B1")])
def test_layer_at_released_widths(kind, batch):
    layer, inp = _layer(kind, batch)
    t64, t32 = _oracle_layer(kind, layer, inp, torch.float64), _oracle_layer(kind, layer, inp, torch.float32)
    layer = layer.cuda()
    tgt = dev(inp["tgt"]).requires_grad_(True)
    args = _layer_args(kind, inp)
    with torch.no_grad():
        want = layer(tgt, *args)
    out = layer(tgt, *args, graph=True)
    assert torch.equal(out, want) and out.grad_fn is not None
    out.backward(dev(inp["go"]))
    got = {k: p.grad for k, p in layer.named_parameters()}
    got["tgt"] = tgt.grad
    compare(kind, got, t64, t32)


def _recorded_launches(monkeypatch):
    """the list that receives the entry-point name of every kernel launch from here on"""
    from rba_amd import ops
    names, launch = [], ops._launch

    def recording(name, *args, **kwargs):
        names.append(name)
        return launch(name, *args, **kwargs)

    monkeypatch.setattr(ops, "_launch", recording)
    return names


@pytest.mark.parametrize("kind, batch, keys", [("self", 1, S), ("self", 2, S), ("cross", 2, 512), ("cross", 1, 64), ("ffn", 2, S)])
def test_a_layers_training_forward_is_its_inference_launches(kind, batch, keys, monkeypatch):
    """graph=True wraps the launches of the inference body in autograd Functions and adds, drops or reorders none: self with the stacked in_proj
    (B Q <= 128) and with split projections, cross with the row-complete key / value launch and on the skinny route (B S <= 128), ffn"""
    layer, inp = _layer(kind, batch, keys)
    layer = layer.cuda()
    tgt = dev(inp["tgt"]).requires_grad_(True)
    args = _layer_args(kind, inp)
    with torch.no_grad():
        layer(tgt, *args)                                    # unrecorded: a first forward also packs the weight images it caches
    names = _recorded_launches(monkeypatch)
    with torch.no_grad():
        layer(tgt, *args)
    inference = list(names)
    del names[:]
    out = layer(tgt, *args, graph=True)
    assert out.grad_fn is not None
    print(kind, batch, keys, inference)
    assert inference and names == inference


# ---------------------------------------------------------------------------------------------- the whole decoder
_cache = {}


def problem(model):
    if model not in _cache:
        a, sd, x, mf, wts = C.make(model)
        t64, am = C.cpu_grads(a, sd, x, mf, wts, torch.float64)
        t32, _ = C.cpu_grads(a, sd, x, mf, wts, torch.float32)
        _cache[model] = (a, sd, x, mf, wts, t64, t32, am)
    return _cache[model]


def predictor(a, sd):
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    return load_checkpoint(MaskFormer(a), sd).cuda().eval().sem_seg_head.predictor


def calls(out):
    return [(o["pred_logits"], o["pred_masks"]) for o in out["aux_outputs"]] + [(out["pred_logits"], out["pred_masks"])]


@pytest.mark.parametrize("model", list(C.MODELS))
def test_whole_decoder(model):
    a, sd, x, mf, wts, t64, t32, am = problem(model)
    assert len(am) == a["dec_layers"] + 1 and C.margin_ok(am), "the chosen seed must keep every thresholded logit 1e-3 from 0 in double"
    pred = predictor(a, sd)
    gx, gmf = [dev(t) for t in x], dev(mf)
    pred.sparse_intermediate_heads = False
    with torch.no_grad():
        want = calls(pred(gx, gmf))
    pred.sparse_intermediate_heads = True
    pred.differentiable_heads = pred.deep_supervision = pred.differentiable_decoder = True
    out = pred(gx, gmf)
    got_calls = calls(out)
    assert len(got_calls) == len(want) == a["dec_layers"] + 1
    for (c, m), (wc, wm) in zip(got_calls, want):                                          # the forward: the inference kernels' bits
        assert torch.equal(c, wc) and torch.equal(m, wm) and c.grad_fn is not None and m.grad_fn is not None
    C.functional(got_calls, [(dev(wc), dev(wm)) for wc, wm in wts]).backward()
    got = {k: p.grad for k, p in pred.named_parameters()}
    assert all(g is not None for g in got.values())
    compare(model, got, t64, t32)
    if model == "tiny3_1dl":                                                               # levels the one layer never visits: exactly zero, not None
        assert bool((got["level_embed.weight"][1:] == 0).all()) and bool((t64["level_embed.weight"][1:] == 0).all())
        assert bool((got["level_embed.weight"][0] != 0).any())


def test_heads_only_guard():
    """only the head parameters require grad: with the flag their gradients are the bits of today's differentiable_heads path; without it no
    layer parameter receives a gradient though all require grad"""
    a, sd, x, mf, wts = problem("tiny3")[:5]
    gx, gmf, gw = [dev(t) for t in x], dev(mf), [(dev(wc), dev(wm)) for wc, wm in wts]
    heads = ("class_embed", "mask_embed", "decoder_norm")

    def run(flag, heads_only):
        pred = predictor(a, sd)
        if heads_only:
            for n, p in pred.named_parameters():
                p.requires_grad_(n.split(".")[0] in heads)
        pred.differentiable_heads = pred.deep_supervision = True
        pred.differentiable_decoder = flag
        C.functional(calls(pred(gx, gmf)), gw).backward()
        return {n: p.grad for n, p in pred.named_parameters()}

    today, flagged = run(False, True), run(True, True)
    for n, g in today.items():
        if n.split(".")[0] in heads:
            assert g is not None and torch.equal(g, flagged[n]), n
        else:
            assert g is None and flagged[n] is None, n
    unset = run(False, False)
    for n, g in unset.items():
        assert (g is not None) == (n.split(".")[0] in heads), n


def test_inference_builds_no_graph(monkeypatch):
    """all four flags off: a forward with grad mode on and every parameter requiring grad is still the inference path"""
    a, sd, x, mf = problem("tiny3")[:4]
    pred = predictor(a, sd)
    for p in pred.parameters():
        p.requires_grad_(True)
    assert not (pred.differentiable_heads or pred.deep_supervision or pred.differentiable_ood_head or pred.differentiable_decoder)
    names = _recorded_launches(monkeypatch)
    assert torch.is_grad_enabled()
    out = pred([dev(t) for t in x], dev(mf))
    tensors = [out["pred_logits"], out["pred_masks"]] + [v for aux in out["aux_outputs"] for v in aux.values()]
    assert len(out["aux_outputs"]) == a["dec_layers"] and all(t.grad_fn is None for t in tensors)
    assert names and not {"rba_masked_xattn_bwd_f32", "rba_mask_logits_bwd_f32"} & set(names)


def test_finetune_outputs_refuses_the_flag_alone():
    from rba_amd._lib import RbaHipError
    from tests import _solver_cases as S_
    model = S_.tiny("tiny1").cuda().eval()
    model.sem_seg_head.predictor.differentiable_decoder = True
    image = torch.zeros(3, 60, 90, dtype=torch.uint8, device="cuda")
    with pytest.raises(RbaHipError, match="differentiable_decoder is set without"):
        model.finetune_outputs([{"image": image}])
