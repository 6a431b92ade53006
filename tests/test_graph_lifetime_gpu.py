"""GPU: what a captured hipGraph reads must stay alive and current for as long as the graph can be replayed.

A replay re-runs the kernels with the addresses they saw at capture time and never calls back into Python.  These tests change what the model would read --
the batch size of an eager call (the initial prediction heads are cached per batch size), the weights (replaced, re-pointed, edited in place), the BatchNorm
statistics of the C1 backbone -- between a capture and the next replay, and compare every replay with an eager forward and with the oracle.

Order of every test: expected result eagerly, capture + replay, a white-box snapshot of what the capture depends on, the change, an assertion ON THE SNAPSHOT
(the tensors are still referenced / the graph key moved), and only then a replay.  A tree that breaks the rule therefore fails on a plain assertion before any
replay touches memory that was handed back.  The replay itself runs after `scribble`: the guard registry of tests/_guard.py lets go of its references and
NaN-filled tensors of the freed sizes take over whatever blocks the caching allocator has free, so that a stale read shows up as a wrong score instead of
the right old values.  Nothing here returns memory to the device (no empty_cache) -- a stale replay reads mapped memory only."""
import weakref

import pytest
import torch

from oracle import ref_model
from rba_amd import arch as A

pytestmark = pytest.mark.gpu


def build(name, seed=0, sd=None):
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS[name])
    sd = A.seeded_weights(a, seed) if sd is None else sd
    model = load_checkpoint(MaskFormer(a), sd).cuda().eval()
    model.graph_replay = True                 # capture at the third call of a shape (the explicit mode)
    return model, a, sd


def maxerr(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).detach().cpu().double()).abs().max().item()


def argmax_bad(arg, sem_ref, tol=1e-4):
    top2 = sem_ref.topk(2, dim=0).values
    flips = arg.cpu().long() != sem_ref.argmax(0)
    return int((flips & ((top2[0] - top2[1]) > tol)).sum())


def image(seed, h=60, w=90):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (3, h, w), generator=g, dtype=torch.uint8).cuda()


def nbytes(t):
    return t.numel() * t.element_size()


def scribble(canary, sizes, copies=4):
    """Make a stale read visible: the guard registry drops its references, then NaN-filled tensors of the given byte sizes (and, with the canary on, of the
    guard buffers the product would have carved them from: HEAD + payload + padding + TAIL) are allocated on the current stream.  Keep the result alive
    through the replay."""
    if canary is not None:
        canary.check()
    want = set()
    for nb in sizes:
        want.add(nb)
        if canary is not None:
            want.add(canary.HEAD + nb + (-nb) % 16 + canary.TAIL)
    keep = [torch.full(((nb + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda") for nb in sorted(want) for _ in range(copies)]
    torch.cuda.current_stream().synchronize()
    return keep


def captured(model, x, exact=True):
    """eager expectation, then three calls: capture + replay of one graph.  exact=False: replay and eager agree to rounding only (C1: the backbone's
    MIOpen convolutions pick their solver differently under capture)"""
    model.graph_replay = False
    want = model.rba_scores([{"image": x}], return_argmax=True)[0]
    model.graph_replay = True
    for _ in range(3):
        rba, arg = model.rba_scores([{"image": x}], return_argmax=True)[0]
        assert (torch.equal(rba, want[0]) and torch.equal(arg, want[1])) if exact else maxerr(rba, want[0]) < 1e-4
    assert model.live_graphs() == 1
    return want


@pytest.mark.parametrize("name", ["tiny1", "tiny3"])
def test_batch_size_change_keeps_what_a_model_graph_replays(name, canary, monkeypatch):
    """The initial prediction heads are cached per batch size; eager calls with batches of 2 and 3 must not free the batch-1 tensors a captured graph of
    rba_scores replays."""
    model, a, sd = build(name, 0)
    pred = model.sem_seg_head.predictor
    assert pred.cache_initial_heads
    x = image(21)
    want = captured(model, x)
    output, (cls0, emb0) = pred._initial_query_side(1, x.device)          # the tensors the capture read
    refs = [weakref.ref(t) for t in (output, cls0, emb0)]
    sizes = [nbytes(t) for t in (output, cls0, emb0)]
    del output, cls0, emb0
    batches = {B: [{"image": image(30 + i)} for i in range(B)] for B in (2, 3)}
    outs = {B: model.predict(b)[:2] for B, b in batches.items()}
    assert all(r() is not None for r in refs), "a call with another batch size dropped the heads a captured graph reads"
    n_graphs = model.live_graphs()
    keep = scribble(canary, sizes)
    for _ in range(3):
        rba, arg = model.rba_scores([{"image": x}], return_argmax=True)[0]
        assert torch.equal(rba, want[0]) and torch.equal(arg, want[1])
    assert model.live_graphs() == n_graphs                                 # replays, not a recapture
    del keep
    ref = ref_model.forward(x.cpu(), sd, a)
    assert maxerr(rba, ref["rba"]) < 1e-4 and argmax_bad(arg, ref["sem_seg"]) == 0
    pred.cache_initial_heads = False
    for B, b in batches.items():
        cls_p, msk_p = model.predict(b)[:2]
        assert torch.equal(outs[B][0], cls_p) and torch.equal(outs[B][1], msk_p), B
    pred.cache_initial_heads = True
    calls = []
    plain = pred._query_side_heads
    monkeypatch.setattr(pred, "_query_side_heads", lambda out: calls.append(out.shape) or plain(out))
    model.graph_replay = False
    r = model.rba_scores([{"image": x}], return_argmax=True)[0]
    assert torch.equal(r[0], want[0]) and torch.equal(r[1], want[1])
    assert len(calls) == pred.num_layers, calls                          # one per decoder layer: the initial heads come from the cache


def test_batch_size_change_keeps_what_an_external_graph_replays(canary):
    """evaluate_ood.GraphedScore captures the whole DenseHybrid forward itself (no delegation to the model): the same rule for a graph the model does not
    own."""
    from rba_amd import evaluate_ood as E
    model, a, sd = build("tiny1_dh", 0)
    pred = model.sem_seg_head.predictor
    x = image(22)
    want = E.get_densehybrid_score(model, x[None]).clone()
    gs = E.GraphedScore(model, E.get_densehybrid_score, torch.cuda.current_stream())
    assert not gs.delegate
    for _ in range(3):
        assert torch.equal(gs(x), want)
    assert sum(1 for e in gs.graphs.values() if isinstance(e, tuple)) == 1
    output, (cls0, emb0) = pred._initial_query_side(1, x.device)
    refs = [weakref.ref(t) for t in (output, cls0, emb0)]
    sizes = [nbytes(t) for t in (output, cls0, emb0)]
    del output, cls0, emb0
    for B in (2, 3):
        model.predict([{"image": image(40 + i)} for i in range(B)])
    assert all(r() is not None for r in refs), "a call with another batch size dropped the heads a captured graph reads"
    keep = scribble(canary, sizes)
    for _ in range(3):
        assert torch.equal(gs(x), want)
    assert sum(1 for e in gs.graphs.values() if isinstance(e, tuple)) == 1
    del keep
    assert torch.equal(E.get_densehybrid_score(model, x[None]), want)


def _new_param(p):
    return torch.nn.Parameter(p.detach() * 1.25 + 0.01)


# one parameter of every cache family a graph of tiny1 reads
PER_PARAM = [
    "backbone.layers.0.blocks.0.mlp.fc1.weight",                                                  # split planes (ops._cached_planes)
    "sem_seg_head.pixel_decoder.transformer.encoder.layers.0.self_attn.value_proj.weight",        # encoder value projection (token planes where MSDA fuses)
    "backbone.layers.0.blocks.0.attn.qkv.weight",                                                 # qkv split planes (K7's block image at 12 x 12 windows)
    "backbone.layers.0.blocks.0.attn.relative_position_bias_table",                               # gathered bias + fragments
    "sem_seg_head.predictor.query_feat.weight",                                                   # initial prediction heads
    "sem_seg_head.predictor.transformer_cross_attention_layers.0.multihead_attn.in_proj_weight",  # key / value views (_kv_views)
    "sem_seg_head.predictor.decoder_norm.weight",                                                 # read by the LayerNorm kernel directly
]
CASES = [("load_state_dict", None), ("load_state_dict_assign", None), ("class_embed_swap", None)] + \
        [(how, p) for p in PER_PARAM for how in ("new_parameter", "set_data")]


@pytest.mark.parametrize("how,path", CASES, ids=[h if p is None else f"{h}-{p.rsplit('.', 2)[-2]}.{p.rsplit('.', 1)[-1]}" for h, p in CASES])
def test_weights_changed_after_a_capture(how, path, canary):
    """After a capture, weights change in every way a caller can change them; the graph key must move before any replay, and the next calls must equal a
    fresh model loaded with the new state dict (bits) and the oracle (1e-4)."""
    from rba_amd import ops
    model, a, sd = build("tiny1", 0)
    x = image(23, 352, 416)
    res5 = (352 // 32) * (416 // 32)
    # more than 128 memory tokens: the decoder's cross-attention key / value projections run on the token kernel through _kv_views (token planes cached)
    assert res5 > 128 and ops.token_linear_pays(res5, a["conv_dim"], a["conv_dim"])
    captured(model, x)
    key0 = model._graph_key(x, True, "rba")
    mods = dict(model.named_modules())
    freed = []
    if how == "load_state_dict":
        model.load_state_dict({k: v.cuda() for k, v in A.seeded_weights(a, 1).items()}, strict=False)
    elif how == "load_state_dict_assign":
        freed = [nbytes(p) for p in model.parameters()]
        model.load_state_dict({k: v.cuda() for k, v in A.seeded_weights(a, 1).items()}, strict=False, assign=True)
    elif how == "class_embed_swap":
        pred = model.sem_seg_head.predictor
        freed = [nbytes(pred.class_embed.weight), nbytes(pred.class_embed.bias)]
        torch.manual_seed(7)
        pred.class_embed = torch.nn.Linear(pred.class_embed.in_features, pred.class_embed.out_features).cuda()
    else:
        mod_path, _, attr = path.rpartition(".")
        mod = mods[mod_path]
        p = getattr(mod, attr)
        freed = [nbytes(p)]
        if how == "new_parameter":
            setattr(mod, attr, _new_param(p))
        else:
            p.data = p.detach() * 0.75 - 0.02
        del p
    assert model._graph_key(x, True, "rba") != key0, "the graph key did not see the weight change"
    sd_after = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fresh, _, _ = build("tiny1", sd=sd_after)
    fresh.graph_replay = False
    want = fresh.rba_scores([{"image": x}], return_argmax=True)[0]
    keep = scribble(canary, freed)
    for _ in range(3):
        rba, arg = model.rba_scores([{"image": x}], return_argmax=True)[0]
        assert torch.equal(rba, want[0]) and torch.equal(arg, want[1])
    assert model.live_graphs() >= 1
    del keep
    ref = ref_model.forward(x.cpu(), sd_after, a)
    assert maxerr(rba, ref["rba"]) < 1e-4 and argmax_bad(arg, ref["sem_seg"]) == 0


@pytest.mark.parametrize("source", ["running_mean", "bias"])
def test_conv_bn_statistics_edited_after_a_capture(source, canary):
    """C1 (ResNet-50): a ConvBN's BatchNorm statistics / bias edited in place after a capture -- the fold is rebuilt on the eager path, the graph key moves
    before any replay, and both paths equal a fresh model loaded with the edited state dict.  C1's convolutions are MIOpen calls, whose last bits may differ
    from one call to the next: the comparison is to 1e-4, where the edit itself moves the scores by far more than that."""
    model, a, _ = build("r50_1dl", 0)
    x = image(24, 64, 128)
    before = captured(model, x, exact=False)
    key0 = model._graph_key(x, True, "rba")
    cb = model.backbone.res2[0].conv1
    w_f, b_f = cb.folded()
    freed = [nbytes(w_f), nbytes(b_f)]
    del w_f, b_f
    with torch.no_grad():
        getattr(cb.norm, source).add_(0.25)
    assert model._graph_key(x, True, "rba") != key0, "the graph key did not see the edit"
    sd_after = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    fresh, _, _ = build("r50_1dl", sd=sd_after)
    fresh.graph_replay = False
    want = fresh.rba_scores([{"image": x}])[0]
    assert maxerr(want, before[0]) > 1e-2                                 # the edit is visible in the scores
    model.graph_replay = False
    assert maxerr(model.rba_scores([{"image": x}])[0], want) < 1e-4, "eager path: stale BatchNorm fold"
    model.graph_replay = True
    keep = scribble(canary, freed)
    for _ in range(3):                                                   # eager, capture + replay, replay
        assert maxerr(model.rba_scores([{"image": x}])[0], want) < 1e-4
    assert model.live_graphs() == 2
    del keep
