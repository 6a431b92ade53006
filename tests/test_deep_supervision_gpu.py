"""Deep supervision in the head fine-tune (MultiScaleMaskedTransformerDecoder.deep_supervision beside differentiable_heads): the bit contract of the
differentiable aux_outputs, the gradient of the WHOLE weighted loss -- final and every ``_{i}`` copy of labels + masks + outlier behind the Hungarian
matcher -- with respect to the ten head tensors against fp64 CPU autograd of the restated heads (tests/_k4_bwd_cases.py) and criterion
(tests/_point_loss_cases.py), a step that lowers that total, and the refusal of one flag without the other.  tiny1 (one aux entry) and tiny3 (four
decoder layers over three levels: four aux entries) on a 60 x 90 image.  Bar: tests/_rba_bwd_cases.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

from tests import _k4_bwd_cases as K4
from tests import _point_loss_cases as C
from tests.test_finetune_heads_gpu import _captured_last_head_call, _head_params, _straddle_the_thresholds, _tiny

pytestmark = pytest.mark.gpu

T, P, EOS = 3, 112, 0.1
BASE = ("loss_ce", "loss_mask", "loss_dice", "outlier_loss")
WEIGHTS = {"loss_ce": 2.0, "loss_mask": 5.0, "loss_dice": 5.0, "outlier_loss": 1.0}
_STATE = {}


def _tiny3():
    """_tiny() of tests/test_finetune_heads_gpu.py on the tiny3 architecture"""
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    _, image, labels = _tiny()
    a = A.complete(A.ARCHS["tiny3"])
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()
    model.graph_replay = False
    pred = model.sem_seg_head.predictor
    pred.differentiable_heads = True
    _, (dec_out, feat) = _captured_last_head_call(pred, lambda: model.finetune_outputs([{"image": image}]))
    _straddle_the_thresholds(pred, dec_out, feat)
    return model, image, labels


def _model(name):
    """(a private copy of the named model with both flags set, image, labels [60,90], number of decoder layers)"""
    if name not in _STATE:
        model, image, labels = _tiny() if name == "tiny1" else _tiny3()
        model = copy.deepcopy(model)
        pred = model.sem_seg_head.predictor
        pred.differentiable_heads = pred.deep_supervision = True
        for p in model.parameters():
            p.requires_grad_(True)
        _STATE[name] = (model, image, labels, pred.num_layers)
    return _STATE[name]


def _all_head_calls(predictor, run):
    """run() with predictor.forward_prediction_heads wrapped -> (run's result, [(decoder-layer output, mask_features)] of every call, in order)"""
    calls, inner = [], predictor.forward_prediction_heads

    def wrapped(output, mask_features, *a, **kw):
        calls.append((output, mask_features))
        return inner(output, mask_features, *a, **kw)

    predictor.forward_prediction_heads = wrapped
    try:
        res = run()
    finally:
        del predictor.forward_prediction_heads
    return res, calls


class _FrozenPerEntry(torch.nn.Module):
    """a matcher that repeats given assignments in SetCriterion.forward's order of calls: the final outputs, then aux entry 0, 1, ..."""

    def __init__(self, per_entry):
        super().__init__()
        self.per_entry, self.calls = per_entry, 0

    def forward(self, outputs, targets, point_coords=None, generator=None):
        self.calls += 1
        return self.per_entry[(self.calls - 1) % len(self.per_entry)]


def _criterion(K, matcher, L):
    from rba_amd.modeling.criterion import SetCriterion
    weights = dict(WEIGHTS)
    weights.update({f"{k}_{i}": v for i in range(L) for k, v in WEIGHTS.items()})
    return SetCriterion(K, matcher, weights, EOS, ["labels", "masks", "outlier"], P, 3.0, 0.75, target="nls", score_norm="tanh", func="squared_hinge",
                        inlier_upper_threshold=-1.0, outlier_lower_threshold=-0.1)


def _fixture(name):
    """(model, image, targets on the GPU, on the CPU, matcher points [P,2], loss points [T,P,2], K, L): T targets that are thresholded enlargements of T
    of the model's own final masks (the fixture of tests/test_finetune_criterion_gpu.py)"""
    key = "fixture " + name
    if key not in _STATE:
        model, image, outlier, L = _model(name)
        with torch.no_grad():
            outputs, _, _ = model.finetune_outputs([{"image": image}])
        masks = outputs["pred_masks"].detach().cpu()
        Q, K = masks.shape[1], outputs["pred_logits"].shape[-1] - 1
        gen = torch.Generator().manual_seed(8600)
        rows = torch.randperm(Q, generator=gen)[:T]
        up = F.interpolate(masks[:, rows], size=tuple(outlier.shape), mode="bilinear", align_corners=False)[0]
        target = {"labels": torch.randint(0, K, (T,), generator=gen), "masks": (up > up.median()).float(), "outlier_masks": outlier.cpu()}
        coords = torch.rand(P, 2, generator=gen), torch.rand(T, P, 2, generator=gen)
        _STATE[key] = (model, image, [{k: v.cuda() for k, v in target.items()}], [target], coords[0].cuda(), coords[1].cuda(), K, L)
    return _STATE[key]


@pytest.mark.parametrize("batch_size", [1, 2])
@pytest.mark.parametrize("name", ["tiny1", "tiny3"])
def test_bit_contract(name, batch_size):
    model, image, _, L = _model(name)
    pred = model.sem_seg_head.predictor
    other = torch.randint(0, 256, (3, 60, 90), generator=torch.Generator().manual_seed(4321), dtype=torch.uint8)
    batch = [{"image": image}, {"image": other}][:batch_size]
    outputs, _, _ = model.finetune_outputs(batch)
    logits, masks, _, _ = model.predict(batch)
    assert torch.equal(outputs["pred_logits"], logits) and torch.equal(outputs["pred_masks"], masks)
    assert outputs["pred_logits"].grad_fn is not None and outputs["pred_masks"].grad_fn is not None
    aux = outputs["aux_outputs"]
    assert len(aux) == L and all(set(a) == {"pred_logits", "pred_masks"} for a in aux)
    assert all(v.grad_fn is not None for a in aux for v in a.values())
    assert all(a["pred_masks"].shape == masks.shape and a["pred_logits"].shape == logits.shape for a in aux)
    with torch.no_grad():                                         # the inference forward, with sparse and with dense intermediate heads
        sparse, _, _ = model.finetune_outputs(batch)
        pred.sparse_intermediate_heads = False
        try:
            dense, _, _ = model.finetune_outputs(batch)
        finally:
            pred.sparse_intermediate_heads = True
    assert len(sparse["aux_outputs"]) == len(dense["aux_outputs"]) == L
    assert torch.equal(sparse["pred_masks"], masks) and torch.equal(dense["pred_masks"], masks)
    for a, s, d in zip(aux, sparse["aux_outputs"], dense["aux_outputs"]):
        assert torch.equal(a["pred_logits"], s["pred_logits"]) and torch.equal(a["pred_logits"], d["pred_logits"])
        assert torch.equal(a["pred_masks"], d["pred_masks"])
        assert "pred_masks" not in s or torch.equal(a["pred_masks"], s["pred_masks"])       # (a level without a sparse plan is dense there too)
    if L > 1:
        assert not torch.equal(aux[0]["pred_masks"], aux[1]["pred_masks"])
    pred.deep_supervision = False                                 # off again: aux entries as in inference, detached
    try:
        off, _, _ = model.finetune_outputs(batch)
    finally:
        pred.deep_supervision = True
    assert off["pred_masks"].grad_fn is not None and torch.equal(off["pred_masks"], masks)
    assert all(not v.requires_grad for a in off["aux_outputs"] for v in a.values())
    assert all(torch.equal(a["pred_logits"], s["pred_logits"]) for a, s in zip(off["aux_outputs"], sparse["aux_outputs"]))


def test_bits_at_the_released_width():
    """The query side runs once on the concatenation of the head calls' inputs: at Q = 100 that is 3 x 2 x 100 rows cut into the Linear's 128-row
    launches at other rows than the per-call evaluation of inference.  A three-layer decoder of the released widths on random inputs."""
    from rba_amd import arch as A
    from rba_amd.modeling.transformer_decoder.mask2former_transformer_decoder import MultiScaleMaskedTransformerDecoder
    from rba_amd.seeded_weights import fill_state_dict_
    a = A.complete(dict(embed_dim=128, depths=[2, 2, 2, 2], num_heads=[4, 8, 16, 32], window_size=12, conv_dim=256, mask_dim=256, nheads=8,
                        num_queries=100, num_classes=19, dim_feedforward=2048, enc_layers=1, dec_layers=3, enc_in=["res5"]))
    dec = MultiScaleMaskedTransformerDecoder(a)
    fill_state_dict_(dec, 0, dict(n_heads=a["nheads"], n_points=a["enc_points"]), prefix="sem_seg_head.predictor.")
    gen = torch.Generator().manual_seed(2025)
    feat = (0.25 * torch.randn(2, 256, 32, 64, generator=gen)).cuda()
    x = [torch.randn(2, 256, 8, 16, generator=gen).cuda()]
    dec = dec.cuda().eval()
    dec.differentiable_heads = dec.deep_supervision = True
    for p in dec.parameters():
        p.requires_grad_(True)
    out = dec(x, feat)
    dec.sparse_intermediate_heads = False
    with torch.no_grad():
        ref = dec(x, feat)
    assert len(out["aux_outputs"]) == len(ref["aux_outputs"]) == 3
    assert torch.equal(out["pred_logits"], ref["pred_logits"]) and torch.equal(out["pred_masks"], ref["pred_masks"])
    for a_, r in zip(out["aux_outputs"], ref["aux_outputs"]):
        assert a_["pred_masks"].grad_fn is not None and a_["pred_logits"].grad_fn is not None
        assert torch.equal(a_["pred_logits"], r["pred_logits"]) and torch.equal(a_["pred_masks"], r["pred_masks"])
    sum(a_["pred_masks"].mean() + a_["pred_logits"].mean() for a_ in out["aux_outputs"]).backward()
    heads = _head_params(dec)
    assert {id(p) for p in dec.parameters() if p.grad is not None} == {id(p) for p in heads.values()}


@pytest.mark.parametrize("name", ["tiny1", "tiny3"])
def test_every_head_tensor_gets_the_restated_gradient_of_the_whole_weighted_loss(name):
    from rba_amd.modeling.matcher import HungarianMatcher
    model, image, targets, targets_cpu, mcoords, lcoords, K, L = _fixture(name)
    pred = model.sem_seg_head.predictor
    crit = _criterion(K, HungarianMatcher(WEIGHTS["loss_ce"], WEIGHTS["loss_mask"], WEIGHTS["loss_dice"], P), L)
    keys = [("", None)] + [(f"_{i}", i) for i in range(L)]
    for p in model.parameters():
        p.requires_grad_(True)
        p.grad = None
    try:
        def run():
            outputs, _, _ = model.finetune_outputs([{"image": image}])
            # each entry's own assignment, from the product's matcher: an aux entry's matching may sit near a tie, and the truth takes the same one
            entries = [outputs] + list(outputs["aux_outputs"])
            indices = [crit.matcher({k: v.detach() for k, v in e.items() if k != "aux_outputs"}, targets, point_coords=mcoords) for e in entries]
            return crit(outputs, targets, matcher_point_coords=mcoords, loss_point_coords=lcoords), indices, outputs

        (losses, indices, outputs), calls = _all_head_calls(pred, run)
        assert len(outputs["aux_outputs"]) == L and len(calls) == L + 1             # _decode's L head calls in order, then the last one
        assert set(losses) == {k + sfx for k in BASE for sfx, _ in keys}
        assert all(ind[0][0].numel() == T for ind in indices)
        weighted = crit.weighted(losses)
        assert set(weighted) == set(crit.weight_dict) == set(losses) and all(v.requires_grad for v in weighted.values())
        sum(weighted.values()).backward()
        heads = _head_params(pred)
        assert {id(p) for p in model.parameters() if p.grad is not None} == {id(p) for p in heads.values()}
        # entry e of the criterion = head call: the final outputs = the last call, aux entry i = call i
        call_of = [L] + list(range(L))
        # no head call's input takes part in a graph or receives a gradient (a one-image batch's initial queries are a view of query_feat.weight: a leaf)
        assert all(o.grad_fn is None and f.grad_fn is None and o.grad is None and f.grad is None for o, f in calls)

        def truth(dtype):
            p = {n: heads[n].detach().cpu().to(dtype).clone().requires_grad_(True) for n in K4.HEAD_TENSORS}
            tg = [{k: (v.to(dtype) if v.is_floating_point() else v) for k, v in t.items()} for t in targets_cpu]
            out, total, aux_total = {}, 0.0, 0.0
            for (sfx, _), c, ind in zip(keys, call_of, indices):
                dec_out, feat = calls[c]
                cls, masks = K4.ref_heads(dec_out.detach().cpu().to(dtype), feat.detach().cpu().to(dtype), p)
                one = C.ref_criterion(cls, masks, tg, [(i.cpu(), j.cpu()) for i, j in ind], float(T), lcoords.cpu().to(dtype), K, EOS)
                part = sum(WEIGHTS[k] * one[k] for k in BASE)
                total = total + part
                if sfx:
                    aux_total = aux_total + part
                out.update({k + sfx: v.detach() for k, v in one.items()})
            g_aux = torch.autograd.grad(aux_total, [p[n] for n in K4.HEAD_TENSORS], retain_graph=True, allow_unused=True)
            total.backward()
            return out, {n: t.grad for n, t in p.items()}, dict(zip(K4.HEAD_TENSORS, g_aux))

        l64, g64, aux64 = truth(torch.float64)
        l32, g32, _ = truth(torch.float32)
        for k in sorted(losses):
            C.check_scalar(k, losses[k].detach(), l32[k], l64[k])
        # the aux part is not negligible: it reaches every head tensor
        assert all(aux64[n] is not None and float(aux64[n].abs().max()) > 0 for n in K4.HEAD_TENSORS)
        for n in K4.HEAD_TENSORS:
            print(f"{n}: max|g| = {float(g64[n].abs().max()):.3e}, of the aux terms alone {float(aux64[n].abs().max()):.3e}")
            C.check(f"grad {n}", heads[n].grad.cpu(), g64[n], C.err(g32[n], g64[n]))
    finally:
        for p in model.parameters():
            p.grad = None


@pytest.mark.parametrize("name", ["tiny1", "tiny3"])
def test_step_lowers_the_full_total_and_inference_is_untouched(name):
    from rba_amd.modeling.matcher import HungarianMatcher
    model, image, targets, _, mcoords, lcoords, K, L = _fixture(name)
    batch = [{"image": image}]
    logits0, masks0, _, _ = model.predict(batch)
    model = copy.deepcopy(model)
    pred = model.sem_seg_head.predictor
    heads = _head_params(pred)
    for p in heads.values():
        p.requires_grad_(True)
    outputs, _, _ = model.finetune_outputs(batch)
    assert torch.equal(outputs["pred_logits"], logits0) and torch.equal(outputs["pred_masks"], masks0)
    matcher = HungarianMatcher(WEIGHTS["loss_ce"], WEIGHTS["loss_mask"], WEIGHTS["loss_dice"], P)
    with torch.no_grad():
        per_entry = [matcher({k: v for k, v in e.items() if k != "aux_outputs"}, targets, point_coords=mcoords)
                     for e in [outputs] + list(outputs["aux_outputs"])]
    crit = _criterion(K, _FrozenPerEntry(per_entry), L)

    def total():
        out, _, _ = model.finetune_outputs(batch)
        w = crit.weighted(crit(out, targets, loss_point_coords=lcoords))
        assert set(w) == set(crit.weight_dict) and all(v.requires_grad for v in w.values())
        return sum(w.values())

    loss = total()
    loss.backward()
    before = float(loss.detach())
    sq = sum(float((p.grad.double() ** 2).sum()) for p in heads.values())
    lr = 0.01 * before / sq                                  # one SGD step sized for a first-order decrease of 1 % of the loss
    with torch.no_grad():
        for p in heads.values():
            p -= lr * p.grad
    after = float(total().detach())
    print(f"total {before:.6f} -> {after:.6f}")
    assert after < before
    pred.differentiable_heads = pred.deep_supervision = False     # both flags off: predict is what it is with them on, on the stepped weights too
    try:
        logits1, masks1, _, _ = model.predict(batch)
    finally:
        pred.differentiable_heads = pred.deep_supervision = True
    logits2, masks2, _, _ = model.predict(batch)
    assert torch.equal(logits1, logits2) and torch.equal(masks1, masks2) and not torch.equal(masks1, masks0)


def test_deep_supervision_without_differentiable_heads_is_refused():
    from rba_amd import ops
    model, image, _, _ = _model("tiny1")
    pred = model.sem_seg_head.predictor
    pred.differentiable_heads = False
    try:
        with pytest.raises(ops.RbaHipError, match="(?s)deep_supervision.*differentiable_heads"):
            model.finetune_outputs([{"image": image}])
    finally:
        pred.differentiable_heads = True
