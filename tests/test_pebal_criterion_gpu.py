"""The PEBAL recipe's whole criterion on the GPU (criterion.pebal_criterion_from_cfg on the reference's recipe, tests/golden/pebal/): every key of
the final outputs and of one aux_outputs entry and the gradients of the weighted total against fp64 CPU autograd of the restatements
(tests/_pebal_cases.py), K1's score computed once per entry, and the gambler loss on rba_amd's own model (tiny1) reaching the ten head tensors
and nothing else.  Bars as in tests/test_gambler_loss_gpu.py."""
import pytest
import torch

from tests import _pebal_cases as G
from tests import _point_loss_cases as P
from tests import _rba_bwd_cases as C

pytestmark = pytest.mark.gpu

KEYS = ("gambler_loss", "smoothness_loss", "sparsity_loss", "outlier_loss")


def _criterion_call(tmp_path):
    from rba_amd.modeling.criterion import pebal_criterion_from_cfg
    logits, masks, aux_logits, aux_masks, om, ss = G.criterion_inputs()
    leaves = [t.cuda().requires_grad_(True) for t in (logits, masks, aux_logits, aux_masks)]
    outputs = {"pred_logits": leaves[0], "pred_masks": leaves[1], "aux_outputs": [{"pred_logits": leaves[2], "pred_masks": leaves[3]}]}
    targets = [{"outlier_masks": o.cuda(), "sem_seg": s.cuda()} for o, s in zip(om, ss)]
    return pebal_criterion_from_cfg(G.recipe_cfg(tmp_path)), leaves, outputs, targets


def test_recipe_criterion_against_fp64(tmp_path):
    criterion, leaves, outputs, targets = _criterion_call(tmp_path)
    t = G.criterion_truth()
    losses = criterion(outputs, targets)
    assert set(losses) == set(KEYS) | {k + "_0" for k in KEYS}
    for k in sorted(losses):
        assert losses[k].dim() == 0
        P.check_scalar(k, losses[k], t["l32"][k], t["l64"][k])
    weighted = criterion.weighted(losses)
    assert set(weighted) == set(losses)
    total = sum(weighted.values())
    P.check_scalar("weighted total", total, t["t32"], t["t64"])
    total.backward()
    for name, leaf, g64, b in zip(("pred_logits", "pred_masks", "aux pred_logits", "aux pred_masks"), leaves, t["g64"], t["b"]):
        C.check("d total / d " + name, leaf.grad.cpu(), g64, b)


def test_k1_score_is_computed_once_per_entry(tmp_path, monkeypatch):
    """smoothness, sparsity and outlier all select energy: one K1 score launch per image and entry, beside the class map's"""
    from rba_amd import ops
    criterion, leaves, outputs, targets = _criterion_call(tmp_path)
    calls = {"score": 0, "sem": 0}
    rba_reduce = ops.rba_reduce

    def counted(mask_pred, cls_prob, want_sem_seg=False, **kw):
        calls["sem" if want_sem_seg else "score"] += 1
        return rba_reduce(mask_pred, cls_prob, want_sem_seg=want_sem_seg, **kw)

    monkeypatch.setattr(ops, "rba_reduce", counted)
    criterion(outputs, targets)
    B, entries = leaves[0].shape[0], 2
    assert calls == {"score": B * entries, "sem": B * entries}


def test_gambler_loss_reaches_the_ten_head_tensors_and_nothing_else():
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    from rba_amd.modeling.criterion import gambler_loss
    a = A.complete(A.ARCHS["tiny1"])
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()
    model.graph_replay = False
    K = a["num_classes"]
    gen = torch.Generator().manual_seed(4322)
    image = torch.randint(0, 256, (3, 60, 90), generator=gen, dtype=torch.uint8)
    sem_seg = torch.randint(0, K, (60, 90), generator=gen)
    r = torch.rand(60, 90, generator=gen)
    outlier_masks = torch.zeros(60, 90, dtype=torch.int64)
    outlier_masks[r < 0.15] = 1
    outlier_masks[(r >= 0.15) & (r < 0.25)] = 255
    pred = model.sem_seg_head.predictor
    pred.differentiable_heads = True
    out = model.finetune_outputs([{"image": image}])[0]
    loss = gambler_loss(out, [{"outlier_masks": outlier_masks.cuda(), "sem_seg": sem_seg.cuda()}], num_classes=K)["gambler_loss"]
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    reached = 0
    for name, p in pred.named_parameters():
        if name.startswith(("class_embed.", "mask_embed.", "decoder_norm.")):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), name
            reached += 1
        else:
            assert p.grad is None, name
    assert reached == 10                                             # class_embed, the three mask_embed layers, decoder_norm: weight and bias each
    for mod in (model.backbone, model.sem_seg_head.pixel_decoder):
        assert all(p.grad is None for p in mod.parameters())
