"""The DenseHybrid fine-tune on rba_amd's own model (MultiScaleMaskedTransformerDecoder.differentiable_ood_head, MaskFormer.finetune_outputs,
criterion.densehybrid_loss): tiny1_dh on a 60 x 90 image with seeded weights (the fixtures' recipe).  The differentiable ``ood_pred`` head against
the inference kernel and against a F.batch_norm restatement, its running statistics, and which parameters the loss reaches."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

_STATE = {}
TRAINED = ("class_embed.", "mask_embed.", "ood_pred.norm.", "ood_pred.conv.", "decoder_norm.")


def _tiny():
    """(model with differentiable heads, image, sem_seg labels [60,90] int64: classes, 15 % outlier (254), 10 % void (255))"""
    if "tiny" not in _STATE:
        from rba_amd import arch as A
        from rba_amd.checkpoint import load_checkpoint
        from rba_amd.maskformer_model import MaskFormer
        a = A.complete(A.ARCHS["tiny1_dh"])
        model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).cuda().eval()
        model.graph_replay = False
        gen = torch.Generator().manual_seed(4321)
        image = torch.randint(0, 256, (3, 60, 90), generator=gen, dtype=torch.uint8)
        labels = torch.randint(0, a["num_classes"], (60, 90), generator=gen)
        r = torch.rand(60, 90, generator=gen)
        labels[r < 0.15] = 254
        labels[(r >= 0.15) & (r < 0.25)] = 255
        model.sem_seg_head.predictor.differentiable_heads = True
        _STATE["tiny"] = (model, image, labels.cuda(), a["num_classes"])
    return _STATE["tiny"]


@pytest.fixture
def tiny():
    model, image, labels, K = _tiny()
    pred = model.sem_seg_head.predictor
    saved = {k: v.clone() for k, v in pred.ood_pred.norm.state_dict().items()}
    yield model, pred, image, labels, K
    pred.differentiable_ood_head = False
    pred.ood_pred.norm.eval()
    pred.ood_pred.norm.load_state_dict(saved)
    for p in model.parameters():
        p.grad = None


def _mask_features(model, image):
    """the mask-feature map the predictor receives (finetune_outputs computes it under no_grad)"""
    seen, pred = [], model.sem_seg_head.predictor
    hook = pred.register_forward_pre_hook(lambda mod, args: seen.append(args[1]))
    try:
        with torch.no_grad():
            model.finetune_outputs([{"image": image}])
    finally:
        hook.remove()
    mf = seen[-1]
    return (mf.materialize() if hasattr(mf, "materialize") else mf).detach()


def test_without_the_attribute_ood_pred_is_the_inference_output(tiny):
    model, pred, image, _, _ = tiny
    assert pred.differentiable_ood_head is False
    out = model.finetune_outputs([{"image": image}])[0]
    assert out["pred_masks"].grad_fn is not None and out["ood_pred"].grad_fn is None and not out["ood_pred"].requires_grad
    with torch.no_grad():
        ref = pred.ood_pred(_mask_features(model, image))
    assert torch.equal(out["ood_pred"], ref)


def test_differentiable_ood_head_in_eval_mode_matches_the_inference_kernel(tiny):
    model, pred, image, _, _ = tiny
    with torch.no_grad():
        ref = pred.ood_pred(_mask_features(model, image))
    pred.differentiable_ood_head = True
    before = {k: v.clone() for k, v in pred.ood_pred.norm.state_dict().items()}
    out = model.finetune_outputs([{"image": image}])[0]
    assert out["ood_pred"].grad_fn is not None and out["ood_pred"].shape == ref.shape
    d = float((out["ood_pred"].detach() - ref).abs().max())
    print(f"max |differentiable - inference kernel| = {d:.3e} (max |ref| = {float(ref.abs().max()):.3e})")
    assert d <= 1e-5
    for k, v in pred.ood_pred.norm.state_dict().items():
        assert torch.equal(v, before[k]), k                          # eval mode: the running statistics stay
    with torch.no_grad():                                            # grad mode off: the inference path, whatever the attribute says
        assert model.finetune_outputs([{"image": image}])[0]["ood_pred"].grad_fn is None


def test_differentiable_ood_head_in_training_mode_is_batch_norm_and_moves_the_running_statistics_once(tiny):
    model, pred, image, _, _ = tiny
    feat = _mask_features(model, image)
    head = pred.ood_pred
    pred.differentiable_ood_head = True
    head.norm.train()
    mean0, var0, n0 = head.norm.running_mean.clone(), head.norm.running_var.clone(), int(head.norm.num_batches_tracked)
    out = model.finetune_outputs([{"image": image}])[0]["ood_pred"]
    assert out.grad_fn is not None
    rm, rv = mean0.clone(), var0.clone()
    with torch.no_grad():
        y = F.relu(F.batch_norm(feat, rm, rv, head.norm.weight, head.norm.bias, True, head.norm.momentum, head.norm.eps))
        want = F.conv2d(y, head.conv.weight, head.conv.bias)
    d = float((out.detach() - want).abs().max())
    print(f"max |head - F.batch_norm restatement| = {d:.3e} (max |want| = {float(want.abs().max()):.3e})")
    assert d <= 1e-5 * max(1.0, float(want.abs().max()))            # the same batch_norm; conv2d against the matmul form
    assert torch.equal(head.norm.running_mean, rm) and torch.equal(head.norm.running_var, rv)      # one momentum step, the restatement's
    assert not torch.equal(rm, mean0) and not torch.equal(rv, var0) and int(head.norm.num_batches_tracked) == n0 + 1


def test_densehybrid_loss_reaches_the_heads_and_the_ood_head_only(tiny):
    from rba_amd.modeling.criterion import densehybrid_loss
    model, pred, image, labels, K = tiny
    pred.differentiable_ood_head = True
    for p in model.parameters():
        p.grad = None
    out = model.finetune_outputs([{"image": image}])[0]
    loss = densehybrid_loss(out, [{"sem_seg": labels}], num_classes=K)["densehybrid_loss"]
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    reached = 0
    for name, p in model.sem_seg_head.predictor.named_parameters():
        if name.startswith(TRAINED):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            if not name.startswith("decoder_norm."):                 # (decoder_norm feeds both heads: it is part of the differentiable last call)
                assert bool(p.grad.any()), name
                reached += 1
        else:
            assert p.grad is None, name
    assert reached == 2 + 6 + 2 + 2                                  # class_embed, the three mask_embed layers, ood_pred.norm, ood_pred.conv
    for mod in (model.backbone, model.sem_seg_head.pixel_decoder):
        assert all(p.grad is None for p in mod.parameters())
