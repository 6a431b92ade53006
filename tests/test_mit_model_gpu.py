"""GPU: the MiT (SegFormer) backbone on K19 -- its parts and the two tiny networks against the fixtures the reference's own module wrote
(tests/golden/make_golden_mit.py), in both split modes and on both K1 paths; no library GEMM / convolution / attention call on the path; graph
replay, in-place weight changes, the fine-tune front end and the evaluate_ood command line from a MiT config."""
import pytest
import torch

from rba_amd import arch as A
from rba_amd.seeded_weights import seeded_tensor
from tests._sweep_align import K_PARITY

pytestmark = pytest.mark.gpu
T = torch.from_numpy


@pytest.fixture(autouse=True)
def guarded_allocations(canary):
    """tests/_guard.py guards a fixed module list: run rba_amd.mit_ops' allocations under the guard bands too (the backbone module allocates
    nothing itself: everything it makes comes out of rba_amd.ops and rba_amd.mit_ops)"""
    import rba_amd.mit_ops as mops
    if canary is None:
        yield
        return
    real, mops.torch = mops.torch, canary._PROXY
    try:
        yield
    finally:
        mops.torch = real


def build(name, seed=0):
    from rba_amd.checkpoint import load_checkpoint
    from rba_amd.maskformer_model import MaskFormer
    a = A.complete(A.ARCHS[name])
    model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, seed)).cuda().eval()
    model.graph_replay = False
    return model, a


def maxerr(a, b):
    return (a.detach().cpu().double() - torch.as_tensor(b).double()).abs().max().item()


def _seed_module(module, prefix):
    """the fixture's weights: every tensor from its key name (rba_amd.seeded_weights), as make_golden_mit.py filled the reference's module"""
    module.load_state_dict({k: seeded_tensor(prefix + k, v, 0) for k, v in module.state_dict().items()})
    return module.cuda().eval()


def _held(got, g, key, mode, where):
    """k x the fixture's own fp32-vs-float64 distance on that tensor, never tighter than 1e-5 max|x| (the rule of tests/_sweep_align.py: k = 5 in
    f16x3 mode, 3 in bf16x6 mode)"""
    want32, want64 = T(g[key]), T(g[key + "64"])
    own = (want32.double() - want64).abs().max().item()
    bound = max(K_PARITY[mode] * own, 1e-5 * want64.abs().max().item())
    err = maxerr(got, want32)
    print(f"{where} [{mode}]: err {err:.3g}, bound {bound:.3g} (own {own:.3g}, max|x| {want64.abs().max().item():.3g})")
    assert err <= bound, where


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
def test_parts_against_the_reference(golden, mode):
    from rba_amd import ops
    from rba_amd.modeling.backbone import mix_transformer as M
    g = golden("g10_mit_parts")
    with ops.split_mode(mode), torch.no_grad():
        for stage in (1, 2, 3, 4):
            Cn, nH, sr, H, W = g[f"block{stage}_cfg"].tolist()
            blk = _seed_module(M.Block(Cn, nH, 4, sr), f"backbone.block{stage}.0.")
            x = T(g[f"block{stage}_x"])
            for tag, xs in (("unit", x), ("small", x * 0.01)):
                y, pending = blk(xs.cuda().clone(), H, W)
                if pending is not None:
                    y = y + pending[0] + pending[1]
                _held(y, g, f"block{stage}_{tag}_out", mode, f"block sr={sr} {tag}")
        for tag, prefix in (("pe7", "backbone.patch_embed1."), ("pe3", "backbone.patch_embed2.")):
            k, s, cin, cout, H, W = g[f"{tag}_cfg"].tolist()
            pe = _seed_module(M.OverlapPatchEmbed(k, s, cin, cout), prefix)
            x = T(g[f"{tag}_x"])
            if k == 7:
                y, Ho, Wo = pe(x.cuda(), H, W, nchw_in=True)
            else:
                y, Ho, Wo = pe(x.permute(0, 2, 3, 1).reshape(x.shape[0], H * W, cin).contiguous().cuda(), H, W)
            assert Ho * Wo == g[f"{tag}_out"].shape[1]
            _held(y, g, f"{tag}_out", mode, tag)
        Cn, hidden, H, W = g["mlp_cfg"].tolist()
        mlp = _seed_module(M.Mlp(Cn, hidden), "backbone.block1.1.mlp.")
        from rba_amd import mit_ops
        h = ops.linear(T(g["mlp_x"]).cuda(), mlp.fc1)
        y = ops.linear(mit_ops.dwconv3x3_gelu(h, mlp.dwconv.taps(), mlp.dwconv.dwconv.bias, H, W), mlp.fc2)
        _held(y, g, "mlp_out", mode, "mlp")


@pytest.mark.parametrize("mode", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("name", ["tiny1_mit_b0", "tiny1_mit_b1"])
def test_tiny_mit_vs_golden(golden, name, mode):
    """the bars test_model_gpu.py::test_tiny_vs_golden applies to tiny1"""
    from rba_amd import ops
    g = golden(f"g10_{name}_60x90")
    model, a = build(name, int(g["seed"]))
    image = T(g["image"])
    sem_ref = T(g["sem_seg"])
    forgiven = torch.zeros(60 * 90, dtype=torch.bool)
    forgiven[T(g["neartie_idx"])] = True
    with ops.split_mode(mode):
        feats = model.backbone(model.preprocess([{"image": image}])[0])
        for k in A.FEATURE_NAMES:
            assert feats[k].shape[1] == a["mit"]["embed_dims"][A.FEATURE_NAMES.index(k)] and maxerr(feats[k][0], g["feat_" + k]) < 5e-5, k
        mask_cls, mask_pred, sizes, padded = model.predict([{"image": image}])
        assert sizes == [(60, 90)] and padded == (64, 96)
        assert maxerr(mask_cls[0], g["pred_logits"]) < 1e-4 and maxerr(mask_pred[0], g["pred_masks"]) < 5e-4
        for fused in (True, False):                                    # both K1 paths
            model.fused_upsample = fused
            out = model([{"image": image}], return_argmax=True)[0]
            assert out["sem_seg"].shape == (19, 60, 90)
            assert maxerr(out["sem_seg"], sem_ref) < 1e-4 and maxerr(out["rba"], g["rba"]) < 1e-4
            flips = (out["argmax"].cpu().long() != sem_ref.argmax(0)).flatten()
            assert not bool((flips & ~forgiven).any()), "argmax differs outside the stored near-tie set"
            rba, arg = model.rba_scores([{"image": image}], return_argmax=True)[0]
            assert torch.equal(rba, out["rba"]) and torch.equal(arg, out["argmax"])


def test_batch_of_two_sizes_equals_the_single_forwards(golden):
    g = golden("g10_tiny1_mit_b0_60x90")
    model, _ = build("tiny1_mit_b0", int(g["seed"]))
    gen = torch.Generator().manual_seed(4)
    ims = [T(g["image"]).cuda(), torch.randint(0, 256, (3, 33, 70), generator=gen, dtype=torch.uint8).cuda()]
    both = model.rba_scores([{"image": im} for im in ims])
    assert maxerr(both[0], g["rba"]) < 1e-4
    single = model.rba_scores([{"image": ims[1]}])[0]           # padded to 64 x 96 alone as well: the same bits
    assert both[1].shape == (33, 70) and torch.equal(both[1], single)


def test_no_library_gemm_convolution_or_attention_on_the_mit_path(monkeypatch):
    import torch.nn.functional as F
    from rba_amd import ops

    def boom(name):
        def f(*a, **k):
            raise AssertionError(f"library call on the product path: {name}")
        return f
    # the entry points test_model_gpu.py::test_no_library_gemm_or_convolution_on_any_path makes raise, for the whole forward ...
    for name in ("linear", "conv2d", "bilinear"):
        monkeypatch.setattr(F, name, boom("F." + name))
    for name in ("matmul", "bmm", "einsum"):
        monkeypatch.setattr(torch, name, boom("torch." + name))
    g = torch.Generator().manual_seed(17)
    ims = [torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8).cuda() for _ in range(2)]
    models = [build(name)[0] for name in ("tiny1_mit_b0", "tiny1_mit_b1")]
    for model in models:
        for mode in ("f16x3", "bf16x6"):
            with ops.split_mode(mode):
                both = model.rba_scores([{"image": im} for im in ims])
                assert all(torch.isfinite(b).all() for b in both)
                assert (both[1] - model.rba_scores([{"image": ims[1]}])[0]).abs().max().item() < 2e-5
    # ... and around the backbone alone also what an attention, a depthwise convolution + GELU, an unfold or a LayerNorm would go through
    with monkeypatch.context() as mp:
        for name in ("unfold", "scaled_dot_product_attention", "gelu", "layer_norm", "softmax", "pad"):
            mp.setattr(F, name, boom("F." + name))
        for name in ("softmax", "conv2d", "baddbmm", "layer_norm"):
            mp.setattr(torch, name, boom("torch." + name))
        for name in ("softmax", "matmul", "__matmul__"):
            mp.setattr(torch.Tensor, name, boom("Tensor." + name))
        for model in models:
            feats = model.backbone(model.preprocess([{"image": im} for im in ims])[0])
            assert all(torch.isfinite(f).all() for f in feats.values())


def test_graph_replay_equals_eager_bit_for_bit():
    model, _ = build("tiny1_mit_b0")
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8).cuda() for _ in range(3)]
    want = [model.rba_scores([{"image": im}], return_argmax=True)[0] for im in imgs]
    model.graph_replay = True
    for rnd in range(4):                                            # eager, capture, replay, replay
        for im, (rba0, arg0) in zip(imgs, want):
            rba, arg = model.rba_scores([{"image": im}], return_argmax=True)[0]
            assert torch.equal(rba, rba0) and torch.equal(arg, arg0), rnd
    assert model.live_graphs() == 1


def test_in_place_weight_changes_are_followed():
    """a dwconv weight and an sr weight changed in place: the cached tap-major image / Linear view are rebuilt, eagerly and under graph replay"""
    model, _ = build("tiny1_mit_b0")
    twin, _ = build("tiny1_mit_b0")
    model.graph_replay = True
    g = torch.Generator().manual_seed(5)
    im = torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8).cuda()
    first = [model.rba_scores([{"image": im}])[0].clone() for _ in range(3)][-1]
    assert torch.equal(first, twin.rba_scores([{"image": im}])[0])
    seen = [first]
    for pick in (lambda m: m.backbone.block1[0].mlp.dwconv.dwconv.weight, lambda m: m.backbone.block2[1].attn.sr.weight):
        with torch.no_grad():
            for m in (model, twin):
                pick(m).mul_(1.5)
        got = [model.rba_scores([{"image": im}])[0].clone() for _ in range(3)][-1]
        assert torch.equal(got, twin.rba_scores([{"image": im}])[0]), "the changed weight is used"
        assert not any(torch.equal(got, s) for s in seen), "the change moves the scores"
        seen.append(got)


def test_finetune_outputs_give_inferences_bits():
    model, _ = build("tiny1_mit_b0")
    g = torch.Generator().manual_seed(6)
    batch = [{"image": torch.randint(0, 256, (3, 60, 90), generator=g, dtype=torch.uint8).cuda()} for _ in range(2)]
    mask_cls, mask_pred, sizes, padded = model.predict(batch)
    model.sem_seg_head.predictor.differentiable_heads = True
    out, sizes2, padded2 = model.finetune_outputs(batch)
    assert sizes2 == sizes and tuple(padded2) == tuple(padded)
    assert torch.equal(out["pred_logits"], mask_cls) and torch.equal(out["pred_masks"], mask_pred)
    assert out["pred_logits"].requires_grad and out["pred_masks"].requires_grad


def test_evaluate_ood_cli_on_a_synthetic_mit_checkpoint(tmp_path):
    import pickle
    import yaml
    from rba_amd import evaluate_ood as E
    from tests.test_datasets_cpu import make_fs_laf, make_road_anomaly
    a = A.complete(A.ARCHS["tiny1_mit_b0"])
    mdir = tmp_path / "ckpts" / "m"
    mdir.mkdir(parents=True)
    cfg = {"MODEL": {"BACKBONE": {"NAME": "mit_b0"},
                     "SEM_SEG_HEAD": {"CONVS_DIM": 64, "MASK_DIM": 64, "TRANSFORMER_ENC_LAYERS": 2, "IN_FEATURES": ["stage1", "stage2", "stage3", "stage4"],
                                      "DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["stage4"]},
                     "MASK_FORMER": {"HIDDEN_DIM": 64, "NHEADS": 2, "NUM_OBJECT_QUERIES": 16, "DIM_FEEDFORWARD": 128, "DEC_LAYERS": 2}}}
    (mdir / "config.yaml").write_text(yaml.safe_dump(cfg))
    torch.save({"model": A.seeded_weights(a, 0)}, mdir / "model_final.pth")
    model = E.get_model(str(mdir / "config.yaml"), str(mdir / "model_final.pth"))
    assert type(model.backbone).__name__ == "mit_b0" and model.arch["enc_in"] == ["res5"]
    data = tmp_path / "data"
    make_road_anomaly(str(data), n=5, h=48, w=80)
    make_fs_laf(str(data), n=5, h=40, w=72)
    res = {}
    for graph in ("0", "1"):
        out = tmp_path / f"res_{graph}"
        E.main(["--models_folder", str(tmp_path / "ckpts"), "--datasets_folder", str(data), "--out_path", str(out), "--verbose", "0",
                "--graph", graph, "--num_workers", "2", "--streams", "2"])
        with open(out / "m" / "results.pkl", "rb") as f:
            res[graph] = pickle.load(f)
    assert res["0"] and all(abs(res["0"][d][k] - res["1"][d][k]) < 1e-12 for d in res["0"] for k in res["0"][d])
