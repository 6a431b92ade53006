"""Which C entry points a Swin stage and the pixel decoder's channels-last path launch, in order, at the smallest shapes that select each launch path of
`SwinTransformerBlock.forward` (attention half A1 K7 block / A2 K7 qkv / A3 unfused; MLP half M1 .. M6) and of the FPN top-down step.  The expected lists are
literals recorded from the commit before the two functions were restated: a rewrite of the model code that selects kernels must reproduce them unchanged.
Entry-point names, not op names, tell the paths apart (M4 and M6 make the same seven op calls)."""
import contextlib
from collections import Counter

import pytest
import torch

pytestmark = pytest.mark.gpu


class _Recorder:
    """stands in for the ctypes handle of the kernel library: forwards every call, keeps the names of the launches (host-side queries are not launches)"""

    def __init__(self, lib):
        self._lib, self.names = lib, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name.endswith(("_bytes", "_elems", "_supported")) or "_workspace_" in name:
            return fn

        def forward(*args):
            self.names.append(name)
            return fn(*args)
        return forward


@contextlib.contextmanager
def _recording():
    from rba_amd import _lib
    rec = _Recorder(_lib.load())
    prev, _lib._lib = _lib._lib, rec
    try:
        yield rec.names
    finally:
        _lib._lib = prev


def _launches(run):
    """(result, [entry point, ...]) of run()'s second call: the first one packs the weights (once per weight load and arithmetic mode)"""
    with torch.no_grad():
        run()
        with _recording() as names:
            out = run()
    torch.cuda.synchronize()
    print(names)
    return out, names


# ---- Swin: one stage of two blocks (the second one shifted), fed as D2SwinTransformer._stages feeds it ---------------------------------------------------------

LN, LN_FRAG = "rba_add_layer_norm_f32", "rba_add_layer_norm_frag_f32"
GEMM, GEMM_RES, GEMM_FRAG, GEMM_GELU_SPLIT = ("rba_split_linear_f16x3_f32", "rba_split_linear_f16x3_res_f32", "rba_split_linear_f16x3_frag_f32",
                                              "rba_split_linear_f16x3_gelu_split_out")
GEMM_BF16 = "rba_split_linear_f32"
K5, K5_SPLIT = "rba_swin_window_attn_f32", "rba_swin_window_attn_split_out_f32"
K7_BLOCK, K7_QKV = "rba_swin_attn_block_f32", "rba_swin_attn_qkv_split_out_f32"
MLP, MLP_LN = "rba_swin_mlp_fused_f16x3_f32", "rba_swin_mlp_fused_ln_f16x3_f32"

SWIN_CASES = {
    # id: (dim, H, W, SWIN_ATTN_FUSED, split mode, launches of block 0 + launches of block 1, fc2 left pending)
    "1-A1-M1": (128, 128, 256, True, "f16x3", [K7_BLOCK, MLP_LN] * 2, False),
    "2-A1-M2": (128, 90, 90, True, "f16x3", [K7_BLOCK, GEMM_GELU_SPLIT, GEMM_FRAG] * 2, False),
    "3-A1-M3": (128, 24, 36, True, "f16x3", [K7_BLOCK, GEMM, GEMM] * 2, True),
    "4-A2-M4": (256, 63, 64, True, "f16x3", [K7_QKV, GEMM_FRAG, LN_FRAG, GEMM_GELU_SPLIT, GEMM_FRAG] * 2, False),
    # C = 192 has K < 256: proj takes a split operand only from 160 tiles of 128 x 128 on (2 column tiles: more than 79 * 128 rows)
    "5-A2-M4-swin-l": (192, 101, 101, True, "f16x3", [K7_QKV, GEMM_FRAG, LN_FRAG, GEMM_GELU_SPLIT, GEMM_FRAG] * 2, False),
    "6-A3-M6": (256, 24, 36, True, "f16x3", [LN_FRAG, GEMM_FRAG, K5, GEMM, LN, GEMM, GEMM] * 2, True),
    "7-A3-K5split-M4": (512, 44, 44, True, "f16x3", [LN_FRAG, GEMM_FRAG, K5_SPLIT, GEMM_FRAG, LN_FRAG, GEMM_GELU_SPLIT, GEMM_FRAG] * 2, False),
    "8-A3-M5": (128, 128, 256, False, "f16x3", [LN_FRAG, GEMM_FRAG, K5_SPLIT, GEMM_FRAG, LN, MLP] * 2, False),
    "9-A3-M6-bf16x6": (128, 90, 90, True, "bf16x6", [LN, GEMM_BF16, K5, GEMM_BF16, LN, GEMM_BF16, GEMM_BF16] * 2, True),
    "10-A3-K5rows-M4": (192, 63, 64, True, "f16x3", [LN_FRAG, GEMM_FRAG, K5, GEMM_RES, LN_FRAG, GEMM_GELU_SPLIT, GEMM_FRAG] * 2, False),
}


@pytest.mark.parametrize("case", list(SWIN_CASES))
def test_swin_stage_launches(case, monkeypatch):
    from rba_amd import ops
    from rba_amd.modeling.backbone.swin import BasicLayer
    from rba_amd.seeded_weights import fill_state_dict_
    dim, H, W, k7, mode, want, want_pending = SWIN_CASES[case]
    monkeypatch.setattr(ops, "SWIN_ATTN_FUSED", k7)
    layer = BasicLayer(dim, 2, dim // 32, 12, 4.0, downsample=False).cuda().eval()
    fill_state_dict_(layer, 0, prefix="backbone.layers.0.")
    x0 = torch.randn(1, H * W, dim, generator=torch.Generator().manual_seed(5)).cuda()

    def run():
        x, pending = x0.clone(), None                              # (the residual stream is updated in place)
        for blk in layer.blocks:
            x, pending = blk(x, H, W, pending)
        return x, pending

    with ops.split_mode(mode):
        (x, pending), got = _launches(run)
    assert got == want
    assert x.shape == (1, H * W, dim) and bool(torch.isfinite(x).all())
    assert (pending is not None) == want_pending
    if pending is not None:
        t, tb = pending
        assert t.shape == x.shape and tb.shape == (dim,) and bool(torch.isfinite(t).all())


# ---- pixel decoder: swin_b_1dl's, on synthetic channels-last feature views -----------------------------------------------------------------------------------

GN, GN_STATS, GN_MERGE = "rba_group_norm_nhwc_f32", "rba_group_norm_nhwc_stats_f32", "rba_group_norm_nhwc_merge_f32"
RESAMPLE = "rba_resample_bilinear_nhwc_gn_f32"
CONV, CONV_SPLIT, CONV_SPLIT_MOM, CONV_BF16 = ("rba_conv3x3_nhwc_f16x3_f32", "rba_conv3x3_nhwc_f16x3_split_in_f32",
                                               "rba_conv3x3_nhwc_f16x3_split_in_gn_moments_f32", "rba_conv3x3_nhwc_f32")
GEMM_MOM = "rba_split_linear_f16x3_gn_moments_f32"
MF, MF_BF16, MF_GN = "rba_split_linear_nchw_out_f16x3_f32", "rba_split_linear_nchw_out_f32", "rba_split_linear_nchw_out_gn_f16x3_f32"
TOKEN, TOKEN_MULTI, MSDA = "rba_token_linear_f32", "rba_token_linear_multi_f32", "rba_msda_fused_f32"

# res4 and res3 on fp32 rows: lateral (res4's few rows on the token kernel), its statistics, folded resample, 3x3, its statistics
FPN_ROWS = [TOKEN, GN_STATS, RESAMPLE, CONV, GN_STATS, GEMM, GN_STATS, RESAMPLE, CONV, GN_STATS]

PD_CASES = {
    # id: (image-equivalent H, W, batch, defer, split mode, launches after the encoder)
    "a-512x512": (512, 512, 1, False, "f16x3", FPN_ROWS + [GEMM_MOM, GN_MERGE, RESAMPLE, CONV_SPLIT_MOM, GN_MERGE, MF_GN]),
    "b-deferred": (512, 512, 1, True, "f16x3", FPN_ROWS + [GEMM_MOM, GN_MERGE, RESAMPLE, CONV_SPLIT_MOM, GN_MERGE]),
    "c-480x800": (480, 800, 1, False, "f16x3", FPN_ROWS + [GEMM, GN_STATS, RESAMPLE, CONV_SPLIT, GN, MF]),
    "d-bf16x6": (512, 512, 1, False, "bf16x6", [GEMM_BF16, GN_STATS, RESAMPLE, CONV_BF16, GN_STATS] * 2 + [GEMM_BF16, GN_STATS, RESAMPLE, CONV_BF16, GN, MF_BF16]),
    "a-batch-of-2": (512, 512, 2, False, "f16x3", [TOKEN, GN_STATS, RESAMPLE, RESAMPLE, CONV, GN_STATS, GEMM, GN_STATS, RESAMPLE, RESAMPLE, CONV, GN_STATS]
                     + [GEMM_MOM, GN_MERGE, RESAMPLE, RESAMPLE, CONV_SPLIT_MOM, GN_MERGE, MF_GN]),
}
# res5's input projection + GroupNorm and the six encoder layers, per arithmetic mode
PD_ENCODER = {"f16x3": [TOKEN, GN] + [TOKEN_MULTI, MSDA, TOKEN, GEMM, TOKEN] * 6,
              "bf16x6": [GEMM_BF16, GN] + [GEMM_BF16, GEMM_BF16, MSDA, GEMM_BF16, LN, GEMM_BF16, GEMM_BF16, LN] * 6}


@pytest.fixture(scope="module")
def pixel_decoder():
    from rba_amd import arch as A
    from rba_amd.modeling.pixel_decoder.msdeformattn import MSDeformAttnPixelDecoder
    from rba_amd.seeded_weights import fill_state_dict_
    a = A.complete(A.ARCHS["swin_b_1dl"])
    pd = MSDeformAttnPixelDecoder(a).cuda().eval()
    fill_state_dict_(pd, 0, meta=dict(n_heads=a["nheads"], n_points=a["enc_points"]), prefix="sem_seg_head.pixel_decoder.")
    return pd, a


@pytest.mark.parametrize("case", list(PD_CASES))
def test_pixel_decoder_launches(case, pixel_decoder):
    from rba_amd import arch as A, ops
    from rba_amd.modeling.pixel_decoder.msdeformattn import DeferredMaskFeatures
    pd, a = pixel_decoder
    H, W, B, defer, mode, want = PD_CASES[case]
    g = torch.Generator().manual_seed(9)
    feats = {}
    for f, C in A.feature_channels(a).items():
        h, w = H // A.FEATURE_STRIDES[f], W // A.FEATURE_STRIDES[f]
        feats[f] = torch.randn(B, h * w, C, generator=g).cuda().view(B, h, w, C).permute(0, 3, 1, 2)
    assert pd._channels_last_ok(feats)
    with ops.split_mode(mode):
        (mf, out0, ms), got = _launches(lambda: pd.forward_features(feats, defer_mask_features=defer))
    assert got == PD_ENCODER[mode] + want
    if B == 2:                                                     # against the B = 1 list: the folded resample is launched per image, everything else once for the batch
        one, two = Counter(PD_ENCODER[mode] + PD_CASES["a-512x512"][5]), Counter(got)
        assert set(one) == set(two)
        for name, n in one.items():
            assert two[name] == (2 * n if name == RESAMPLE else n), name
    d, md = a["conv_dim"], a["mask_dim"]
    assert mf.shape == (B, md, H // 4, W // 4)
    if defer:
        assert isinstance(mf, DeferredMaskFeatures)
        assert bool(torch.isfinite(mf.prev).all()) and bool(torch.isfinite(mf.mr).all())
    else:
        assert isinstance(mf, torch.Tensor) and bool(torch.isfinite(mf).all())
    assert out0.shape == (B, d, H // 32, W // 32) and bool(torch.isfinite(out0).all())
    assert len(ms) == 1 and ms[0] is out0
