"""MSDeformAttn pixel decoder, inference only (reference: pixel_decoder/msdeformattn.py:32-367).
Same parameter names; K2 (deformable attention) and the bilinear FPN top-down sum are HIP kernels, the 1x1 / 3x3
convolutions and the encoder FFN are this library's split-precision MFMA GEMMs / implicit GEMM (K6, conv3x3.hip) -- no rocBLAS / MIOpen call on any path (round 5)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...arch import FEATURE_NAMES, feature_channels, num_fpn_levels
from ...lru import ShapeCache, derived, source_key
from ...registry import SEM_SEG_HEADS_REGISTRY
from ..transformer_decoder.position_encoding import PositionEmbeddingSine
from .ops.ms_deform_attn import MSDeformAttn


class DeferredMaskFeatures:
    """The mask-feature map `mask_features(layer_1(y))` (reference :357-362) NOT yet computed: the raw rows of the last 3 x 3 convolution `prev` [B*P, d], their
    GroupNorm statistics `mr` [B, G, 2] and affine, the packed planes and bias of the 1 x 1 convolution, and (h, w).  The masked decoder either asks for the tensor
    (`materialize`: the launch the pixel decoder would have made, bit for bit) or -- docs/kernels/K4.md -- never builds it: `gather` projects only the rows an
    attention mask samples, `contract` folds the final einsum("bqc,bchw->bqhw") into the projection."""

    def __init__(self, prev, mr, norm, conv, planes, hw, num_groups=32, relu=True):
        self.prev, self.mr, self.norm, self.conv, self.planes, self.hw = prev, mr, norm, conv, planes, hw
        self.num_groups, self.relu = num_groups, relu
        self.batch = mr.shape[0]
        self._tensor = None

    @property
    def shape(self):
        return torch.Size((self.batch, self.conv.weight.shape[0]) + tuple(self.hw))

    @property
    def device(self):
        return self.prev.device

    @property
    def rows_per_image(self):
        return self.hw[0] * self.hw[1]

    def _project(self, planes, bias, N, rows=None):
        return ops.split_linear_nchw_out_gn_rows(self.prev, self.mr, self.norm.weight, self.norm.bias, self.num_groups, self.relu, planes, bias,
                                                 self.rows_per_image, out_features=N, rows=rows)

    def materialize(self):
        """-> mask_features [B, md, h, w], once"""
        if self._tensor is None:
            md = self.conv.weight.shape[0]
            self._tensor = ops.split_linear_nchw_out_gn(self.prev, self.mr, self.norm.weight, self.norm.bias, self.num_groups, self.relu, self.planes,
                                                        self.conv.bias, self.rows_per_image, out_features=md).view(self.shape)
        return self._tensor

    def gather(self, rows):
        """rows: ops.RowIndex [B, R] -> mask_features.flatten(2)[:, :, rows] [B, md, R], the very bits, from a projection of those rows alone"""
        return self._project(self.planes, self.conv.bias, self.conv.weight.shape[0], rows)

    def contract(self, embed):
        """embed [B, Q, md] -> einsum("bqc,bchw->bqhw", embed, mask_features) [B, Q, h, w]: the pixels contract with embed[b] @ W directly"""
        w = self.conv.weight
        planes, bias_q = ops.compose_query_operand(embed, w.detach().view(w.shape[0], -1), self.conv.bias)
        return self._project(planes, bias_q, embed.shape[1]).view((self.batch, embed.shape[1]) + tuple(self.hw))


class _LinearView:
    """A 1x1 convolution's parameters seen as an nn.Linear (weight [N,C], bias) for ops.linear."""

    def __init__(self, weight, bias):
        self.weight, self.bias = weight, bias


def _cached_linear_view(mod):
    """The nn.Linear view of a 1x1 convolution module, cached on the module per weight load."""
    w, b = mod.weight, mod.bias                    # the view holds the bias OBJECT: a replaced bias is a new key
    return derived(mod, "linear_view", (w, b), lambda: _LinearView(w.view(w.shape[0], -1), b))


def _conv3x3_planes(mod):
    """ops.conv3x3_weight of a 3x3 convolution module, one entry PER arithmetic mode: a bf16x6 re-score does not evict the f16x3 planes"""
    w = mod.weight
    return derived(mod, ("conv3x3", ops.SPLIT_MODE), (w, mod.bias), lambda: ops.conv3x3_weight(w.detach()))


def _conv1x1_nchw(x, mod):
    """1x1 convolution of an NCHW map [B,C,h,w] as the token Linear it is (``ops.linear``: the repository's kernels where they pay, a library GEMM otherwise)
    instead of a MIOpen convolution.  Why: on some MI355X boxes MIOpen's solver for the tiny test net's input projection ([1,256,4,6] x [64,256,1,1]) returned
    different last bits from one call to the next in the same process -- the first op to move in the one run-to-run difference this repository ever saw
    (tests/_optrace.py, DESIGN.md "known issue").  Only the NCHW fallback layout comes here; the channels-last path never called MIOpen."""
    B, C, h, w = x.shape
    y = ops.linear(x.permute(0, 2, 3, 1).reshape(B * h * w, C), _cached_linear_view(mod))
    return y.view(B, h, w, -1).permute(0, 3, 1, 2).contiguous()


class ConvNorm(nn.Module):
    """Detectron2 ``Conv2d`` wrapper as a parameter holder: ``weight`` (+ ``bias``) and an optional ``norm`` child
    (conv -> GroupNorm(32) -> optional ReLU), keys ``<name>.weight``, ``<name>.norm.{weight,bias}``."""

    def __init__(self, cin, cout, k, bias, norm, relu=False):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(cout, cin, k, k))
        self.bias = nn.Parameter(torch.zeros(cout)) if bias else None
        self.norm = nn.GroupNorm(32, cout) if norm else None
        self.padding, self.relu = k // 2, relu

    def forward(self, x):
        if self.padding == 0:
            x = _conv1x1_nchw(x, self)
        elif self.weight.shape[1] % 32 == 0:
            # round 5: the NCHW fallback layout's 3 x 3 convolutions run the library's own implicit-GEMM kernel too (one transpose in, one out): MIOpen -- the
            # one component that ever returned different bits from one call to the next (profiles/r04_flake_cause.txt) -- is out of the product
            y = ops.conv3x3_nhwc(x.permute(0, 2, 3, 1).contiguous(), _conv3x3_planes(self), self.bias, out_features=self.weight.shape[0])
            x = y.permute(0, 3, 1, 2).contiguous()
        else:                                                                    # (no released configuration: conv_dim is 256)
            x = F.conv2d(x, self.weight, self.bias, padding=self.padding)
        if self.norm is not None:
            return ops.group_norm(x.contiguous(), 32, self.norm.weight, self.norm.bias, self.norm.eps, relu=self.relu)
        return F.relu(x) if self.relu else x


class MSDeformAttnTransformerEncoderLayer(nn.Module):
    def __init__(self, d_model, d_ffn, n_levels, n_heads, n_points):
        super().__init__()
        self.self_attn = MSDeformAttn(d_model, n_levels, n_heads, n_points)
        self.norm1 = nn.LayerNorm(d_model)
        self.linear1 = nn.Linear(d_model, d_ffn)
        self.linear2 = nn.Linear(d_ffn, d_model)
        self.norm2 = nn.LayerNorm(d_model)

    def forward(self, src, pos, reference_points, spatial_shapes, level_start_index):
        """msdeformattn.py:131-140 (dropout = identity).  Round 4: `src + pos`, value_proj and the sampling Linears are one launch, the output
        projection carries `norm1(src + .)` and linear2 carries `norm2(src + .)` in their epilogues (csrc/token_linear.hip): 5 launches per
        layer where round 3 had 9, none of them a library GEMM."""
        src = self.self_attn(src, reference_points, src, spatial_shapes, level_start_index, query_pos=pos, post=(src, self.norm1))
        hid = ops.linear(src, self.linear1, relu=True)                        # N = d_ffn: K6
        N2, K2 = self.linear2.weight.shape
        if ops.token_linear_pays(hid.numel() // K2, N2, K2):
            return ops.token_linear(hid, self.linear2, residual=src, norm=self.norm2)
        src2 = ops.linear(hid, self.linear2, use_bias=False)
        return ops.add_layer_norm(src, self.norm2.weight, self.norm2.bias, self.norm2.eps, src2, self.linear2.bias)[1]


class MSDeformAttnTransformerEncoder(nn.Module):
    def __init__(self, layer_args, num_layers):
        super().__init__()
        self.layers = nn.ModuleList(MSDeformAttnTransformerEncoderLayer(*layer_args) for _ in range(num_layers))

    @staticmethod
    def get_reference_points(spatial_shapes, device):
        """Pixel centres (i+0.5)/H per level, broadcast over levels; valid_ratios == 1 (msdeformattn.py:149-162)."""
        refs = []
        for H_, W_ in spatial_shapes:
            ry = (torch.arange(H_, dtype=torch.float32, device=device) + 0.5) / H_
            rx = (torch.arange(W_, dtype=torch.float32, device=device) + 0.5) / W_
            refs.append(torch.stack((rx[None, :].expand(H_, W_), ry[:, None].expand(H_, W_)), -1).reshape(-1, 2))
        ref = torch.cat(refs, 0)[None]
        return ref[:, :, None, :].repeat(1, 1, len(spatial_shapes), 1).contiguous()


class MSDeformAttnTransformerEncoderOnly(nn.Module):
    def __init__(self, d_model, nhead, num_encoder_layers, dim_feedforward, num_feature_levels, enc_n_points):
        super().__init__()
        self.encoder = MSDeformAttnTransformerEncoder(
            (d_model, dim_feedforward, num_feature_levels, nhead, enc_n_points), num_encoder_layers)
        self.level_embed = nn.Parameter(torch.zeros(num_feature_levels, d_model))
        self._ref_cache = ShapeCache(8)
        self._pos_cache = ShapeCache(8)

    def forward(self, srcs, pos_embeds, tokens=None):
        """msdeformattn.py:70-98; returns (memory [B,S,C], shapes list, level_start list).  tokens: the levels as [B, h*w, C] token tensors
        when the caller has them (channels-last pixel decoder): no flatten / transpose copies."""
        dev = srcs[0].device
        shapes = [tuple(int(v) for v in s.shape[-2:]) for s in srcs]
        B = srcs[0].shape[0]
        if tokens is not None:
            src = tokens[0].contiguous() if len(tokens) == 1 else torch.cat(tokens, 1)
        else:
            src = torch.cat([s.flatten(2).transpose(1, 2) for s in srcs], 1)

        def build_pos():                # pos + level_embed depends on the shapes and on one parameter: built once per (shapes, batch, version)
            p_ = torch.cat([p.flatten(2).transpose(1, 2) + self.level_embed[l].view(1, 1, -1) for l, p in enumerate(pos_embeds)], 1)
            return p_.expand(B, -1, -1).contiguous()

        pos = self._pos_cache.get((tuple(shapes), B, dev, source_key(self.level_embed)), build_pos)

        def build():
            sh_ = torch.as_tensor(shapes, dtype=torch.long, device=dev)
            lsi_ = torch.cat((sh_.new_zeros((1,)), sh_.prod(1).cumsum(0)[:-1]))
            return sh_, lsi_, MSDeformAttnTransformerEncoder.get_reference_points(shapes, dev)

        sh, lsi, ref = self._ref_cache.get((tuple(shapes), dev), build)
        if B > 1:
            ref = ref.expand(B, -1, -1, -1).contiguous()
        out = src
        for layer in self.encoder.layers:
            out = layer(out, pos, ref, sh, lsi)
        return out, shapes


@SEM_SEG_HEADS_REGISTRY.register()
class MSDeformAttnPixelDecoder(nn.Module):
    def __init__(self, arch):
        super().__init__()
        a = arch
        d = a["conv_dim"]
        chans = feature_channels(a)
        self.in_features = list(FEATURE_NAMES)
        self.transformer_in_features = list(a["enc_in"])
        self.transformer_num_feature_levels = len(a["enc_in"])
        self.maskformer_num_feature_levels = len(a["enc_in"])
        self.input_proj = nn.ModuleList(
            nn.Sequential(nn.Conv2d(chans[f], d, kernel_size=1), nn.GroupNorm(32, d)) for f in a["enc_in"][::-1])
        self.transformer = MSDeformAttnTransformerEncoderOnly(
            d, a["nheads"], a["enc_layers"], a["enc_dim_feedforward"], len(a["enc_in"]), a["enc_points"])
        self.pe_layer = PositionEmbeddingSine(d // 2, normalize=True)
        self.mask_features = nn.Conv2d(d, a["mask_dim"], kernel_size=1)
        self.num_fpn_levels = num_fpn_levels(a)
        for j in range(1, self.num_fpn_levels + 1):
            self.add_module(f"adapter_{j}", ConvNorm(chans[FEATURE_NAMES[j - 1]], d, 1, bias=False, norm=True))
            self.add_module(f"layer_{j}", ConvNorm(d, d, 3, bias=False, norm=True, relu=True))

    # ---- channels-last (token layout) path --------------------------------------------------------------------------
    # Swin hands its feature maps over as channels-last views of [B, h*w, C] token tensors.  On that layout every 1x1
    # convolution is a Linear on the tokens and the 3x3 output convolutions are implicit GEMMs (K6, bf16x6), GroupNorm and the
    # top-down resample+add have channels-last kernels, and the mask-feature projection writes NCHW for K4: no layout
    # transposes, no MIOpen.  Same arithmetic as the NCHW path below (msdeformattn.py:323-367), which stays for other layouts.
    @staticmethod
    def _tokens(x):
        """[B,C,h,w] channels-last view -> [B, h*w, C] token view (no copy), or None for any other layout."""
        t = x.permute(0, 2, 3, 1)
        return t.reshape(x.shape[0], -1, x.shape[1]) if (x.is_cuda and x.dtype == torch.float32 and t.is_contiguous()) else None

    def _conv1x1(self, tok, mod, use_bias=True):
        """1x1 convolution of `mod` (weight [N,C,1,1]) on tokens [B,P,C] -> [B,P,N]."""
        lin = _cached_linear_view(mod)
        N, K = lin.weight.shape
        M = tok.numel() // K
        if not ops.split_linear_pays(M, N, K) and ops.token_linear_pays(M, N, K) and tok.is_contiguous():
            return ops.token_linear(tok, lin, use_bias=use_bias)              # the 2 048-token input projection of res5: was a library GEMM
        return ops.linear(tok, lin, use_bias=use_bias)

    def _channels_last_ok(self, features):
        d = self.mask_features.weight.shape[1]
        if d % 32 or (d // 32) % 4 or 256 % (d // 4) or d > 1024:
            return False
        need = set(self.transformer_in_features) | set(self.in_features[:self.num_fpn_levels])
        return all(self._tokens(features[f]) is not None and features[f].shape[1] % 32 == 0 for f in need)

    def _encode_channels_last(self, features):
        """Input projections + encoder on the token layout -> (multi-scale outs, finest encoder level as NHWC [B, h, w, d])"""
        srcs, pos, tks = [], [], []
        for idx, f in enumerate(self.transformer_in_features[::-1]):
            x = features[f]
            B, _, h, w = x.shape
            conv, gn = self.input_proj[idx][0], self.input_proj[idx][1]
            y = ops.group_norm_nhwc(self._conv1x1(self._tokens(x), conv), 32, gn.weight, gn.bias, gn.eps)
            tks.append(y.view(B, h * w, -1))
            srcs.append(y.view(B, h, w, -1).permute(0, 3, 1, 2))
            pos.append(self.pe_layer(x))
        y, shapes = self.transformer(srcs, pos, tokens=tks)
        B, d = y.shape[0], y.shape[2]
        toks = [z.contiguous() for z in torch.split(y, [h * w for h, w in shapes], dim=1)]
        # multi-scale features for the masked decoder: channels-last VIEWS of the token tensors (the decoder reads them as tokens again)
        outs = [z.view(B, h, w, d).permute(0, 3, 1, 2) for z, (h, w) in zip(toks, shapes)]
        return outs, toks[-1].view(B, *shapes[-1], d)

    def _top_down_level(self, prev, prev_norm, j, x):
        """FPN level j (reference :343-360) from the coarser level's `prev` [B, ph, pw, d] and backbone feature x -> (prev, prev_norm) of this level: the RAW
        output of its 3 x 3 convolution and (mr [B, G, 2] | None, module), the GroupNorm + ReLU its consumer applies (prev_norm None: `prev` is used as it is)."""
        B, d = prev.shape[0], prev.shape[-1]
        h, w = int(x.shape[-2]), int(x.shape[-1])
        ad, ly = getattr(self, f"adapter_{j}"), getattr(self, f"layer_{j}")
        tok = self._tokens(x)
        if tok.is_contiguous() and ops.linear_emits_gn_moments(B * h * w, d, tok.shape[-1], h * w, 32):
            # round 4: the lateral convolution's epilogue leaves the GroupNorm moments of its output -- no statistics pass over `lat`
            lat, lat_mr = ops.linear_gn_stats(tok, _cached_linear_view(ad), 32, ad.norm.eps, h * w, use_bias=False)
        else:
            lat = self._conv1x1(tok, ad, use_bias=False)                               # raw lateral convolution [B, h*w, d]
            lat_mr = ops.group_norm_nhwc_stats(lat, 32, ad.norm.eps)
        # the sum feeds only the 3x3 convolution: where that kernel takes one, written straight as its split operand (ops.SplitActivations)
        split = ops.conv3x3_takes_split(B * h * w, d) and d % 32 == 0
        yy = ops.SplitActivations.empty((B, h, w, d), prev.device) if split else None
        # round 3: both GroupNorms of the top-down step are folded into the resample kernel's loads -- the lateral's (no ReLU) into its
        # `add` operand, the previous level's (+ ReLU) into its taps: their "apply" passes (268 MB each at 256 x 512) are never run
        ups = []
        for b in range(B):
            xn = None if prev_norm is None else (prev_norm[0][b], prev_norm[1].weight, prev_norm[1].bias, True)
            ups.append(ops.resample_bilinear_nhwc_gn(prev[b], (h, w), lat[b].view(h, w, d), 32, x_norm=xn,
                                                     add_norm=(lat_mr[b], ad.norm.weight, ad.norm.bias), split_into=yy, image=b))
        if not split:
            yy = ups[0][None] if B == 1 else torch.stack(ups)
        planes = _conv3x3_planes(ly)
        if split and ops.conv3x3_emits_gn_moments(B, h, w, d, 32):
            prev, mr = ops.conv3x3_nhwc_gn_stats(yy, planes, 32, ly.norm.eps, None, out_features=d)     # round 4: statistics from the convolution's epilogue
            return prev, (mr, ly.norm)
        prev = ops.conv3x3_nhwc(yy, planes, None, out_features=d)
        # the last level's GroupNorm is applied inside the mask-feature projection, which takes its statistics where it needs them
        return prev, (ops.group_norm_nhwc_stats(prev.flatten(1, 2), 32, ly.norm.eps) if j > 1 else None, ly.norm)

    def _mask_features(self, prev, prev_norm, defer):
        """mask_features(ReLU(GroupNorm(prev))) (reference :357-362) of the last level's raw rows -> [B, md, h, w], or a DeferredMaskFeatures"""
        B, ph, pw, d = prev.shape
        mr, norm = prev_norm
        mfw = self.mask_features.weight
        planes = derived(self.mask_features, ("mf_planes", ops.SPLIT_MODE), (mfw, self.mask_features.bias),      # per arithmetic form (f16x3 since round 3)
                         lambda: ops.split_weight(mfw.detach().view(mfw.shape[0], -1).contiguous()))
        if ops.split_linear_nchw_out_takes_gn(planes, ph * pw, d, 32):
            # round 4: the last level's GroupNorm + ReLU feeds only the mask-feature projection -- applied inside that kernel's loads, the
            # normalised 1/4-resolution map (134 MB at 1024 x 2048) is never written or read back
            if mr is None:
                mr = ops.group_norm_nhwc_stats(prev.flatten(1, 2), 32, norm.eps)
            mf = DeferredMaskFeatures(prev.view(B * ph * pw, d), mr, norm, self.mask_features, planes, (ph, pw), num_groups=32, relu=True)
            # deferred: the masked decoder decides whether the map is ever written; materialize() is the one launch site of the folded projection
            return mf if defer else mf.materialize()
        prev = ops.group_norm_nhwc(prev.flatten(1, 2), 32, norm.weight, norm.bias, norm.eps, relu=True)
        return ops.split_linear_nchw_out(prev.view(B * ph * pw, d), planes, self.mask_features.bias, ph * pw,
                                         out_features=mfw.shape[0]).view(B, mfw.shape[0], ph, pw)

    def _forward_features_channels_last(self, features, defer_mask_features=False):
        outs, prev = self._encode_channels_last(features)
        prev_norm = None
        for j in range(self.num_fpn_levels, 0, -1):
            prev, prev_norm = self._top_down_level(prev, prev_norm, j, features[self.in_features[j - 1]])
        return self._mask_features(prev, prev_norm, defer_mask_features), outs[0], outs[:self.maskformer_num_feature_levels]

    def forward_features(self, features, defer_mask_features=False):
        """-> (mask_features [B,md,H/4,W/4], out[0], multi_scale_features) (msdeformattn.py:323-367).  ``defer_mask_features`` (the head passes it for a
        predictor that takes one): mask_features may come back as a DeferredMaskFeatures instead -- only where the GroupNorm-folded projection applies."""
        if self.num_fpn_levels > 0 and self._channels_last_ok(features):
            return self._forward_features_channels_last(features, defer_mask_features)
        srcs, pos = [], []
        for idx, f in enumerate(self.transformer_in_features[::-1]):
            x = features[f].float().contiguous()                       # (channels-last views from Swin are copied to NCHW here)
            conv, gn = self.input_proj[idx][0], self.input_proj[idx][1]
            srcs.append(ops.group_norm(_conv1x1_nchw(x, conv), 32, gn.weight, gn.bias, gn.eps))
            pos.append(self.pe_layer(x))
        y, shapes = self.transformer(srcs, pos)
        B = y.shape[0]
        outs = [z.transpose(1, 2).reshape(B, -1, shapes[i][0], shapes[i][1]).contiguous()
                for i, z in enumerate(torch.split(y, [h * w for h, w in shapes], dim=1))]
        for idx, f in enumerate(self.in_features[:self.num_fpn_levels][::-1]):
            j = self.num_fpn_levels - idx
            cur = getattr(self, f"adapter_{j}")(features[f].float().contiguous())
            yy = ops.resample_bilinear(outs[-1], cur.shape[-2:], add=cur.contiguous())   # :357-358 fused sum
            outs.append(getattr(self, f"layer_{j}")(yy))
        mf = _conv1x1_nchw(outs[-1], self.mask_features)
        return mf, outs[0], outs[:self.maskformer_num_feature_levels]
