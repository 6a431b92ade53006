"""Test infrastructure of K19 and the MiT backbone (not product code): a functional torch restatement of the reference's MixVisionTransformer
(mask2former/modeling/backbone/mix_transformer.py) over a flat state dict with its key names, in the style of oracle/ref_model.py -- it runs in
the dtype of the tensors it is handed, so the same code gives the fp32 composition and the float64 truth -- plus the input generators and
float64 truths of the kernel tests.  Pinned by tests/golden/g10_*.npz, which the reference's own module wrote (tests/test_mit_cpu.py)."""
import torch
import torch.nn.functional as F

BLOCK_EPS, PLAIN_EPS = 1e-6, 1e-5          # partial(nn.LayerNorm, eps=1e-6) of the blocks and stage norms (:399); nn.LayerNorm's default elsewhere (:81, :179)


def _ln(x, sd, p, eps):
    return F.layer_norm(x, (x.shape[-1],), sd[p + ".weight"], sd[p + ".bias"], eps)


def _lin(x, sd, p):
    return F.linear(x, sd[p + ".weight"], sd[p + ".bias"])


def cast(sd, dtype):
    return {k: v.to(dtype) if v.dtype.is_floating_point else v for k, v in sd.items()}


# ---------------------------------------------------------------------------------------------------------------- the network
def attention(y, H, W, sd, p, num_heads, sr):
    """Attention.forward (:100-121) on y = norm1(x) [B,N,C]"""
    B, N, C = y.shape
    hd = C // num_heads
    q = _lin(y, sd, p + ".q").view(B, N, num_heads, hd).transpose(1, 2)
    if sr > 1:
        m = F.conv2d(y.transpose(1, 2).reshape(B, C, H, W), sd[p + ".sr.weight"], sd[p + ".sr.bias"], stride=sr)
        y = _ln(m.flatten(2).transpose(1, 2), sd, p + ".norm", PLAIN_EPS)
    kv = _lin(y, sd, p + ".kv").view(B, -1, 2, num_heads, hd)
    k, v = kv[:, :, 0].transpose(1, 2), kv[:, :, 1].transpose(1, 2)
    a = torch.softmax(q @ k.transpose(-2, -1) * hd ** -0.5, dim=-1)
    return _lin((a @ v).transpose(1, 2).reshape(B, N, C), sd, p + ".proj")


def mlp(y, H, W, sd, p):
    """Mlp.forward (:52-59): fc1, depthwise 3x3 on the map, GELU, fc2"""
    B, N, _ = y.shape
    h = _lin(y, sd, p + ".fc1")
    C = h.shape[-1]
    m = F.conv2d(h.transpose(1, 2).reshape(B, C, H, W), sd[p + ".dwconv.dwconv.weight"], sd[p + ".dwconv.dwconv.bias"], padding=1, groups=C)
    return _lin(F.gelu(m.flatten(2).transpose(1, 2)), sd, p + ".fc2")


def block(x, H, W, sd, p, num_heads, sr):
    """Block.forward (:157-161)"""
    x = x + attention(_ln(x, sd, p + ".norm1", BLOCK_EPS), H, W, sd, p + ".attn", num_heads, sr)
    return x + mlp(_ln(x, sd, p + ".norm2", BLOCK_EPS), H, W, sd, p + ".mlp")


def patch_embed(x, sd, p, k, stride):
    """OverlapPatchEmbed.forward (:198-204): x [B,Cin,H,W] -> tokens, H', W'"""
    m = F.conv2d(x, sd[p + ".proj.weight"], sd[p + ".proj.bias"], stride=stride, padding=k // 2)
    return _ln(m.flatten(2).transpose(1, 2), sd, p + ".norm", PLAIN_EPS), m.shape[2], m.shape[3]


def backbone(x, sd, mit, p="backbone"):
    """MixVisionTransformer.forward_features (:334-370) -> {"res2".."res5"} (the reference's stage1..stage4)"""
    outs = {}
    for s in range(4):
        t, H, W = patch_embed(x, sd, f"{p}.patch_embed{s + 1}", 7 if s == 0 else 3, 4 if s == 0 else 2)
        for i in range(mit["depths"][s]):
            t = block(t, H, W, sd, f"{p}.block{s + 1}.{i}", mit["num_heads"][s], mit["sr_ratios"][s])
        t = _ln(t, sd, f"{p}.norm{s + 1}", BLOCK_EPS)
        x = t.view(x.shape[0], H, W, -1).permute(0, 3, 1, 2).contiguous()
        outs[f"res{s + 2}"] = x
    return outs


# ---------------------------------------------------------------------------------------------------------------- K19a
ATTN_HEAD_DIMS, ATTN_HEADS, ATTN_BATCHES = (32, 64), (1, 2, 5), (1, 2)
ATTN_N, ATTN_S = (1, 31, 64, 65, 129), (1, 6, 63, 64, 65, 130)
ATTN_BOUND = 1e-5          # absolute, K5_BOUND's bar for the same distribution (tests/test_attention_kernel_fuzz_gpu.py)


def attn_case(B, N, S, nH, hd, seed=0):
    """q [B,N,nH*hd], kv [B,S,2*nH*hd] randn, then three planted query rows of (batch 0, head 0), each on the unit key direction it needs:
    row 0: one key of the LAST key tile scores +40 (the running maximum moves in the last tile: every earlier tile is rescaled);
    row 1 (N > 1): every score is about -80;
    row 2 (N > 2): |q . k| * scale about 30 on one key.
    Keys are left as drawn except the planted ones, which are unit vectors scaled so the products come out as stated."""
    g = torch.Generator().manual_seed(1000 * seed + 131 * N + 17 * S + 7 * nH + hd + B)
    C = nH * hd
    q = torch.randn(B, N, C, generator=g)
    kv = torch.randn(B, S, 2 * C, generator=g)
    scale = hd ** -0.5
    last = S - 1 - ((S - 1) % 32) // 2                 # a key inside the last tile of 32
    u = torch.zeros(hd)
    u[3] = 1.0
    kv[0, last, :hd] = u * 4.0                           # k = 4 e3
    q[0, 0, :hd] = u * (40.0 / 4.0 / scale)              # q . k * scale = +40
    if N > 1:                                            # q = -c * mean direction of the keys' first coordinate block: push every score to about -80
        kv[0, :, 5] = 2.0                                # every key of head 0 has k[5] = 2
        q[0, 1, :hd] = 0.0
        q[0, 1, 5] = -80.0 / 2.0 / scale
    if N > 2:
        first = 0 if last != 0 else S - 1
        kv[0, first, :hd] = 0.0
        kv[0, first, 7] = 3.0
        if N > 1:
            kv[0, first, 5] = 2.0
        q[0, 2, :hd] = 0.0
        q[0, 2, 7] = 30.0 / 3.0 / scale
    return q, kv


def attn_truth(q, kv, nH):
    """float64 softmax(q k^T * hd^-0.5) v, head-major (:113-117)"""
    B, N, C = q.shape
    hd = C // nH
    q64 = q.double().view(B, N, nH, hd).transpose(1, 2)
    kv64 = kv.double().view(B, -1, 2, nH, hd)
    k, v = kv64[:, :, 0].transpose(1, 2), kv64[:, :, 1].transpose(1, 2)
    a = torch.softmax(q64 @ k.transpose(-2, -1) * hd ** -0.5, dim=-1)
    return (a @ v).transpose(1, 2).reshape(B, N, C)


# ---------------------------------------------------------------------------------------------------------------- K19b
DW_MAPS, DW_CHANNELS, DW_BATCHES = ((1, 1), (1, 7), (7, 1), (2, 3), (5, 9), (16, 24)), (4, 128, 132), (1, 2)


def dwconv_case(B, H, W, C, seed=0):
    """x [B,H*W,C] randn with image 1 (where there is one) a constant 1e3: a row of it leaking into image 0's bottom padding moves image 0 by ~1e3"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * W + C + B)
    x = torch.randn(B, H * W, C, generator=g)
    if B > 1:
        x[1] = 1e3
    return x, torch.randn(C, 1, 3, 3, generator=g) / 3.0, 0.05 * torch.randn(C, generator=g)


def dwconv_compose(x, weight, bias, H, W):
    """GELU(depthwise3x3(x) + bias) as the reference composes it (:53-55, :384-390), in x's dtype"""
    B, _, C = x.shape
    m = F.conv2d(x.transpose(1, 2).reshape(B, C, H, W), weight.to(x.dtype), bias.to(x.dtype), padding=1, groups=C)
    return F.gelu(m.flatten(2).transpose(1, 2))


# ---------------------------------------------------------------------------------------------------------------- K19c
IM2COL_WINDOWS = ((7, 4, 3), (3, 2, 1), (8, 8, 0), (4, 4, 0), (2, 2, 0))
IM2COL_MAPS, IM2COL_CHANNELS, IM2COL_BATCHES = ((1, 1), (5, 7), (16, 24), (17, 25)), (3, 32, 160), (1, 2)


def im2col_case(B, H, W, C, seed=0):
    """x NCHW [B,C,H,W] randn (the test hands the kernel its channels-last token view, or, for C = 3, the tensor itself)"""
    g = torch.Generator().manual_seed(1000 * seed + 97 * H + 13 * W + C + B)
    return torch.randn(B, C, H, W, generator=g)


def im2col_reference(x, k, stride, pad, Kp):
    """F.unfold's columns (c, ky, kx) re-ordered to (ky, kx, c) and zero-padded to Kp -> [B, Ho*Wo, Kp]; [B, 0, Kp] where no window fits"""
    B, C, H, W = x.shape
    if H + 2 * pad < k or W + 2 * pad < k:
        return torch.zeros(B, 0, Kp)
    u = F.unfold(x, k, padding=pad, stride=stride)                        # [B, C*k*k, L]
    u = u.view(B, C, k * k, -1).permute(0, 3, 2, 1).reshape(B, -1, k * k * C)
    return F.pad(u, (0, Kp - k * k * C))
