"""Test helper of the composed mask head: seeded operands of the mask-feature projection and its float64 restatement (shared by the GPU test files)."""
import torch

G = 32
EPS = 1e-5


def operands(B, P, K, C, Q, seed, device="cuda", embed_std=2.0):
    """y [B*P, K] ~ N(0, 1) raw convolution rows with their REAL GroupNorm statistics, a GroupNorm affine, the 1 x 1 convolution W [C, K] / bias [C] and
    mask embeddings E [B, Q, C] ~ N(0, embed_std^2)"""
    from rba_amd import ops
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)
    o = dict(y=r(B * P, K), gamma=1.0 + 0.25 * r(K), beta=0.25 * r(K), W=r(C, K) / K ** 0.5, bias=0.5 * r(C), E=embed_std * r(B, Q, C))
    o = {k: v.to(device).contiguous() for k, v in o.items()}
    o["mr"] = ops.group_norm_nhwc_stats(o["y"].view(B, P, K), G, EPS)
    o["planes"] = ops.split_weight(o["W"], "f16x3")
    o.update(B=B, P=P, K=K, C=C, Q=Q)
    return o


def normalised64(y, mr, gamma, beta, B, relu=True):
    """ReLU(GroupNorm(y)) in float64 from the (mean, rstd) the kernels are handed: [B, P, K]"""
    K = y.shape[1]
    x = y.double().cpu().view(B, -1, K)
    m = mr.double().cpu()
    a = gamma.double().cpu().view(1, K) * m[:, :, 1].repeat_interleave(K // G, dim=1)        # [B, K]
    b = beta.double().cpu().view(1, K) - m[:, :, 0].repeat_interleave(K // G, dim=1) * a
    g = x * a[:, None, :] + b[:, None, :]
    return g.clamp_min(0) if relu else g


def logits64(y, mr, gamma, beta, W, bias, E, B):
    """einsum("bqc,bcp->bqp", E, W g + bias) in float64 -> [B, Q, P]"""
    g = normalised64(y, mr, gamma, beta, B)
    mf = torch.einsum("bpk,ck->bcp", g, W.double().cpu())
    if bias is not None:
        mf = mf + bias.double().cpu().view(1, -1, 1)
    return torch.einsum("bqc,bcp->bqp", E.double().cpu(), mf)
