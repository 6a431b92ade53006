"""Inputs and truth of tests/test_decoder_backward_gpu.py: the whole transformer decoder on seeded random multi-scale features, differentiated on
the CPU through oracle.ref_model.transformer_decoder (every head call reached through taps["aux"]).  Test infrastructure, not product code.

The decoder thresholds its attention-mask logits (sigmoid < 0.5): a decision, not arithmetic.  Two precisions can only be compared where they
decide alike, so the feature seed of each model is CHOSEN (searched once on the CPU with the oracle, `python -m tests._decoder_bwd_cases`) such
that every thresholded logit of every head call keeps |x| >= MARGIN in double; the test asserts it before it compares anything."""
import copy

import torch

from oracle import ref_model
from tests._msda_cases import bar, err           # noqa: F401

MARGIN = 1e-3
P = "sem_seg_head.predictor"
B = 2
MASK_HW = (16, 24)
# model -> (arch name, dec_layers override | None, feature seed); "tiny3_1dl": three levels, one layer -- levels 1 and 2 are never visited
MODELS = {"tiny3": ("tiny3", None, 11), "tiny1": ("tiny1", None, 1), "tiny3_1dl": ("tiny3", 1, 4)}


def arch(model):
    from rba_amd import arch as A
    name, layers, _ = MODELS[model]
    a = copy.deepcopy(A.ARCHS[name])
    if layers is not None:
        a["dec_layers"] = layers
    return A.complete(a)


def level_sizes(a):
    n = len(a["enc_in"])
    return [(MASK_HW[0] // 8 * 2 ** i, MASK_HW[1] // 8 * 2 ** i) for i in range(n)] if n > 1 else [(MASK_HW[0] // 8, MASK_HW[1] // 8)]


def make(model, seed=None):
    """-> (arch, state dict (seeded weights), multi-scale features [B,C,h,w] coarse to fine, mask features [B,md,16,24], functional weights): CPU fp32.
    The functional: one (w_cls [B,Q,K+1], w_mask [B,Q,16,24]) pair per head call, the last pair for the final outputs."""
    from rba_amd import arch as A
    a = arch(model)
    sd = A.seeded_weights(a, 0)
    g = torch.Generator().manual_seed(MODELS[model][2] if seed is None else seed)
    x = [torch.randn(B, a["conv_dim"], h, w, generator=g) for h, w in level_sizes(a)]
    mf = torch.randn(B, a["mask_dim"], *MASK_HW, generator=g)
    Q, K = a["num_queries"], a["num_classes"]
    wts = [(torch.randn(B, Q, K + 1, generator=g), torch.randn(B, Q, *MASK_HW, generator=g) / 16) for _ in range(a["dec_layers"] + 1)]
    return a, sd, x, mf, wts


def functional(calls, wts):
    """calls: [(class logits, mask logits)] per head call, the final one last"""
    return sum((c * wc.to(c)).sum() + (m * wm.to(m)).sum() for (c, m), (wc, wm) in zip(calls, wts))


def cpu_grads(a, sd, x, mf, wts, dtype):
    """-> ({predictor parameter name: gradient}, [thresholded attention-mask logits per head call]) through the oracle in `dtype`"""
    torch.set_default_dtype(dtype)
    try:
        sdd = {k: (v.to(dtype).clone().requires_grad_(True) if k.startswith(P + ".") and v.is_floating_point() else v) for k, v in sd.items()}
        taps = {}
        ref_model.transformer_decoder([t.to(dtype) for t in x], mf.to(dtype), sdd, a, p=P, taps=taps)
        functional([(c, m) for c, m, _ in taps["aux"]], wts).backward()
        grads = {k[len(P) + 1:]: v.grad for k, v in sdd.items() if isinstance(v, torch.Tensor) and v.requires_grad and v.grad is not None}
        return grads, [t.detach() for t in taps["am_logits"]]
    finally:
        torch.set_default_dtype(torch.float32)


def margin_ok(am_logits):
    return all(float(t.abs().min()) >= MARGIN for t in am_logits)


if __name__ == "__main__":
    for model in MODELS:
        for seed in range(200):
            a, sd, x, mf, wts = make(model, seed)
            with torch.no_grad():
                torch.set_default_dtype(torch.float64)
                try:
                    taps = {}
                    ref_model.transformer_decoder([t.double() for t in x], mf.double(), {k: v.double() if v.is_floating_point() else v for k, v in sd.items()},
                                                  a, p=P, taps=taps)
                finally:
                    torch.set_default_dtype(torch.float32)
            if margin_ok(taps["am_logits"]):
                print(model, "seed", seed, "min |logit|", min(float(t.abs().min()) for t in taps["am_logits"]),
                      "blocked share", [round(float((t.sigmoid() < 0.5).float().mean()), 3) for t in taps["am_logits"]])
                break
        else:
            print(model, "no seed below 200")
