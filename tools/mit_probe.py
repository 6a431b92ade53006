"""K19 timing probe (docs/kernels/K19.md): the three MiT kernels at the full-size stage shapes of mit_b5 at 1024 x 2048, each against its torch
composition on the same device in the same run, and images/s of `mit_b5_1dl` at 1024 x 2048 through MaskFormer.rba_scores.

    python tools/mit_probe.py [--launches 30] [--warmup 5] [--out FILE] [--no-model]

Runs on an MI355X only.  Each launch is bracketed by its own pair of HIP events on the current stream; after the warm-up launches, `--launches` timed
launches, the median and the minimum are reported (an event pair includes the launch's own cost).  The torch compositions get their best layout
(NCHW-contiguous inputs for conv2d and unfold, pre-split q / k / v for the attention): matmul + softmax + matmul, conv2d(groups=C) + gelu, F.unfold.
Results are compared before anything is timed.  The model figure is a host clock around `--launches` eager forwards that end in a synchronise."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

H, W = 1024, 2048
# mit_b5 (mix_transformer.py:479-484): (stage, map, C, heads, sr)
STAGES = [(1, (H // 4, W // 4), 64, 1, 8), (2, (H // 8, W // 8), 128, 2, 4), (3, (H // 16, W // 16), 320, 5, 2), (4, (H // 32, W // 32), 512, 8, 1)]
PEAK_FP32_MFMA = 157.3e12


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return {"median_us": round(float(np.median(us)), 1), "min_us": round(float(us.min()), 1)}


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("--launches", type=int, default=30)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--out", default=None, help="also write the JSON lines to this file")
    p.add_argument("--no-model", action="store_true")
    args = p.parse_args(argv)
    from rba_amd import arch as A, mit_ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(0)
    lines = []

    def emit(**row):
        lines.append(row)
        print(json.dumps(row), flush=True)

    def both(kernel, torch_fn, check):
        got, want = kernel(), torch_fn()
        err = check(got, want)
        k = timed(kernel, args.launches, args.warmup)
        del got, want
        t = timed(torch_fn, args.launches, args.warmup)
        return k, t, err

    for stage, (h, w), C, nH, sr in STAGES:
        N, S, hd = h * w, (h // sr) * (w // sr), C // nH
        # K19a
        q = torch.randn(1, N, C, device=dev, generator=g)
        kv = torch.randn(1, S, 2 * C, device=dev, generator=g)
        q4 = q.view(1, N, nH, hd).transpose(1, 2).contiguous()
        k4 = kv.view(1, S, 2, nH, hd)[:, :, 0].transpose(1, 2).contiguous()
        v4 = kv.view(1, S, 2, nH, hd)[:, :, 1].transpose(1, 2).contiguous()
        k, t, err = both(lambda: mit_ops.sr_attention(q, kv, nH),
                         lambda: torch.matmul(torch.softmax(torch.matmul(q4, k4.transpose(-2, -1)) * hd ** -0.5, dim=-1), v4),
                         lambda a, b: (a.view(1, N, nH, hd).transpose(1, 2) - b).abs().max().item())
        flops = 4.0 * N * S * hd * nH
        emit(kernel="K19a sr_attention", stage=stage, N=N, S=S, heads=nH, head_dim=hd, k19=k, torch_composition=t, max_abs_diff=err,
             gflop=round(flops / 1e9, 1), tflops=round(flops / k["median_us"] / 1e6, 1), of_fp32_mfma_peak=round(flops / k["median_us"] / 1e-6 / PEAK_FP32_MFMA, 3),
             speedup_median=round(t["median_us"] / k["median_us"], 2))
        del q, kv, q4, k4, v4
        # K19b
        Ch = 4 * C
        x = torch.randn(1, N, Ch, device=dev, generator=g)
        wt = torch.randn(Ch, 1, 3, 3, device=dev, generator=g) / 3
        b = torch.randn(Ch, device=dev, generator=g) * 0.05
        w9 = mit_ops.dwconv_taps(wt)
        xn = x.transpose(1, 2).reshape(1, Ch, h, w).contiguous()
        k, t, err = both(lambda: mit_ops.dwconv3x3_gelu(x, w9, b, h, w), lambda: F.gelu(F.conv2d(xn, wt, b, padding=1, groups=Ch)),
                         lambda a, c: (a.view(1, h, w, Ch).permute(0, 3, 1, 2) - c).abs().max().item())
        byt = 8.0 * N * Ch
        emit(kernel="K19b dwconv3x3_gelu", stage=stage, map=[h, w], C=Ch, k19=k, torch_composition=t, max_abs_diff=err, mbytes_floor=round(byt / 1e6, 1),
             gbytes_per_s=round(byt / k["median_us"] / 1e3, 1), speedup_median=round(t["median_us"] / k["median_us"], 2))
        del x, xn, wt, w9
        # K19c: this stage's patch embedding (from the previous stage's map) and its sr convolution
        windows = [("patch_embed", (7, 4, 3) if stage == 1 else (3, 2, 1), (H, W) if stage == 1 else (2 * h, 2 * w), 3 if stage == 1 else STAGES[stage - 2][2])]
        if sr > 1:
            windows.append(("attn.sr", (sr, sr, 0), (h, w), C))
        for what, (kk, st, pd), (ih, iw), ci in windows:
            xn = torch.randn(1, ci, ih, iw, device=dev, generator=g)
            xt = xn if ci == 3 else xn.permute(0, 2, 3, 1).reshape(1, ih * iw, ci).contiguous()
            Kp = mit_ops.padded_columns(kk, ci)

            def check(a, u):
                u = u.view(1, ci, kk * kk, -1).permute(0, 3, 2, 1).reshape(1, -1, kk * kk * ci)
                return float(not torch.equal(a[0][..., : kk * kk * ci], u))
            k, t, err = both(lambda: mit_ops.im2col_nhwc(xt, ih, iw, kk, st, pd, nchw_in=ci == 3), lambda: F.unfold(xn, kk, padding=pd, stride=st), check)
            rows = mit_ops.conv_out_size(ih, kk, st, pd) * mit_ops.conv_out_size(iw, kk, st, pd)
            emit(kernel="K19c im2col_nhwc", stage=stage, what=what, window=[kk, st, pd], map=[ih, iw], C=ci, Kp=Kp, cols_mbytes=round(4.0 * rows * Kp / 1e6, 1),
                 k19=k, torch_composition=t, mismatch=err, gbytes_per_s_written=round(4.0 * rows * Kp / k["median_us"] / 1e3, 1),
                 speedup_median=round(t["median_us"] / k["median_us"], 2))
            del xn, xt
        torch.cuda.empty_cache()

    if not args.no_model:
        from rba_amd.checkpoint import load_checkpoint
        from rba_amd.maskformer_model import MaskFormer
        a = A.complete(A.ARCHS["mit_b5_1dl"])
        model = load_checkpoint(MaskFormer(a), A.seeded_weights(a, 0)).to(dev).eval()
        model.graph_replay = False
        image = torch.randint(0, 256, (3, H, W), dtype=torch.uint8, device=dev)
        for _ in range(3):
            rba = model.rba_scores([{"image": image}])[0]
        torch.cuda.synchronize()
        ts = []
        for _ in range(10):
            t0 = time.perf_counter()
            model.rba_scores([{"image": image}])
            torch.cuda.synchronize()
            ts.append(time.perf_counter() - t0)
        emit(model="mit_b5_1dl", image=[H, W], path="rba_scores, eager, one stream", ms_median=round(1e3 * float(np.median(ts)), 2), ms_min=round(1e3 * min(ts), 2),
             images_per_s=round(1.0 / float(np.median(ts)), 2), finite=bool(torch.isfinite(rba).all()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.writelines(json.dumps(ln) + "\n" for ln in lines)


if __name__ == "__main__":
    main()
