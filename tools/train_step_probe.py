#!/usr/bin/env python3
"""Time one Trainer.step() of the PEBAL recipe on swin_b_1dl (seeded weights, synthetic 512 x 1024 batch of 2): heads only
(FREEZE_TRANSFORMER_DECODER_EXCEPT_MLP) and with the whole transformer decoder trainable (the released recipe, differentiable_decoder).
Host clock around steps that end in a device synchronise; median of 10 after 3 warm-up steps.  A record for docs/measurements.md, not a bar."""
import os
import pathlib
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import _solver_cases as C  # noqa: E402

H, W = 512, 1024


def batch(iteration, device="cuda"):
    from rba_amd.dataset_mappers import Instances
    gen = torch.Generator().manual_seed(4242 + iteration)
    out = []
    for _ in range(2):
        image = torch.randint(0, 256, (3, H, W), generator=gen, dtype=torch.uint8)
        sem = torch.randint(0, 8, (H // 32, W // 32), generator=gen).repeat_interleave(32, 0).repeat_interleave(32, 1)
        sem[torch.rand(H, W, generator=gen) < 0.1] = 255
        sem[200:300, 300:500] = 254
        outlier = torch.where(sem == 255, 255, torch.where(sem == 254, 1, 0))
        classes = torch.tensor([c for c in range(19) if bool((sem == c).any())], dtype=torch.int64)
        inst = Instances((H, W), classes, sem[None] == classes[:, None, None])
        out.append({"image": image.to(device), "sem_seg": sem.to(device), "outlier_mask": outlier.to(device), "instances": inst.to(device)})
    return out


def run(tmp, whole):
    from rba_amd.solver import WarmupPolyLR, build_optimizer
    from rba_amd.train_net import Trainer, criterion_for_recipe
    cfg = C.recipe_cfg(tmp, C.RECIPES["pebal"][0], ["SOLVER.MAX_ITER", "100"] + ([] if whole else C.PEBAL_OPTS))
    model = C.tiny("swin_b_1dl").cuda().eval()
    model.graph_replay = False
    opt = build_optimizer(cfg, model, differentiable_decoder=whole)
    batches = [batch(i) for i in range(4)]
    t = Trainer(cfg, model, criterion_for_recipe(cfg), lambda it: batches[it % 4], opt, WarmupPolyLR(cfg), str(tmp / "out"), log_period=0)
    ts = []
    for i in range(13):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t.step()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return len(opt.names), ts[len(ts) // 2], ts[0], ts[-1], float(t.last_loss)


def main():
    assert torch.cuda.is_available(), "the probe needs a HIP device"
    torch.backends.cuda.matmul.allow_tf32 = False
    with tempfile.TemporaryDirectory() as d:
        for whole in (False, True):
            n, med, lo, hi, loss = run(pathlib.Path(d) / ("whole" if whole else "heads"), whole)
            print(f"swin_b_1dl PEBAL step, 2 x 512 x 1024, {'whole decoder' if whole else 'heads only'}: {n} trained tensors, "
                  f"{med:.1f} ms median of 10 [{lo:.1f} .. {hi:.1f}], last loss {loss:.4f}", flush=True)


if __name__ == "__main__":
    main()
