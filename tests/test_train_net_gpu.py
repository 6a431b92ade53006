"""rba_amd.train_net.Trainer on the device, tiny1 / tiny3 / tiny1_dh at 60 x 90: the head tensors after three iterations against the float64 restatement fed
the recorded gradients, the schedule's learning rates, the step that inference sees (the stale-cache trap), the checkpoint a fresh model loads, the full
criteria of the recipes, the DenseHybrid recipe's trainable set, and a resumed run that repeats the uninterrupted one in every bit."""
import math
import os

import pytest
import torch

from tests import _solver_cases as C

pytestmark = pytest.mark.gpu

H, W = 60, 90
SHORT = ["SOLVER.MAX_ITER", "3", "SOLVER.CHECKPOINT_PERIOD", "2"]


def _batch(iteration, device="cuda"):
    """two mapper-like dicts, seeded by the iteration: image, sem_seg (classes 0..18, 254 = pasted outlier, 255 = void), outlier_mask, instances"""
    from rba_amd.dataset_mappers import Instances
    gen = torch.Generator().manual_seed(4242 + iteration)
    batch = []
    for _ in range(2):
        image = torch.randint(0, 256, (3, H, W), generator=gen, dtype=torch.uint8)
        sem = torch.randint(0, 4, (H // 10, W // 10), generator=gen).repeat_interleave(10, 0).repeat_interleave(10, 1)      # coarse class regions
        r = torch.rand(H, W, generator=gen)
        sem[r < 0.1] = 255
        sem[20:35, 30:50] = 254
        outlier = torch.where(sem == 255, 255, torch.where(sem == 254, 1, 0))
        classes = torch.tensor([c for c in range(19) if bool((sem == c).any())], dtype=torch.int64)
        inst = Instances((H, W), classes, sem[None] == classes[:, None, None])
        batch.append({"image": image.to(device), "sem_seg": sem.to(device), "outlier_mask": outlier.to(device), "instances": inst.to(device)})
    return batch


def _trainer(tmp_path, recipe, arch, criterion="recipe", opts=(), out="run"):
    from rba_amd.modeling.criterion import outlier_loss_from_cfg
    from rba_amd.solver import WarmupPolyLR, build_optimizer
    from rba_amd.train_net import Trainer, criterion_for_recipe
    cfg = C.recipe_cfg(tmp_path, C.RECIPES[recipe][0], SHORT + list(opts))
    model = C.tiny(arch).cuda().eval()
    model.graph_replay = False
    opt = build_optimizer(cfg, model)
    crit = outlier_loss_from_cfg(cfg) if criterion == "outlier" else criterion_for_recipe(cfg)
    return Trainer(cfg, model, crit, _batch, opt, WarmupPolyLR(cfg), str(tmp_path / out), log_period=1)


def _heads(opt):
    return [p.detach().cpu().clone() for p in opt.params]


def test_three_outlier_iterations_against_the_restatement(tmp_path):
    from rba_amd import arch as A
    from rba_amd.checkpoint import load_checkpoint, read_state_dict
    from rba_amd.maskformer_model import MaskFormer
    t = _trainer(tmp_path, "coco_mix", "tiny1", criterion="outlier")
    opt, model = t.optimizer, t.model
    probe = [{"image": _batch(99)[0]["image"]}]
    logits0, masks0, _, _ = model.predict(probe)
    p0 = _heads(opt)
    seen, step = [], opt.step

    def recording_step(lr):
        seen.append((lr, [g.detach().cpu().clone() for g in opt._slices(opt.grad)], [p._version for p in opt.params]))
        step(lr)
    opt.step = recording_step
    t.train()
    assert t.iteration == 3 and len(seen) == 3
    # the schedule, exactly: WARMUP_ITERS 0, power 0.9, MAX_ITER 3
    assert [s[0] for s in seen] == [1e-4 * 1.0 * (1.0 - i / 3) ** 0.9 for i in range(3)]
    assert all(float(torch.cat([g.flatten() for g in s[1]]).norm()) > 0 for s in seen)
    grads, lrs = [s[1] for s in seen], [s[0] for s in seen]
    got = (_heads(opt), [m.cpu() for m in opt._slices(opt.exp_avg)], [v.cpu() for v in opt._slices(opt.exp_avg_sq)], None)
    before = C.restate64(p0, grads, lrs[:2], 0.01, 1.0, opt.weight_decays, opt.lr_mults)[0]
    kw = dict(weight_decays=opt.weight_decays, lr_mults=opt.lr_mults)
    t64 = C.restate64(p0, grads, lrs, 0.01, 1.0, **kw)
    t32 = C.torch32(p0, grads, lrs, 0.01, 1.0, **kw)
    # the last update, taken on every side against the restatement's parameters after two steps
    got = got[:3] + ([p.double() - b for p, b in zip(got[0], before)],)
    t32 = t32[:3] + ([p.double() - b for p, b in zip(t32[0], before)],)
    b = [[C.err(a, a64) for a, a64 in zip(q32, q64)] for q32, q64 in zip(t32, t64)]
    C.check("trainer", got, t64, b, names=[n.rsplit("predictor.", 1)[1] for n in opt.names])
    assert all(v1 > v0 for s0, s1 in zip(seen, seen[1:]) for v0, v1 in zip(s0[2], s1[2]))
    # the step reaches inference (packed weights are keyed on the version counters) ...
    logits1, masks1, _, _ = model.predict(probe)
    assert not torch.equal(logits1, logits0) and not torch.equal(masks1, masks0)
    # ... and the written folder is a model folder: model_final.pth through the default (weights_only) reader, config.yaml beside it
    final = os.path.join(t.output_dir, "model_final.pth")
    assert sorted(os.listdir(t.output_dir)) == ["config.yaml", "model_0000002.pth", "model_0000003.pth", "model_final.pth"]
    sd = read_state_dict(final)
    assert all(isinstance(v, torch.Tensor) for v in sd.values())
    a = A.complete(A.ARCHS["tiny1"])
    fresh = load_checkpoint(MaskFormer(a), final).cuda().eval()
    logits2, masks2, _, _ = fresh.predict(probe)
    assert torch.equal(logits2, logits1) and torch.equal(masks2, masks1)
    from rba_amd.config import load_cfg
    assert load_cfg(os.path.join(t.output_dir, "config.yaml")).SOLVER.MAX_ITER == 3


@pytest.mark.parametrize("recipe, arch, opts", [
    ("coco_mix", "tiny3", ["MODEL.MASK_FORMER.DEC_LAYERS", "5"]),
    ("pebal", "tiny3", C.PEBAL_OPTS + ["MODEL.MASK_FORMER.DEC_LAYERS", "5"]),
], ids=["labels_masks_outlier", "pebal"])
def test_the_recipes_criteria_run_with_finite_losses(tmp_path, recipe, arch, opts):
    t = _trainer(tmp_path, recipe, arch, opts=opts)
    p0 = _heads(t.optimizer)
    for _ in range(3):
        t.step()                                                   # log_period 1: a non-finite loss or norm raises FloatingPointError here
        assert math.isfinite(float(t.last_loss)) and float(t.optimizer.grad_norm) > 0
    assert all(not torch.equal(a, b) for a, b in zip(p0, _heads(t.optimizer)))


def test_densehybrid_recipe_moves_the_heads_and_nothing_frozen(tmp_path):
    t = _trainer(tmp_path, "densehybrid", "tiny1_dh")
    names = set(t.optimizer.names)
    assert len(names) == 12 and sum("ood_pred" in n for n in names) == 4
    before = {k: v.detach().clone() for k, v in t.model.state_dict().items()}
    for _ in range(3):
        t.step()
    after = t.model.state_dict()
    for k, v in before.items():
        if k in names:
            assert not torch.equal(after[k], v), k
        else:
            assert torch.equal(after[k], v), k


def test_resume_repeats_the_uninterrupted_run(tmp_path):
    # (the outlier loss: every kernel on its path is bitwise reproducible; the matcher and loss_masks draw random points)
    a = _trainer(tmp_path, "coco_mix", "tiny1", criterion="outlier", out="a")
    a.train()
    b = _trainer(tmp_path, "coco_mix", "tiny1", criterion="outlier", out="b")
    assert b.resume(os.path.join(a.output_dir, "model_0000002.pth")) == 2 and b.optimizer.step_count == 2
    b.train()
    assert b.iteration == 3
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert torch.equal(a.optimizer.exp_avg, b.optimizer.exp_avg) and torch.equal(a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq)
    # and from the folder itself, as --resume does
    from rba_amd.train_net import last_checkpoint
    assert os.path.basename(last_checkpoint(a.output_dir)) == "model_0000003.pth"


# ---- the command line on a synthetic Cityscapes + COCO tree, the model shrunk to tiny1's sizes through KEY VALUE pairs
TINY_OPTS = ["MODEL.SWIN.EMBED_DIM", "32", "MODEL.SWIN.DEPTHS", "[2, 2, 2, 2]", "MODEL.SWIN.NUM_HEADS", "[1, 2, 4, 8]", "MODEL.SWIN.WINDOW_SIZE", "6",
             "MODEL.SEM_SEG_HEAD.CONVS_DIM", "64", "MODEL.SEM_SEG_HEAD.MASK_DIM", "64", "MODEL.SEM_SEG_HEAD.TRANSFORMER_ENC_LAYERS", "2",
             "MODEL.MASK_FORMER.HIDDEN_DIM", "64", "MODEL.MASK_FORMER.NUM_OBJECT_QUERIES", "16", "MODEL.MASK_FORMER.NHEADS", "2",
             "MODEL.MASK_FORMER.DIM_FEEDFORWARD", "128", "MODEL.WEIGHTS", "",
             # the whole 64 x 128 frame with an object pasted into every image: the DenseHybrid loss is NaN (the reference's too) on a batch without an outlier pixel,
             # and the trainer raises FloatingPointError there, as it should
             "INPUT.MIN_SIZE_TRAIN", "[64]", "INPUT.MAX_SIZE_TRAIN", "256", "INPUT.CROP.ENABLED", "True", "INPUT.CROP.TYPE", "absolute",
             "INPUT.CROP.SIZE", "[64, 128]", "INPUT.COLOR_AUG_SSD", "True", "INPUT.FORMAT", "RGB", "INPUT.OOD_PROB", "1.0",
             "SOLVER.IMS_PER_BATCH", "2", "SOLVER.CHECKPOINT_PERIOD", "2"]


def _write_trees(root):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(5)
    for i in range(5):
        for kind, sub in (("leftImg8bit", "leftImg8bit"), ("gtFine", "gtFine")):
            os.makedirs(root / "cityscapes" / sub / "train" / "aachen", exist_ok=True)
        stem = f"aachen_{i:06d}_000019"
        Image.fromarray(rng.integers(0, 256, (64, 128, 3), dtype=np.uint8)).save(root / "cityscapes" / "leftImg8bit" / "train" / "aachen" / f"{stem}_leftImg8bit.png")
        lab = np.repeat(np.repeat(rng.integers(0, 5, (8, 16), dtype=np.uint8), 8, 0), 8, 1)
        lab[:4] = 255
        Image.fromarray(lab).save(root / "cityscapes" / "gtFine" / "train" / "aachen" / f"{stem}_gtFine_labelTrainIds.png")
    os.makedirs(root / "coco" / "annotations" / "ood_seg_train2017")
    os.makedirs(root / "coco" / "train2017")
    for i in range(3):
        m = np.zeros((30, 40), dtype=np.uint8)
        m[3 + i:17, 5:21 + i] = 254
        Image.fromarray(m).save(root / "coco" / "annotations" / "ood_seg_train2017" / f"{i:012d}.png")
        Image.fromarray(rng.integers(0, 256, (30, 40, 3), dtype=np.uint8)).save(root / "coco" / "train2017" / f"{i:012d}.jpg", quality=95)


@pytest.mark.parametrize("recipe", ["coco_mix", "densehybrid", "pebal"])
def test_command_line_trains_resumes_and_leaves_a_model_folder(tmp_path, recipe):
    from rba_amd import evaluate_ood as E
    from rba_amd import train_net
    _write_trees(tmp_path)
    C.recipe_cfg(tmp_path, C.RECIPES[recipe][0])                                       # writes the recipe and its _BASE_ chain
    config = str(tmp_path / "a" / "b" / os.path.basename(C.RECIPES[recipe][0]))
    out = str(tmp_path / "out" / "model")
    argv = ["--config-file", config, "--cityscapes_root", str(tmp_path / "cityscapes"), "--coco_root", str(tmp_path / "coco"), "--output_dir", out,
            "--num_workers", "2", "--log_period", "1"]
    opts = TINY_OPTS + (C.PEBAL_OPTS if recipe == "pebal" else [])
    t = train_net.main(argv + opts + ["SOLVER.MAX_ITER", "3"])
    assert t.iteration == 3 and sorted(os.listdir(out)) == ["config.yaml", "model_0000002.pth", "model_0000003.pth", "model_final.pth"]
    assert len(t.optimizer.names) == (12 if recipe == "densehybrid" else 8)
    # the folder is a model folder of the evaluators as it is
    model = E.get_model(os.path.join(out, "config.yaml"), os.path.join(out, "model_final.pth"), device="cuda")
    sd, trained = model.state_dict(), t.model.state_dict()
    assert all(torch.equal(sd[k], trained[k]) for k in trained)
    image = torch.randint(0, 256, (3, H, W), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).cuda()
    assert bool(torch.isfinite(model.rba_scores([{"image": image}])[0]).all())
    # --resume picks the last checkpoint up and goes on to the new MAX_ITER
    t2 = train_net.main(argv + ["--resume"] + opts + ["SOLVER.MAX_ITER", "4"])
    assert t2.iteration == 4 and t2.optimizer.step_count == 4 and os.path.exists(os.path.join(out, "model_0000004.pth"))
    assert any(not torch.equal(t2.model.state_dict()[n], trained[n]) for n in t.optimizer.names)


def test_command_line_refuses_a_batch_the_world_does_not_divide(tmp_path, monkeypatch):
    from rba_amd import distributed as D
    from rba_amd import train_net
    C.recipe_cfg(tmp_path, C.RECIPES["coco_mix"][0])
    config = str(tmp_path / "a" / "b" / os.path.basename(C.RECIPES["coco_mix"][0]))
    monkeypatch.setattr(D, "init_from_env", lambda backend=None: (0, 3, 0))
    with pytest.raises(ValueError, match="IMS_PER_BATCH 16 is not divisible by the world size 3"):
        train_net.main(["--config-file", config, "--cityscapes_root", str(tmp_path)])
