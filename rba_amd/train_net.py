"""The fine-tune trainer: the reference's ``train_net.py`` loop (Detectron2's SimpleTrainer / DefaultTrainer behind ``Trainer``) for the three head fine-tune
recipes, on this library's differentiable heads, criteria, device mapper and K15 optimizer step.

    python -m rba_amd.train_net --config-file RECIPE.yaml --cityscapes_root DIR [--coco_root DIR] [--resume] [KEY VALUE ...]
    python -m torch.distributed.run --nproc_per_node N -m rba_amd.train_net ...          # IMS_PER_BATCH / N images per rank, one all_reduce per step

An iteration is ``finetune_outputs`` -> ``prepare_targets`` -> the recipe's criterion -> ``backward`` -> ``all_reduce_grads`` -> ``optimizer.step``.  Nothing
is read back except every ``log_period`` iterations (loss and gradient norm; a non-finite value raises FloatingPointError there).  Checkpoints
(``model_%07d.pth`` every SOLVER.CHECKPOINT_PERIOD iterations, ``model_final.pth`` at the end) hold tensors and numbers only, and the resolved
``config.yaml`` is written beside them, so the output folder is a model folder of ``evaluate_ood`` / ``evaluate_semseg`` as it is.
"""
import argparse
import collections
import itertools
import logging
import math
import os
import re
from concurrent.futures import ThreadPoolExecutor

import torch
import yaml

from .config import load_cfg

logger = logging.getLogger(__name__)


class _WeightedLoss:
    """a one-loss recipe (DenseHybrid) with the interface of the criteria: ``__call__`` -> the loss dict, ``weighted`` -> times weight_dict"""

    def __init__(self, loss, weight_dict):
        self.loss, self.weight_dict = loss, dict(weight_dict)

    def __call__(self, outputs, targets):
        return self.loss(outputs, targets)

    def weighted(self, losses):
        return {k: v * self.weight_dict[k] for k, v in losses.items() if k in self.weight_dict}


def criterion_for_recipe(cfg):
    """The criterion maskformer_model.py:112-195 builds for the cfg's loss flags, from the three builders of rba_amd.modeling.criterion:
    DENSE_HYBRID_LOSS -> the densehybrid loss alone (it displaces every other loss there); GAMBLER_LOSS -> PebalCriterion; else SetCriterion."""
    from .modeling import criterion as K
    mf = cfg.MODEL.MASK_FORMER
    if mf.get("DENSE_HYBRID_LOSS", False):
        return _WeightedLoss(K.densehybrid_loss_from_cfg(cfg), {"densehybrid_loss": float(mf.get("DENSE_HYBRID_WEIGHT", 1.0))})
    if mf.get("GAMBLER_LOSS", False):
        return K.pebal_criterion_from_cfg(cfg)
    return K.criterion_from_cfg(cfg)


def _plain(x):
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    return x


_CKPT = re.compile(r"model_(\d{7})\.pth$")


def last_checkpoint(output_dir):
    """-> the path of the newest ``model_%07d.pth`` of the folder (a finished run's ``model_final.pth`` repeats the last of them), or None"""
    found = sorted(f for f in os.listdir(output_dir) if _CKPT.match(f)) if os.path.isdir(output_dir) else []
    return os.path.join(output_dir, found[-1]) if found else None


class Trainer:
    """``data``: ``data(iteration)`` -> this rank's batch of mapper dicts, a function of the iteration so that a resumed run sees the batches of the
    uninterrupted one.  ``criterion``: ``criterion(outputs, targets)`` -> the loss dict, summed through its ``weighted`` when it has one (SetCriterion,
    PebalCriterion, the DenseHybrid wrapper), else as it is (a bare loss such as ``outlier_loss_from_cfg``'s)."""

    def __init__(self, cfg, model, criterion, data, optimizer, scheduler, output_dir, log_period=20):
        self.cfg, self.model, self.criterion, self.data, self.optimizer, self.scheduler = cfg, model, criterion, data, optimizer, scheduler
        self.output_dir, self.log_period = output_dir, int(log_period)
        self.max_iter, self.checkpoint_period = int(cfg.SOLVER.MAX_ITER), int(cfg.SOLVER.CHECKPOINT_PERIOD)
        self.iteration = 0
        self.last_loss = self.last_lr = None
        import torch.distributed as dist
        self.rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0

    def step(self):
        batch = self.data(self.iteration)
        outputs, _, padded = self.model.finetune_outputs(batch)
        targets = self.model.prepare_targets(batch, padded)
        losses = self.criterion(outputs, targets)
        weighted = self.criterion.weighted(losses) if hasattr(self.criterion, "weighted") else losses
        total = sum(weighted.values())
        self.optimizer.zero_grad()
        total.backward()
        self.optimizer.all_reduce_grads()
        self.last_lr = self.scheduler.lr(self.iteration)
        self.optimizer.step(self.last_lr)
        self.last_loss = total.detach()
        self.iteration += 1
        if self.log_period > 0 and self.iteration % self.log_period == 0:
            self.log()

    def log(self):
        """the one read-back: the last iteration's weighted loss and gradient norm"""
        loss, norm = float(self.last_loss), float(self.optimizer.grad_norm)
        if not (math.isfinite(loss) and math.isfinite(norm)):
            raise FloatingPointError(f"iteration {self.iteration}: loss {loss}, gradient norm {norm}")
        if self.rank == 0:
            logger.info("iter %d  loss %.6g  grad_norm %.4g  lr %.6g", self.iteration, loss, norm, self.last_lr)
        return loss, norm

    def train(self):
        if self.rank == 0:
            self.write_config()
        while self.iteration < self.max_iter:
            self.step()
            if self.checkpoint_period > 0 and self.iteration % self.checkpoint_period == 0:
                self.save(f"model_{self.iteration:07d}.pth")
        if self.log_period > 0:
            self.log()
        self.save(f"model_{self.iteration:07d}.pth")
        self.save("model_final.pth")

    def write_config(self):
        os.makedirs(self.output_dir, exist_ok=True)
        with open(os.path.join(self.output_dir, "config.yaml"), "w") as f:
            yaml.safe_dump(_plain(self.cfg), f)

    def save(self, name):
        """{"model", "optimizer", "iteration"}: tensors and numbers only, so ``read_state_dict``'s default (weights_only) path loads it"""
        if self.rank != 0:
            return None
        os.makedirs(self.output_dir, exist_ok=True)
        path = os.path.join(self.output_dir, name)
        state = {"model": {k: v.detach().cpu() for k, v in self.model.state_dict().items()}, "optimizer": self.optimizer.state_dict(),
                 "iteration": self.iteration}
        torch.save(state, path + ".tmp")
        os.replace(path + ".tmp", path)
        return path

    def resume(self, path=None):
        """continue from ``path`` (default: the folder's last checkpoint; none: start from the beginning) -> the iteration resumed at"""
        path = path or last_checkpoint(self.output_dir)
        if path is None:
            return 0
        state = torch.load(path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(state["model"])               # copies in place: the optimizer's pointers stay, the version counters move
        self.optimizer.load_state_dict(state["optimizer"])
        self.iteration = int(state["iteration"])
        return self.iteration


# ---------------------------------------------------------------------------------------------------------------- the command line
def training_indices(size, seed, rank=0, world=1, shuffle=True):
    """Detectron2's ``TrainingSampler``: an infinite stream of seeded permutations of range(size), one after another, of which this rank takes every
    world-th index starting at its own."""
    def infinite():
        g = torch.Generator()
        g.manual_seed(int(seed))
        while True:
            yield from (torch.randperm(size, generator=g) if shuffle else torch.arange(size)).tolist()
    return itertools.islice(infinite(), rank, None, world)


class CityscapesTrainStream:
    """``stream(iteration)`` -> this rank's batch: Cityscapes train frames in TrainingSampler order, decoded ahead on a host thread pool, each through
    the COCO-mix mapper on the device.  The mapper's draws are seeded by (seed, rank, iteration), so a resumed run repeats the uninterrupted one."""

    def __init__(self, cfg, dataset, coco, device, per_rank, seed=0, rank=0, world=1, num_workers=8, start_iteration=0):
        import random

        import numpy as np
        from .dataset_mappers import MaskFormerSemanticCocoMixDatasetMapper
        self.dataset, self.per_rank, self.seed, self.rank = dataset, int(per_rank), int(seed), int(rank)
        self._np, self._random = np, random
        self.mapper = MaskFormerSemanticCocoMixDatasetMapper(cfg, device=device, coco=coco, lut=dataset.lut)
        self.indices = training_indices(len(dataset), seed, rank, world)
        for _ in range(start_iteration * self.per_rank):
            next(self.indices)
        self.next_iteration = start_iteration
        self.pool = ThreadPoolExecutor(max_workers=max(1, min(16, int(num_workers))))
        self.pending = collections.deque()
        self.depth = 2 * self.per_rank

    def _fill(self):
        while len(self.pending) < self.depth:
            self.pending.append(self.pool.submit(self.dataset.raw_item, next(self.indices)))

    def __call__(self, iteration):
        if iteration != self.next_iteration:
            raise ValueError(f"the stream is at iteration {self.next_iteration}, asked for {iteration}")
        self.next_iteration += 1
        key = (self.seed * 1000003 + iteration) * 4099 + self.rank
        self.mapper.np_rng, self.mapper.py_rng = self._np.random.RandomState(key % (1 << 32)), self._random.Random(key)
        batch = []
        for _ in range(self.per_rank):
            self._fill()
            image, label = self.pending.popleft().result()
            batch.append(self.mapper({"image": image.permute(2, 0, 1).contiguous(), "sem_seg_gt": label}))
        return batch


def build_parser():
    p = argparse.ArgumentParser(description="Fine-tune the prediction heads by one of the reference's recipes (rba_amd)")
    p.add_argument("--config-file", required=True)
    p.add_argument("--cityscapes_root", required=True, help="the folder that holds leftImg8bit/ and gtFine/")
    p.add_argument("--coco_root", default=None, help="the folder that holds train2017/ and annotations/ood_seg_train2017/ (default: "
                                                     "$DETECTRON2_DATASETS/INPUT.COCO_ROOT)")
    p.add_argument("--output_dir", default=None, help="default: the cfg's OUTPUT_DIR, else ./output")
    p.add_argument("--resume", action="store_true")
    p.add_argument("--differentiable_decoder", action="store_true",
                   help="train whatever the cfg leaves trainable inside the transformer decoder (the released PEBAL recipe: all of it; "
                        "FREEZE_TRANSFORMER_DECODER_EXCEPT_OBJECT_QUERIES: the queries); without it such a cfg is refused")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--num_workers", type=int, default=8, help="image-decoding threads (at most 16)")
    p.add_argument("--log_period", type=int, default=20)
    p.add_argument("--device", default="cuda")
    p.add_argument("--dist_backend", default=None, choices=[None, "nccl", "gloo"])
    p.add_argument("opts", nargs=argparse.REMAINDER, help="KEY VALUE pairs overlaid on the config")
    return p


def main(argv=None):
    from . import distributed as D
    from .checkpoint import load_checkpoint
    from .dataset_mappers import CocoOodObjects
    from .evaluate_ood import build_model
    from .sem_seg_datasets import CityscapesSemSeg
    from .solver import WarmupPolyLR, build_optimizer
    args = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    rank, world, local = D.init_from_env(args.dist_backend)
    cfg = load_cfg(args.config_file, args.opts)
    ims = int(cfg.SOLVER.IMS_PER_BATCH)
    if ims % world:
        raise ValueError(f"SOLVER.IMS_PER_BATCH {ims} is not divisible by the world size {world}")
    device = torch.device(args.device, local) if args.device == "cuda" else torch.device(args.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    output_dir = args.output_dir or cfg.get("OUTPUT_DIR", None) or "output"
    model = build_model(cfg)
    weights = cfg.MODEL.get("WEIGHTS", "")
    if weights and os.path.exists(weights):
        load_checkpoint(model, weights, trusted=os.environ.get("RBA_TRUSTED_CHECKPOINT") == "1")
    elif rank == 0:
        logger.info("MODEL.WEIGHTS %r not found: training from the model's initial weights", weights)
    model.to(device)
    model.graph_replay = False
    optimizer = build_optimizer(cfg, model, differentiable_decoder=args.differentiable_decoder)      # after .to(device): the step holds the parameters' device pointers
    scheduler, criterion = WarmupPolyLR(cfg), criterion_for_recipe(cfg)
    trainer = Trainer(cfg, model, criterion, None, optimizer, scheduler, output_dir, log_period=args.log_period)
    start = trainer.resume() if args.resume else 0
    dataset = CityscapesSemSeg(args.cityscapes_root, "train")
    s = cfg.INPUT
    coco_root = args.coco_root or os.path.join(os.getenv("DETECTRON2_DATASETS", "datasets"), s.COCO_ROOT)
    import random
    coco = CocoOodObjects(coco_root, int(s.COCO_PROXY_SIZE), py_rng=random.Random(args.seed), ood_label=int(s.OOD_LABEL))
    trainer.data = CityscapesTrainStream(cfg, dataset, coco, device, ims // world, seed=args.seed, rank=rank, world=world,
                                         num_workers=args.num_workers, start_iteration=start)
    try:
        trainer.train()
    finally:
        trainer.data.pool.shutdown(wait=False, cancel_futures=True)
        if world > 1:
            torch.distributed.barrier()
            torch.distributed.destroy_process_group()
    return trainer


if __name__ == "__main__":
    main()
