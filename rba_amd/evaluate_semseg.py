"""Closed-set evaluation from the command line: Cityscapes mIoU / fwIoU / mACC / pACC of every model folder, the number BASELINE.md and MODEL_ZOO.md
list beside the OoD metrics (the reference gets it from Detectron2's SemSegEvaluator through ``train_net.py --eval-only``, :96-121, 138-148).

    python -m rba_amd.evaluate_semseg --models_folder ckpts/ --cityscapes_root /data/cityscapes [--split val] [--tta]

Flags are named as ``rba_amd.evaluate_ood``'s.  Per image: one forward (``MaskFormer.rba_scores(return_argmax=True)``, or the ``--tta`` wrapper's), one
launch of K13 on the int32 argmax map and the label map; nothing is read back until the end.  Under ``torch.distributed.run`` the images are sharded
over the ranks and the matrices summed with one all_reduce.  Rank 0 writes ``<out_path>/<model>/sem_seg.json``: the metrics, the summed confusion
matrix as nested lists, the number of images and whether TTA was on.  A serial loop on one stream, as evaluate_ood's ``--tta`` path is."""
import argparse
import json
import os
from pathlib import Path

import torch

from . import evaluate_ood as E
from .config import load_cfg


def build_parser():
    p = argparse.ArgumentParser(description="Closed-set semantic segmentation evaluation (rba_amd)")
    p.add_argument("--models_folder", type=str, default="ckpts/")
    p.add_argument("--selected_models", nargs="*", type=str, default=[], help="default: every model folder")
    p.add_argument("--cityscapes_root", type=str, required=True, help="the folder that holds leftImg8bit/ and gtFine/")
    p.add_argument("--split", type=str, default="val")
    p.add_argument("--labels", type=str, default="auto", choices=["auto", "trainIds", "labelIds"],
                   help="labelTrainIds PNGs, or the raw labelIds PNGs read through the id -> trainId table inside the kernel; auto: trainIds when present")
    p.add_argument("--out_path", type=str, default="results")
    p.add_argument("--upper_limit", type=int, default=1 << 30)
    p.add_argument("--num_workers", type=int, default=8, help="image-decoding threads")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--dist_backend", type=str, default=os.environ.get("RBA_EVAL_BACKEND") or None, choices=[None, "nccl", "gloo"])
    p.add_argument("--share_device", type=int, default=int(os.environ.get("RBA_EVAL_SHARE_DEVICE", "0")),
                   help="1: every rank uses device 0 and the matrices are summed on gloo -- a plumbing test on a one-GPU box, never a measurement")
    p.add_argument("--tta", action="store_true", help="score through SemanticSegmentorWithTTA (the views of the checkpoint config's TEST.AUG); also on "
                                                      "when that config has TEST.AUG.ENABLED")
    return p


def run_evaluation(model, dataset, args, rank=0, world=1):
    """This rank's shard of `dataset` through `model` (a MaskFormer or the TTA wrapper) -> (metrics OrderedDict, summed matrix, images of this rank)"""
    from . import distributed as D
    from .datasets import prefetch
    from .sem_seg_evaluation import SemSegEvaluator
    dev = model.device
    ev = SemSegEvaluator(dataset.num_classes, dataset.ignore_label, dataset.class_names, lut=dataset.lut, device=dev)
    n = min(len(dataset), args.upper_limit)
    mine = D.shard_indices(n, rank, world)
    nw = max(0, int(args.num_workers))
    for image, label in prefetch(dataset, mine, nw, pin=nw > 0, raw=True):
        x = image.to(dev, non_blocking=True).permute(2, 0, 1).contiguous()              # [3,H,W] as the model takes it
        _, arg = model.rba_scores([{"image": x}], return_argmax=True)[0]
        ev.process([{"sem_seg": label}], [{"argmax": arg}])
    res = ev.evaluate()
    return res, ev.matrix, ev.images


def print_table(model_name, res, tta, file=None):
    m = res["sem_seg"]
    print(f"{model_name}: {'TTA (multi-scale + flip)' if tta else 'single scale'}   mIoU {m['mIoU']:.2f}  fwIoU {m['fwIoU']:.2f}  mACC {m['mACC']:.2f}  "
          f"pACC {m['pACC']:.2f}", file=file)
    print(f"  {'class':16s} {'IoU':>7s} {'ACC':>7s}", file=file)
    for k in m:
        if k.startswith("IoU-"):
            print(f"  {k[4:]:16s} {m[k]:7.2f} {m['ACC-' + k[4:]]:7.2f}", file=file)


def main(argv=None):
    from . import distributed as D
    from .sem_seg_datasets import CityscapesSemSeg
    from .test_time_augmentation import SemanticSegmentorWithTTA
    args = build_parser().parse_args(argv)
    if args.share_device:
        os.environ["LOCAL_RANK"] = "0"
    rank, world, local = D.init_from_env(args.dist_backend or ("gloo" if args.share_device else None))
    device = torch.device(args.device, local) if args.device == "cuda" else torch.device(args.device)
    if device.type == "cuda":
        torch.cuda.set_device(device)
    dataset = CityscapesSemSeg(args.cityscapes_root, args.split, args.labels)
    models = sorted(m for m in os.listdir(args.models_folder) if os.path.isdir(os.path.join(args.models_folder, m)))
    if args.selected_models:
        models = [m for m in models if m in args.selected_models]
    if not models:
        raise ValueError("Number of models chosen is 0, either the models folder is empty or no models were selected")
    for model_name in models:
        exp = os.path.join(args.models_folder, model_name)
        model_path = next((os.path.join(exp, f) for f in ("model_final.pth", "model_final.pkl") if os.path.exists(os.path.join(exp, f))), None)
        if model_path is None:
            if rank == 0:
                print(f"{model_name}: model path does not exist, skipping")
            continue
        cfg_path = os.path.join(exp, "config.yaml")
        model = E.get_model(cfg_path, model_path, device=device)
        if model.arch["num_classes"] != dataset.num_classes:
            raise ValueError(f"{model_name} has {model.arch['num_classes']} classes, Cityscapes {dataset.num_classes}")
        model, _ = E.with_tta(model, load_cfg(cfg_path), args)
        tta = isinstance(model, SemanticSegmentorWithTTA)
        res, matrix, _ = run_evaluation(model, dataset, args, rank, world)
        if rank == 0:
            print_table(model_name, res, tta)
            store = os.path.join(args.out_path, model_name)
            Path(store).mkdir(exist_ok=True, parents=True)
            with open(os.path.join(store, "sem_seg.json"), "w") as f:
                json.dump({"sem_seg": res["sem_seg"], "confusion_matrix": matrix.tolist(), "images": min(len(dataset), args.upper_limit),
                           "tta": tta, "split": args.split, "labels": dataset.label_source}, f, indent=1)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
