"""Minimal reader for the reference's Detectron2/yacs YAML configs (no detectron2 / yacs dependency).

``load_cfg(path)`` handles both the fully-resolved dumps next to released weights (``ckpts/*/config.yaml``, the
load path of evaluate_ood.py:264-265) and the training chains under ``configs/**`` (``_BASE_`` inheritance,
python/eval tags such as Base-Cityscapes-SemanticSegmentation.yaml:37 are read as plain strings and ignored).
Keys the inference path consumes but older dumps lack get the defaults of mask2former/config.py:6-244
(e.g. ckpts/swin_l_1dl/config.yaml has no DENSE_HYBRID_LOSS).
"""
import os

import yaml


class CfgNode(dict):
    """dict with attribute access (read-only use)."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


def _wrap(x):
    if isinstance(x, dict):
        return CfgNode({k: _wrap(v) for k, v in x.items()})
    if isinstance(x, list):
        return [_wrap(v) for v in x]
    return x


def _merge(dst, src):
    for k, v in src.items():
        if isinstance(v, dict) and isinstance(dst.get(k), dict):
            _merge(dst[k], v)
        else:
            dst[k] = v
    return dst


class _Loader(yaml.SafeLoader):
    pass


def _any_tag(loader, suffix, node):
    if isinstance(node, yaml.ScalarNode):
        return loader.construct_scalar(node)
    if isinstance(node, yaml.SequenceNode):
        return loader.construct_sequence(node, deep=True)
    return loader.construct_mapping(node, deep=True)


_Loader.add_multi_constructor("tag:yaml.org,2002:python/", _any_tag)
_Loader.add_multi_constructor("!", _any_tag)

# defaults of the keys read by rba_amd.arch.arch_from_cfg (detectron2 defaults + add_maskformer2_config)
_DEFAULTS = {
    "MODEL": {
        "META_ARCHITECTURE": "MaskFormer",
        "PIXEL_MEAN": [123.675, 116.28, 103.53],
        "PIXEL_STD": [58.395, 57.12, 57.375],
        "BACKBONE": {"NAME": "D2SwinTransformer"},
        "SWIN": {"PRETRAIN_IMG_SIZE": 224, "PATCH_SIZE": 4, "EMBED_DIM": 96, "DEPTHS": [2, 2, 6, 2],
                 "NUM_HEADS": [3, 6, 12, 24], "WINDOW_SIZE": 7, "MLP_RATIO": 4.0, "QKV_BIAS": True, "QK_SCALE": None,
                 "DROP_RATE": 0.0, "ATTN_DROP_RATE": 0.0, "DROP_PATH_RATE": 0.3, "APE": False, "PATCH_NORM": True,
                 "OUT_FEATURES": ["res2", "res3", "res4", "res5"], "USE_CHECKPOINT": False},
        # detectron2/config/defaults.py MODEL.RESNETS (build_resnet_backbone: BASELINE config C1)
        "RESNETS": {"DEPTH": 50, "OUT_FEATURES": ["res4"], "NUM_GROUPS": 1, "NORM": "FrozenBN", "WIDTH_PER_GROUP": 64,
                    "STRIDE_IN_1X1": True, "RES5_DILATION": 1, "RES2_OUT_CHANNELS": 256, "STEM_OUT_CHANNELS": 64,
                    "DEFORM_ON_PER_STAGE": [False, False, False, False]},
        "SEM_SEG_HEAD": {"NAME": "MaskFormerHead", "IN_FEATURES": ["res2", "res3", "res4", "res5"], "NUM_CLASSES": 19,
                         "IGNORE_VALUE": 255, "LOSS_WEIGHT": 1.0, "CONVS_DIM": 256, "MASK_DIM": 256, "NORM": "GN",
                         "PIXEL_DECODER_NAME": "MSDeformAttnPixelDecoder", "TRANSFORMER_ENC_LAYERS": 6,
                         "DEFORMABLE_TRANSFORMER_ENCODER_IN_FEATURES": ["res3", "res4", "res5"], "COMMON_STRIDE": 4},
        "MASK_FORMER": {"TRANSFORMER_DECODER_NAME": "MultiScaleMaskedTransformerDecoder",
                        "TRANSFORMER_IN_FEATURE": "multi_scale_pixel_decoder", "HIDDEN_DIM": 256,
                        "NUM_OBJECT_QUERIES": 100, "NHEADS": 8, "DROPOUT": 0.0, "DIM_FEEDFORWARD": 2048,
                        "DEC_LAYERS": 10, "PRE_NORM": False, "ENFORCE_INPUT_PROJ": False, "SIZE_DIVISIBILITY": 32,
                        "DENSE_HYBRID_LOSS": False,
                        "OPEN_PANOPTIC": True,
                        "TEST": {"SEMANTIC_ON": True, "INSTANCE_ON": False, "PANOPTIC_ON": False,
                                 "OBJECT_MASK_THRESHOLD": 0.0, "OVERLAP_THRESHOLD": 0.0,
                                 "SEM_SEG_POSTPROCESSING_BEFORE_INFERENCE": False}},
    },
    # the keys rba_amd.dataset_mappers reads: detectron2/config/defaults.py INPUT, add_maskformer2_config (mask2former/config.py:13-20) and the
    # reference's own (config.py:187-230); the Cityscapes base config sets MIN_SIZE_TRAIN 512 .. 2048, MAX_SIZE_TRAIN 4096, the absolute 512 x 1024
    # crop, COLOR_AUG_SSD and FORMAT "RGB"
    "INPUT": {"MIN_SIZE_TRAIN": [800], "MIN_SIZE_TRAIN_SAMPLING": "choice", "MAX_SIZE_TRAIN": 1333, "MIN_SIZE_TEST": 800, "MAX_SIZE_TEST": 1333,
              "RANDOM_FLIP": "horizontal", "FORMAT": "BGR", "MASK_FORMAT": "polygon",
              "CROP": {"ENABLED": False, "TYPE": "relative_range", "SIZE": [0.9, 0.9], "SINGLE_CATEGORY_MAX_AREA": 1.0},
              "DATASET_MAPPER_NAME": "mask_former_semantic", "COLOR_AUG_SSD": False, "SIZE_DIVISIBILITY": -1,
              "OOD_LABEL": 254, "OOD_PROB": 0.2, "COCO_ROOT": "coco/", "COCO_PROXY_SIZE": 300, "REPEAT_INSTANCE_MASKS": 1},
    # the keys rba_amd.solver and rba_amd.train_net read.  Detectron2 is not installed here, so its defaults (detectron2/config/defaults.py SOLVER and the
    # DeepLab project's add_deeplab_config: POLY_LR_POWER, POLY_LR_CONSTANT_ENDING) are RESTATED, their parity unpinned; WEIGHT_DECAY_EMBED, OPTIMIZER and
    # BACKBONE_MULTIPLIER are add_maskformer2_config's (mask2former/config.py:24-27).  The Cityscapes base config sets IMS_PER_BATCH 16, BASE_LR 1e-4,
    # MAX_ITER 90000, WARMUP_FACTOR 1.0, WARMUP_ITERS 0, WEIGHT_DECAY 0.05, ADAMW, WarmupPolyLR, full_model clipping at 0.01 and AMP
    # (tests/golden/solver/base_solver.yaml)
    "SOLVER": {"FORCE_REGION_PARTITION": False,
               "LR_SCHEDULER_NAME": "WarmupMultiStepLR", "MAX_ITER": 40000, "BASE_LR": 0.001, "WEIGHT_DECAY": 0.0001, "WEIGHT_DECAY_NORM": 0.0,
               "WEIGHT_DECAY_EMBED": 0.0, "OPTIMIZER": "ADAMW", "BACKBONE_MULTIPLIER": 0.1, "MOMENTUM": 0.9,
               "WARMUP_FACTOR": 0.001, "WARMUP_ITERS": 1000, "WARMUP_METHOD": "linear", "POLY_LR_POWER": 0.9, "POLY_LR_CONSTANT_ENDING": 0.0,
               "CHECKPOINT_PERIOD": 5000, "IMS_PER_BATCH": 16,
               "CLIP_GRADIENTS": {"ENABLED": False, "CLIP_TYPE": "value", "CLIP_VALUE": 1.0, "NORM_TYPE": 2.0},
               "AMP": {"ENABLED": False}},
    # detectron2/config/defaults.py TEST.AUG (rba_amd.test_time_augmentation); the Cityscapes base config sets [512 .. 1792], 4096, FLIP
    # ... and TEST.DETECTIONS_PER_IMAGE, the top-k of instance inference (maskformer_model.py:218)
    "TEST": {"DETECTIONS_PER_IMAGE": 100,
             "AUG": {"ENABLED": False, "MIN_SIZES": [400, 500, 600, 700, 800, 900, 1000, 1100, 1200], "MAX_SIZE": 4000, "FLIP": True}},
}


def _read(path, seen=()):
    path = os.path.abspath(path)
    if path in seen:
        raise ValueError(f"_BASE_ cycle at {path}")
    with open(path) as f:
        d = yaml.load(f, Loader=_Loader) or {}
    base = d.pop("_BASE_", None)
    if base is not None:
        if not os.path.isabs(base):
            base = os.path.join(os.path.dirname(path), base)
        d = _merge(_read(base, seen + (path,)), d)
    return d


def load_cfg(path, opts=None) -> CfgNode:
    """Read ``path`` (following ``_BASE_``), overlay it on the defaults, apply ``opts`` = [KEY.PATH, value, ...]."""
    import copy

    d = _merge(copy.deepcopy(_DEFAULTS), _read(path))
    if opts:
        if len(opts) % 2:
            raise ValueError("opts must be KEY VALUE pairs")
        for k, v in zip(opts[0::2], opts[1::2]):
            node = d
            parts = k.split(".")
            for p in parts[:-1]:
                node = node.setdefault(p, {})
            node[parts[-1]] = yaml.safe_load(v) if isinstance(v, str) else v
    return _wrap(d)
