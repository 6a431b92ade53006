"""``MaskFormer`` meta-architecture, inference branch only (reference: mask2former/maskformer_model.py:23-386).

Drop-in surface: ``model([{"image": uint8/float [3,H,W] RGB 0..255}]) -> [{"sem_seg": [K,H,W] fp32}]`` on the model's
device, identical to the reference, so the unmodified ``get_RbA`` / ``get_logits`` of evaluate_ood.py work on it.
In addition each result dict carries ``"rba"`` ([H,W], the RbA score of evaluate_ood.py:150 produced by the same
fused kernel) and, on request, ``"argmax"``; ``model.rba_scores(...)`` skips materialising ``sem_seg`` altogether.
"""
import itertools

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import instance_ops, ops, panoptic_ops
from .h2d import to_device
from .arch import backbone_name as _backbone_name, complete
from .graph_replay import GraphKey, GraphReplay, capture
from .lru import ShapeCache
from .modeling.backbone import mix_transformer as _mix_transformer  # noqa: F401  (registers mit_b0..mit_b5)
from .modeling.backbone import resnet as _resnet  # noqa: F401  (registers build_resnet_backbone)
from .modeling.backbone import swin as _swin  # noqa: F401  (registers D2SwinTransformer)
from .modeling.meta_arch import mask_former_head as _head  # noqa: F401
from .registry import BACKBONE_REGISTRY, META_ARCH_REGISTRY, SEM_SEG_HEADS_REGISTRY

# Generation of the module trees of this process: torch's global registration hooks fire whenever any module gets a parameter, buffer or submodule set
# (construction, load_state_dict(assign=True), `mod.weight = nn.Parameter(..)`, a submodule swap); MaskFormer._weights_version walks its tree again only
# after that.  A hook that returns None changes nothing.
_REGISTRATIONS = [0]
_EPOCHS = itertools.count(1)


def _registered(*_):
    _REGISTRATIONS[0] += 1


for _hook in (nn.modules.module.register_module_parameter_registration_hook, nn.modules.module.register_module_buffer_registration_hook,
              nn.modules.module.register_module_module_registration_hook):
    _hook(_registered)


def _class_prob(mask_cls):
    """F.softmax(mask_cls, -1)[..., :-1] (reference maskformer_model.py:381-383), one launch.  The kernel (2 <= classes + 1 <= 64) uses its own exp / sum order:
    equal to F.softmax to ~1e-7 (tests/test_kernels_gpu.py::test_softmax_drop_last_vs_torch), so `sem_seg` / argmax agree with the fp32 torch path except on
    near-ties -- the tolerance every end-to-end fixture already grants (top-2 gap < 1e-4)."""
    if 2 <= mask_cls.shape[-1] <= 64:
        return ops.softmax_drop_last(mask_cls.contiguous())
    return F.softmax(mask_cls, dim=-1)[..., :-1].contiguous()


@META_ARCH_REGISTRY.register()
class MaskFormer(nn.Module):
    def __init__(self, arch, backbone_name=None, head_name="MaskFormerHead"):
        super().__init__()
        a = complete(arch)
        self.arch = a
        self.backbone = BACKBONE_REGISTRY.get(backbone_name or _backbone_name(a))(a)
        self.sem_seg_head = SEM_SEG_HEADS_REGISTRY.get(head_name)(a)
        self.num_queries = a["num_queries"]
        self.size_divisibility = a["size_divisibility"] if a["size_divisibility"] > 0 else self.backbone.size_divisibility
        self.register_buffer("pixel_mean", torch.tensor(a["pixel_mean"], dtype=torch.float32).view(-1, 1, 1), False)
        self.register_buffer("pixel_std", torch.tensor(a["pixel_std"], dtype=torch.float32).view(-1, 1, 1), False)
        self._mean3 = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in a["pixel_mean"])      # fp32-rounded, as the buffers hold them
        self._std3 = tuple(float(torch.tensor(v, dtype=torch.float32)) for v in a["pixel_std"])
        self.fused_front_end = True
        # rba_scores(): batch-1 forwards replayed from a per-shape hipGraph.  "auto" (default, round 6): per shape, only where the eager launches are MEASURED to be
        # launch-bound (host issue time vs GPU span of an eager call, see _graphed_scores) -- at 1024 x 2048 the GPU is the bottleneck and eager is 4 % faster than
        # replay on one stream (BENCH_r05: 124.7 vs 119.7 images/s), at 720 x 1280 / 9 layers and on small images replay wins.  True: always (the evaluator with
        # several streams, tests); False: never.
        self.graph_replay = "auto"
        self.fused_upsample = True      # K1 reads the low-res logits and up-samples on the fly (rba_reduce_up4)
        # panoptic inference (maskformer_model.py:202-220): off unless TEST.PANOPTIC_ON
        self.panoptic_on, self.open_panoptic = bool(a["panoptic_on"]), bool(a["open_panoptic"])
        # instance inference (maskformer_model.py:213-218): off unless TEST.INSTANCE_ON; TEST.SEMANTIC_ON: False drops "sem_seg" / "rba" from the results
        self.semantic_on, self.instance_on = bool(a["semantic_on"]), bool(a["instance_on"])
        self.test_topk_per_image = int(a["test_topk_per_image"])
        self.instance_boxes = False                     # True: pred_boxes = the masks' bounding boxes (K17a has them anyway); False: zeros, as the reference
        self.instance_mask_dtype = torch.float32        # pred_masks' element type: the reference's float32, or torch.uint8 (a quarter of the bytes)
        self.sem_seg_postprocess_before_inference = bool(a["postprocess_before_inference"]) or self.panoptic_on or self.instance_on
        self.object_mask_threshold, self.overlap_threshold = float(a["object_mask_threshold"]), float(a["overlap_threshold"])
        self.thing_classes = frozenset(int(c) for c in a["thing_classes"])
        self.eval()

    @property
    def device(self):
        return self.pixel_mean.device

    # ------------------------------------------------------------------ pre-processing (:255-257)
    def preprocess(self, batched_inputs):
        images = [(to_device(x["image"], self.device).float() - self.pixel_mean) / self.pixel_std for x in batched_inputs]
        sizes = [tuple(int(v) for v in im.shape[-2:]) for im in images]
        d = self.size_divisibility
        H = (max(s[0] for s in sizes) + d - 1) // d * d
        W = (max(s[1] for s in sizes) + d - 1) // d * d
        batch = images[0].new_zeros((len(images), images[0].shape[0], H, W))
        for i, im in enumerate(images):
            batch[i, :, : sizes[i][0], : sizes[i][1]] = im       # ImageList.from_tensors: zero pad bottom/right
        return batch, sizes

    # ------------------------------------------------------------------ network
    @torch.no_grad()
    def _predict_outputs(self, batched_inputs):
        pe = getattr(self.backbone, "patch_embed", None)
        if (self.fused_front_end and pe is not None and hasattr(self.backbone, "forward_images") and pe.fused_ok()
                and all(x["image"].dim() == 3 and x["image"].shape[0] == 3 and x["image"].dtype in (torch.uint8, torch.float32)
                        for x in batched_inputs)):
            # normalisation + ImageList padding + patch im2col in one kernel, the projection on K6 (backbone/swin.py PatchEmbed.forward_images)
            images = [to_device(x["image"], self.device).contiguous() for x in batched_inputs]
            sizes = [tuple(int(v) for v in im.shape[-2:]) for im in images]
            d = self.size_divisibility
            H = (max(s[0] for s in sizes) + d - 1) // d * d
            W = (max(s[1] for s in sizes) + d - 1) // d * d
            features = self.backbone.forward_images(images, self._mean3, self._std3, H, W)
            return self.sem_seg_head(features), sizes, (H, W)
        batch, sizes = self.preprocess(batched_inputs)
        features = self.backbone(batch)
        return self.sem_seg_head(features), sizes, tuple(batch.shape[-2:])

    @torch.no_grad()
    def predict(self, batched_inputs):
        """-> (pred_logits [B,Q,K+1], pred_masks [B,Q,H/4,W/4], image_sizes, padded (H,W))."""
        outputs, sizes, padded = self._predict_outputs(batched_inputs)
        return outputs["pred_logits"], outputs["pred_masks"], sizes, padded

    def finetune_outputs(self, batched_inputs):
        """-> (outputs, image_sizes, padded (H,W)): _predict_outputs for the outlier-supervised fine-tune of the two prediction heads.  Backbone and
        pixel decoder run under no_grad exactly as in `predict`; the predictor runs in the caller's grad mode with its ``differentiable_heads`` honoured, so
        ``outputs["pred_logits"]`` / ``["pred_masks"]`` carry the bits `predict` gives and a graph over the ten head tensors
        (``criterion.outlier_loss(outputs, targets)["outlier_loss"].backward()``); with the predictor's ``deep_supervision`` set too, so does every
        ``aux_outputs`` entry.  On a model with the DenseHybrid head, ``outputs["ood_pred"]`` [B,2,H/4,W/4] is the inference kernel's output without
        a graph, or -- with the predictor's ``differentiable_ood_head`` set -- the head in plain torch with a graph over its four parameters
        (``criterion.densehybrid_loss(outputs, targets, num_classes=K)["densehybrid_loss"].backward()``).  With the predictor's
        ``differentiable_decoder`` set too, the graph also covers the decoder layers and the three embeddings (the released PEBAL recipe; see
        ``MultiScaleMaskedTransformerDecoder``).  Eager launches only: graph replay is never used here."""
        predictor = self.sem_seg_head.predictor
        if not getattr(predictor, "differentiable_heads", False):
            if getattr(predictor, "deep_supervision", False):
                raise ops.RbaHipError("finetune_outputs: predictor.deep_supervision is set without predictor.differentiable_heads; deep supervision "
                                      "is the differentiable heads' aux_outputs, so set differentiable_heads = True as well")
            if getattr(predictor, "differentiable_decoder", False):
                raise ops.RbaHipError("finetune_outputs: predictor.differentiable_decoder is set without predictor.differentiable_heads; the decoder "
                                      "layers' graph hangs off the differentiable head calls, so set differentiable_heads = True as well")
            raise ops.RbaHipError("finetune_outputs: set model.sem_seg_head.predictor.differentiable_heads = True first (without it the outputs "
                                  "carry no autograd graph)")
        with torch.no_grad():
            pe = getattr(self.backbone, "patch_embed", None)
            if (self.fused_front_end and pe is not None and hasattr(self.backbone, "forward_images") and pe.fused_ok()
                    and all(x["image"].dim() == 3 and x["image"].shape[0] == 3 and x["image"].dtype in (torch.uint8, torch.float32)
                            for x in batched_inputs)):
                images = [to_device(x["image"], self.device).contiguous() for x in batched_inputs]      # the front end of _predict_outputs
                sizes = [tuple(int(v) for v in im.shape[-2:]) for im in images]
                d = self.size_divisibility
                padded = ((max(s[0] for s in sizes) + d - 1) // d * d, (max(s[1] for s in sizes) + d - 1) // d * d)
                features = self.backbone.forward_images(images, self._mean3, self._std3, *padded)
            else:
                batch, sizes = self.preprocess(batched_inputs)
                padded = tuple(batch.shape[-2:])
                features = self.backbone(batch)
            mask_features, _, multi_scale_features = self.sem_seg_head.pixel_decoder.forward_features(features)
        return predictor(multi_scale_features, mask_features), sizes, padded

    def prepare_targets(self, batched_inputs, padded):
        """The criterion's targets from a training batch (maskformer_model.py:262-274, 358-379): per input, whose ``instances`` carry ``gt_classes`` and
        ``gt_masks`` (rba_amd.dataset_mappers), {"labels": gt_classes, "masks": gt_masks zero-padded bottom / right to ``padded`` (H, W) -- the third
        value of ``finetune_outputs`` --, and, where the input has them, "outlier_masks" and "sem_seg"}, on the model's device."""
        h_pad, w_pad = int(padded[0]), int(padded[1])
        dev = self.device
        new_targets = []
        for x in batched_inputs:
            gt_masks = to_device(x["instances"].gt_masks, dev)
            if gt_masks.shape[1] > h_pad or gt_masks.shape[2] > w_pad:
                raise ValueError(f"prepare_targets: masks of size {tuple(gt_masks.shape[1:])} do not fit the padded size {(h_pad, w_pad)}")
            padded_masks = torch.zeros((gt_masks.shape[0], h_pad, w_pad), dtype=gt_masks.dtype, device=dev)
            padded_masks[:, : gt_masks.shape[1], : gt_masks.shape[2]] = gt_masks
            entry = {"labels": to_device(x["instances"].gt_classes, dev), "masks": padded_masks}
            if "outlier_mask" in x:
                entry["outlier_masks"] = to_device(x["outlier_mask"], dev)
            if "sem_seg" in x:
                entry["sem_seg"] = to_device(x["sem_seg"], dev)
            new_targets.append(entry)
        return new_targets

    def _post(self, mask_cls, mask_pred, image_size, padded, want_sem_seg, want_argmax, score="rba", with_void=False):
        """Up-sample (:294-299), semantic inference (:381-386), crop (:330-332), RbA (evaluate_ood.py:150).  with_void: semantic_inference_with_void
        (:388-392) -- K1 on the [Q,K+1] probabilities, the void column kept."""
        prob = F.softmax(mask_cls, dim=-1).contiguous() if with_void else _class_prob(mask_cls)
        H, W = padded
        exact4 = mask_pred.shape[-2] * 4 == H and mask_pred.shape[-1] * 4 == W
        if self.fused_upsample and exact4 and prob.shape[1] <= 32:
            return ops.rba_reduce_up4(mask_pred.contiguous(), prob, image_size, want_sem_seg, want_argmax, score)
        up = ops.resample_bilinear(mask_pred.contiguous(), (H, W))
        rba, sem, arg = ops.rba_reduce(up, prob, want_sem_seg, want_argmax, score)
        h, w = image_size
        if (h, w) != (H, W):
            rba = rba[:h, :w].contiguous()
            sem = sem[:, :h, :w].contiguous() if sem is not None else None
            arg = arg[:h, :w].contiguous() if arg is not None else None
        return rba, sem, arg

    # ------------------------------------------------------------------ open-set panoptic inference (:394-486)
    @torch.no_grad()
    def panoptic_inference(self, mask_cls, mask_pred, open_panoptic=False, ood_threshold=-0.1, pixel_min=300,
                           return_ood_pred=False, ood_mask=None):
        """mask_cls [Q,K+1] logits, mask_pred [Q,H,W] logits at the output resolution ->
        (panoptic_seg int32 [H,W], segments_info[, rba map]).  Closed-set part: the Mask2Former merge (:395-452) -- queries whose
        best class is not void and scores above ``object_mask_threshold`` compete per pixel by score x sigmoid(mask); a query
        keeps its pixels if enough of its own >= 0.5 area wins (``overlap_threshold``); "stuff" classes merge into one segment.
        One pass over the mask planes (K16a), one read-back of its 3 Q counters, the reference's loop on the host over Python ints, one
        gather (K16b): docs/kernels/K16.md.
        Open-set part (:454-481): the RbA map (K1) thresholded, 3x3 opened and closed, 4-connected components of at least
        ``pixel_min`` still-unclaimed pixels become new "thing" segments of category 255.  ``ood_mask``: the RbA map [H,W] where the
        caller has it already (forward() does); None: K1 runs here."""
        return self._panoptic(mask_cls, mask_pred, None, open_panoptic, ood_threshold, pixel_min, return_ood_pred, ood_mask)

    def _panoptic(self, mask_cls, mask_pred, crop, open_panoptic, ood_threshold, pixel_min, return_ood_pred, ood_mask):
        """panoptic_inference; with ``crop`` = (H, W), mask_pred is the quarter-resolution [Q,h,w] and the merge runs on the [H,W] window of
        its virtual x4 up-sampling (K16a's up4 form): the full-resolution planes are never written."""
        H, W = (mask_pred.shape[-2:] if crop is None else crop)
        K = mask_cls.shape[-1] - 1
        prob_all = F.softmax(mask_cls, dim=-1)
        scores, labels = prob_all.max(-1)
        keep = labels.ne(K) & (scores > self.object_mask_threshold)
        classes = torch.where(keep, labels, torch.full_like(labels, -1)).tolist()     # one read-back: who is kept, and as which class
        if all(c < 0 for c in classes):
            # (the reference also skips the open-set part here, :414-416)
            return torch.zeros((H, W), dtype=torch.int32, device=mask_pred.device), []
        panoptic_seg, segments_info, current = panoptic_ops.panoptic_segments(
            mask_pred.contiguous(), scores.contiguous(), keep.to(torch.uint8), classes, self.thing_classes, self.overlap_threshold, crop)
        if not open_panoptic:
            return panoptic_seg, segments_info
        if ood_mask is None:
            full = mask_pred if crop is None else ops.resample_bilinear(mask_pred.contiguous(), (4 * mask_pred.shape[-2], 4 * mask_pred.shape[-1]))[:, :H, :W]
            ood_mask = ops.rba_reduce(full.contiguous(), prob_all[:, :-1].contiguous())[0]      # -sum_k tanh(sem_k), K1
        elif tuple(ood_mask.shape) != (H, W):
            raise ops.RbaHipError(f"ood_mask must have the output resolution {(H, W)}, got {tuple(ood_mask.shape)}")
        comp, n = ops.ood_components(ood_mask, ood_threshold)
        if n:
            free = panoptic_seg == 0
            sizes = torch.bincount(comp[free].long(), minlength=n + 1)
            ok = sizes >= pixel_min
            ok[0] = False                                                                     # background
            new_id = current + torch.cumsum(ok.to(torch.int32), 0, dtype=torch.int32)         # in component (= raster) order
            sel = free & ok[comp.long()]
            panoptic_seg[sel] = new_id[comp.long()][sel]
            for _ in range(int(ok.sum())):
                current += 1
                segments_info.append({"id": current, "isthing": True, "category_id": 255})
        if return_ood_pred:
            return panoptic_seg, segments_info, ood_mask
        return panoptic_seg, segments_info

    # ------------------------------------------------------------------ instance inference (:488-527)
    @torch.no_grad()
    def instance_inference(self, mask_cls, mask_pred):
        """mask_cls [Q,K+1] logits, mask_pred [Q,H,W] logits at the output resolution -> Instances(image_size) with pred_masks [N,H,W]
        (``instance_mask_dtype``: mask_pred > 0), pred_classes [N], scores [N] (class score x mean sigmoid over the mask) and pred_boxes [N,4] (zeros as the
        reference, or with ``instance_boxes`` the masks' XYXY boxes) of the ``test_topk_per_image`` best (query, class) pairs, in DESCENDING class score
        (the reference's ``sorted=False`` leaves the order unspecified); with ``panoptic_on`` only the "thing" classes are kept (:506-513).  One pass over
        the planes of the queries in the top-k (K17a) and one write of the result planes (K17b): docs/kernels/K17.md."""
        return self._instances(mask_cls, mask_pred.contiguous(), None)

    def _instances(self, mask_cls, mask, crop):
        """instance_inference; with ``crop`` = (H, W), mask is the quarter-resolution [Q,h,w] and everything runs on the [H,W] window of its virtual x4
        up-sampling (K17's up4 forms): the full-resolution planes are never written."""
        from .dataset_mappers import Instances
        planes, classes, scores, boxes = instance_ops.instance_segments(
            mask_cls.contiguous(), mask, self.test_topk_per_image, mask_cls.shape[-1] - 1, crop, self.thing_classes if self.panoptic_on else None,
            self.instance_boxes, self.instance_mask_dtype)
        size = tuple(int(v) for v in (mask.shape[-2:] if crop is None else crop))
        return Instances(size, pred_masks=planes, pred_boxes=boxes, scores=scores, pred_classes=classes)

    @torch.no_grad()
    def forward(self, batched_inputs, include_void=False, return_separately=False, return_aux=False,
                return_ood_pred=False, return_argmax=False, panoptic_ood_threshold=-0.3, panoptic_pixel_min=200,
                return_panoptic_ood=False, **kwargs):
        """include_void: "sem_seg" is semantic_inference_with_void's (:388-392), K + 1 channels with the void class last; "rba" stays the score over the K
        real classes.  return_separately: -> (results, mask_cls_result, mask_pred_result) of the LAST image (:353-354), its mask logits materialised at the
        resolution its inference heads saw."""
        if return_aux or kwargs:
            raise NotImplementedError("return_aux and other keyword arguments of the reference's MaskFormer.forward are not provided (semantic, panoptic "
                                      "and instance inference are)")
        outputs, sizes, padded = self._predict_outputs(batched_inputs)
        mask_cls, mask_pred = outputs["pred_logits"], outputs["pred_masks"]
        ood_pred = None
        if return_ood_pred:                                     # :303-305: up-sampled to the FIRST image's size, align_corners=True
            if "ood_pred" not in outputs:
                raise KeyError("ood_pred: the model has no DenseHybrid head (MODEL.MASK_FORMER.DENSE_HYBRID_LOSS)")
            ood_pred = ops.resample_bilinear_ac(outputs["ood_pred"].contiguous(), sizes[0])
        up4 = mask_pred.shape[-2] * 4 == padded[0] and mask_pred.shape[-1] * 4 == padded[1]
        results = []
        for i, inp in enumerate(batched_inputs):
            height, width = inp.get("height", sizes[i][0]), inp.get("width", sizes[i][1])
            resized = (height, width) != sizes[i]
            planes = []

            def materialised():
                """the mask logits at the output resolution (:294-299, :316-320), written once for whichever head asks"""
                if not planes:
                    mp = ops.resample_bilinear(mask_pred[i].contiguous(), padded)[:, : sizes[i][0], : sizes[i][1]].contiguous()
                    planes.append(ops.resample_bilinear(mp, (height, width)) if resized else mp)
                return planes[0]

            def semantic(with_void):
                if resized and self.sem_seg_postprocess_before_inference:
                    # :316-320: crop + resize the MASK LOGITS to the requested resolution first, semantic inference on those
                    prob = F.softmax(mask_cls[i], dim=-1).contiguous() if with_void else _class_prob(mask_cls[i])
                    return ops.rba_reduce(materialised(), prob, True, return_argmax and not with_void)
                rba, sem, arg = self._post(mask_cls[i], mask_pred[i], sizes[i], padded, True, return_argmax and not with_void, with_void=with_void)
                if resized:                       # :330-332: sem_seg_postprocess of the class maps to the requested resolution
                    sem = ops.resample_bilinear(sem, (height, width))
                    rba = -sem.tanh().sum(dim=0)
                    arg = sem.argmax(0).to(torch.int32) if return_argmax else None
                return rba, sem, arg

            r, rba = {}, None
            if self.semantic_on:
                rba, sem, arg = semantic(False)
                r = {"sem_seg": semantic(True)[1] if include_void else sem, "rba": rba}
                if return_argmax:
                    r["argmax"] = arg
            if self.panoptic_on:                                   # :337-341; masks first brought to the output resolution (:318-321)
                if not resized:
                    # the merge's resolution is `rba`'s: the RbA map is handed over, and where the padded size is exactly x4 the merge
                    # up-samples on the fly (K16a's up4 form) instead of reading [Q,H,W] planes written for it
                    r["panoptic_seg"] = self._panoptic(mask_cls[i], mask_pred[i] if up4 else materialised(), sizes[i] if up4 else None, self.open_panoptic,
                                                       panoptic_ood_threshold, panoptic_pixel_min, return_panoptic_ood, rba)
                else:
                    # `rba` is the score of these resized mask logits only on the postprocess-before-inference path (on the other it comes from resized class maps)
                    r["panoptic_seg"] = self.panoptic_inference(mask_cls[i], materialised(), self.open_panoptic, panoptic_ood_threshold, panoptic_pixel_min,
                                                                return_panoptic_ood, ood_mask=rba if self.sem_seg_postprocess_before_inference else None)
            if self.instance_on:                                   # :343-346; the same resolution rule, K17's up4 forms where they apply
                if not resized and up4:
                    r["instances"] = self._instances(mask_cls[i], mask_pred[i].contiguous(), sizes[i])
                else:
                    r["instances"] = self._instances(mask_cls[i], materialised(), None)
            results.append(r)
        if return_ood_pred:
            return results, ood_pred                            # :350-351
        if return_separately:
            return results, mask_cls[-1], materialised()        # :353-354: the loop's last image
        return results

    # ------------------------------------------------------------------ hipGraph replay of the scoring path
    GRAPH_MAX = 8            # live graphs per model (each keeps its own activation pool: ~1.5 GB at 1024 x 2048)
    GRAPH_THRASH_MAX = 4     # never-replayed graphs evicted before the model gives up capturing new keys
    LAUNCH_BOUND_RATIO = 0.95      # graph_replay = "auto": capture a shape when host issue time >= this fraction of the GPU span of an eager forward
    GRAPH_REMEASURE_EVERY = 32     # ... and measure a GPU-bound shape again after this many eager calls

    def _replay_state(self):
        """the one transient home of everything graph replay remembers (graph_replay.GraphReplay); never copied or pickled"""
        return self.__dict__.get("_replay") or self.__dict__.setdefault("_replay", GraphReplay())

    def graph_decisions(self):
        """graph_replay = "auto": {(image shape, dtype, return_argmax, score): {"decision": "eager" | "replay", "host_issue_ms", "gpu_span_ms"}} of the last
        measurement of every shape met so far (bench.py reports it; tests assert on it)"""
        return dict(self._replay_state().decisions)

    def _measured_eager(self, key, batched_inputs, return_argmax, score):
        import time
        dev = self.device
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record(torch.cuda.current_stream(dev))
        out = self._rba_scores_eager(batched_inputs, return_argmax, score)
        e1.record(torch.cuda.current_stream(dev))
        self._replay_state().measured(key, time.perf_counter() - t0, e0, e1)
        return out

    def _weights_version(self):
        """The weights' part of the graph key: (epoch, sum of the versions) over a flat list of every parameter AND buffer (BatchNorm statistics are read
        by the graphs too).  The module tree is walked only when torch's global module-registration hooks fired since the last call (a parameter, buffer
        or submodule was set anywhere: load_state_dict(assign=True), `mod.weight = nn.Parameter(..)`, a submodule swap); the walk -- 1.3 ms for Swin-B,
        paid by a serial caller in front of every image's first launch -- is never per call.  The epoch moves when the walk finds other objects or a
        tensor's data pointer moved (`p.data = t` changes no version); within an epoch versions only grow, so their sum changes with every in-place edit.
        Not seen (as by every weight cache of this package): in-place edits through `p.data`, which bypass the version counter."""
        st = self.__dict__.get("_param_flat")
        gen = _REGISTRATIONS[0]
        if st is None or st[0] != gen:
            flat = list(self.parameters()) + list(self.buffers())
            same = st is not None and len(flat) == len(st[2]) and all(a is b for a, b in zip(flat, st[2]))
            st = self.__dict__["_param_flat"] = [gen, st[1] if same else next(_EPOCHS), flat, st[3] if same else None]
        v = 0
        for t_ in st[2]:
            v += t_._version
        ptrs = [t_.data_ptr() for t_ in st[2]]
        if ptrs != st[3]:
            if st[3] is not None:
                st[1] = next(_EPOCHS)
            st[3] = ptrs
        return st[1], v

    def _graph_key(self, image, return_argmax, score):
        return GraphKey(tuple(image.shape), image.dtype, image.device, torch.cuda.current_stream(image.device).cuda_stream, bool(return_argmax), score,
                        self.fused_upsample, self.fused_front_end, ops.SPLIT_MODE, ops.SPLIT_ACTIVATIONS, ops.TILES_MIN, ops.MLP_FUSED_MIN_ROWS,
                        ops.concurrent_streams(), ops.SWIN_ATTN_FUSED,
                        (getattr(self.sem_seg_head.predictor, "sparse_intermediate_heads", None), ops.COMPOSED_MASK_HEAD), self._weights_version())

    def drop_graphs(self, release_constants=False):
        """Forget every captured graph (their pools are freed); the next calls run eagerly, then capture again.  release_constants: also
        un-pin the per-shape constants captures have read (lru.ShapeCache) -- only safe when no graph captured OUTSIDE the model (bench.py,
        evaluate_ood.GraphedScore) is still alive, e.g. after a device move."""
        if release_constants:
            for m_ in self.modules():
                for v_ in vars(m_).values():
                    if isinstance(v_, ShapeCache):
                        v_.unpin()
        self._replay_state().drop()

    _TRANSIENT = ("_replay", "_param_flat")       # hipGraphs / events cannot be copied or pickled; a copy captures its own

    def __getstate__(self):
        st = dict(super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__)
        for k in self._TRANSIENT:
            st.pop(k, None)
        return st

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in self._TRANSIENT:
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def _apply(self, fn, *args, **kwargs):
        self.__dict__.pop("_param_flat", None)
        self.drop_graphs(release_constants=True)   # .to() / .cuda() / .float(): every captured graph holds the old parameter addresses
        return super()._apply(fn, *args, **kwargs)

    def _graphed_scores(self, image, return_argmax, score):
        """One batch-1 image (already on the device) -> (rba, argmax | None), replayed from a hipGraph captured per GraphKey (image shape, dtype, stream,
        outputs, arithmetic mode, weight version ...).  A forward is ~330 kernel launches that take the Python thread 6-7 ms to issue against ~8 ms of GPU
        time; a caller that waits for every score (the reference's loop does: `.cpu()` per image, support.py:375) pays both in series.  When and whether a key
        is captured is GraphReplay.step's decision; a replay copies the image into the graph's input and runs on the CURRENT stream, the result is a fresh
        tensor.  Returns None when the caller is to run eagerly, and the key when that eager run is the one to be measured (_measured_eager)."""
        state = self._replay_state()
        key = self._graph_key(image, return_argmax, score)
        what = state.step(key, self.graph_replay == "auto", self)
        if what == "measure":
            return key
        if what == "capture":
            try:
                cap = torch.cuda.Stream(device=image.device)       # its own capture stream: per-stream state (K1's tile counter) is this graph's alone
                state.captured(key, *capture(lambda x: self._rba_scores_eager([{"image": x}], return_argmax, score)[0], image, cap), stream=cap)
            except Exception as e:                                   # noqa: BLE001 -- an optimisation only
                import sys
                print(f"[rba_amd] hipGraph capture failed for image shape {tuple(image.shape)} ({type(e).__name__}: {e}); eager launches",
                      file=sys.stderr)
                torch.cuda.synchronize(image.device)
                state.captured(key)
        rec = state.graphs.get(key) if what in ("replay", "capture") else None
        if rec is None or rec.state != "captured":
            return None
        rec.static_in.copy_(image, non_blocking=True)
        rec.graph.replay()
        r = rec.static_out
        return (r[0].clone(), r[1].clone()) if return_argmax else r.clone()

    def live_graphs(self):
        return self._replay_state().live()

    @torch.no_grad()
    def rba_scores(self, batched_inputs, return_argmax=False, score="rba"):
        """Fast path: anomaly-score maps (and optional int32 argmax maps) without materialising sem_seg.
        score: "rba" (evaluate_ood.py:143-150), "energy" (:152-159) or "neg_logit_sum" (support.py:115-132).
        Batch-1 calls on a HIP device are replayed from a captured hipGraph -- with ``model.graph_replay = True`` from the third call of an image shape on, with
        the default "auto" from the fourth call on and only for shapes whose eager launches are measured to be launch-bound (see _graphed_scores);
        ``model.graph_replay = False`` opts out."""
        if (self.graph_replay and len(batched_inputs) == 1 and self.device.type == "cuda"
                and not torch.cuda.is_current_stream_capturing()):
            image = batched_inputs[0]["image"]
            if torch.is_tensor(image) and image.dim() == 3 and image.dtype in (torch.uint8, torch.float32) \
                    and set(batched_inputs[0]) <= {"image"}:
                image = to_device(image, self.device).contiguous()
                batched_inputs = [{"image": image}]
                if self.graph_replay == "auto":
                    # a shape measured to be GPU-bound stays eager for GRAPH_REMEASURE_EVERY calls without even building the graph key (the key walks every
                    # parameter's version: host time in front of the image's first launch, which the serial caller pays in full).  A stale entry costs
                    # speed only -- eager launches are always right.
                    fast = self._replay_state().eager_left
                    fk = (tuple(image.shape), image.dtype, bool(return_argmax), score, ops.SPLIT_MODE, torch.cuda.current_stream(image.device).cuda_stream)
                    left = fast.get(fk, 0)
                    if left > 0:
                        fast[fk] = left - 1
                        return self._rba_scores_eager(batched_inputs, return_argmax, score)
                r = self._graphed_scores(image, return_argmax, score)
                if isinstance(r, GraphKey):                     # graph_replay = "auto": this eager call is the one that is measured
                    return self._measured_eager(r, batched_inputs, return_argmax, score)
                if r is not None:
                    return [r]
        return self._rba_scores_eager(batched_inputs, return_argmax, score)

    @torch.no_grad()
    def _rba_scores_eager(self, batched_inputs, return_argmax=False, score="rba"):
        mask_cls, mask_pred, sizes, padded = self.predict(batched_inputs)
        out = []
        for i in range(len(batched_inputs)):
            rba, _, arg = self._post(mask_cls[i], mask_pred[i], sizes[i], padded, False, return_argmax, score)
            out.append((rba, arg) if return_argmax else rba)
        return out
