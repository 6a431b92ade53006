/*
 * rba_hip.h -- C ABI of librba_hip.so, the MI355X (gfx950) kernels on RbA's inference hot path.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer owned by the caller; nothing is allocated; no environment variables are read and
 *     there is no mutable global state except the launch-geometry hint of rba_set_concurrent_streams -- `nm -D librba_hip.so` shows no writable rba_ symbol:
 *     the kernel-variant knobs of csrc/knobs.h are compile-time constants here and variables only in the tools' knobs build librba_hip_knobs.so (the
 *     only other process-wide side effects: the first launch of a kernel that needs more than 64 KiB of LDS sets that kernel's
 *     hipFuncAttributeMaxDynamicSharedMemorySize once, and the persistent kernels cache the device's CU count); re-entrant; tensors
 *     are dense row-major ("contiguous") in the index order written next to them;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); kernels are only enqueued;
 *   - return value is a hipError_t as int (0 = hipSuccess); argument errors return hipErrorInvalidValue (1);
 *   - fp32 everywhere (the reference op refuses half: pixel_decoder/msdeformattn.py:323,329).
 *
 * Reference interfaces replaced (paths relative to the reference repo NazirNayal8/RbA):
 *   rba_ms_deform_attn_fwd_f32  <- MultiScaleDeformableAttention.ms_deform_attn_forward
 *                                  (pixel_decoder/ops/src/vision.cpp:19, ops/src/ms_deform_attn.h:25-44,
 *                                   ops/src/cuda/ms_deform_attn_cuda.cu:25-85, ms_deform_im2col_cuda.cuh:242-304,928-959)
 *   rba_ms_deform_attn_bwd_f32  <- MultiScaleDeformableAttention.ms_deform_attn_backward
 *                                  (pixel_decoder/ops/src/vision.cpp:20, ops/src/ms_deform_attn.h:46-66,
 *                                   ops/src/cuda/ms_deform_attn_cuda.cu:88-158)
 *   rba_reduce_f32              <- MaskFormer.semantic_inference (mask2former/maskformer_model.py:381-386)
 *                                  + get_RbA (evaluate_ood.py:143-150) + argmax (support.py:385-388)
 *   rba_reduce_bwd_f32          <- autograd's backward of SetCriterion.outlier_loss's score (mask2former/modeling/criterion.py:449-463)
 *   rba_sem_seg_bwd_f32         <- autograd's backward of the class map einsum("bqc,bqhw->bchw", softmax, sigmoid) (criterion.py:394-405)
 *   rba_reduce_up4_f32          <- the same preceded by the x4 mask upsample (maskformer_model.py:294-299)
 *                                  and followed by the sem_seg_postprocess crop (maskformer_model.py:330-332)
 *   rba_resample_bilinear_f32   <- F.interpolate(mode="bilinear", align_corners=False) call sites
 *                                  (maskformer_model.py:294-299, msdeformattn.py:358, mask2former_transformer_decoder.py:483)
 *   rba_masked_xattn_f32        <- nn.MultiheadAttention core with bool attn_mask
 *                                  (mask2former_transformer_decoder.py:106-118, 433, 483-487)
 *   rba_masked_xattn_bwd_f32    <- autograd's backward of that core (the whole-decoder fine-tune of the PEBAL recipe)
 *   rba_mask_logits_f32         <- torch.einsum("bqc,bchw->bqhw") (mask2former_transformer_decoder.py:479)
 *   rba_mask_logits_f16x3_f32   <- the same call site, f16x3 arithmetic
 *   rba_mask_logits_bwd_f32     <- autograd's backward of that einsum (mask2former_transformer_decoder.py:479 under autograd)
 *   rba_point_sample_f32        <- detectron2's point_sample (mask2former/modeling/criterion.py:216-234, matcher.py:122-132)
 *   rba_mask_point_loss_fwd_f32 <- point_sample of the matched masks + sigmoid_ce_loss + dice_loss (criterion.py:23-68, 230-239);
 *   rba_mask_point_loss_bwd_f32    autograd's backward of the three
 *   rba_match_cost_f32          <- the cost matrix of HungarianMatcher.memory_efficient_forward (matcher.py:105-149)
 *   rba_outlier_tail_fwd_f32    <- SetCriterion.outlier_loss behind its score map: F.interpolate(align_corners=True), the masked terms and
 *   rba_outlier_tail_bwd_f32       means (criterion.py:474-518); autograd's backward of them
 *   rba_dense_hybrid_loss_fwd_f32 <- SetCriterion.densehybrid_loss behind its class map: the two F.interpolate(align_corners=True), log_softmax,
 *   rba_dense_hybrid_loss_bwd_f32    logsumexp, get_batch_avg and the two nll_loss (criterion.py:93-97, 406-431); autograd's backward of them
 *   rba_gambler_loss_fwd_f32    <- SetCriterion.gambler_loss behind its class map: F.interpolate(align_corners=True), softmax, logsumexp,
 *   rba_gambler_loss_bwd_f32       GaussianBlur(7, 1) of the squared reward, the masked log terms (criterion.py:337-388); autograd's backward
 *   rba_gaussian_blur_planes_f32 / _adjoint_f32 <- that blur on B planes and autograd's backward of it
 *   rba_score_reg_fwd_f32       <- SetCriterion.smoothness_loss / sparsity_loss behind their score map (criterion.py:270-279, 311-319);
 *   rba_score_reg_bwd_f32          autograd's backward of them
 *   rba_tta_merge_f32           <- SemanticSegmentorWithTTA._inference_one_image behind the per-view forwards: sem_seg_postprocess, flip, +=, / n
 *                                  (mask2former/test_time_augmentation.py:83-97, maskformer_model.py:330-332) + the score functions of K1
 *   rba_resize_u8_pil_bilinear  <- Detectron2's ResizeTransform on a uint8 image = Pillow's Image.resize(BILINEAR), with HFlipTransform folded in
 *                                  (DatasetMapperTTA; TEST.AUG of configs/cityscapes/semantic-segmentation/Base-Cityscapes-SemanticSegmentation.yaml)
 *   rba_confusion_accum         <- Detectron2's SemSegEvaluator.process: np.bincount((K + 1) * pred + gt) per image (train_net.py:96-121 builds it)
 *   rba_train_view_u8           <- MaskFormerSemanticCocoMixDatasetMapper.__call__ behind the decode: mix_object, ResizeShortestEdge, RandomCrop,
 *                                  ColorAugSSDTransform, RandomFlip, the pad and the outlier mask (mask_former_semantic_coco_mix_dataset_mapper.py)
 *   rba_grad_sqnorm_f32         <- Trainer.build_optimizer's FullModelGradientClippingOptimizer over torch.optim.AdamW: clip_grad_norm_ and the
 *   rba_clip_adamw_step_f32        AdamW step of every trained tensor (train_net.py:303-328)
 *   rba_swin_window_attn_f32    <- WindowAttention core + window_partition/reverse + roll + pad
 *                                  (backbone/swin.py:44-71, 131-171, 251-284)
 *   rba_skinny_linear_f32       <- nn.Linear / in_proj / MLP on the decoder's [100, B, 256] query tensors
 *                                  (mask2former_transformer_decoder.py:25-212)
 *   rba_bn_relu_conv1x1_f32     <- BNReluConv(hidden_dim, 2, k=1) `ood_pred` head (mask2former_transformer_decoder.py:216-230, 467-468)
 *   rba_split_linear_f32        <- nn.Linear on the backbone's token tensors: qkv / proj / Mlp.fc1(+GELU) / Mlp.fc2 /
 *                                  PatchMerging.reduction (backbone/swin.py:44-71, 131-171, 319-343)
 *   rba_token_linear_f32        <- nn.Linear on the encoder / decoder-memory token tensors (pixel_decoder/msdeformattn.py:101-140,
 *                                  ops/modules/ms_deform_attn.py:95-121, mask2former_transformer_decoder.py:83-143) [+ residual + LayerNorm]
 *   rba_gaussian_blur_f32       <- transforms.GaussianBlur(7, sigma=1) on the anomaly map (support.py:366-383)
 *   rba_threshold_u8 / rba_morph3x3_u8 / rba_ccl4_roots_i32 <- the open-set branch of MaskFormer.panoptic_inference
 *                                  (maskformer_model.py:454-481: threshold, cv2.morphologyEx open/close, cv2.connectedComponents)
 *   rba_panoptic_merge_f32 / rba_panoptic_merge_up4_f32 / rba_panoptic_assign_i32 <- the closed-set merge of MaskFormer.panoptic_inference
 *                                  (maskformer_model.py:395-452: sigmoid, score product, argmax, the per-query area tests' sums, the id writes)
 *   rba_segment_pairs_accum     <- pq_compute_single_core's np.unique(pan_gt * OFFSET + pan_pred) (mask2former/evaluation/evaluation.py:152-159)
 *   rba_instance_stats_f32 / rba_instance_stats_up4_f32 / rba_instance_masks_{f32,u8} / rba_instance_masks_up4_{f32,u8} <- MaskFormer.instance_inference
 *                                  (maskformer_model.py:503-524: the gathered planes, `> 0`, sigmoid, product, the two sums; BitMasks boxes of :520)
 *   rba_subset_curves_{totals,walk,finish} / rba_labelled_tags_i32 <- OODEvaluator.evaluate_ood_bootstrapped behind ONE scoring pass: the per-trial
 *                                  roc_curve, auc, average_precision_score and FPR95 of every image subset (support.py:247-285, 305-351)
 *   rba_add_layer_norm_f32      <- `x = x + proj(...)` followed by nn.LayerNorm (swin.py:284-293 and the post-norm layers
 *                                  of msdeformattn.py:134-138, mask2former_transformer_decoder.py:48-58,106-118,171-175)
 *   rba_group_norm_f32          <- GroupNorm(32) [+ ReLU] behind Detectron2's Conv2d(norm=get_norm("GN"), activation)
 *                                  (pixel_decoder/msdeformattn.py:222-235, 278-297)
 */
#ifndef RBA_HIP_H
#define RBA_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Library/ABI version (major*100 + minor). */
int rba_hip_version(void);

/* Launch-geometry hint, the library's only caller-set state: the number of streams of this process that launch forwards concurrently
 * (default 1).  With n >= 2 the K6 launches that fill only half the chip take whole CUs (8-wave 256 x 128 workgroups) and leave the rest to the
 * other streams' kernels.  Affects speed only: every kernel form gives bit-identical results.  Returns the previous setting (n < 1 counts as 1).
 * Not thread-safe against concurrent launches; set it before the streams start (bench.py, evaluate_ood.run_evaluations do). */
int rba_set_concurrent_streams(int n);

/* K1.  mask [Q,HW] full-resolution mask logits; cls_prob [Q,K] = softmax(class logits)[:, :-1].
 *   sem[k,p]  = sum_q cls_prob[q,k] * sigmoid(mask[q,p])      (ascending-q fp32 FMA order)
 *   rba[p]    = - sum_k tanh(sem[k,p])                     (score_mode 0, RbA: evaluate_ood.py:143-150)
 *             = - logsumexp_k sem[k,p]                     (score_mode 1, energy: evaluate_ood.py:152-159)
 *             = - sum_k sem[k,p]                           (score_mode 2, negative logit sum: support.py:115-132)
 *   argmax[p] = first k maximising sem[k,p]
 * rba [HW] required; sem_seg [K,HW] and argmax [HW] (int32) optional (NULL = not written).  1 <= K <= 160. */
int rba_reduce_f32(const float* mask, const float* cls_prob, float* rba, float* sem_seg, int32_t* argmax,
                   int Q, int K, int64_t HW, int score_mode, void* stream);

/* The same with dynamic tile assignment: `workspace` = 8 bytes of device memory owned by the caller, zero before the first use
 * (the kernel leaves it zero); one workspace per stream that may run K1 concurrently.  Workgroups fetch their tiles from an atomic
 * counter in it, which evens out the per-CU rate spread of the static split (same results bit for bit). */
int rba_reduce_ws_f32(const float* mask, const float* cls_prob, float* rba, float* sem_seg, int32_t* argmax, int Q, int K,
                      int64_t HW, int score_mode, void* workspace, void* stream);

/* K1 fused with the x4 bilinear upsample (align_corners=False) in front and the crop behind it.
 * mask_lowres [Q,h,w]; the virtual full-resolution map is [Q,4h,4w]; outputs cover rows < crop_h and
 * columns < crop_w of it: rba [crop_h,crop_w], sem_seg [K,crop_h,crop_w] or NULL, argmax or NULL. */
int rba_reduce_up4_f32(const float* mask_lowres, const float* cls_prob, float* rba, float* sem_seg,
                       int32_t* argmax, int Q, int K, int h, int w, int crop_h, int crop_w, int score_mode, void* stream);

/* K1 backward.  Gradients of rba_reduce_f32's score with respect to mask and cls_prob, given grad_score [HW] = dL/d rba (the heavy differentiable
 * piece of SetCriterion.outlier_loss, mask2former/modeling/criterion.py:449-463: sigmoid, einsum("bqc,bqhw->bchw"), tanh / logsumexp / sum):
 *   sig = sigmoid(mask);  s[k,p] = sum_q cls_prob[q,k] sig[q,p]          (recomputed: nothing but the forward's two inputs is needed)
 *   u[k,p] = grad_score[p] * ( -(1 - tanh^2 s) | -softmax_k(s) | -1 )    (score_mode 0 | 1 | 2; the softmax is max-subtracted)
 *   grad_mask[q,p] = sig (1 - sig) sum_k cls_prob[q,k] u[k,p]            (sig (1 - sig) from sig: exactly 0 where sig is 0 or 1, never NaN)
 *   grad_prob[q,k] = sum_p sig[q,p] u[k,p]
 * grad_mask [Q,HW] and grad_prob [Q,K] are each optional (NULL = not computed), at least one is required.  Both are written element by element
 * with plain stores, whatever they held before, and are bitwise reproducible from launch to launch: grad_prob is summed per 128-pixel tile into
 * `workspace` and then over the tiles in a fixed order (no float atomics).  `workspace`: device memory owned by the caller, 4-byte aligned, at
 * least rba_reduce_bwd_workspace_f32's byte count, needed only with grad_prob; its contents on entry do not matter.  1 <= K <= 160, Q >= 1,
 * HW >= 1; anything else returns hipErrorInvalidValue without a launch. */
int rba_reduce_bwd_workspace_f32(int Q, int K, int64_t HW, int64_t* bytes);
int rba_reduce_bwd_f32(const float* mask, const float* cls_prob, const float* grad_score,
                       float* grad_mask /* [Q,HW] or NULL */, float* grad_prob /* [Q,K] or NULL */,
                       int Q, int K, int64_t HW, int score_mode,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* The per-class adjoint of K1: the same kernel with u[k,p] = grad_sem[k,p] given instead of derived from a one-channel grad_score -- the
 * gradients of sem_seg[k,p] = sum_q cls_prob[q,k] sigmoid(mask[q,p]) (rba_reduce_f32's sem_seg output; K10's input) with respect to mask and
 * cls_prob, given grad_sem [K,HW] = dL/d sem_seg:  grad_mask[q,p] = sig (1 - sig) sum_k cls_prob[q,k] grad_sem[k,p],  grad_prob[q,k] =
 * sum_p sig[q,p] grad_sem[k,p].  Tiling, workspace (rba_reduce_bwd_workspace_f32), fixed-order sum, optional outputs, domain and refusals are
 * rba_reduce_bwd_f32's. */
int rba_sem_seg_bwd_f32(const float* mask, const float* cls_prob, const float* grad_sem /* [K,HW] */,
                        float* grad_mask /* [Q,HW] or NULL */, float* grad_prob /* [Q,K] or NULL */,
                        int Q, int K, int64_t HW, void* workspace, int64_t workspace_bytes, void* stream);

/* Bilinear resample, align_corners=False, no antialias (ATen upsample_bilinear2d semantics):
 * in [C,h,w] -> out [C,H,W];  if `add` != NULL (same shape as out): out = resample(in) + add. */
int rba_resample_bilinear_f32(const float* in, const float* add, float* out, int C, int h, int w, int H, int W,
                              void* stream);

/* K2.  Multi-scale deformable attention forward.
 * value [N,S,M,D]; spatial_shapes [L,2] int64 (H_l,W_l); level_start_index [L] int64;
 * sampling_loc [N,Lq,M,L,P,2] (x,y) normalised to [0,1]; attn_weight [N,Lq,M,L,P]; out [N,Lq,M*D].
 * Sample position h = y*H_l - 0.5, w = x*W_l - 0.5; bilinear, taps outside the map contribute 0. */
int rba_ms_deform_attn_fwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const float* sampling_loc, const float* attn_weight, float* out,
                               int N, int S, int M, int D, int L, int Lq, int P, void* stream);
/* The same op in double precision -- the reference FFI dispatches float and double (ops/src/cuda/ms_deform_attn_cuda.cu:69, AT_DISPATCH_FLOATING_TYPES;
 * ops/test.py:35-47 checks the double path first).  Same shapes and checks; generic kernel. */
int rba_ms_deform_attn_fwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const double* sampling_loc, const double* attn_weight, double* out,
                               int N, int S, int M, int D, int L, int Lq, int P, void* stream);

/* K2 backward.  Gradients of the op above with respect to value, sampling_loc and attn_weight, given grad_out [N,Lq,M*D]
 * (replaces MultiScaleDeformableAttention.ms_deform_attn_backward: pixel_decoder/ops/src/vision.cpp:20, ops/src/ms_deform_attn.h:46-66,
 * ops/src/cuda/ms_deform_attn_cuda.cu:88-158).  Inputs as the forward; grad_value [N,S,M,D], grad_sampling_loc [N,Lq,M,L,P,2],
 * grad_attn_weight [N,Lq,M,L,P].  On return (stream order) all three outputs are fully defined whatever they held before: grad_value is
 * zero-filled here (hipMemsetAsync on `stream`) and then summed with float atomics -- its last bits depend on arrival order and may differ
 * from launch to launch; the other two are written element by element with plain stores and are bitwise reproducible.  A sample outside the
 * window (h <= -1, h >= H_l, w <= -1 or w >= W_l) gets exactly 0 in grad_sampling_loc and grad_attn_weight.  N == 0 or Lq == 0: success
 * without a kernel launch (grad_value still zero-filled when it has elements). */
int rba_ms_deform_attn_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const float* sampling_loc, const float* attn_weight, const float* grad_out,
                               float* grad_value, float* grad_sampling_loc, float* grad_attn_weight,
                               int N, int S, int M, int D, int L, int Lq, int P, void* stream);
/* The same in double precision (the reference dispatches both; its gradient test, ops/test.py:66-89, runs in double).  Generic kernel. */
int rba_ms_deform_attn_bwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                               const double* sampling_loc, const double* attn_weight, const double* grad_out,
                               double* grad_value, double* grad_sampling_loc, double* grad_attn_weight,
                               int N, int S, int M, int D, int L, int Lq, int P, void* stream);

/* The sampling parameters of MSDeformAttn.forward in one pass (pixel_decoder/ops/modules/ms_deform_attn.py:95-115):
 * raw [rows, M*L*P*2 | M*L*P] = the sampling_offsets and attention_weights Linears evaluated as one; reference_points [rows, L, 2];
 * spatial_shapes [L,2] int64 (H, W) -> loc [rows, M, L, P, 2] = reference + offset / (W_l, H_l), attw [rows, M, L, P] = softmax over L*P. */
int rba_msda_prepare_f32(const float* raw, const float* reference_points, const int64_t* spatial_shapes, float* loc, float* attw,
                         int64_t rows, int M, int L, int P, void* stream);

/* MSDeformAttn.forward's core in one launch: sampling locations + softmax (ms_deform_attn.py:95-115) computed inside the gather kernel
 * from `raw` (layout as rba_msda_prepare_f32), reference_points [N*Lq, L, 2], value [N, S, M, 32] -> out [N, Lq, M*32].
 * head_dim 32, P = 4, L in {1, 3}; bit-identical to rba_msda_prepare_f32 + rba_ms_deform_attn_fwd_f32. */
int rba_msda_fused_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index, const float* raw,
                       const float* reference_points, float* out, int N, int S, int M, int D, int L, int Lq, int P, void* stream);

/* K3.  Masked multi-head cross attention core (projections are done by the caller):
 * q [B,Q,nH,hd] (already includes the in_proj bias, NOT yet scaled), k,v [B,S,nH,hd];
 * mask_logits [B,Q,S] or NULL: key s is blocked for query q (all heads) iff sigmoid(mask_logits) < 0.5,
 * except that a row with every key blocked attends to all keys.  out [B,Q,nH*hd].
 * scale = hd^-0.5 applied to q.  hd must be 32.
 * workspace: rba_masked_xattn_workspace_bytes(B,Q,S,nH) bytes of scratch enables the split-key matrix-pipe path
 * (partial (m,l,O) per key range + merge); NULL selects the one-workgroup-per-(query,head) kernel. */
int64_t rba_masked_xattn_workspace_bytes(int B, int Q, int S, int nH);
int rba_masked_xattn_f32(const float* q, const float* k, const float* v, const float* mask_logits, float* out,
                         float* workspace, int B, int Q, int S, int nH, int hd, void* stream);

/* K3 backward.  Gradients of the op above with respect to q, k and v, given grad_out [B,Q,nH*hd] = d loss / d out.  Inputs exactly as the
 * forward's (q unscaled); mask_logits [B,Q,S] or NULL receives no gradient (the reference detaches it, mask2former_transformer_decoder.py:487).
 * Mask rule bit for bit the forward's: a pair is blocked iff mask_logits <= -0x1.7ffffep-23 (torch's fp32 sigmoid(x) < 0.5), a row whose keys
 * are all blocked attends to every key; a blocked (query, key) pair contributes exactly nothing to any gradient.
 *   s = hd^-0.5 q.k, p = softmax over the row's un-blocked keys, dp = grad_out.v, delta = sum_s p dp
 *   grad_v[s] = sum_q p grad_out[q]     ds = p (dp - delta) hd^-0.5     grad_k[s] = sum_q ds q     grad_q[q] = sum_s ds k[s]
 * Flash-style: the row statistics are recomputed, nothing of size [B*nH,Q,S] is written.  Exact fp32 FMA, no half-precision operand.
 * grad_q [B,Q,nH,hd], grad_k and grad_v [B,S,nH,hd] are each optional (NULL = not wanted and not computed; all three NULL is a no-op).  Every
 * requested output is written element by element with plain stores, whatever it held before, by ONE writer in a fixed summation order: all
 * three are bitwise reproducible from launch to launch (no float atomics, no hand-off between workgroups: grad_q is summed by the workgroup
 * that owns the whole query row).  `workspace`: device memory owned by the caller, 16-byte aligned, rba_masked_xattn_bwd_workspace_bytes
 * bytes (the row statistics; its contents on entry do not matter), required whenever a kernel is launched.  k, v, grad_k, grad_v 16-byte
 * aligned.  hd must be 32; S >= 1; 0 <= B, nH <= 65535; Q >= 0 (any, also > 128).  B == 0: success without a launch.  Q == 0: grad_k / grad_v
 * are zero-filled (hipMemsetAsync on `stream`), no kernel.  Anything else returns hipErrorInvalidValue without a launch. */
int64_t rba_masked_xattn_bwd_workspace_bytes(int B, int Q, int S, int nH);
int rba_masked_xattn_bwd_f32(const float* q, const float* k, const float* v, const float* mask_logits, const float* grad_out,
                             float* grad_q /* or NULL */, float* grad_k /* or NULL */, float* grad_v /* or NULL */, float* workspace,
                             int B, int Q, int S, int nH, int hd, void* stream);

/* K4.  Mask logits: out[b,q,n] = sum_c embed[b,q,c] * feat[b,c,n]   (embed [B,Q,C], feat [B,C,N], out [B,Q,N]). */
int rba_mask_logits_f32(const float* embed, const float* feat, float* out, int B, int Q, int C, int64_t N,
                        void* stream);
/* The same contraction in f16x3 arithmetic (three f16 matrix-pipe products per fp32 product, main + low accumulators; |x| < 65504, NaN
 * beyond): the form the model uses in its default arithmetic mode.  Shapes outside Q <= 112, C % 32 == 0, C <= 256 run rba_mask_logits_f32. */
int rba_mask_logits_f16x3_f32(const float* embed, const float* feat, float* out, int B, int Q, int C, int64_t N,
                              void* stream);

/* K4 backward.  With grad_out [B,Q,N] = d loss / d out of the contraction above (any arithmetic mode of the forward):
 *   grad_embed[b,q,c] = sum_n grad_out[b,q,n] feat[b,c,n]          grad_feat[b,c,n] = sum_q embed[b,q,c] grad_out[b,q,n]
 * in exact fp32 (v_mfma_f32_16x16x4_f32; a plain VALU form when N % 4 != 0 or a pointer is not 16-byte aligned).  grad_embed [B,Q,C] and
 * grad_feat [B,C,N] are each optional (NULL = not computed), at least one is required; `embed` is read only for grad_feat and `feat` only for
 * grad_embed, and the one that is not read may be NULL.  Both are written element by element with plain stores, whatever they held before,
 * and are bitwise reproducible from launch to launch: grad_embed is summed per slice of the pixel axis into `workspace` and then over the
 * slices in a fixed order (no float atomics).  `workspace`: device memory owned by the caller, 4-byte aligned, at least
 * rba_mask_logits_bwd_workspace_f32's byte count, needed only with grad_embed; its contents on entry do not matter.  Every shape of the
 * forward is accepted (Q, N >= 0, C >= 1, 0 <= B <= 65535); B, Q or N of 0 is a no-op that returns 0.  A negative size, both outputs NULL, a
 * NULL input that would be read, or grad_embed with a NULL or too small workspace returns hipErrorInvalidValue without a launch. */
int rba_mask_logits_bwd_workspace_f32(int B, int Q, int C, int64_t N, int64_t* bytes);
int rba_mask_logits_bwd_f32(const float* embed, const float* feat, const float* grad_out,
                            float* grad_embed /* may be NULL */, float* grad_feat /* may be NULL */,
                            int B, int Q, int C, int64_t N, void* workspace, int64_t workspace_bytes, void* stream);

/* K8.  Point-sampled mask losses and the matcher's cost (docs/kernels/K8.md).  Sampling rule of all four entry points = detectron2's point_sample,
 * F.grid_sample(x, 2 c - 1, mode="bilinear", padding_mode="zeros", align_corners=False): a point c = (x, y) in normalised coordinates reads the
 * plane [h,w] at the pixel coordinates (c_x w - 0.5, c_y h - 0.5) from its four neighbours floor / floor + 1; a neighbour outside the plane
 * contributes 0 and is never read.  Coordinates are finite floats; nothing else is assumed about them.
 *
 * rba_point_sample_f32: out[n,p] = planes[plane_index[n]] sampled at coords[n,p] (shared_coords = 0, coords [N,P,2]) or at coords[p]
 * (shared_coords = 1, coords [P,2]); planes [num_planes,h,w]; plane_index [N] int64 with repeats allowed, NULL = row n reads plane n (then
 * N <= num_planes).  A row whose index lies outside [0, num_planes) reads nothing and gets NaN.  N == 0 or P == 0: success without a launch.
 * N <= 65535; h w < 2^31.  Bitwise reproducible. */
int rba_point_sample_f32(const float* planes, const int64_t* plane_index /* may be NULL */, const float* coords, float* out,
                         int64_t num_planes, int N, int h, int w, int P, int shared_coords, void* stream);

/* The fused mask loss of N matched masks.  Mask n is plane plane_index[n] of pred_masks [num_planes,h,w] (num_planes = B Q; no copy of the matched
 * planes is made), sampled at coords[n] [N,P,2] to logits x[n,p] and reduced against labels [N,P] (fractional labels allowed) to
 *   sums[n] = ( sum_p max(x,0) - x t + log1p(exp(-|x|)),  a = sum_p sigmoid(x) t,  b = sum_p sigmoid(x),  c = sum_p t )          [N,4]
 *   losses[0] = loss_mask = sum_n (sums[n,0] / P) / num_masks         losses[1] = loss_dice = sum_n [1 - (2 a + 1) / (b + c + 1)] / num_masks
 * One workgroup per mask and a fixed-order finish: sums and both losses are bitwise reproducible from launch to launch (no float atomics).
 *
 * rba_mask_point_loss_bwd_f32: grad_masks [num_planes,h,w] = d (g_m loss_mask + g_d loss_dice) / d pred_masks with g_m = *grad_loss_mask and
 * g_d = *grad_loss_dice read on the device (no host synchronisation; one of the two may be NULL = 0); x and sigmoid(x) are recomputed from the
 * forward's inputs and `sums`.  On return (stream order) grad_masks is fully defined whatever it held before: it is zero-filled here
 * (hipMemsetAsync on `stream`), so the planes no mask names are exactly 0, and each named plane then receives its P x 4 bilinear contributions
 * with float atomics -- its last bits depend on arrival order and may differ from launch to launch.  The matcher gives a plane to at most one
 * mask; planes named twice receive the sum of both masks' contributions.  A mask whose index lies outside [0, num_planes) gives NaN sums and
 * losses and writes no gradient.  1 <= N <= 65535, P >= 1, num_masks > 0, h w < 2^31; anything else, or a NULL pointer other than one of the two
 * upstream gradients, returns hipErrorInvalidValue without a launch. */
int rba_mask_point_loss_fwd_f32(const float* pred_masks, const int64_t* plane_index, const float* coords, const float* labels,
                                float* sums, float* losses, int64_t num_planes, int N, int h, int w, int P, float num_masks, void* stream);
int rba_mask_point_loss_bwd_f32(const float* pred_masks, const int64_t* plane_index, const float* coords, const float* labels,
                                const float* sums, const float* grad_loss_mask /* may be NULL */, const float* grad_loss_dice /* may be NULL */,
                                float* grad_masks, int64_t num_planes, int N, int h, int w, int P, float num_masks, void* stream);

/* The matcher's cost matrix of one image in one call: pred_masks [Q,h,w] and tgt_masks [T,H,W] sampled at the shared coords [P,2] to x[q,p], t[m,p],
 *   cost[q,m] = w_mask ( sum_p softplus(x) - sum_p x t ) / P  +  w_class ( - cls_prob[q, tgt_ids[m]] )
 *             + w_dice ( 1 - (2 sum_p sigmoid(x) t + 1) / (sum_p sigmoid(x) + sum_p t + 1) )                                          [Q,T]
 * (batch_sigmoid_ce_loss's pos t + neg (1 - t) is softplus(x) - x t).  cls_prob [Q,K1] (K1 = K + 1 classes), tgt_ids [T] int64 in [0, K1); a target
 * whose id lies outside gets a NaN column.  Neither sampled tensor goes to memory: per-slice partial sums over the points go to `workspace` and are
 * added in a fixed order (no float atomics), so the matrix is bitwise reproducible from launch to launch.  `workspace`: device memory owned by
 * the caller, 4-byte aligned, at least rba_match_cost_workspace_f32's byte count; its contents on entry do not matter.  Q, T, P, K1 >= 1 of any
 * size (the target axis is walked in blocks); h w, H W < 2^31; anything else returns hipErrorInvalidValue without a launch. */
int rba_match_cost_workspace_f32(int Q, int T, int P, int64_t* bytes);
int rba_match_cost_f32(const float* pred_masks, const float* tgt_masks, const float* coords, const float* cls_prob, const int64_t* tgt_ids,
                       float* cost, int Q, int T, int P, int h, int w, int H, int W, int K1, float w_mask, float w_class, float w_dice,
                       void* workspace, int64_t workspace_bytes, void* stream);

/* K9.  The tail of SetCriterion.outlier_loss behind the score map (mask2former/modeling/criterion.py:474-518; docs/kernels/K9.md): score [B,h,w] is
 * upsampled to the labels' [B,H,W] as F.interpolate(mode="bilinear", align_corners=True) does -- scale = (h - 1) / (H - 1) as an fp32 quotient (0
 * when H == 1), src = scale Y, y0 = (int)src, y1 = y0 + (y0 < h - 1), ly = src - y0, hy = 1 - ly, columns alike, s = hy (hx v00 + lx v01) +
 * ly (hx v10 + lx v11) -- and reduced against labels (label_bytes = 8: int64, 1: uint8; 0 = inlier, 1 = outlier, anything else ignored):
 *   label 0: d = s - thr_in    label 1: d = thr_out - s    term = relu(d)^2 | d^2 | |d|   (func 0 | 2 | 3)
 *   stats = (sum_in, n_in, sum_out, n_out);  loss = sum_in / n_in, and with n_out > 0: 0.5 (sum_in / n_in + sum_out / n_out)
 *   func 1: binary cross-entropy with logits against (label == 1) over all B H W pixels (ignored labels are target 0, as in the reference):
 *           stats = (sum, B H W, 0, 0), loss = 0.5 sum / (B H W)
 * Kept from the reference: without an outlier pixel the inlier mean is not halved, and without an inlier pixel the loss is NaN (the mean of
 * nothing).  Per-workgroup partial sums go to `workspace` with plain stores and one workgroup adds them in a fixed order and forms the loss on the
 * device: no float atomics, no host read, loss [1] and stats [4] bitwise reproducible from launch to launch.  `workspace`: device memory owned by
 * the caller, 4-byte aligned, at least rba_outlier_tail_workspace_f32's byte count; its contents on entry do not matter.
 *
 * rba_outlier_tail_bwd_f32: grad_score [B,h,w] = *grad_loss d loss / d score, from the forward's inputs and `stats`; *grad_loss [1] and stats are read
 * on the device.  Gather form, one thread per score pixel over the label pixels whose taps name it, the taps recomputed exactly as the forward
 * does; written with plain stores whatever it held before, bitwise reproducible; a score pixel no label pixel samples (H < h) gets 0.
 * Subgradients as torch: relu'(0) = 0, sign(0) = 0.  A thread's walk is H W / (h w) label pixels times ~4, so an axis with h == 1 is walked
 * whole by every thread of it.
 * Every B, h, w, H, W >= 1 with B H W and B h w < 2^31 (H == 1, W == 1, h == 1 and down-sampling included); anything else, another label_bytes
 * or func, or a NULL pointer returns hipErrorInvalidValue without a launch. */
int rba_outlier_tail_workspace_f32(int B, int H, int W, int64_t* bytes);
int rba_outlier_tail_fwd_f32(const float* score, const void* labels, int label_bytes /* 1 or 8 */, int B, int h, int w, int H, int W, int func,
                             float thr_in, float thr_out, float* workspace, float* loss /* [1] */,
                             float* stats /* [4]: sum_in, n_in, sum_out, n_out */, void* stream);
int rba_outlier_tail_bwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, int func,
                             float thr_in, float thr_out, const float* stats, const float* grad_loss /* device, [1] */,
                             float* grad_score /* [B,h,w] */, void* stream);

/* K10.  SetCriterion.densehybrid_loss behind its class map (mask2former/modeling/criterion.py:406-431; docs/kernels/K10.md).  sem [B,K,h,w] (the
 * class map einsum("bqc,bqhw->bchw", softmax(cls)[..., :-1], sigmoid(mask))) and ood [B,2,h,w] (ood_pred) are sampled at every label pixel as
 * F.interpolate(mode="bilinear", align_corners=True) does (K9's tap arithmetic) -- the up-sampled maps are never written -- and reduced against
 * labels [B,H,W] (label_bytes = 8: int64, 1: uint8; < K: that class, 254: outlier, anything else ignored by the segmentation term).  Per pixel
 * x_k, o_c = the samples, L = logsumexp_k x_k:
 *   S_seg = sum_{label<K} (L - x_label), n_seg        S_ood = sum_{label=254} L, n_ood
 *   S_th = sum over ALL B H W pixels of (logsumexp_c o_c - o_[label=254]) (void pixels are target 0, as in the reference)   S_x = sum_all sum_k x_k
 *   m = S_x / (B K H W) (get_batch_avg; detached in the reference, no gradient here)
 *   loss_seg = S_seg / n_seg   loss_ood = S_ood / n_ood - m   loss_th = S_th / (B H W)   loss = loss_seg + beta loss_ood + 10 beta loss_th
 *   losses [4] = (loss, loss_seg, loss_ood, loss_th);  stats [8] = (S_seg, S_ood, S_th, S_x, n_seg, n_ood, B H W, m);  lse [B,H,W] = L
 * n_seg == 0 or n_ood == 0 gives NaN, the mean of nothing, as in the reference.  Per-workgroup partial sums (counts as integers) go to
 * `workspace` with plain stores and one workgroup adds them in a fixed order: no float atomics, no host read, every output bitwise reproducible
 * from launch to launch.  `workspace`: device memory owned by the caller, 4-byte aligned, at least rba_dense_hybrid_loss_workspace_f32's byte
 * count; its contents on entry do not matter.
 *
 * rba_dense_hybrid_loss_bwd_f32: with g = *grad_loss (the gradient of losses[0]; read on the device like stats), p_k = exp(x_k - L), q = softmax(o):
 *   d / d x_k (P) = g ([label<K] (p_k - [k = label]) / n_seg + beta [label=254] p_k / n_ood)     d / d o_c (P) = g 10 beta (q_c - [c = [label=254]]) / (B H W)
 * pulled back through the bilinear weights into grad_sem [B,K,h,w] and grad_ood [B,2,h,w].  Gather form: 16 lanes own one quarter-resolution pixel
 * and share the label pixels whose taps name it, the taps recomputed exactly as the forward does, L read from `lse`; a fixed order, plain stores
 * whatever the outputs held before, bitwise reproducible; a pixel no label pixel samples (H < h) gets 0.
 * Every B, h, w, H, W >= 1 with B H W and B K h w < 2^31 (non-integer ratios, down-sampling, h == 1 included), 1 <= K <= 32; anything else, another
 * label_bytes or a NULL pointer returns hipErrorInvalidValue without a launch. */
int rba_dense_hybrid_loss_workspace_f32(int B, int H, int W, int64_t* bytes);
int rba_dense_hybrid_loss_fwd_f32(const float* sem, const float* ood, const void* labels, int label_bytes /* 1 or 8 */, int B, int K, int h, int w,
                                  int H, int W, float beta, float* workspace, float* losses /* [4] */, float* stats /* [8] */,
                                  float* lse /* [B,H,W] */, void* stream);
int rba_dense_hybrid_loss_bwd_f32(const float* sem, const float* ood, const void* labels, int label_bytes, const float* lse, int B, int K, int h,
                                  int w, int H, int W, float beta, const float* stats, const float* grad_loss /* device, [1] */,
                                  float* grad_sem /* [B,K,h,w] */, float* grad_ood /* [B,2,h,w] */, void* stream);

/* K11a.  SetCriterion.gambler_loss behind its class map (mask2former/modeling/criterion.py:337-388; docs/kernels/K11.md).  sem [B,K+1,h,w] = the
 * class map einsum("bqc,bqhw->bchw", softmax(cls), sigmoid(mask)) WITH the no-object column: channel K is the reservation channel.  Every label
 * pixel samples its K + 1 values as F.interpolate(mode="bilinear", align_corners=True) does (K9's tap arithmetic); the up-sampled map is never
 * written.  labels [B,H,W] in K10's convention (label_bytes = 8: int64, 1: uint8; < K: an inlier pixel of that class, 254: outlier, anything
 * else void).  Per pixel, x_k = the samples:
 *   L_in = logsumexp_{k<K} x_k   L = logsumexp_{k<=K} x_k   p_k = exp(x_k - L)   reward r = L_in^2   R = GaussianBlur(7, sigma = 1)(r) per plane
 *   res = p_K / R     inlier: t_in = log(p_label + res) (no clamp)     outlier: t_out = sum_{k<K} log(max(p_k + res, 1e-7))
 *   losses [3] = (loss, S_in / n_in, [n_ood > 0] S_out / (n_ood K)),  loss = -(losses[1] + ood_reg losses[2]);  stats [4] = (S_in, S_out, n_in, n_ood)
 * n_in == 0 gives NaN, the mean of nothing, as in the reference; the reference's `ood_mask.sum() > 0` is decided on the device.  `reward` and R are
 * [B,H,W] maps (reward: scratch of the call; R: an output, kept for the backward); `workspace`: device memory owned by the caller, 4-byte aligned,
 * at least rba_gambler_loss_workspace_f32's byte count; its contents on entry do not matter.  No float atomics, no host read, every output
 * bitwise reproducible from launch to launch.
 *
 * rba_gambler_loss_bwd_f32: grad_sem [B,K+1,h,w] = *grad_loss d losses[0] / d sem, the gradient through the blurred reward included, from the
 * forward's inputs, `stats` and R (*grad_loss and stats are read on the device).  grad_R and grad_reward are [B,H,W] scratch maps of the call
 * (d / d R per pixel, then its pull-back through the adjoint of the reflect-padded blur).  Gather form as K10's backward: plain stores whatever
 * the outputs held before, bitwise reproducible; a pixel no label pixel samples (H < h) gets 0.
 * Every B, h, w >= 1 and H, W >= 4 (the blur's reflect padding of 3 needs a larger map) with B H W and B (K+1) h w < 2^31, B <= 65535,
 * 1 <= K <= 31; anything else, another label_bytes or a NULL pointer returns hipErrorInvalidValue without a launch. */
int rba_gambler_loss_workspace_f32(int B, int H, int W, int64_t* bytes);
int rba_gambler_loss_fwd_f32(const float* sem, const void* labels, int label_bytes /* 1 or 8 */, int B, int K, int h, int w, int H, int W,
                             float ood_reg, float* workspace, float* reward /* [B,H,W] scratch */, float* losses /* [3] */, float* stats /* [4] */,
                             float* R /* [B,H,W] */, void* stream);
int rba_gambler_loss_bwd_f32(const float* sem, const void* labels, int label_bytes, const float* R, int B, int K, int h, int w, int H, int W,
                             float ood_reg, const float* stats, const float* grad_loss /* device, [1] */, float* grad_R /* [B,H,W] scratch */,
                             float* grad_reward /* [B,H,W] scratch */, float* grad_sem /* [B,K+1,h,w] */, void* stream);

/* rba_gaussian_blur_f32 on B planes [B,H,W] per launch (for B = 1: its very bits), and the adjoint of that linear map -- NOT the blur itself:
 * within kernel_size / 2 pixels of a border the taps that the reflect padding folds back add.  grad_in = A^T grad_out in gather form, plain
 * stores, bitwise reproducible.  Odd kernel_size <= 15, sigma > 0, H and W > kernel_size / 2, 1 <= B <= 65535, in != out. */
int rba_gaussian_blur_planes_f32(const float* in, float* out, int B, int H, int W, int kernel_size, float sigma, void* stream);
int rba_gaussian_blur_planes_adjoint_f32(const float* grad_out, float* grad_in, int B, int H, int W, int kernel_size, float sigma, void* stream);

/* K11b.  SetCriterion.smoothness_loss and sparsity_loss behind their score map (criterion.py:270-279, 311-319; docs/kernels/K11.md).  score [B,h,w];
 * labels [B,H,W] (label_bytes = 8: int64, 1: uint8; 1 = outlier) or NULL (no "outlier_masks": H and W are then unused but must be >= 1).
 *   losses[0] = smoothness = 1/2 (sum_{y<h-1} (s[y+1,x] - s[y,x])^2 + sum_{x<w-1} (s[y,x+1] - s[y,x])^2)       (a sum, not a mean)
 *   losses[1] = sparsity = sqrt(sum_{label=1} up(s)^2), up = the align_corners=True bilinear upsample (K9's taps); 0 without labels or outlier pixel
 *   stats [2] = the two sums.  K9's partial / finish scheme: `workspace` as there (rba_score_reg_workspace_f32), bitwise reproducible, no host read.
 * rba_score_reg_bwd_f32: grad_score [B,h,w] = *grad_smooth d smoothness / d score + *grad_sparse d sparsity / d score (either pointer may be NULL = 0,
 * not both; read on the device), one thread per score pixel in K9's gather form; the sparsity part is 0 where the norm is 0 (torch.norm's backward).
 * Every B, h, w, H, W >= 1 with B H W and B h w < 2^31. */
int rba_score_reg_workspace_f32(int B, int h, int w, int H, int W, int64_t* bytes);
int rba_score_reg_fwd_f32(const float* score, const void* labels /* or NULL */, int label_bytes, int B, int h, int w, int H, int W, float* workspace,
                          float* losses /* [2] */, float* stats /* [2] */, void* stream);
int rba_score_reg_bwd_f32(const float* score, const void* labels /* or NULL */, int label_bytes, int B, int h, int w, int H, int W,
                          const float* stats, const float* grad_smooth /* device, [1] or NULL */, const float* grad_sparse /* device, [1] or NULL */,
                          float* grad_score /* [B,h,w] */, void* stream);

/* K5.  Swin (shifted-)window attention core over a token map, fusing zero-pad to a multiple of the window,
 * cyclic shift, window partition, q*scale @ k^T + relative-position bias (+ shift mask), softmax, @ v,
 * window reverse, un-shift and crop.
 * qkv [B,H*W,3,nH,hd] = Linear(norm1(x)) of the UNPADDED tokens; padded tokens take qkv_bias [3*nH*hd]
 * (= Linear(0)).  bias [nH,ws*ws,ws*ws] gathered relative-position bias.  shift = 0 or ws/2.
 * bias_frag: optional (NULL = unused) copy of `bias` permuted by rba_swin_bias_fragments_f32 into the order the
 * MFMA path's lanes consume it (coalesced loads); computed once per weight load.
 * out [B,H*W,nH*hd] (attention output before the proj Linear).  hd in {16,32,64}; ws*ws <= 256. */
int rba_swin_window_attn_f32(const float* qkv, const float* qkv_bias, const float* bias, const float* bias_frag,
                             float* out, int B, int H, int W, int nH, int hd, int ws, int shift, void* stream);
/* bias [nH,ws*ws,ws*ws] -> frag with rba_swin_bias_fragments_elems(nH, ws) floats. */
int64_t rba_swin_bias_fragments_elems(int nH, int ws);
int rba_swin_bias_fragments_f32(const float* bias, float* frag, int nH, int ws, void* stream);

/* GroupNorm over x [B,C,HW] with G groups (statistics over (C/G) x HW), y = (x-mean)*rstd*gamma[c] + beta[c],
 * optional ReLU.  `workspace` must hold rba_group_norm_workspace_bytes(B,C,HW,G) bytes (per-chunk moments).
 * x and y may alias. */
int64_t rba_group_norm_workspace_bytes(int B, int C, int HW, int G);
int rba_group_norm_f32(const float* x, const float* gamma, const float* beta, float* y, float* workspace,
                       int B, int C, int HW, int G, float eps, int relu, void* stream);

/* Channels-last variants of the two operators above for the token-layout (NHWC) FPN path:
 * group norm over x [B,P,C] (statistics per image and group over P x C/G elements; (C/G) % 4 == 0, 256 % (C/4) == 0, C <= 1024),
 * bilinear resample in [h,w,C] -> out [H,W,C] (+ add [H,W,C]); C % 4 == 0. */
int64_t rba_group_norm_nhwc_workspace_bytes(int B, int P, int C, int G);
int rba_group_norm_nhwc_f32(const float* x, const float* gamma, const float* beta, float* y, float* workspace, int B, int P, int C,
                            int G, float eps, int relu, void* stream);
int rba_resample_bilinear_nhwc_f32(const float* in, const float* add, float* out, int C, int h, int w, int H, int W, void* stream);

/* Fused residual add + LayerNorm over rows of length C (C % 4 == 0, C <= 8192):
 *   s = x (+ t) (+ t_bias[c]);  sum_out = s (optional, may alias x);  y = (s - mean) * rstd * gamma + beta.
 * t, t_bias, sum_out may be NULL.  (swin.py:284-293, msdeformattn.py:134-138, mask2former_transformer_decoder.py:48-58) */
int rba_add_layer_norm_f32(const float* x, const float* t, const float* t_bias, const float* gamma, const float* beta,
                           float* sum_out, float* y, int64_t rows, int C, float eps, void* stream);

/* PatchMerging's 2x2 gather + LayerNorm in one pass (backbone/swin.py:311-337): x [B, H, W, Cin] token-major ->
 * y [B * ceil(H/2) * ceil(W/2), 4*Cin] = LN(cat(x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2])), odd maps zero-padded. */
int rba_merge_layer_norm_f32(const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int Cin, float eps,
                             void* stream);

/* Skinny linear layer: out[m,n] = act(sum_k x[m,k] * weight[n,k] + bias[n]), x [M,K] with M <= 128, weight [N,K]
 * (nn.Linear layout), bias [N] or NULL, relu != 0 applies torch.relu exactly (NaN stays NaN -- the f16x3 kernels' loud answer to an out-of-range
 * operand must reach the score map --, +inf stays +inf, -inf becomes 0; every ReLU of this library: csrc/common.h rba_relu).  K % 32 == 0.  For the decoder's 100-query GEMMs
 * (mask2former_transformer_decoder.py:25-212). */
int rba_skinny_linear_f32(const float* x, const float* weight, const float* bias, float* out, int M, int N, int K,
                          int relu, void* stream);
/* The same with the query position embedding folded in: output columns n < add_cols (a multiple of 16) see x + x_add, the others x -- the
 * q / k / v projections of a self-attention layer (q = k = W (tgt + query_pos), v = W tgt; mask2former_transformer_decoder.py:48-58) as ONE
 * launch over the stacked in_proj weight [3E, E] with add_cols = 2E; x_add may be NULL.  seg_n > 0 (N % seg_n == 0) writes the result as
 * N / seg_n contiguous [M, seg_n] blocks (q, k, v separately contiguous) instead of [M, N]. */
int rba_skinny_linear_add_f32(const float* x, const float* x_add, int add_cols, const float* weight, const float* bias, float* out,
                              int M, int N, int K, int relu, int seg_n, void* stream);

/* fp32-accurate Linear on the bf16 matrix pipe: every fp32 value is the exact sum of three bf16 values, and six
 * bf16 x bf16 MFMAs (exact products, fp32 accumulation) reproduce the fp32 product to < 2^-24 relative.
 * rba_split_weight_bf16x3: weight [N,K] fp32 -> `packed`, 6*Np*K bytes (Np = N rounded up to 128, padding rows zero): the
 *                          three bf16 planes tiled as the kernel's LDS image, [Np/128][K/16][3][128][2][8] bf16 with the
 *                          8-element half h of row r in slot h ^ ((r >> 3) & 1).  Once per weight load.  K % 32 == 0.
 * rba_split_linear_f32:    out[m,n] = act(sum_k x[m,k] * weight[n,k] + bias[n]); x [M,K] fp32, `weight_packed` from
 *                          rba_split_weight_bf16x3 for the same (N, K), bias [N] or NULL; act 0 = none, 1 = exact (erf) GELU, 2 = ReLU. */
int rba_split_weight_bf16x3(const float* weight, void* packed, int N, int K, void* stream);
int rba_split_linear_f32(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                         int act, void* stream);

/* The same Linear with THREE f16 MFMAs per fp32 product (csrc/split_linear_h3.h): x = h + 2^-11 l with h = f16(x),
 * l = f16((x - h) 2^11); x w = h_x h_w + 2^-11 (h_x l_w + l_x h_w) to 2^-22 relative per term (as accurate as an fp32 GEMM,
 * whose accumulation rounding dominates), for |x|, |w| < 65504 -- beyond f16's range the output row is NaN.
 * rba_split_weight_f16x2:     weight [N,K] fp32 -> `packed`, 4*Np*K bytes: [Np/128][K/16][2][128][2][8] f16, sub-stage 2b+g of the
 *                             32-wide k block b holds for row r, in slot h ^ ((r >> 3) & 1), k = 32b + 16h + 8g + (0..7).  K % 32 == 0.
 * rba_split_linear_f16x3_f32: as rba_split_linear_f32 with `weight_packed` from rba_split_weight_f16x2. */
int rba_split_weight_f16x2(const float* weight, void* packed, int N, int K, void* stream);
int rba_split_linear_f16x3_f32(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                               int act, void* stream);
/* out = (residual + x W^T) + bias, no activation: the `x = x + proj(...)` / `x = x + fc2(...)` of a transformer block folded into the
 * GEMM epilogue (backbone/swin.py:284-293), in the order of operations of rba_add_layer_norm_f32's own add (bit-identical to it).
 * residual [M,N]; `out` may be `residual` itself. */
int rba_split_linear_f16x3_res_f32(const float* x, const void* weight_packed, const float* bias, const float* residual, float* out,
                                   int64_t M, int N, int K, void* stream);

/* Split activations: a [M, K] fp32 activation matrix held ONLY as the f16x3 GEMM's A operand, written by its producer (one split per
 * element instead of one per column tile of every consumer; contiguous 1 KiB wave loads and no arithmetic in the GEMM).  Image =
 * ceil(M / 32) * 32 * K * 4 bytes: per (32-row group rg, 32-wide block b of K) four 1 KiB pieces [h g0 | l g0 | h g1 | l g1], each
 * [half][row & 31][8 f16] with k = 32 b + 16 half + 8 g + i; h = f16(x) (rne), l = f16((x - h) * 2^11).  Rows M .. are padding and never
 * written.  K % 32 == 0.
 *   rba_add_layer_norm_frag_f32     = rba_add_layer_norm_f32 with y written as that image (norm1 -> qkv, norm2 -> fc1 of
 *                                     backbone/swin.py:235-295)
 *   rba_split_linear_f16x3_frag_f32 = rba_split_linear_f16x3_f32 / _res_f32 (residual non-NULL, act 0) reading it; bit-identical to the
 *                                     fp32-input entry points on the same values. */
int rba_add_layer_norm_frag_f32(const float* x, const float* t, const float* t_bias, const float* gamma, const float* beta,
                                float* sum_out, void* y_frag, int64_t rows, int C, float eps, void* stream);
int rba_split_linear_f16x3_frag_f32(const void* x_frag, const void* weight_packed, const float* bias, const float* residual, float* out,
                                    int64_t M, int N, int K, int act, void* stream);
/*   rba_swin_window_attn_split_out_f32 = rba_swin_window_attn_f32 with the attention output written as the proj Linear's split image
 *                                     (backbone/swin.py:165-168 -> :169); head_dim 32, 12 x 12 windows, bias_frag required. */
int rba_swin_window_attn_split_out_f32(const float* qkv, const float* qkv_bias, const float* bias_frag, void* out_frag, int B, int H, int W,
                                       int nH, int hd, int ws, int shift, void* stream);
/* K7 -- the attention half of a Swin block in one launch (backbone/swin.py:235-284: norm1 -> pad / roll / window_partition ->
 * WindowAttention (:131-171: qkv, relative-position bias, SW-MSA mask of :413-440, softmax, proj) -> window_reverse / un-roll / crop ->
 * `x = shortcut + x`), and optionally norm2 of :284-293:
 *     x [B, H*W, C] <- x + proj(window_attention(qkv(norm1(x))));    y2 [B, H*W, C] = norm2(x) when y2 != NULL
 * One workgroup per 12 x 12 window; f16x3 arithmetic (|values| < 65504, NaN beyond).  weight_image = rba_swin_attn_block_pack_f32 of
 * qkv.weight [3C, C] and proj.weight [C, C] (rba_swin_attn_block_weight_bytes(C) bytes); bias_frag = rba_swin_bias_fragments_f32 of the
 * gathered relative-position bias [C/32, 144, 144].  rba_swin_attn_block_supported(C, ws) says which geometries have a kernel
 * (hipErrorInvalidValue otherwise: the caller keeps the unfused sequence rba_add_layer_norm -> rba_split_linear -> rba_swin_window_attn
 * -> rba_split_linear). */
int rba_swin_attn_block_supported(int C, int ws);
int64_t rba_swin_attn_block_weight_bytes(int C);
int rba_swin_attn_block_pack_f32(const float* qkv_weight, const float* proj_weight, void* image, int C, void* stream);
int rba_swin_attn_block_f32(float* x, float* y2, const float* norm1_weight, const float* norm1_bias, float eps1, const void* weight_image,
                            const float* qkv_bias, const float* bias_frag, const float* proj_bias, const float* norm2_weight,
                            const float* norm2_bias, float eps2, int B, int H, int W, int C, int ws, int shift, void* stream);
/* K7, attention only: the same kernel without proj / residual -- norm1 -> qkv -> (shifted-)window attention, its output written as the proj Linear's split
 * image (rba_split_linear_f16x3_frag_f32 reads it; layout of rba_swin_window_attn_split_out_f32): the qkv tensor and norm1's output never exist.  For the
 * widths whose proj accumulators do not fit beside the resident rows (C = 256: Swin-B stage 2; C = 192: Swin-L stage 1); x is only read.  out_frag: ceil(B H W / 32) * 32 * C * 4 bytes. */
int rba_swin_attn_qkv_supported(int C, int ws);
int rba_swin_attn_qkv_split_out_f32(const float* x, void* out_frag, const float* norm1_weight, const float* norm1_bias, float eps1,
                                    const void* weight_image, const float* qkv_bias, const float* bias_frag, int B, int H, int W, int C, int ws,
                                    int shift, void* stream);
/*   rba_resample_bilinear_nhwc_split_out_f32 -> rba_conv3x3_nhwc_f16x3_split_in_f32 = the FPN's `lateral + F.interpolate(prev)` sum handed to
 *                                     its 3 x 3 output convolution as a split image of [B H W, C] rows (pixel_decoder/msdeformattn.py:352-361);
 *                                     the convolution (>= 256 tiles of 128 x 128) gathers the pieces of the neighbour pixels' rows. */
int rba_resample_bilinear_nhwc_split_out_f32(const float* in, const float* add, void* out_frag, int C, int h, int w, int H, int W,
                                             int64_t row0, void* stream);

/* The FPN's top-down step with its GroupNorms folded into the loads (pixel_decoder/msdeformattn.py:352-358): in = the previous level's raw
 * output-convolution result (normalised + ReLU'd on the fly when in_mr is given), add = the raw lateral-convolution result (normalised on
 * the fly when add_mr is given); *_mr = [G][2] (mean, rstd) of the image from rba_group_norm_nhwc_stats_f32.  out = fp32 [H, W, C] or, with
 * split_out, rows row0 .. of the split image the 3 x 3 convolution reads.  The arithmetic of the unfused GroupNorm + resample launches (equal up to fma contraction: one ulp). */
int rba_resample_bilinear_nhwc_gn_f32(const float* in, const float* in_mr, const float* in_gamma, const float* in_beta, int in_relu,
                                      const float* add, const float* add_mr, const float* add_gamma, const float* add_beta, void* out,
                                      int split_out, int C, int G, int h, int w, int H, int W, int64_t row0, void* stream);
/* (mean, rstd) per image and group of channels-last x [B, P, C]: the statistics half of rba_group_norm_nhwc_f32. */
int rba_group_norm_nhwc_stats_f32(const float* x, float* mr, float* workspace, int B, int P, int C, int G, float eps, void* stream);
int rba_conv3x3_nhwc_f16x3_split_in_f32(const void* x_frag, const void* weight_packed, const float* bias, float* out, int B, int H, int W,
                                        int C, int N, void* stream);
/*   rba_swin_mlp_fused_f16x3_f32 = the whole Mlp + residual of a Swin block with C = 128 in one kernel (csrc/mlp_fused_h3.h): the [M, HID]
 *                                     hidden tensor never leaves the registers (fc1's transposed accumulators become fc2's A fragments after
 *                                     one v_permlane32_swap); bit-identical to the two-kernel hand-over below. */
int rba_swin_mlp_fused_f16x3_f32(const float* x, const void* w1_packed, const float* b1, const void* w2_packed, const float* b2,
                                 const float* residual, float* out, int64_t M, int C, int HID, void* stream);
/*   rba_swin_mlp_fused_ln_f16x3_f32 = the same kernel with norm2 in its prologue: x <- x + fc2(GELU(fc1(LayerNorm(x)))) in place (backbone/swin.py:293). */
int rba_swin_mlp_fused_ln_f16x3_f32(float* x, const float* norm_weight, const float* norm_bias, float eps, const void* w1_packed, const float* b1,
                                    const void* w2_packed, const float* b2, int64_t M, int C, int HID, void* stream);
/*   rba_split_linear_f16x3_gelu_split_out = GELU(x W^T + bias) written as the split image of the NEXT Linear (Mlp.fc1 -> fc2,
 *                                     backbone/swin.py:35-41): the GEMM runs with its MFMA operands swapped (D^T = W x^T), so a lane ends
 *                                     up with consecutive output channels of one row and stores 16-byte pieces.  x: fp32 rows
 *                                     (x_is_split 0) or a split image (1).  N % 32 == 0; out_frag ceil(M / 32) * 32 * N * 4 bytes. */
int rba_split_linear_f16x3_gelu_split_out(const void* x, int x_is_split, const void* weight_packed, const float* bias, void* out_frag,
                                          int64_t M, int N, int K, void* stream);

/* The same GEMM with NHWC rows in and NCHW out: out[(b*N + n)*P + p] = sum_k x[b*P + p, k] * weight[n, k] + bias[n],
 * P = rows_per_image, M % P == 0 (the mask-feature 1x1 convolution of pixel_decoder/msdeformattn.py:298-306). */
int rba_split_linear_nchw_out_f32(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N,
                                  int K, int rows_per_image, void* stream);

/* The same operator (NHWC rows in, NCHW out) on the f16x3 kernel; weight_packed = rba_split_weight_f16x2.  The mask-feature projection
 * `self.mask_features(y)` (pixel_decoder/msdeformattn.py:362). */
int rba_split_linear_nchw_out_f16x3_f32(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                                        int rows_per_image, void* stream);

/* The same projection on a RAW convolution output x whose GroupNorm(G) (+ ReLU when relu != 0) is applied while the rows are loaded:
 * `self.mask_features(self.layer_1(y))` (pixel_decoder/msdeformattn.py:357-362; Conv2d(norm=GN, activation=relu) :278-297) without the pass
 * that writes the normalised map.  mr [B][G][2] = (mean, rstd) from rba_group_norm_nhwc_stats_f32; gamma / beta [K]; K % G == 0,
 * (K / G) % 4 == 0, rows_per_image % 128 == 0.  Bit-identical to rba_group_norm_nhwc_f32 followed by the entry above. */
int rba_split_linear_nchw_out_gn_f16x3_f32(const float* x, const float* mr, const float* gamma, const float* beta, int G, int relu,
                                           const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                                           int rows_per_image, void* stream);

/* The mask heads of the masked decoder WITHOUT the 1/4-resolution mask-feature map (docs/kernels/K4.md).  Nothing stands between
 * `self.mask_features(...)` (pixel_decoder/msdeformattn.py:362, a plain Conv2d(conv_dim, mask_dim, 1)) and
 * `torch.einsum("bqc,bchw->bqhw", mask_embed, mask_features)` (mask2former_transformer_decoder.py:479), so
 *     pred_masks[b,q,p] = sum_k (E W)[b,q,k] g[b,p,k] + (E bias)[b,q],   g = ReLU(GroupNorm(y)).
 *
 * rba_split_linear_nchw_out_gn_rows_f16x3_f32: rba_split_linear_nchw_out_gn_f16x3_f32 with
 *   - row_index [B][R] int32 or NULL: output row r of image b is source row row_index[b][r] of that image's P rows (out [B][N][R]) -- what
 *     `mask_features.flatten(2).index_select(2, plan)` picks from the full map (the 4 h w pixels the attention mask of :481-489 samples),
 *     bit for bit.  Values outside [0, P) are clamped (no out-of-bounds read); callers validate a plan once.  NULL: R == P, rows in order;
 *   - weight_image_stride (bytes, a multiple of 16) and bias_image_stride (elements): 0 = one weight image / bias for every image; otherwise
 *     image b reads weight_packed + b * weight_image_stride and bias + b * bias_image_stride (the composed operand below).
 *   x [B*P][K] raw convolution rows; mr, gamma, beta, G, relu as above; N >= 1 (only N channel planes are written); K % 32 == 0,
 *   (K / G) % 4 == 0, P % 128 == 0, R % 128 == 0, P * K < 2^30.
 * rba_compose_query_operand_f16x2: embed [B][Q][C] fp32, weight [C][K] (the convolution's matrix), bias [C] or NULL -> packed = B planes of
 *   512 * K bytes, each exactly rba_split_weight_f16x2's image of the [Q, K] matrix embed[b] * weight (rows Q .. 127 zero), and
 *   bias_q [B][Q] = embed[b] * bias (zeros for NULL).  fp32 FMAs over four quarters of c, added in a fixed order: deterministic.  A product beyond f16's range
 *   packs to +-inf: the projection's row is NaN (the f16x3 overflow contract).  Q <= 128, C <= 256, C % 4 == 0, K % 32 == 0, B <= 65535. */
int rba_split_linear_nchw_out_gn_rows_f16x3_f32(const float* x, const float* mr, const float* gamma, const float* beta, int G, int relu,
                                                const void* weight_packed, int64_t weight_image_stride, const float* bias,
                                                int bias_image_stride, const int32_t* row_index, float* out, int B, int P, int R, int N,
                                                int K, void* stream);
int rba_compose_query_operand_f16x2(const float* embed, const float* weight, const float* bias, void* packed, float* bias_q, int B, int Q,
                                    int C, int K, void* stream);

/* 3x3 / stride 1 / pad 1 convolution over NHWC activations as an implicit GEMM on the same kernel:
 * x [B,H,W,C] -> out [B,H,W,N]; weight_packed = rba_split_weight_bf16x3 of the [N, 9*C] matrix w[n][(3*ky + kx)*C + c]
 * (conv weight [N,C,3,3] permuted to [N,3,3,C]); bias [N] or NULL.  C % 32 == 0.
 * (the FPN output convolutions `layer_{j}` of pixel_decoder/msdeformattn.py:278-297, 357-360) */
int rba_conv3x3_nhwc_f32(const float* x, const void* weight_packed, const float* bias, float* out, int B, int H, int W, int C,
                         int N, void* stream);

/* The same convolution on the f16x3 kernel: weight_packed = rba_split_weight_f16x2 of the [N, 9*C] matrix above.  C % 32 == 0. */
int rba_conv3x3_nhwc_f16x3_f32(const float* x, const void* weight_packed, const float* bias, float* out, int B, int H, int W, int C,
                               int N, void* stream);

/* GroupNorm statistics without a pass over the tensor (round 4): the FPN's lateral 1x1 convolution (fp32 rows in, K <= 256) and its 3x3 output
 * convolution (split image in) also leave, per 128-row tile and group of N/G consecutive output channels, the moments (n, mean, M2) of their OUTPUT:
 * moments [B][G][rows_per_image/128][3] floats.  rba_group_norm_nhwc_merge_f32 merges them (Chan, in double) into mr [B][G][2] = (mean, rstd) --
 * what rba_group_norm_nhwc_stats_f32 computes by reading the output again (pixel_decoder/msdeformattn.py:222-235, 278-297: Conv2d(norm=GroupNorm(32, C))).
 * N % 128 == 0, N/G in {4, 8, 16, 32}, rows_per_image % 128 == 0 (H*W for the convolution).  The outputs are those of the entries without moments, bit for bit. */
int rba_split_linear_f16x3_gn_moments_f32(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                                          int rows_per_image, int G, float* moments, void* stream);
int rba_conv3x3_nhwc_f16x3_split_in_gn_moments_f32(const void* x_frag, const void* weight_packed, const float* bias, float* out, int B, int H,
                                                   int W, int C, int N, int G, float* moments, void* stream);
int rba_group_norm_nhwc_merge_f32(const float* moments, float* mr, int B, int G, int splits, float eps, void* stream);

/* Front end of the Swin path in one pass: (image - mean) / std, ImageList zero padding to Hp x Wp, and the im2col of PatchEmbed's
 * 4x4 / stride-4 convolution (maskformer_model.py:255-257, backbone/swin.py:479-495): image [3,h,w] (device; uint8 or fp32) ->
 * out [(Hp/4)*(Wp/4), 64] fp32 with out[token][c*16 + ky*4 + kx] and columns 48..63 zero; mean / std: 3 host floats each.
 * Followed by rba_split_linear_f16x3_f32 with the [E, 64] zero-padded projection weight and by rba_add_layer_norm_f32. */
int rba_patch_im2col_u8(const uint8_t* image, float* out, int h, int w, int Hp, int Wp, const float* mean, const float* std, void* stream);
int rba_patch_im2col_f32(const float* image, float* out, int h, int w, int Hp, int Wp, const float* mean, const float* std, void* stream);

/* Gaussian smoothing of the score map (the evaluator's optional transforms.GaussianBlur(7, sigma=1), support.py:366-383):
 * out[H,W] = correlation of in[H,W] (reflect-padded by kernel_size/2) with the normalised outer-product kernel of
 * exp(-0.5 (x/sigma)^2), x = -(k-1)/2 .. (k-1)/2.  kernel_size odd, <= 15; in != out. */
int rba_gaussian_blur_f32(const float* in, float* out, int H, int W, int kernel_size, float sigma, void* stream);

/* Two small steps of the masked decoder (decoder_small.hip):
 * rba_quad_mean_f32:         out[r][s] = ((v[r][0][s] + v[r][1][s]) + (v[r][2][s] + v[r][3][s])) * 0.25 for v [rows, 4, S]: the bilinear sample at the
 *                            centre of a 2 x 2 cell = the attention-mask logits of an intermediate decoder layer from mask logits evaluated at the
 *                            four source pixels of every attention cell (what F.interpolate of the whole map gives, bit for bit;
 *                            mask2former_transformer_decoder.py:472-489).
 * rba_softmax_drop_last_f32: prob[r][k] = softmax(logits[r][:])[k] for k < K1 - 1 (F.softmax(mask_cls, -1)[..., :-1], maskformer_model.py:381-383:
 *                            K1's class probabilities without the "no object" column).  2 <= K1 <= 64. */
int rba_quad_mean_f32(const float* v, float* out, int64_t rows, int S, void* stream);
int rba_softmax_drop_last_f32(const float* logits, float* prob, int64_t rows, int K1, void* stream);

/* Open-set panoptic epilogue of the RbA map (MaskFormer.panoptic_inference, maskformer_model.py:454-481):
 * rba_threshold_u8:   out[i] = score[i] > threshold
 * rba_morph3x3_u8:    3x3 box erosion (dilate = 0) or dilation (dilate = 1) of a 0/1 map, out-of-image neighbours ignored
 *                     (cv2.morphologyEx's default border); opening = erode, dilate; closing = dilate, erode.  in != out.
 * rba_ccl4_roots_i32: 4-connected components: roots[p] = smallest linear index of p's component, -1 on background
 *                     (numbering the distinct roots in increasing order gives cv2.connectedComponents' raster-order labels). */
int rba_threshold_u8(const float* score, uint8_t* out, int64_t n, float threshold, void* stream);
int rba_morph3x3_u8(const uint8_t* in, uint8_t* out, int H, int W, int dilate, void* stream);
int rba_ccl4_roots_i32(const uint8_t* mask, int32_t* roots, int H, int W, void* stream);

/* DenseHybrid anomaly head (mask2former_transformer_decoder.py:216-230, 365-366, 467-468; maskformer_model.py:303-305).
 * rba_bn_relu_conv1x1_f32:      out[b,o,p] = bias[o] + sum_c weight[o,c] * relu(x[b,c,p] * scale[c] + shift[c]); x [B,C,P], out [B,O,P],
 *                               O in {1,2,4}; scale/shift = eval-mode BatchNorm2d folded by the caller; bias may be NULL.
 * rba_resample_bilinear_ac_f32: F.interpolate(mode="bilinear", align_corners=True): x [C,h,w] -> out [C,H,W]. */
int rba_bn_relu_conv1x1_f32(const float* x, const float* scale, const float* shift, const float* weight, const float* bias, float* out,
                            int B, int C, int O, int64_t P, void* stream);
int rba_resample_bilinear_ac_f32(const float* x, float* out, int C, int h, int w, int H, int W, void* stream);

/* Row-complete token Linear for the path's SMALL Linears (fewer than 64 tiles of 128 x 128: not served by rba_split_linear_*): the
 * MSDeformAttn encoder's value / sampling / output projections and linear2 (pixel_decoder/msdeformattn.py:101-140,
 * ops/modules/ms_deform_attn.py:95-121), the decoder's key / value projections of the memory
 * (transformer_decoder/mask2former_transformer_decoder.py:83-143), the 1x1 input projection (msdeformattn.py:328-333).  f16x3 arithmetic
 * (fp32-GEMM accuracy for |v| < 65504, NaN beyond).  One workgroup owns 16 rows and all N <= 256 columns:
 * rba_token_linear_pack_f16x2: weight [N,K] fp32 -> `packed`, ceil(N/16) * (K/32) * 2048 bytes, [N/16][K/32][h | l][64 lanes][8 f16], lane
 *                             (n = lane % 16, kb = lane / 16) holding W[16 nt + n][32 b + 8 kb + 0..7]; rows beyond N zero.  K % 32 == 0.
 * rba_token_linear_f32:       out[m,:] = act((x[m,:] + x_add[m,:]) W^T + bias), act 0 none / 2 ReLU; with ln_weight != NULL instead
 *                             out[m,:] = LayerNorm(residual[m,:] + (x W^T + bias)) * ln_weight + ln_bias (N % 16 == 0, act 0): the
 *                             post-norm `src = norm(src + dropout(src2))` of msdeformattn.py:134-138 in the GEMM's epilogue.
 *                             x_add, bias may be NULL; residual only with ln_weight.  out must not alias x.
 * rba_token_linear_multi_f32: up to three Linears over the SAME rows x [M,K] in ONE launch, problem i:
 *                             out_i[m * ld_out + n] = act((x[m,:] + x_add_i[m,:]) W_i^T + bias_i)[n], n < N_i (x_add, bias may be NULL; N % 4 == 0,
 *                             ld_out >= N lets a problem fill a column slice of a wider tensor): value = value_proj(src) beside the
 *                             sampling_offsets / attention_weights Linears of `src + pos` (ms_deform_attn.py:102-110), or k = k_proj(memory + pos)
 *                             beside v = v_proj(memory) (mask2former_transformer_decoder.py:106-118). */
typedef struct {
  const float* x_add;  /* [M,K] or NULL */
  const void* packed;  /* rba_token_linear_pack_f16x2 of the weight [N,K] */
  const float* bias;   /* [N] or NULL */
  float* out;
  int N;
  int ld_out;          /* row stride of out, in floats */
  int act;             /* 0 none, 2 ReLU */
} rba_token_linear_problem;
int rba_token_linear_pack_f16x2(const float* weight, void* packed, int N, int K, void* stream);
int rba_token_linear_f32(const float* x, const float* x_add, const void* packed, const float* bias, const float* residual,
                         const float* ln_weight, const float* ln_bias, float ln_eps, float* out, int64_t M, int N, int K, int act,
                         void* stream);
int rba_token_linear_multi_f32(const float* x, const rba_token_linear_problem* problems, int n_problems, int64_t M, int K, void* stream);

/* K12a.  The multi-view merge of test-time augmentation (mask2former/test_time_augmentation.py:83-97 over the per-view sem_seg_postprocess of
 * maskformer_model.py:330-332; docs/kernels/K12.md).  A views, 1 <= A <= RBA_TTA_MAX_VIEWS; view a is sem[a] [K, h[a], w[a]] (device pointer; the class map
 * rba_reduce_up4_f32 writes for that view) and flip[a] != 0 when the view's image was flipped horizontally.  `views` itself is a HOST pointer, read
 * before the call returns.  For every output pixel (y, x) of the H x W grid and every class k:
 *   s_a[k]   = the align_corners=False bilinear sample of sem[a][k] at (y, flip[a] ? W - 1 - x : x), rba_resample_bilinear_f32's arithmetic (the
 *              resized map flipped, not the source flipped)
 *   mean[k]  = (s_0[k] + s_1[k] + ... + s_{A-1}[k]) / A        (added in ascending view order from s_0, one true division)
 *   score, argmax = rba_reduce_f32's epilogue on mean (score_mode 0 | 1 | 2, first maximum)
 * score [H,W] required; sem_seg [K,H,W] (the mean) and argmax [H,W] (int32) optional (NULL = not written).  Plain stores whatever the outputs held
 * before, no atomics, no workspace: bitwise reproducible, and the score does not depend on which optional outputs are asked for.  1 <= K <= 32; every
 * H, W, h[a], w[a] >= 1 with K H W and K h[a] w[a] < 2^31; anything else returns hipErrorInvalidValue without a launch. */
#define RBA_TTA_MAX_VIEWS 16
typedef struct {
  const float* sem[RBA_TTA_MAX_VIEWS];
  int h[RBA_TTA_MAX_VIEWS];
  int w[RBA_TTA_MAX_VIEWS];
  int flip[RBA_TTA_MAX_VIEWS];
} rba_tta_views;
int rba_tta_merge_f32(const rba_tta_views* views /* host */, int A, int K, int H, int W, int score_mode, float* score, float* sem_seg /* or NULL */,
                      int32_t* argmax /* or NULL */, void* stream);

/* K12b.  Pillow's Image.resize(BILINEAR) of a uint8 image (what Detectron2's ResizeTransform applies to the views of test-time augmentation), CHW in
 * and CHW out, equal to Pillow in every byte: the horizontal pass, then the vertical pass on its rounded uint8 result, each
 *   out = clip(((1 << 21) + sum_{j < n} kk[j] * pixel[lo + j]) >> 22, 0, 255)
 * with one coefficient table per axis built by the caller in double as Pillow builds it (rba_amd.ops.pil_bilinear_coeffs): kx int32 [W][ksize_x],
 * bx int32 [W][2] = (lo, n) with lo >= 0, 0 <= n <= ksize_x, lo + n <= w; ky, by likewise for the rows -- device pointers, trusted.  An axis whose
 * size does not change is skipped and its tables may be NULL; with both axes unchanged the image is copied.  flip != 0: the result is stored
 * flipped horizontally (column W - 1 - x).  tmp: [C,h,W] bytes of device memory, needed only when both axes change; its contents on entry do not
 * matter.  in, out and tmp must not overlap.  C, h, w, H, W >= 1 with C h w, C h W and C H W < 2^31. */
int rba_resize_u8_pil_bilinear(const uint8_t* in /* [C,h,w] */, uint8_t* out /* [C,H,W] */, uint8_t* tmp /* [C,h,W] or NULL */, int C, int h, int w,
                               int H, int W, const int32_t* kx, const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y,
                               int flip, void* stream);

/* K13.  The confusion matrix of closed-set segmentation evaluation (Detectron2's SemSegEvaluator.process: np.bincount((K + 1) * pred + gt) on the host;
 * docs/kernels/K13.md).  pred: n_pixels int32 predictions (K1's or K12a's argmax map); gt: n_pixels labels, uint8 (gt_bytes = 1) or int64 (gt_bytes = 8).
 * Per pixel p:
 *   g = gt[p];  with lut: g in 0..255 becomes lut[g], any other g is a bad label;  g == ignore_label (ignore_label >= 0 only) becomes K
 *   0 <= g <= K and 0 <= pred[p] < K:  conf[pred[p] * (K+1) + g] += 1        (rows = predictions, columns = ground truth, column K = ignored)
 *   otherwise nothing is added to conf and  bad[0] += 1 (g out of range, whatever pred[p] is)  or  bad[1] += 1 (only pred[p] out of range)
 * conf [(K+1),(K+1)] and bad [2] are ACCUMULATED into (64-bit integer atomics: bitwise reproducible); the caller zeroes them once per evaluation.
 * No workspace, no synchronisation, no read-back; capturable.  pred may be 4-byte and gt element-aligned only (a slice of a larger tensor): 16-byte loads
 * are issued on 16-byte aligned addresses only.  1 <= K <= 255; 1 <= n_pixels <= 2^40; lut: 256 entries on the device or NULL; anything else returns
 * hipErrorInvalidValue without a launch. */
int rba_confusion_accum(const int32_t* pred, const void* gt, int gt_bytes /* 1 = uint8, 8 = int64 */, int64_t n_pixels, int K,
                        int ignore_label /* < 0: none */, const uint8_t* lut /* 256 entries or NULL */, int64_t* conf /* [(K+1),(K+1)] */,
                        int64_t* bad /* [2] */, void* stream);

/* K14.  The training view of the COCO-mix fine-tune mapper (mask_former_semantic_coco_mix_dataset_mapper.py over Detectron2's ResizeShortestEdge,
 * RandomCrop, ColorAugSSDTransform, RandomFlip; docs/kernels/K14.md): one launch writes the finished view from the source frame, every element equal
 * to the host composition.  All pointers are device pointers; the struct itself is read on the host.
 *   source read at (r, c): obj / ood_label where (r - py, c - px) lies in the [bh, bw] box and objmask == ood_label there, else img / lab (lab through
 *     lut when lut is given) -- the reference's mix_object folded into the fetch; bh = bw = 0: no paste.
 *   image (y, x), channel c, with Y = y0 + y, X = x0 + (flip ? cw - 1 - x : x): Pillow's horizontal pass first, the vertical pass on its rounded
 *     uint8 result (K12b's arithmetic and tables: kx [new_w][ksize_x], bx [new_w][2], ky [new_h][ksize_y], by [new_h][2], trusted; tables whose
 *     bounds grow with the index, as Pillow's do); an axis whose size does not change has no pass and its tables may be NULL.  Then, with
 *     color.enabled, ColorAugSSDTransform(img_format = "RGB") on the pixel's three bytes: brightness; with `order` contrast, saturation, hue, else
 *     saturation, hue, contrast; a leg that is off is skipped.  convert(p, alpha, beta) = uint8(trunc(clip(fl(fl(float(p) * alpha) + beta), 0, 255)))
 *     with two separately rounded fp32 operations; the 8-bit BGR <-> HSV conversions are the ones docs/kernels/K14.md defines.
 *   sem_seg (y, x): the label at source pixel (ny[Y], nx[X]), the source indices F.interpolate(mode = "nearest") applies along each axis to the
 *     float64 labels (Detectron2 resizes a non-uint8 array with it, not with Pillow): ny int32 [new_h], nx int32 [new_w], built by the caller from
 *     ATen itself (rba_amd.ops.nearest_index_tables; ATen's arithmetic there depends on the data type and the shape, docs/kernels/K14.md), values
 *     outside the axis are brought back into it; an axis whose size does not change reads the index itself and its table may be NULL.
 *   convert's two operations, and every fp32 product of the HSV -> BGR conversion, are rounded on their own: never a fused multiply-add.
 *   image [3, pad_h, pad_w] pad value 128; sem_seg [pad_h, pad_w] pad value ignore_label; outlier_mask [ch, cw] (not padded) = ignore_label where
 *     sem_seg == ignore_label, else 1 where sem_seg == ood_label, else 0; hist [256] = the count of each label value in the ch x cw crop (zeroed by
 *     the call; integer atomics: bitwise reproducible).
 * h, w, new_h, new_w, ch, cw >= 1; 0 <= y0, y0 + ch <= new_h, 0 <= x0, x0 + cw <= new_w; pad_h >= ch, pad_w >= cw; the box inside the source or
 * absent; 0 <= ood_label <= 255; 3 h w and 3 pad_h pad_w < 2^31.  Anything else returns hipErrorInvalidValue without a launch; nothing is clamped. */
typedef struct {
  int enabled;                 /* 0: colour augmentation off, the other fields are ignored */
  int brightness;
  float beta;
  int order;                   /* != 0: contrast, saturation, hue; 0: saturation, hue, contrast */
  int contrast;
  float contrast_alpha;
  int saturation;
  float saturation_alpha;
  int hue;
  int hue_delta;
} rba_train_view_color;
typedef struct {
  const uint8_t* img;          /* [3,h,w] */
  const uint8_t* lab;          /* [h,w] */
  const uint8_t* lut;          /* 256 entries or NULL */
  const uint8_t* obj;          /* [3,bh,bw] or NULL */
  const uint8_t* objmask;      /* [bh,bw] or NULL */
  const int32_t* kx;
  const int32_t* bx;
  const int32_t* ky;
  const int32_t* by;
  const int32_t* ny;           /* [new_h] or NULL */
  const int32_t* nx;           /* [new_w] or NULL */
  uint8_t* image;              /* [3,pad_h,pad_w] */
  int64_t* sem_seg;            /* [pad_h,pad_w] */
  int64_t* outlier_mask;       /* [ch,cw] */
  int32_t* hist;               /* [256] */
  int h, w, bh, bw, py, px, new_h, new_w, ksize_x, ksize_y, y0, x0, ch, cw, flip, pad_h, pad_w, ignore_label, ood_label;
  rba_train_view_color color;
} rba_train_view;
int rba_train_view_u8(const rba_train_view* view /* host */, void* stream);

/* K15.  The optimizer step of the head fine-tune: torch.nn.utils.clip_grad_norm_(params, max_norm) + torch.optim.AdamW(amsgrad=False).step()
 * (train_net.py:303-328 of the reference) as two launches over flat fp32 state (docs/kernels/K15.md).  grad, exp_avg and exp_avg_sq are flat buffers of
 * one layout: tensor t occupies [offset, offset + n), every offset is a multiple of 4 elements and the gaps hold zeros; the buffers are 16-byte
 * aligned.  The parameters stay where the model has them (element-aligned is enough: a view of a larger tensor).
 *   K15a  rba_grad_sqnorm_f32: partials[b] = the sum of (grad[i] * grad_scale)^2 over workgroup b's fixed share of [0, n), 1 <= n_partials <=
 *         RBA_ADAMW_MAX_PARTIALS, every slot written.  No atomics: bitwise reproducible.
 *   K15b  rba_clip_adamw_step_f32: norm = sqrt(sum of the partials, summed by every workgroup in one fixed order); coef = max_norm / (norm + 1e-6)
 *         where that is below 1, else 1 (a NaN stays NaN); max_norm <= 0: coef = 1.  stats[0] = norm.  Then for every element of every tensor, with
 *         lr_t = lr * lr_mult, g = grad * grad_scale * coef:
 *             p *= 1 - lr_t * weight_decay;  m += (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g^2;
 *             p -= (lr_t / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)
 *         the two host scalars of torch (1 - lr_t * weight_decay, lr_t / bias_correction1) formed in double and rounded to fp32 once, as torch does.
 *         grad is not written: it keeps the unclipped, unscaled sum.
 * tensors: the descriptors on the device; blocks: n_blocks pairs (tensor index, chunk index) on the device, workgroup b steps elements
 * [chunk index * chunk, + chunk) of its tensor; chunk a multiple of 4.  Both tables are trusted (the caller built them): every pair must name a chunk
 * that starts inside its tensor, and together they must cover every element once.  A bad scalar or a misaligned buffer returns hipErrorInvalidValue
 * without a launch.  No workspace besides partials, no synchronisation, no read-back; capturable. */
#define RBA_ADAMW_MAX_PARTIALS 1024
typedef struct {
  float* param;                /* n elements, where the model keeps them */
  int64_t offset;              /* of the tensor's slice in the flat buffers, a multiple of 4 */
  int64_t n;
  double lr_mult;              /* the group's learning rate is lr * lr_mult */
  double weight_decay;
} rba_adamw_tensor;
int rba_grad_sqnorm_f32(const float* grad, int64_t n, float grad_scale, float* partials, int n_partials, void* stream);
typedef struct {               /* one step's scalars, read on the host */
  double lr;                   /* of a group with multiplier 1 */
  double beta1, beta2, eps;
  double bias_correction1;     /* 1 - beta1^step */
  double bias_correction2_sqrt; /* sqrt(1 - beta2^step) */
  float grad_scale, max_norm;
} rba_adamw_hyper;
int rba_clip_adamw_step_f32(const rba_adamw_tensor* tensors, const int32_t* blocks /* [n_blocks][2] */, int n_blocks, int chunk, const float* grad,
                            float* exp_avg, float* exp_avg_sq, const float* partials, int n_partials, const rba_adamw_hyper* hyper /* host */,
                            float* stats /* [1] */, void* stream);

/* K16a.  The closed-set panoptic merge (maskformer_model.py:395-452) for every kept query in one pass over the mask logits.
 * mask [Q,HW] mask logits at the output resolution; score [Q] = the queries' class scores; keep [Q] uint8, non-zero = the query competes.
 * Per pixel p, over the kept q in ascending order:  s = sigmoid(mask[q,p]),  v = score[q] * s (one fp32 multiply);  best = the first q that
 * attains the largest v;  solid_q = (s >= 0.5f).
 *   counts[0][best] += 1                          the area best won             (the reference's `cur_mask_ids == k`)
 *   counts[1][q]    += solid_q  for every kept q  q's own >= 0.5 area           (`cur_masks[k] >= 0.5`)
 *   counts[2][best] += solid_best                 their intersection            (`mask_area` of the pixels that are written)
 *   winner[p]        = solid_best ? best : 0xFF
 * winner [HW] uint8 is written everywhere; counts [3,Q] int32 is ADDED into with integer atomics (bitwise reproducible; the caller zeroes it) and
 * rows of queries that are not kept are left alone.  mask may be only 4-byte aligned and winner not at all: 16-byte loads are issued on 16-byte
 * aligned addresses only.  1 <= Q <= 255 (0xFF is the "nobody" byte), 1 <= HW < 2^31; anything else returns hipErrorInvalidValue without a launch.
 * With no kept query every winner is 0xFF and counts stays as it is.  Non-finite logits: a NaN product never wins (v > best is false), a pixel
 * whose kept products are all NaN has no winner (0xFF, no counter moves); score is expected finite and >= 0. */
int rba_panoptic_merge_f32(const float* mask, const float* score, const uint8_t* keep, uint8_t* winner, int32_t* counts, int Q, int64_t HW,
                           void* stream);

/* K16a fused with the x4 bilinear upsample (align_corners=False, ATen's tap order) in front and the crop behind it, rba_reduce_up4_f32's contract:
 * mask_lowres [Q,h,w]; the per-pixel rule above runs on rows < crop_h and columns < crop_w of the virtual [Q,4h,4w] map; winner [crop_h,crop_w].
 * 1 <= crop_h <= 4h, 1 <= crop_w <= 4w. */
int rba_panoptic_merge_up4_f32(const float* mask_lowres, const float* score, const uint8_t* keep, uint8_t* winner, int32_t* counts, int Q,
                               int h, int w, int crop_h, int crop_w, void* stream);

/* K16b.  panoptic[p] = winner[p] == 0xFF ? 0 : seg_of_query[winner[p]]  (a byte >= Q counts as 0xFF).  seg_of_query [Q] int32: the segment id the
 * host loop gave each query, 0 = dropped.  The reference's sequential `panoptic_seg[mask] = id` writes touch disjoint pixels: their order is free. */
int rba_panoptic_assign_i32(const uint8_t* winner, const int32_t* seg_of_query, int32_t* panoptic, int Q, int64_t HW, void* stream);

/* K16c.  The segment-pair histogram of panoptic evaluation (evaluation.py:152-159: np.unique(pan_gt * OFFSET + pan_pred, return_counts=True)) on
 * dense ids: per pixel, 0 <= gt < G and 0 <= pred < P  ->  counts[gt * P + pred] += 1, otherwise bad[0] += 1.  counts [G,P] and bad [1] are int64
 * and ADDED into with 64-bit integer atomics (the caller zeroes them); nothing is allocated or read back.  gt and pred may be only 4-byte aligned.
 * 1 <= G, P, G * P <= 2^24, 1 <= n <= 2^40. */
int rba_segment_pairs_accum(const int32_t* gt, const int32_t* pred, int64_t n, int G, int P, int64_t* counts, int64_t* bad, void* stream);

/* K17a.  The per-query sums of MaskFormer.instance_inference (maskformer_model.py:517-524) and the boxes it leaves commented out (:520), for every kept
 * query in one pass over the kept planes.  mask [Q,H,W] mask logits at the output resolution; keep [Q] uint8, non-zero = the query is in the top-k.
 * For every kept q and every pixel (x, y) with logit m > 0 (a NaN logit is not > 0 and contributes nothing):
 *   count[q] += 1
 *   ssum[q]  += (int64)(sigmoid(m) * 2^32)        an integer: a sigmoid of a positive logit is an fp32 value of at least ~0.5, so ssum is the EXACT
 *                                                 sum of the fp32 sigmoids in units of 2^-32 -- independent of arrival order, bitwise reproducible
 *   box[q]    = (min x, min y, max x, max y)      through atomic min / max
 * count [Q] int32 and ssum [Q] int64 are ADDED into with integer atomics and box [Q,4] int32 is min / max-ed into: the caller zeroes count and ssum and
 * sets every box to (W, H, -1, -1); rows of queries that are not kept are left alone.  mask may be only 4-byte aligned: 16-byte loads are issued on
 * 16-byte aligned addresses only.  1 <= Q <= 255, 1 <= H * W < 2^31; anything else returns hipErrorInvalidValue without a launch. */
int rba_instance_stats_f32(const float* mask, const uint8_t* keep, int32_t* count, int64_t* ssum, int32_t* box, int Q, int H, int W, void* stream);

/* K17a fused with the x4 bilinear upsample (align_corners=False, ATen's tap order) in front and the crop behind it, rba_panoptic_merge_up4_f32's
 * contract: mask_lowres [Q,h,w]; the rule above runs on rows < crop_h and columns < crop_w of the virtual [Q,4h,4w] map (the caller's boxes start at
 * (crop_w, crop_h, -1, -1)).  1 <= crop_h <= 4h, 1 <= crop_w <= 4w. */
int rba_instance_stats_up4_f32(const float* mask_lowres, const uint8_t* keep, int32_t* count, int64_t* ssum, int32_t* box, int Q, int h, int w,
                               int crop_h, int crop_w, void* stream);

/* K17b.  The result planes of instance_inference (:503, :517): out[n,p] = mask[qidx[n],p] > 0 ? 1 : 0 as float or as uint8.  mask [Q,HW], qidx [N]
 * int32, out [N,HW].  A qidx outside [0, Q) is refused ON THE DEVICE: that plane is written as zeros and no logit is read for it.  A query may appear
 * several times in qidx (once per class it is detected as); its plane is then read once per appearance.  out may be only element aligned: wide stores
 * are issued on addresses aligned to four elements only.  1 <= Q, 1 <= N <= 65535, 1 <= HW < 2^31. */
int rba_instance_masks_f32(const float* mask, const int32_t* qidx, float* out, int Q, int N, int64_t HW, void* stream);
int rba_instance_masks_u8(const float* mask, const int32_t* qidx, uint8_t* out, int Q, int N, int64_t HW, void* stream);

/* K17b on the crop_h x crop_w window of the virtual x4 map of mask_lowres [Q,h,w] (the taps of rba_instance_stats_up4_f32, so the planes agree with its
 * counts pixel by pixel): out [N,crop_h,crop_w]. */
int rba_instance_masks_up4_f32(const float* mask_lowres, const int32_t* qidx, float* out, int Q, int N, int h, int w, int crop_h, int crop_w,
                               void* stream);
int rba_instance_masks_up4_u8(const float* mask_lowres, const int32_t* qidx, uint8_t* out, int Q, int N, int h, int w, int crop_h, int crop_w,
                              void* stream);

/* K18.  The ROC and precision-recall curves of up to 64 image subsets ("trials" of a bootstrap) from ONE globally sorted pixel list
 * (support.py:305-351 behind its scoring loop; docs/kernels/K18.md).  score [n] fp32 sorted DESCENDING; tag [n] int32 = (image_index << 1) | label, label
 * in {0, 1}, in the same order; member [n_images] uint64, bit t set = the image belongs to trial t (bits >= T are ignored).  A threshold is a run of
 * equal scores of the global order; a trial's curve has a point at the end of every run that holds at least one of its pixels.
 *
 * The list is cut into ceil(n / chunk) chunks of `chunk` pixels, one wave each; a run may span any number of chunks.  The per-chunk integers are
 * laid out [T][2][chunks]: the (tp, cnt) planes of each trial (cnt = tp + fp) with the chunk index innermost, the dimension their prefix runs along.
 *   rba_subset_curves_totals : per chunk c and trial t  totals[t][.][c] = (tp, cnt) of the chunk's member pixels,
 *                              upto_end[t][.][c] = the same counted up to the LAST run end inside the chunk, has_end[c] = 1 if there is one, else 0
 *                              (then upto_end[.][.][c] = 0).  All int32, written (not added).
 *   rba_subset_curves_walk   : base [T][2][chunks] int64 = the counts in front of each chunk (the exclusive prefix of totals), prev [T][2][chunks]
 *                              int64 = the counts at the last run end in front of it (0 if none).  Adds, per trial, over the run ends inside the chunk
 *                              with a step (dtp, dfp) != (0, 0):   auroc2[t] += dfp * (tp_prev + tp)   exact, 64-bit integer atomics (the caller zeroes)
 *                                                                  ap_part[t][c] = sum  dtp * tp / (tp + fp)   float64, in run order, dtp > 0 only
 *   rba_subset_curves_finish : one workgroup per trial.  ap[t] = ap_part[t][0] + ap_part[t][1] + ... in chunk order (no float atomics: bitwise
 *                              reproducible).  at95[t] = (fp, tp) int64 at the first point of the trial's ROC curve after scikit-learn's
 *                              drop_intermediate (a point stays if the step into it differs from the step out of it, or it is the first or the last)
 *                              whose (double)tp / (double)P > 0.95; (0, 0) when P = 0.  It walks forward from the chunk in which `ends` [T][2][chunks]
 *                              int64 (the INCLUSIVE prefix of totals; its last column is (P, P + N)) places the crossing.
 * 1 <= T <= 64, 1 <= n < 2^31, chunk a multiple of 64 in [64, 2^20], every image_index < n_images <= 2^30 (an index outside the table reads no
 * membership: the pixel belongs to no trial).  Nothing is allocated, synchronised or read back. */
int rba_subset_curves_totals(const float* score, const int32_t* tag, const uint64_t* member, int64_t n, int n_images, int T, int chunk,
                             int32_t* totals, int32_t* upto_end, int32_t* has_end, void* stream);
int rba_subset_curves_walk(const float* score, const int32_t* tag, const uint64_t* member, int64_t n, int n_images, int T, int chunk,
                           const int64_t* base, const int64_t* prev, int64_t* auroc2, double* ap_part, void* stream);
int rba_subset_curves_finish(const float* score, const int32_t* tag, const uint64_t* member, int64_t n, int n_images, int T, int chunk,
                             const int64_t* base, const int64_t* prev, const int64_t* ends, const double* ap_part, double* ap, int64_t* at95,
                             void* stream);

/* K18's input.  Appends (score[p], (image_index << 1) | label[p]) for every pixel p of one image whose label is 0 or 1 to out_score / out_tag
 * [capacity] at the device-side cursor: cursor[0] (int64) is advanced by the number of labelled pixels with one integer atomic per workgroup;
 * a pixel whose slot would lie at or past `capacity` is not written and sets cursor[1] to 1.  The caller zeroes cursor once, appends any number of
 * images and reads it once: min(cursor[0], capacity) pairs are valid when cursor[1] is 0.  Order within the buffer is unspecified (a sort follows).
 * labels: uint8 (label_bytes = 1) or int64 (label_bytes = 8).  1 <= n < 2^31, 0 <= image_index < 2^30, capacity >= 0. */
int rba_labelled_tags_i32(const float* score, const void* labels, int label_bytes, int64_t n, int image_index, float* out_score, int32_t* out_tag,
                          int64_t capacity, int64_t* cursor, void* stream);

/* K19 -- the MiT (SegFormer) backbone's pieces that are not Linears or LayerNorms (mask2former/modeling/backbone/mix_transformer.py;
 * docs/kernels/K19.md).  No atomics, no workspace, nothing allocated, synchronised or read back; every output has one fixed summation order.
 *
 * K19a.  The spatial-reduction attention core (:113-117): out[b,n,h,:] = softmax_s(q[b,n,h,:] . k[b,s,h,:] * scale) v[b,s,h,:].  q [B,N,nH*hd] (unscaled),
 * kv [B,S,2*nH*hd] as the kv Linear leaves it (k = the first nH*hd columns, v = the rest, head-major), out [B,N,nH*hd] head-major.  Flash-style, online
 * softmax in fp32, exact fp32 products (v_mfma_f32_32x32x2_f32): nothing of size [B*nH,N,S] exists.  hd in {32, 64}, N >= 1, 1 <= S <= 2^30, B and nH
 * <= 65535, pointers 16-byte aligned; anything else returns hipErrorInvalidValue without a launch. */
int rba_sr_attn_f32(const float* q, const float* kv, float* out, int B, int N, int S, int nH, int hd, float scale, void* stream);

/* K19b.  y = GELU(depthwise3x3(x) + bias) (erf GELU, stride 1, zero padding 1; Mlp :53-55, DWConv :384-390) on channels-last tokens x, y [B,H*W,C].
 * w9 [9,C] is the [C,1,3,3] weight tap-major (w9[3 ky + kx][c]).  C % 4 == 0, pointers 16-byte aligned.  Images are independent: no row of image
 * b + 1 feeds the padding of image b. */
int rba_dwconv3x3_gelu_nhwc_f32(const float* x, const float* w9, const float* bias, float* y, int B, int H, int W, int C, void* stream);

/* K19c.  The operand of a k x k / stride / pad convolution as a GEMM: cols [B*Ho*Wo, Kp] with Ho = floor((H + 2 pad - k) / stride) + 1 (0 where no
 * window fits; Wo alike), column (ky * k + kx) * C + c = x[b][oy * stride - pad + ky][ox * stride - pad + kx][c], zeros outside the image and in
 * columns k*k*C .. Kp - 1.  x: channels-last [B,H,W,C], or with nchw_in != 0 the [B,C,H,W] image batch.  Kp % 4 == 0, Kp >= k*k*C, 0 <= pad < k <= 64,
 * cols 16-byte aligned. */
int rba_im2col_nhwc_f32(const float* x, float* cols, int B, int H, int W, int C, int k, int stride, int pad, int Kp, int nchw_in, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RBA_HIP_H */
