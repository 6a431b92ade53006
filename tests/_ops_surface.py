"""The entry surface of rba_amd.ops as plain lists (no device, no torch): which wrapper has its rows in which table.

tests/test_ops_surface_cpu.py walks rba_amd.ops and fails for a wrapper that is in none of them, so the next wrapper cannot arrive without rows;
tests/test_ops_refusals_gpu.py and tests/test_operand_placement_gpu.py check that their tables hold exactly the names listed here."""

# tests/test_ops_refusals_gpu.py, _table: the inference wrappers that existed when the argument contracts were written once
REFUSAL_ROWS_FIRST_TABLE = [
    "add_layer_norm", "bn_relu_conv1x1", "conv3x3_nhwc", "conv3x3_nhwc_gn_stats", "group_norm", "group_norm_nhwc", "group_norm_nhwc_stats", "masked_xattn",
    "merge_layer_norm", "mlp_fused_ln", "ms_deform_attn_backward", "ms_deform_attn_forward", "resample_bilinear", "resample_bilinear_nhwc",
    "resample_bilinear_nhwc_gn", "skinny_linear", "split_linear", "split_linear_nchw_out", "split_linear_nchw_out_gn", "swin_attn_block", "swin_attn_qkv",
    "swin_window_attn", "token_linear", "token_linear_multi",
]

# tests/test_ops_refusals_gpu.py, _table2: everything added since, and the older wrappers that had no row
REFUSAL_ROWS_SECOND_TABLE = [
    # K1, K3 / K4
    "rba_reduce", "rba_reduce_up4", "rba_reduce_backward", "sem_seg_backward", "masked_xattn_backward", "mask_logits", "mask_logits_backward",
    # K8 - K11
    "point_sample", "mask_point_loss", "mask_point_loss_backward", "match_cost", "outlier_tail", "outlier_tail_backward", "dense_hybrid_loss",
    "dense_hybrid_loss_backward", "gambler_loss", "gambler_loss_backward", "gaussian_blur_planes", "gaussian_blur_planes_adjoint", "score_reg",
    "score_reg_backward",
    # K12 - K15
    "tta_merge", "resize_u8_pil_bilinear", "confusion_accumulate", "train_view", "adamw_plan", "grad_sqnorm", "clip_adamw_step",
    # older wrappers
    "swin_bias_fragments", "swin_attn_block_weights", "msda_prepare", "msda_fused", "mlp_fused", "linear_gn_stats", "split_linear_nchw_out_gn_rows",
    "patch_im2col", "resample_bilinear_ac", "gaussian_blur", "quad_mean", "softmax_drop_last", "ood_components", "compose_query_operand",
    "split_weight", "conv3x3_weight", "linear",
]

# tests/test_operand_placement_gpu.py: the wrappers whose operands are handed over off a 16-byte boundary, one at a time and all together
PLACEMENT_ROWS = [
    "rba_reduce", "resample_bilinear", "resample_bilinear_ac", "group_norm", "bn_relu_conv1x1", "mask_logits", "mask_logits_backward", "ms_deform_attn_forward", "msda_fused",
    "resize_u8_pil_bilinear", "tta_merge", "skinny_linear", "masked_xattn", "rba_reduce_backward", "quad_mean", "softmax_drop_last", "gaussian_blur",
    "gaussian_blur_planes", "gaussian_blur_planes_adjoint", "patch_im2col", "ood_components", "score_reg", "score_reg_backward", "add_layer_norm", "merge_layer_norm", "group_norm_nhwc",
    "group_norm_nhwc_stats", "resample_bilinear_nhwc", "token_linear", "token_linear_multi", "masked_xattn_backward", "sem_seg_backward", "msda_prepare",
    "confusion_accumulate", "train_view", "rba_reduce_up4", "ms_deform_attn_backward", "point_sample", "mask_point_loss", "mask_point_loss_backward",
    "match_cost", "outlier_tail", "outlier_tail_backward", "dense_hybrid_loss", "dense_hybrid_loss_backward", "gambler_loss", "gambler_loss_backward",
    "split_linear", "split_linear_nchw_out", "linear", "split_weight", "conv3x3_weight", "swin_attn_block_weights", "swin_bias_fragments", "conv3x3_nhwc",
    "split_linear_nchw_out_gn", "split_linear_nchw_out_gn_rows", "mlp_fused", "mlp_fused_ln", "linear_gn_stats", "conv3x3_nhwc_gn_stats",
    "compose_query_operand", "swin_window_attn", "swin_attn_qkv", "swin_attn_block", "resample_bilinear_nhwc_gn",
    # through rba_amd.solver.ClipAdamW, in a test of their own (test_k15_steps_parameters_wherever_they_lie)
    "adamw_plan", "grad_sqnorm", "clip_adamw_step",
]
PLACEMENT_ROWS_OUTSIDE_THE_CASE_TABLE = ["adamw_plan", "grad_sqnorm", "clip_adamw_step"]


# wrappers that need no rows: pure-host helpers, each with its reason
EXEMPT = {
    "split_mode": "a context manager that sets the calling thread's arithmetic mode: it takes no tensor and reaches no entry point",
    "unpack_split_weight": "torch indexing on an already packed tensor, for inspection and tests: it calls no entry point of the kernel library",
}
