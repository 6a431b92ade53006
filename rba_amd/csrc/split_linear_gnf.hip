// K6 -- the mask-feature projection with the last GroupNorm (+ ReLU) of the pixel decoder folded into its A path (split_linear_h3l_kernel<NCHW, GNF>,
// split_linear_h3.h; reference pixel_decoder/msdeformattn.py:357-362).  Its own translation unit because it is compiled WITHOUT packed fp32 instructions
// (build.py: UNPACKED_ALWAYS).  Round 5 (profiles/r05_gnfold_select.txt, tools/gnf_asm_probe.py): in builds where the compiler wrote the coefficient
// a = gamma * rstd of the fold as `v_pk_mul_f32 vD[0:1], v_gamma[0:1], v_(mean, rstd)[0:1] op_sel:[0,1]` (the LOW product takes the HIGH register of
// source 1), that LOW product came out as exactly 0 in lanes 48-63 of a wave a few hundred times per launch -- whole rows of the staged tile normalised with
// a = 0, b = beta.  Hand-edited assembly of such a build pins it on that one instruction form: the same products written as two v_mul_f32, as a packed
// multiply on a broadcast pair, or with the operands swapped (`op_sel:[1,0]`: the cross select on source 0) are exact in every run; wait states, s_waitcnt
// vmcnt(0) / lgkmcnt(0), other destination or source registers and a drained matrix pipe change nothing.  Which form the compiler picks depends on register
// allocation (the ReLU variants of the round-5 search only moved it).  Without packed fp32 there is no such instruction in this kernel.
// tools/micro/pk_opsel_after_load.hip reproduces it standalone (profiles/r05_pk_opsel_erratum.txt): beside a wave that issues MFMAs with plain VALU between them, the LOW result
// of v_pk_mul_f32 / v_pk_add_f32 with the LOW select on source 1 is 0 in lanes 48-63 for up to 10 % of those lanes' results; every other select form is exact.
#include "split_linear_h3.h"

// The same projection reading a RAW convolution output: GroupNorm(G groups, statistics mr [B][G][2] from rba_group_norm_nhwc_stats_f32) (+ ReLU) is applied
// while the rows are staged -- `mask_features(output_conv(y))` (pixel_decoder/msdeformattn.py:357-362) without ever writing the normalised 1/4-resolution map
// (268 MB of traffic at 1024 x 2048).  Same arithmetic as rba_group_norm_nhwc_f32 followed by the entry above: bit-identical.  rows_per_image % 128 == 0.
extern "C" int rba_split_linear_nchw_out_gn_f16x3_f32(const float* x, const float* mr, const float* gamma, const float* beta, int G, int relu,
                                                      const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                                                      int rows_per_image, void* stream) {
  RBA_CHECK_ARG(N >= 1 && rows_per_image >= 1 && G >= 1 && (K % G) == 0 && ((K / G) % 4) == 0);
  RBA_GEMM_PROLOGUE(M, K, x && mr && gamma && beta && weight_packed && out && (M % rows_per_image) == 0 && (rows_per_image % 128) == 0, x, weight_packed, out,
                    gamma, beta);
  H3Args a{x, reinterpret_cast<const u32x4_t*>(weight_packed), bias, out, M, N, K, (hipStream_t)stream};
  a.rows_per_image = rows_per_image;
  a.gn = GnFold{mr, gamma, beta, G, K / G, relu ? 1 : 0};
  return rba_gemm_status(h3_wide(M, N) ? launch_h3l<0, 4, H3_NCHW | H3_GNF>(a) : launch_h3l<0, 2, H3_NCHW | H3_GNF>(a));
}

// The two mask heads of the masked decoder on the DEFERRED mask-feature operand (docs/kernels/K4.md): the entry above with an optional per-image row index
// and optional per-image operands.
//   row_index [B][R] int32 (or NULL: R == P, every row in order): output row r of image b is the projection of x[b P + row_index[b][r]] -- the columns
//     `mask_features.flatten(2).index_select(2, plan)` would pick from the full map (mask2former_transformer_decoder.py:479-489: the attention mask samples
//     the mask logits at 4 h w pixels), bit for bit, without the map.  A value outside [0, P) is clamped by the kernel (no out-of-bounds read); callers
//     validate their plan once.
//   weight_image_stride (bytes, % 16) / bias_image_stride (elements): 0 = one weight image and bias for every image, as above; otherwise image b reads
//     weight_packed + b * weight_image_stride and bias + b * bias_image_stride -- the composed operand of rba_compose_query_operand_f16x2, with which
//     out [B][N = Q][P] IS einsum("bqc,bchw->bqhw", mask_embed, mask_features(y)) (:479 after pixel_decoder/msdeformattn.py:362).
// out [B][N][R]; only N channel planes are written (N need not be a multiple of 128).  P % 128 == 0, R % 128 == 0, P K < 2^30.
extern "C" int rba_split_linear_nchw_out_gn_rows_f16x3_f32(const float* x, const float* mr, const float* gamma, const float* beta, int G, int relu,
                                                           const void* weight_packed, int64_t weight_image_stride, const float* bias, int bias_image_stride,
                                                           const int32_t* row_index, float* out, int B, int P, int R, int N, int K, void* stream) {
  RBA_CHECK_ARG(B >= 0 && N >= 1 && P >= 1 && R >= 1 && G >= 1 && (K % G) == 0 && ((K / G) % 4) == 0);
  RBA_CHECK_ARG(weight_image_stride >= 0 && (weight_image_stride % 16) == 0 && bias_image_stride >= 0 && (row_index || R == P));
  const int64_t M = (int64_t)B * R;
  RBA_GEMM_PROLOGUE(M, K, x && mr && gamma && beta && weight_packed && out && (P % 128) == 0 && (R % 128) == 0 && (int64_t)P * K < (int64_t)1 << 30, x,
                    weight_packed, out, gamma, beta);
  H3Args a{x, reinterpret_cast<const u32x4_t*>(weight_packed), bias, out, M, N, K, (hipStream_t)stream};
  a.rows_per_image = R;
  a.gn = GnFold{mr, gamma, beta, G, K / G, relu ? 1 : 0};
  a.rw = H3Rows{row_index, P, bias_image_stride, weight_image_stride};
  const bool per_image = weight_image_stride != 0 || bias_image_stride != 0, wide = h3_wide(M, N);
  constexpr unsigned F = H3_NCHW | H3_GNF;
  if (row_index && per_image) return rba_gemm_status(wide ? launch_h3l<0, 4, F | H3_ROWIDX | H3_PERIMG>(a) : launch_h3l<0, 2, F | H3_ROWIDX | H3_PERIMG>(a));
  if (row_index) return rba_gemm_status(wide ? launch_h3l<0, 4, F | H3_ROWIDX>(a) : launch_h3l<0, 2, F | H3_ROWIDX>(a));
  if (per_image) return rba_gemm_status(wide ? launch_h3l<0, 4, F | H3_PERIMG>(a) : launch_h3l<0, 2, F | H3_PERIMG>(a));
  return rba_gemm_status(wide ? launch_h3l<0, 4, F>(a) : launch_h3l<0, 2, F>(a));
}
