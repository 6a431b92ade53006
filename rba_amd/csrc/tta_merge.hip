// K12a: the multi-view merge of test-time augmentation (reference: mask2former/test_time_augmentation.py:83-97 over the per-view
// sem_seg_postprocess of maskformer_model.py:330-332).  Per view the reference resizes the view's class map to the output size
// (F.interpolate, bilinear, align_corners=False), flips it when the view was flipped, adds the views in order and divides once by their
// number; the evaluator then takes a score of the mean (evaluate_ood.py:143-159).  None of those K x H x W maps exists here: one thread owns four
// consecutive output columns of one row and all K classes (the [KMAX][4] accumulators of the fused K1), gathers its four taps from every
// view's own class map with resample_kernel's arithmetic, and ends in K1's epilogue (rba_reduce_kernels.h: score modes, first-maximum argmax).
// No atomics, no workspace; every output word is stored whatever it held before.  docs/kernels/K12.md.
#include "rba_reduce_kernels.h"

namespace {

using namespace rba_k1;

// one launch's views, by value in the kernel arguments (388 bytes): sem[a] [K, h[a], w[a]]; sh / sw = the ATen scales h / H, w / W formed in float on the host,
// exactly as rba_resample_bilinear_f32 forms them
struct TtaViews {
  const float* sem[RBA_TTA_MAX_VIEWS];
  int h[RBA_TTA_MAX_VIEWS], w[RBA_TTA_MAX_VIEWS];
  float sh[RBA_TTA_MAX_VIEWS], sw[RBA_TTA_MAX_VIEWS];
  unsigned flips;                                  // bit a: view a was flipped horizontally
};

template <int KMAX>
__global__ __launch_bounds__(256) void tta_merge_kernel(const TtaViews v, int A, int K, int H, int W, int wq, int xblocks, int mode,
                                                        float* __restrict__ score, float* __restrict__ sem, int32_t* __restrict__ argmax) {
  const int y = blockIdx.x / xblocks;                                              // rows x column blocks in one grid dimension: H is not bound by 65535
  const int xg = (blockIdx.x - y * xblocks) * blockDim.x + threadIdx.x;
  if (xg >= wq) return;
  const int x0 = xg * 4;
  float acc[KMAX][4];
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[k][r] = 0.f;
  for (int a = 0; a < A; ++a) {
    const int h = v.h[a], w = v.w[a];
    const bool flip = (v.flips >> a) & 1u;
    const BilinearTap ty = bilinear_tap(y, v.sh[a], h);
    BilinearTap tx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int x = x0 + r < W ? x0 + r : W - 1;                                  // ragged right edge: a valid column, never stored
      tx[r] = bilinear_tap(flip ? W - 1 - x : x, v.sw[a], w);                     // the RESIZED map flipped: column W - 1 - x of the output grid
    }
    const float* base = v.sem[a];
    const int64_t plane = (int64_t)h * w;
    const float* r0 = base + (int64_t)ty.i0 * w;
    const float* r1 = base + (int64_t)ty.i1 * w;
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      if (k < K) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          // ATen's order (resample_kernel): l0h * (l0w * v00 + l1w * v01) + l1h * (l0w * v10 + l1w * v11), with the fused multiply-adds WRITTEN: under
          // -ffp-contract=fast the compiler is free to pick which product of `a * b + c * d` it fuses.  Every product below feeds an fma's addend or is one
          // and no sum has a product operand: nothing is left to choose.
          const float top = fmaf(tx[r].l0, r0[tx[r].i0], tx[r].l1 * r0[tx[r].i1]);
          const float bot = fmaf(tx[r].l0, r1[tx[r].i0], tx[r].l1 * r1[tx[r].i1]);
          const float s = fmaf(ty.l0, top, ty.l1 * bot);
          acc[k][r] = a == 0 ? s : acc[k][r] + s;                                 // v0, then += v1, ... in view order
        }
        r0 += plane;
        r1 += plane;
      }
    }
  }
  const float n = (float)A;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[k][r] = acc[k][r] / n;                        // one true division (final_predictions / count_predictions)
  const int64_t oplane = (int64_t)H * W;
  const int64_t p0 = (int64_t)y * W + x0;
  // K1's epilogue (rba_reduce_kernels.h: rba_score, first-maximum argmax, the stores of rba_epilogue and of the fused kernel's ragged edge) with the two
  // optional outputs as run-time, workgroup-uniform branches around their stores only: the arithmetic is ONE instruction stream whatever is asked for
  float sc[4];
  rba_score<KMAX, 4>(acc, K, mode, sc);
  int best[4];
  float bestv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { best[i] = 0; bestv[i] = acc[0][i]; }
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (acc[k][i] > bestv[i]) { bestv[i] = acc[k][i]; best[i] = k; }
  if (x0 + 3 < W && (W & 3) == 0) {                                                // 16-byte stores
    if (sem) {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) store_vec<4>(sem + (int64_t)k * oplane + p0, acc[k]);
    }
    store_vec<4>(score + p0, sc);
    if (argmax) *reinterpret_cast<rba_u32x4*>(argmax + p0) = (rba_u32x4){(uint32_t)best[0], (uint32_t)best[1], (uint32_t)best[2], (uint32_t)best[3]};
  } else {                                                                          // ragged right edge / unaligned rows: scalar stores
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (x0 + i >= W) break;
      if (sem) {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) sem[(int64_t)k * oplane + p0 + i] = acc[k][i];
      }
      score[p0 + i] = sc[i];
      if (argmax) argmax[p0 + i] = best[i];
    }
  }
}

template <int KMAX>
int launch_tta_merge(const TtaViews& v, int A, int K, int H, int W, int mode, float* score, float* sem, int32_t* argmax, hipStream_t st) {
  const int wq = (W + 3) / 4;
  const int threads = wq >= 256 ? 256 : (wq >= 128 ? 128 : 64);
  const int xblocks = (wq + threads - 1) / threads;
  const int64_t blocks = (int64_t)xblocks * H;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(tta_merge_kernel<KMAX>, dim3((unsigned)blocks), dim3(threads), 0, st, v, A, K, H, W, wq, xblocks, mode, score, sem, argmax);
  return rba_launch_status();
}

}  // namespace

extern "C" int rba_tta_merge_f32(const rba_tta_views* views, int A, int K, int H, int W, int score_mode, float* score, float* sem_seg,
                                 int32_t* argmax, void* stream) {
  RBA_CHECK_ARG(views && score && A >= 1 && A <= RBA_TTA_MAX_VIEWS && K >= 1 && K <= 32 && H >= 1 && W >= 1);
  RBA_CHECK_ARG(score_mode >= 0 && score_mode <= 2 && (int64_t)K * H * W < (1LL << 31));
  // the 16-byte stores of the aligned form (W % 4 == 0) need 16-byte aligned maps; 4-byte alignment is every fp32 tensor's
  RBA_CHECK_ARG(((((uintptr_t)score | (uintptr_t)sem_seg | (uintptr_t)argmax) & ((W & 3) == 0 ? 15 : 3)) == 0));
  TtaViews v;
  v.flips = 0;
  for (int a = 0; a < RBA_TTA_MAX_VIEWS; ++a) {
    const int s = a < A ? a : 0;                                                   // unused slots repeat view 0: no uninitialised kernel argument
    RBA_CHECK_ARG(views->sem[s] && (((uintptr_t)views->sem[s]) & 3) == 0 && views->h[s] >= 1 && views->w[s] >= 1 &&
                  (int64_t)K * views->h[s] * views->w[s] < (1LL << 31));
    v.sem[a] = views->sem[s];
    v.h[a] = views->h[s];
    v.w[a] = views->w[s];
    v.sh[a] = (float)views->h[s] / (float)H;                                       // ATen: scale = in / out in float (area_pixel_compute_scale)
    v.sw[a] = (float)views->w[s] / (float)W;
    if (a < A && views->flip[a]) v.flips |= 1u << a;
  }
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  if (K <= 20) return launch_tta_merge<20>(v, A, K, H, W, score_mode, score, sem_seg, argmax, st);
  return launch_tta_merge<32>(v, A, K, H, W, score_mode, score, sem_seg, argmax, st);
}
