// The align_corners=True bilinear taps shared by K9 (outlier_tail.hip) and K10 (dense_hybrid_loss.hip), forward and backward: torch's
// upsample_bilinear2d restated -- scale = (in - 1) / (out - 1) as an fp32 quotient (0 when out == 1), src = scale * dst, i0 = (int)src,
// i1 = i0 + (i0 < in - 1), l = src - i0, h = 1 - l; value = hy (hx v00 + lx v01) + ly (hx v10 + lx v11) -- and the candidate range of the gather-form
// backward kernels.  One function for both directions, so a backward's taps and weights are its forward's bits.
#pragma once
#include <math.h>
#include "common.h"

struct AcTap {
  int i0, i1;
  float l, h;
};

__host__ __device__ __forceinline__ float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

__device__ __forceinline__ AcTap tap_of(int dst, float scale, int in) {
  const float src = scale * (float)dst;
  int i0 = (int)src;                                    // src >= 0: trunc == floor
  i0 = i0 < in - 1 ? i0 : in - 1;                       // never past the map, whatever the product's rounding
  AcTap t;
  t.i0 = i0;
  t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
  t.l = src - (float)i0;
  t.h = 1.0f - t.l;
  return t;
}

__device__ __forceinline__ float upsampled(const float* __restrict__ plane, int w, const AcTap& ty, const AcTap& tx) {
  const float* r0 = plane + (int64_t)ty.i0 * w;
  const float* r1 = plane + (int64_t)ty.i1 * w;
  return ty.h * (tx.h * r0[tx.i0] + tx.l * r0[tx.i1]) + ty.l * (tx.h * r1[tx.i0] + tx.l * r1[tx.i1]);
}

// the share of source row / column p in a destination's tap pair: a pair that coincides (i0 == i1, the last row) contributes both weights
__device__ __forceinline__ float tap_weight(const AcTap& t, int p) { return (t.i0 == p ? t.h : 0.f) + (t.i1 == p ? t.l : 0.f); }

// the label rows / columns [lo, hi] whose source coordinate scale * dst can lie in (p - 1, p + 1), one wider on each side, clamped to [0, out - 1]
__device__ __forceinline__ void candidates(int p, float scale, int out, int& lo, int& hi) {
  lo = 0;
  hi = out - 1;
  if (scale > 0.f) {
    // (the 1e-6 covers the rounding of scale * dst and of the two quotients, four relative errors of 2^-24 at the most)
    const float a = fmaxf(floorf((float)(p - 1) / scale * (1.0f - 1e-6f)) - 1.0f, 0.f);
    const float b = fmaxf(ceilf((float)(p + 1) / scale * (1.0f + 1e-6f)) + 1.0f, 0.f);
    const int64_t top = out - 1, ia = (int64_t)fminf(a, 4e9f), ib = (int64_t)fminf(b, 4e9f);
    lo = (int)(ia < top ? ia : top);
    hi = (int)(ib < top ? ib : top);
  }
}

__device__ __forceinline__ int wave_reduce_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RBA_WAVE);
  return v;
}
