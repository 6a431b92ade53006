// The align_corners=True bilinear taps shared by K9 (outlier_tail.hip), K10 (dense_hybrid_loss.hip) and K11 (pebal_loss.hip), forward and backward: torch's
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

// ---- the per-label-pixel walk over a K-channel map, shared by K10 (dense_hybrid_loss.hip) and K11 (pebal_loss.hip)

// the label as 0 .. 255: every int64 value outside [0, 255) is one more ignored value.  The dtype is a template parameter of the kernels
template <int LB>
__device__ __forceinline__ int ac_label(const void* __restrict__ labels, int64_t i) {
  if constexpr (LB == 1) {
    return (int)reinterpret_cast<const uint8_t*>(labels)[i];
  } else {
    const int64_t v = reinterpret_cast<const int64_t*>(labels)[i];
    return v >= 0 && v < 255 ? (int)v : 255;
  }
}

struct AcTaps4 {          // the four taps of a label pixel as offsets into an [h, w] plane, and its weights
  int o00, o01, o10, o11;
  float hy, ly, hx, lx;
};

__device__ __forceinline__ AcTaps4 ac_taps4(const AcTap& ty, const AcTap& tx, int w) {
  AcTaps4 t;
  t.o00 = ty.i0 * w + tx.i0;
  t.o01 = ty.i0 * w + tx.i1;
  t.o10 = ty.i1 * w + tx.i0;
  t.o11 = ty.i1 * w + tx.i1;
  t.hy = ty.h, t.ly = ty.l, t.hx = tx.h, t.lx = tx.l;
  return t;
}

// ATen's operation order (upsampled, above)
__device__ __forceinline__ float ac_sample(const float* __restrict__ plane, const AcTaps4& t) {
  return t.hy * (t.hx * plane[t.o00] + t.lx * plane[t.o01]) + t.ly * (t.hx * plane[t.o10] + t.lx * plane[t.o11]);
}

// the destination rows / columns [lo, hi] whose tap pair names source row / column p: contiguous, because tap_of's i0 never decreases with dst
// and a destination names p exactly while i0 is p - 1 (with i1 = p) or p.  lo > hi: nobody samples p.
__device__ __forceinline__ void ac_naming(int p, float scale, int in, int out, int& lo, int& hi) {
  int a, b;
  candidates(p, scale, out, a, b);
  lo = b + 1;
  hi = a - 1;
  for (int d = a; d <= b; ++d) {
    const AcTap t = tap_of(d, scale, in);
    if (t.i0 == p || t.i1 == p) {
      lo = d < lo ? d : lo;
      hi = d;
    }
  }
}

__device__ __forceinline__ int wave_reduce_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RBA_WAVE);
  return v;
}
