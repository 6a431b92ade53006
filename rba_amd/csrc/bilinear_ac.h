// The align_corners=True bilinear taps shared by K9 (outlier_tail.hip), K10 (dense_hybrid_loss.hip) and K11 (pebal_loss.hip), forward and backward: torch's
// upsample_bilinear2d restated -- scale = (in - 1) / (out - 1) as an fp32 quotient (0 when out == 1), src = scale * dst, i0 = (int)src,
// i1 = i0 + (i0 < in - 1), l = src - i0, h = 1 - l; value = hy (hx v00 + lx v01) + ly (hx v10 + lx v11) -- the label reader, and the two walks of the
// gather-form backward kernels: ac_visit_naming (one thread per source pixel: K9, K11b) and AcOwner (16 lanes per source pixel: K10, K11a).  One function for
// both directions, so a backward's taps and weights are its forward's bits.
#pragma once
#include <math.h>
#include "common.h"

struct AcTap {
  int i0, i1;
  float l, h;
};

__host__ __device__ __forceinline__ float ac_scale(int in, int out) { return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f; }

__device__ __forceinline__ AcTap tap_of(int dst, float scale, int in) {
  // the product rounded ONCE, for the floor and for the weight alike: written as scale * dst, -ffp-contract=fast fused it into `l` below in some
  // callers (K10 / K11a's backward) and not in others -- fma(scale, dst, -i0) is one ulp of src away from src - i0, so a tap whose weight is exactly 0
  // in torch (src an integer) got about -2^-22 there, and a backward's weights were no longer its forward's bits.  An fma with +0 is not a product
  // the compiler may contract (it would have to prove the product is not -0).
  const float src = fmaf(scale, (float)dst, 0.0f);
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

// the sequential gather walk (K9's tail_bwd_kernel, K11b's sr_bwd_kernel): one thread owns source pixel (b, y, x) of an [h, w] plane and visits, in ascending
// Y then X, every pixel of the [H, W] label map whose taps name it -- body(ty, tx, weight = wy wx of (y, x) in that pixel's sample, its flat label index).
// A fixed order in one thread: what the body adds up is bitwise reproducible; nobody samples the pixel (H < h): no visit.
template <class Body>
__device__ __forceinline__ void ac_visit_naming(int b, int y, int x, int h, int w, int H, int W, Body body) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  int Y0, Y1, X0, X1;
  candidates(y, sy, H, Y0, Y1);
  candidates(x, sx, W, X0, X1);
  for (int Y = Y0; Y <= Y1; ++Y) {
    const AcTap ty = tap_of(Y, sy, h);
    if (ty.i0 != y && ty.i1 != y) continue;
    const float wy = tap_weight(ty, y);
    const int64_t row = ((int64_t)b * H + Y) * W;
    for (int X = X0; X <= X1; ++X) {
      const AcTap tx = tap_of(X, sx, w);
      if (tx.i0 != x && tx.i1 != x) continue;
      body(ty, tx, wy * tap_weight(tx, x), row + X);
    }
  }
}

// ---- the per-label-pixel walk over a K-channel map, shared by K10 (dense_hybrid_loss.hip) and K11 (pebal_loss.hip)

// THE label reader of K9 - K11: the label as 0 .. 255, every int64 value outside [0, 255) one more ignored value (255).  The dtype is a template parameter
// of the kernels.  K9 / K11b's "inlier" and "outlier" are exactly ac_label == 0 and ac_label == 1, for every int64 and every uint8 value: 0 and 1 pass
// through, and no other value maps onto them.
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

// ---- the 16-lane gather walk (K10's dh_bwd_kernel, K11a's gm_bwd_kernel): AC_SPLIT lanes own one source pixel (b, y, x) of every channel.  They find the
// label rows / columns whose taps name it (ac_naming: a contiguous range), split that rectangle among themselves -- lane `sub` takes candidates sub,
// sub + 16, ... in ascending order -- add what the kernel's own arithmetic makes of each candidate, and ac_split_sum joins the 16 lanes in a fixed xor tree;
// lane 0 stores.  Plain stores, fixed orders: bitwise reproducible; a pixel nobody samples gets 0.
constexpr int AC_SPLIT = 16;

struct AcOwner {
  bool live;                 // an owner past the end walks nothing (n = 0) and stores nothing, but takes part in the shuffles
  int sub, b, r, y, x;       // this lane's share; the owner pixel and r = y w + x
  int h, w, H, W;
  float sy, sx;
  int Y0, X0;                // the rectangle's corner, nX columns, n candidates (<= H W < 2^31: c + 16 stays below 2^32)
  uint32_t nX, n;
};

struct AcCandidate {         // label pixel P = (b, Y, X): its taps and the weight of the owner pixel in its sample
  AcTaps4 t;
  float wgt;
  int64_t P;
};

// workgroups of AC_SPLIT * owners_per_group threads over `pixels` = B h w owner pixels
__device__ __forceinline__ AcOwner ac_owner(int owners_per_group, int64_t pixels, int h, int w, int H, int W) {
  AcOwner o;
  o.sub = threadIdx.x & (AC_SPLIT - 1);
  const int64_t owner = (int64_t)blockIdx.x * owners_per_group + threadIdx.x / AC_SPLIT;
  o.live = owner < pixels;
  const int64_t i = o.live ? owner : pixels - 1;
  const int hw = h * w;
  o.b = (int)(i / hw), o.r = (int)(i - (int64_t)o.b * hw), o.y = o.r / w, o.x = o.r - o.y * w;
  o.h = h, o.w = w, o.H = H, o.W = W;
  o.sy = ac_scale(h, H), o.sx = ac_scale(w, W);
  int Y1, X1;
  ac_naming(o.y, o.sy, h, H, o.Y0, Y1);
  ac_naming(o.x, o.sx, w, W, o.X0, X1);
  o.nX = X1 >= o.X0 ? X1 - o.X0 + 1 : 0;
  o.n = o.live && Y1 >= o.Y0 ? (uint32_t)(Y1 - o.Y0 + 1) * o.nX : 0;
  return o;
}

__device__ __forceinline__ AcCandidate ac_candidate(const AcOwner& o, uint32_t c) {
  const uint32_t dy = c / o.nX;
  const int Y = o.Y0 + (int)dy, X = o.X0 + (int)(c - dy * o.nX);
  const AcTap ty = tap_of(Y, o.sy, o.h), tx = tap_of(X, o.sx, o.w);
  AcCandidate q;
  q.wgt = tap_weight(ty, o.y) * tap_weight(tx, o.x);
  q.t = ac_taps4(ty, tx, o.w);
  q.P = ((int64_t)o.b * o.H + Y) * o.W + X;
  return q;
}

// the 16 lanes of an owner, a fixed xor tree (every lane of the wave must be here)
__device__ __forceinline__ float ac_split_sum(float v) {
#pragma unroll
  for (int o = AC_SPLIT / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, RBA_WAVE);
  return v;
}
