// K9 -- the tail of SetCriterion.outlier_loss behind the score map (reference: mask2former/modeling/criterion.py:474-518): the align_corners=True
// bilinear upsample of the one-channel score [B,h,w] to the labels' [B,H,W], the per-pixel term, the masked means, the halving rule -- and all of
// it backward.  fp32, wave64, no MFMA, no LDS beyond the reduction's 16 words per wave, no scratch.  docs/kernels/K9.md.
//
// Upsample (tap_of, bilinear_ac.h -- shared with K10): torch's upsample_bilinear2d with align_corners=True -- scale = (in - 1) / (out - 1) as an fp32 quotient (0 when out == 1),
// src = scale * dst, i0 = (int)src, i1 = i0 + (i0 < in - 1), l = src - i0, h = 1 - l; value = hy (hx v00 + lx v01) + ly (hx v10 + lx v11).
// Forward and backward call the same function, so the backward's taps and weights are the forward's bits.
//
// Term (label 0: d = s - thr_in, label 1: d = thr_out - s, anything else ignored): func 0 relu(d)^2, 2 d^2, 3 |d|, summed per class; func 1 =
// binary cross-entropy with logits against (label == 1) over ALL pixels (ignored labels are target 0, as in the reference).
//
// (a) tail_partial_kernel: a workgroup walks pixels wg 256 + tid + k G 256, every thread a fixed set in ascending order, a fixed shuffle / LDS
//     tree; its four partial results (sum_in, n_in, sum_out, n_out; the counts as integers) go to the caller's workspace with plain stores.
//     tail_finish_kernel = one workgroup that adds the partials in a fixed order and forms the loss on the device:
//     L = sum_in / n_in; n_out > 0: L = 0.5 (L + sum_out / n_out); n_in == 0: NaN (the mean of nothing).  func 1: L = 0.5 sum / (B H W), and
//     stats = (sum, B H W, 0, 0).  No float atomics; no word of the workspace has to start from a known value; loss and stats are bitwise reproducible.
// (b) tail_bwd_kernel, gather form: one thread per score pixel (b, y, x).  It walks the label rows / columns whose source coordinate can touch
//     it (the range from dividing by the scale, one wider on each side, clamped), recomputes each candidate's taps with tap_of, skips those that do
//     not name the pixel, recomputes the upsampled score there and adds weight * d term / d s * the class factor from `stats` and *grad_loss
//     (both read on the device).  Plain stores, a fixed loop order: bitwise reproducible; a pixel nobody samples (H < h) gets 0.
//     Subgradients as torch: relu'(0) = 0, sign(0) = 0.
#include "bilinear_ac.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int OT_THREADS = 256, OT_MAX_GROUPS = 2048, OT_PER_THREAD = 4;

// 0 = inlier, 1 = outlier, anything else = ignored
__device__ __forceinline__ int label_at(const void* __restrict__ labels, int label_bytes, int64_t i) {
  if (label_bytes == 1) return (int)reinterpret_cast<const uint8_t*>(labels)[i];
  const int64_t v = reinterpret_cast<const int64_t*>(labels)[i];
  return v == 0 ? 0 : v == 1 ? 1 : 255;
}

// `func` is a template parameter of every kernel, chosen by the launchers' switch: as a run-time (uniform) argument the compiler folded the chain
// `func == 0 ? ... : func == 2 ? ... : |d|` inside the pixel loop into a branch structure whose func == 3 path added an undefined register to the sum
// (read in the ISA; l1's sums came out as denormals on MI355X).  No run-time selection of the term is left.
template <int FUNC>
__device__ __forceinline__ float term_of(float d) {
  if constexpr (FUNC == 0) {
    const float r = fmaxf(d, 0.f);
    return r * r;
  } else if constexpr (FUNC == 2) {
    return d * d;
  } else {
    return fabsf(d);
  }
}
// d term / d d
template <int FUNC>
__device__ __forceinline__ float dterm_of(float d) {
  if constexpr (FUNC == 0) {
    return d > 0.f ? 2.0f * d : 0.f;
  } else if constexpr (FUNC == 2) {
    return 2.0f * d;
  } else {
    return d > 0.f ? 1.0f : d < 0.f ? -1.0f : 0.f;
  }
}

int groups_of(int64_t total) {
  const int64_t g = (total + OT_THREADS * OT_PER_THREAD - 1) / (OT_THREADS * OT_PER_THREAD);
  return (int)(g < OT_MAX_GROUPS ? g : OT_MAX_GROUPS);
}

// workspace: [G][4] words = (sum_in float, n_in int, sum_out float, n_out int)
template <int FUNC>
__global__ __launch_bounds__(OT_THREADS) void tail_partial_kernel(const float* __restrict__ score, const void* __restrict__ labels, int label_bytes,
                                                                  int h, int w, int H, int W, int64_t total, float thr_in, float thr_out,
                                                                  float* __restrict__ ws) {
  __shared__ float red_f[OT_THREADS / 64][2];
  __shared__ int red_n[OT_THREADS / 64][2];
  const int tid = threadIdx.x;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int64_t HW = (int64_t)H * W, stride = (int64_t)gridDim.x * OT_THREADS;
  float s_in = 0.f, s_out = 0.f;
  int n_in = 0, n_out = 0;
  for (int64_t i = (int64_t)blockIdx.x * OT_THREADS + tid; i < total; i += stride) {
    const int lab = label_at(labels, label_bytes, i);
    if (FUNC != 1 && lab != 0 && lab != 1) continue;
    const int b = (int)(i / HW), r = (int)(i - (int64_t)b * HW), Y = r / W, X = r - Y * W;
    const float s = upsampled(score + (int64_t)b * h * w, w, tap_of(Y, sy, h), tap_of(X, sx, w));
    if constexpr (FUNC == 1) {
      s_in += fmaxf(s, 0.f) - (lab == 1 ? s : 0.f) + log1pf(expf(-fabsf(s)));
    } else {
      if (lab == 0) {
        s_in += term_of<FUNC>(s - thr_in);
        ++n_in;
      } else {
        s_out += term_of<FUNC>(thr_out - s);
        ++n_out;
      }
    }
  }
  s_in = wave_reduce_sum(s_in);
  s_out = wave_reduce_sum(s_out);
  n_in = wave_reduce_sum_int(n_in);
  n_out = wave_reduce_sum_int(n_out);
  if ((tid & 63) == 0) {
    red_f[tid >> 6][0] = s_in;
    red_f[tid >> 6][1] = s_out;
    red_n[tid >> 6][0] = n_in;
    red_n[tid >> 6][1] = n_out;
  }
  __syncthreads();
  if (tid < 2) {
    float* out = ws + 4 * (int64_t)blockIdx.x;
    out[2 * tid] = (red_f[0][tid] + red_f[1][tid]) + (red_f[2][tid] + red_f[3][tid]);
    out[2 * tid + 1] = __int_as_float((red_n[0][tid] + red_n[1][tid]) + (red_n[2][tid] + red_n[3][tid]));
  }
}

// thread t takes the partials t, t + 256, ... in ascending order, then a fixed tree
__global__ __launch_bounds__(OT_THREADS) void tail_finish_kernel(const float* __restrict__ ws, int G, int64_t total, int bce, float* __restrict__ loss,
                                                                 float* __restrict__ stats) {
  __shared__ float red_f[OT_THREADS / 64][2];
  __shared__ int red_n[OT_THREADS / 64][2];
  const int tid = threadIdx.x;
  float s_in = 0.f, s_out = 0.f;
  int n_in = 0, n_out = 0;
  for (int g = tid; g < G; g += OT_THREADS) {
    const float* p = ws + 4 * (int64_t)g;
    s_in += p[0];
    n_in += __float_as_int(p[1]);
    s_out += p[2];
    n_out += __float_as_int(p[3]);
  }
  s_in = wave_reduce_sum(s_in);
  s_out = wave_reduce_sum(s_out);
  n_in = wave_reduce_sum_int(n_in);
  n_out = wave_reduce_sum_int(n_out);
  if ((tid & 63) == 0) {
    red_f[tid >> 6][0] = s_in;
    red_f[tid >> 6][1] = s_out;
    red_n[tid >> 6][0] = n_in;
    red_n[tid >> 6][1] = n_out;
  }
  __syncthreads();
  if (tid == 0) {
    const float a = (red_f[0][0] + red_f[1][0]) + (red_f[2][0] + red_f[3][0]), c = (red_f[0][1] + red_f[1][1]) + (red_f[2][1] + red_f[3][1]);
    const int na = (red_n[0][0] + red_n[1][0]) + (red_n[2][0] + red_n[3][0]), nc = (red_n[0][1] + red_n[1][1]) + (red_n[2][1] + red_n[3][1]);
    if (bce) {
      stats[0] = a;
      stats[1] = (float)total;
      stats[2] = 0.f;
      stats[3] = 0.f;
      *loss = 0.5f * (a / (float)total);
    } else {
      stats[0] = a;
      stats[1] = (float)na;
      stats[2] = c;
      stats[3] = (float)nc;
      float L = a / (float)na;                            // n_in == 0: 0 / 0 = NaN, the mean of nothing
      if (nc > 0) L = 0.5f * (L + c / (float)nc);
      *loss = L;
    }
  }
}

template <int FUNC>
__global__ __launch_bounds__(OT_THREADS) void tail_bwd_kernel(const float* __restrict__ score, const void* __restrict__ labels, int label_bytes, int h,
                                                              int w, int H, int W, int64_t pixels, int64_t total, float thr_in,
                                                              float thr_out, const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                              float* __restrict__ grad_score) {
  const int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x;
  if (i >= pixels) return;
  const int hw = h * w, b = (int)(i / hw), r = (int)(i - (int64_t)b * hw), y = r / w, x = r - y * w;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const float g = *grad_loss;
  // d loss / d (a class's sum): the mean's 1 / n and the halving rule
  float f_in, f_out;
  if constexpr (FUNC == 1) {
    f_in = f_out = 0.5f * g / (float)total;
  } else {
    const float n_in = stats[1], n_out = stats[3];
    f_in = (n_out > 0.f ? 0.5f * g : g) / n_in;
    f_out = n_out > 0.f ? 0.5f * g / n_out : 0.f;
  }
  const float* plane = score + (int64_t)b * hw;
  int Y0, Y1, X0, X1;
  candidates(y, sy, H, Y0, Y1);
  candidates(x, sx, W, X0, X1);
  float acc = 0.f;
  for (int Y = Y0; Y <= Y1; ++Y) {
    const AcTap ty = tap_of(Y, sy, h);
    if (ty.i0 != y && ty.i1 != y) continue;
    const float wy = (ty.i0 == y ? ty.h : 0.f) + (ty.i1 == y ? ty.l : 0.f);
    const int64_t row = ((int64_t)b * H + Y) * W;
    for (int X = X0; X <= X1; ++X) {
      const AcTap tx = tap_of(X, sx, w);
      if (tx.i0 != x && tx.i1 != x) continue;
      const int lab = label_at(labels, label_bytes, row + X);
      if (FUNC != 1 && lab != 0 && lab != 1) continue;
      const float wx = (tx.i0 == x ? tx.h : 0.f) + (tx.i1 == x ? tx.l : 0.f);
      const float s = upsampled(plane, w, ty, tx);
      float ds;                                           // d loss / d s at (Y, X)
      if constexpr (FUNC == 1)
        ds = f_in * (1.0f / (1.0f + expf(-s)) - (lab == 1 ? 1.0f : 0.f));
      else if (lab == 0)
        ds = f_in * dterm_of<FUNC>(s - thr_in);
      else
        ds = -f_out * dterm_of<FUNC>(thr_out - s);
      acc += wy * wx * ds;
    }
  }
  grad_score[i] = acc;
}

bool shape_ok(int B, int h, int w, int H, int W) {
  return B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)B * h * w <= 0x7fffffffLL &&
         (int64_t)H * W <= 0x7fffffffLL && (int64_t)h * w <= 0x7fffffffLL;
}

}  // namespace

extern "C" int rba_outlier_tail_workspace_f32(int B, int H, int W, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL);
  *bytes = (int64_t)groups_of((int64_t)B * H * W) * 4 * (int64_t)sizeof(float);
  return 0;
}

extern "C" int rba_outlier_tail_fwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, int func,
                                        float thr_in, float thr_out, float* workspace, float* loss, float* stats, void* stream) {
  RBA_CHECK_ARG(shape_ok(B, h, w, H, W) && (label_bytes == 1 || label_bytes == 8) && func >= 0 && func <= 3);
  RBA_CHECK_ARG(score && labels && workspace && loss && stats && (((uintptr_t)workspace) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * H * W;
  const int G = groups_of(total);
#define OT_PARTIAL(F) \
  hipLaunchKernelGGL(tail_partial_kernel<F>, dim3(G), dim3(OT_THREADS), 0, st, score, labels, label_bytes, h, w, H, W, total, thr_in, thr_out, workspace)
  switch (func) {
    case 0: OT_PARTIAL(0); break;
    case 1: OT_PARTIAL(1); break;
    case 2: OT_PARTIAL(2); break;
    default: OT_PARTIAL(3); break;
  }
#undef OT_PARTIAL
  if (const int e = rba_launch_status()) return e;
  hipLaunchKernelGGL(tail_finish_kernel, dim3(1), dim3(OT_THREADS), 0, st, workspace, G, total, (int)(func == 1), loss, stats);
  return rba_launch_status();
}

extern "C" int rba_outlier_tail_bwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, int func,
                                        float thr_in, float thr_out, const float* stats, const float* grad_loss, float* grad_score, void* stream) {
  RBA_CHECK_ARG(shape_ok(B, h, w, H, W) && (label_bytes == 1 || label_bytes == 8) && func >= 0 && func <= 3);
  RBA_CHECK_ARG(score && labels && stats && grad_loss && grad_score);
  rba_begin();
  const int64_t pixels = (int64_t)B * h * w;
#define OT_BWD(F)                                                                                                                              \
  hipLaunchKernelGGL(tail_bwd_kernel<F>, dim3((unsigned)((pixels + OT_THREADS - 1) / OT_THREADS)), dim3(OT_THREADS), 0, (hipStream_t)stream, score, \
                     labels, label_bytes, h, w, H, W, pixels, (int64_t)B * H * W, thr_in, thr_out, stats, grad_loss, grad_score)
  switch (func) {
    case 0: OT_BWD(0); break;
    case 1: OT_BWD(1); break;
    case 2: OT_BWD(2); break;
    default: OT_BWD(3); break;
  }
#undef OT_BWD
  return rba_launch_status();
}
