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
// (a) tail_partial_kernel + tail_finish_kernel: the partial / finish scheme of loss_reduce.h, two sums and two counts (sum_in, sum_out, n_in, n_out),
//     OT_PER_THREAD = 4 pixels to a thread before the cap.  The finish forms the loss on the device:
//     L = sum_in / n_in; n_out > 0: L = 0.5 (L + sum_out / n_out); n_in == 0: NaN (the mean of nothing).  func 1: L = 0.5 sum / (B H W), and
//     stats = (sum, B H W, 0, 0).  Loss and stats are bitwise reproducible.
// (b) tail_bwd_kernel, gather form: one thread per score pixel (b, y, x), the sequential walk of bilinear_ac.h (ac_visit_naming) over the label
//     pixels whose taps name it; at each it recomputes the upsampled score and adds weight * d term / d s * the class factor from `stats` and
//     *grad_loss (both read on the device).  Plain stores, a fixed loop order: bitwise reproducible; a pixel nobody samples (H < h) gets 0.
//     Subgradients as torch: relu'(0) = 0, sign(0) = 0.
// The label width is a template parameter of the kernels (ac_label<LB>, bilinear_ac.h), like `func`: the launchers' switch chooses both.
#include "bilinear_ac.h"
#include "loss_reduce.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int OT_THREADS = LOSS_THREADS, OT_PER_THREAD = 4, OT_WS = 4;    // workspace words per workgroup: sum_in sum_out n_in n_out

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

template <int FUNC, int LB>
__global__ __launch_bounds__(OT_THREADS) void tail_partial_kernel(const float* __restrict__ score, const void* __restrict__ labels, int h, int w, int H,
                                                                  int W, int64_t total, float thr_in, float thr_out, float* __restrict__ ws) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int64_t HW = (int64_t)H * W, stride = (int64_t)gridDim.x * OT_THREADS;
  LossSums<2, 2> a{};                                     // f: sum_in, sum_out; n: n_in, n_out
  for (int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x; i < total; i += stride) {
    const int lab = ac_label<LB>(labels, i);
    if (FUNC != 1 && lab != 0 && lab != 1) continue;
    const int b = (int)(i / HW), r = (int)(i - (int64_t)b * HW), Y = r / W, X = r - Y * W;
    const float s = upsampled(score + (int64_t)b * h * w, w, tap_of(Y, sy, h), tap_of(X, sx, w));
    if constexpr (FUNC == 1) {
      a.f[0] += fmaxf(s, 0.f) - (lab == 1 ? s : 0.f) + log1pf(expf(-fabsf(s)));
    } else {
      if (lab == 0) {
        a.f[0] += term_of<FUNC>(s - thr_in);
        ++a.n[0];
      } else {
        a.f[1] += term_of<FUNC>(thr_out - s);
        ++a.n[1];
      }
    }
  }
  loss_store_partial<OT_WS>(a, ws);
}

__global__ __launch_bounds__(OT_THREADS) void tail_finish_kernel(const float* __restrict__ ws, int G, int64_t total, int bce, float* __restrict__ loss,
                                                                 float* __restrict__ stats) {
  loss_finish<OT_WS, 2, 2>(ws, G, [=](const LossSums<2, 2>& t) {
    const float a = t.f[0], c = t.f[1];
    const int na = t.n[0], nc = t.n[1];
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
  });
}

template <int FUNC, int LB>
__global__ __launch_bounds__(OT_THREADS) void tail_bwd_kernel(const float* __restrict__ score, const void* __restrict__ labels, int h, int w, int H, int W,
                                                              int64_t pixels, int64_t total, float thr_in, float thr_out,
                                                              const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                              float* __restrict__ grad_score) {
  const int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x;
  if (i >= pixels) return;
  const int hw = h * w, b = (int)(i / hw), r = (int)(i - (int64_t)b * hw), y = r / w, x = r - y * w;
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
  float acc = 0.f;
  ac_visit_naming(b, y, x, h, w, H, W, [&](const AcTap& ty, const AcTap& tx, float wgt, int64_t P) {
    const int lab = ac_label<LB>(labels, P);
    if (FUNC != 1 && lab != 0 && lab != 1) return;
    const float s = upsampled(plane, w, ty, tx);
    float ds;                                             // d loss / d s at P
    if constexpr (FUNC == 1)
      ds = f_in * (1.0f / (1.0f + expf(-s)) - (lab == 1 ? 1.0f : 0.f));
    else if (lab == 0)
      ds = f_in * dterm_of<FUNC>(s - thr_in);
    else
      ds = -f_out * dterm_of<FUNC>(thr_out - s);
    acc += wgt * ds;
  });
  grad_score[i] = acc;
}

bool shape_ok(int B, int h, int w, int H, int W) {
  return B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)B * h * w <= 0x7fffffffLL &&
         (int64_t)H * W <= 0x7fffffffLL && (int64_t)h * w <= 0x7fffffffLL;
}

}  // namespace

extern "C" int rba_outlier_tail_workspace_f32(int B, int H, int W, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL);
  *bytes = (int64_t)loss_groups((int64_t)B * H * W, OT_PER_THREAD) * OT_WS * (int64_t)sizeof(float);
  return 0;
}

// the launchers' switch: func 0 .. 3, labels of 1 | 8 bytes -- no run-time selection inside the kernels
#define OT_LABELS(LAUNCH, F)           \
  do {                                 \
    if (label_bytes == 1) LAUNCH(F, 1); \
    else LAUNCH(F, 8);                 \
  } while (0)
#define OT_DISPATCH(LAUNCH)                 \
  switch (func) {                           \
    case 0: OT_LABELS(LAUNCH, 0); break;    \
    case 1: OT_LABELS(LAUNCH, 1); break;    \
    case 2: OT_LABELS(LAUNCH, 2); break;    \
    default: OT_LABELS(LAUNCH, 3); break;   \
  }

extern "C" int rba_outlier_tail_fwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, int func,
                                        float thr_in, float thr_out, float* workspace, float* loss, float* stats, void* stream) {
  RBA_CHECK_ARG(shape_ok(B, h, w, H, W) && (label_bytes == 1 || label_bytes == 8) && func >= 0 && func <= 3);
  RBA_CHECK_ARG(score && labels && workspace && loss && stats && (((uintptr_t)workspace) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * H * W;
  const int G = loss_groups(total, OT_PER_THREAD);
#define OT_PARTIAL(F, LB) \
  hipLaunchKernelGGL((tail_partial_kernel<F, LB>), dim3(G), dim3(OT_THREADS), 0, st, score, labels, h, w, H, W, total, thr_in, thr_out, workspace)
  OT_DISPATCH(OT_PARTIAL);
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
#define OT_BWD(F, LB)                                                                                                                             \
  hipLaunchKernelGGL((tail_bwd_kernel<F, LB>), dim3((unsigned)((pixels + OT_THREADS - 1) / OT_THREADS)), dim3(OT_THREADS), 0, (hipStream_t)stream, score, \
                     labels, h, w, H, W, pixels, (int64_t)B * H * W, thr_in, thr_out, stats, grad_loss, grad_score)
  OT_DISPATCH(OT_BWD);
#undef OT_BWD
  return rba_launch_status();
}
