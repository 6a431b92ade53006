// K11 -- the PEBAL fine-tune recipe's three losses behind K1 (reference: mask2former/modeling/criterion.py:245-388): SetCriterion.gambler_loss behind
// its (K+1)-channel class map (K11a), and smoothness_loss / sparsity_loss behind their score map (K11b) -- forward and backward.  No up-sampled
// map exists in either direction: every label pixel samples its values out of the quarter-resolution map (bilinear_ac.h's taps).
// fp32, wave64, no MFMA, no scratch, no float atomics, nothing read back.  docs/kernels/K11.md.
// Shared pieces: the partial / finish reduction (loss_reduce.h), the label reader and the two gather walks (bilinear_ac.h), the blur (gaussian_blur.h).
//
// K11a, per label pixel P:  x_k = sample of sem[b,k] (k < K: the classes, k = K: the reservation channel),
//   L_in = logsumexp_{k<K} x_k,  L = logsumexp_{k<=K} x_k,  p_k = exp(x_k - L),  reward r(P) = L_in^2,  R = blur_{7, sigma 1}(r) per image plane
//   (torchvision's GaussianBlur, gaussian_blur.hip),  res = p_K / R
//   label < K: t_in = log(p_label + res) (no clamp);   label 254: t_out = sum_{k<K} log(max(p_k + res, 1e-7));   anything else: void
//   loss = -(S_in / n_in + [n_ood > 0] ood_reg S_out / (n_ood K))                        n_in == 0: NaN, the mean of nothing, as in the reference
// forward:  (a) gm_reward_kernel: r;  (b) the blur: R;  (c) gm_partial_kernel + gm_finish_kernel: two sums, two counts.
// backward: (a) gm_dR_kernel: dR(P) = -(p_K / R^2) c sum 1 / (p_k + res) over P's live terms (a clamped term: 0; equality passes, as torch.clamp),
//           c = -g / n_in | -g ood_reg / (n_ood K);  (b) the blur's adjoint: dr = A^T dR;
//           (c) gm_bwd_kernel, the 16-lane gather walk (AcOwner): 16 lanes own one quarter-resolution pixel of all K + 1 channels, split the
//           rectangle of label pixels whose taps name it, recompute samples, L, L_in and the terms, and add
//           weight [d (direct softmax terms) / d x_k + dr(P) 2 L_in exp(x_k - L_in) [k < K]]; ac_split_sum, plain stores.
//
// K11b:  smoothness = 1/2 (sum_{y<h-1} (s[y+1,x] - s[y,x])^2 + sum_{x<w-1} (s[y,x+1] - s[y,x])^2)   (a sum; the last row / column add 0)
//        sparsity   = sqrt(sum_{label=1} up(s)^2), up = the align_corners=True upsample to the labels' size; 0 without labels or outlier pixel
// sr_partial_kernel / sr_finish_kernel: two sums, no count;  sr_bwd_kernel: one thread per score pixel, the four-neighbour stencil of the differences
// plus the sequential gather walk (ac_visit_naming) of w up(s)(P) / norm; 0 where the norm is 0 (torch.norm's backward).
#include "bilinear_ac.h"
#include "gaussian_blur.h"
#include "loss_reduce.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int PB_THREADS = LOSS_THREADS, PB_WS = 4;                 // workspace words per workgroup: two sums, two integer counts
constexpr int PB_OWNERS = PB_THREADS / AC_SPLIT;                    // gather backward: owner pixels per workgroup
constexpr int GM_OUTLIER = 254;
constexpr int GM_BLUR_K = 7;
constexpr float GM_BLUR_SIGMA = 1.0f, GM_CLAMP = 1e-7f;

// ---------------------------------------------------------------------------------------------------------------- the per-pixel arithmetic of K11a
// the K class samples x[k < K] -> e_k = exp(x_k - max_in) in place, their sum, and L_in = logsumexp_{k<K} x_k.  One function for every kernel,
// so the backward's L_in is the forward's bits.
template <int KMAX>
__device__ __forceinline__ void gm_inlier(float (&x)[KMAX], int K, float& mx_in, float& s_in, float& L_in) {
  mx_in = x[0];
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K) mx_in = fmaxf(mx_in, x[k]);
  s_in = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) {
      x[k] = expf(x[k] - mx_in);
      s_in += x[k];
    }
  L_in = mx_in + logf(s_in);
}

// with the reservation sample xr: L = logsumexp_{k<=K} x_k, f = exp(max_in - L) (so p_k = e_k f for k < K) and p_K = exp(xr - L)
__device__ __forceinline__ void gm_all(float mx_in, float s_in, float xr, float& f, float& pK) {
  const float mx = fmaxf(mx_in, xr);
  const float L = mx + logf(s_in * expf(mx_in - mx) + expf(xr - mx));
  f = expf(mx_in - L);
  pK = expf(xr - L);
}

template <int KMAX>
__device__ __forceinline__ void gm_samples(const float* __restrict__ sp, int hw, const AcTaps4& t, int K, float (&x)[KMAX]) {
#pragma unroll
  for (int k = 0; k < KMAX; ++k) x[k] = k < K ? ac_sample(sp + (int64_t)k * hw, t) : 0.f;
}

// forward (a): r(P) = L_in^2
template <int KMAX>
__global__ __launch_bounds__(PB_THREADS) void gm_reward_kernel(const float* __restrict__ sem, int K, int h, int w, int H, int W, int64_t total,
                                                               float* __restrict__ reward) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int hw = h * w;
  const uint32_t HW = (uint32_t)H * W, stride = gridDim.x * PB_THREADS, end = (uint32_t)total;    // B H W < 2^31: i + stride stays below 2^32
  for (uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x; i < end; i += stride) {
    const int b = (int)(i / HW), r = (int)(i - (uint32_t)b * HW), Y = r / W, X = r - Y * W;
    const AcTaps4 t = ac_taps4(tap_of(Y, sy, h), tap_of(X, sx, w), w);
    float x[KMAX], mx_in, s_in, L_in;
    gm_samples<KMAX>(sem + (int64_t)b * (K + 1) * hw, hw, t, K, x);
    gm_inlier<KMAX>(x, K, mx_in, s_in, L_in);
    reward[i] = L_in * L_in;
  }
}

// forward (c): the terms against the blurred reward R; a workgroup's record = (S_in, S_out, n_in, n_ood)
template <int KMAX, int LB>
__global__ __launch_bounds__(PB_THREADS) void gm_partial_kernel(const float* __restrict__ sem, const void* __restrict__ labels,
                                                                const float* __restrict__ R, int K, int h, int w, int H, int W, int64_t total,
                                                                float* __restrict__ ws) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int hw = h * w;
  const uint32_t HW = (uint32_t)H * W, stride = gridDim.x * PB_THREADS, end = (uint32_t)total;
  LossSums<2, 2> a{};                                     // f: S_in, S_out; n: n_in, n_ood
  for (uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x; i < end; i += stride) {
    const int lab = ac_label<LB>(labels, i);
    if (lab >= K && lab != GM_OUTLIER) continue;
    const int b = (int)(i / HW), r = (int)(i - (uint32_t)b * HW), Y = r / W, X = r - Y * W;
    const AcTaps4 t = ac_taps4(tap_of(Y, sy, h), tap_of(X, sx, w), w);
    const float* sp = sem + (int64_t)b * (K + 1) * hw;
    float x[KMAX], mx_in, sum_in, L_in, f, pK;
    gm_samples<KMAX>(sp, hw, t, K, x);
    gm_inlier<KMAX>(x, K, mx_in, sum_in, L_in);
    gm_all(mx_in, sum_in, ac_sample(sp + (int64_t)K * hw, t), f, pK);
    const float res = pK / R[i];
    if (lab < K) {
      float e_lab = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) e_lab = k == lab ? x[k] : e_lab;
      a.f[0] += logf(e_lab * f + res);
      ++a.n[0];
    } else {
      float t_out = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) t_out += logf(fmaxf(x[k] * f + res, GM_CLAMP));
      a.f[1] += t_out;
      ++a.n[1];
    }
  }
  loss_store_partial<PB_WS>(a, ws);
}

__global__ __launch_bounds__(PB_THREADS) void gm_finish_kernel(const float* __restrict__ ws, int G, int K, float ood_reg, float* __restrict__ losses,
                                                               float* __restrict__ stats) {
  loss_finish<PB_WS, 2, 2>(ws, G, [=](const LossSums<2, 2>& t) {
    const int Nood = t.n[1];
    const float N_in = (float)t.n[0], N_ood = (float)Nood;
    const float in_mean = t.f[0] / N_in;                                  // 0 / 0 = NaN, the mean of nothing
    const float out_mean = Nood > 0 ? t.f[1] / (N_ood * (float)K) : 0.f;  // the reference's `ood_mask.sum() > 0`, decided here
    losses[0] = -(in_mean + ood_reg * out_mean);
    losses[1] = in_mean;
    losses[2] = out_mean;
    stats[0] = t.f[0], stats[1] = t.f[1], stats[2] = N_in, stats[3] = N_ood;
  });
}

// d loss / d (a term of an inlier | outlier pixel): the means' 1 / n, the sign and ood_reg
__device__ __forceinline__ void gm_factors(const float* __restrict__ stats, const float* __restrict__ grad_loss, int K, float ood_reg, float& c_in,
                                           float& c_out) {
  const float g = *grad_loss;
  c_in = -g / stats[2];
  c_out = stats[3] > 0.f ? -g * ood_reg / (stats[3] * (float)K) : 0.f;
}

// backward (a): dR(P)
template <int KMAX, int LB>
__global__ __launch_bounds__(PB_THREADS) void gm_dR_kernel(const float* __restrict__ sem, const void* __restrict__ labels, const float* __restrict__ R,
                                                           int K, int h, int w, int H, int W, int64_t total, float ood_reg,
                                                           const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                           float* __restrict__ dR) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int hw = h * w;
  const uint32_t HW = (uint32_t)H * W, stride = gridDim.x * PB_THREADS, end = (uint32_t)total;
  float c_in, c_out;
  gm_factors(stats, grad_loss, K, ood_reg, c_in, c_out);
  for (uint32_t i = blockIdx.x * PB_THREADS + threadIdx.x; i < end; i += stride) {
    const int lab = ac_label<LB>(labels, i);
    float d = 0.f;
    if (lab < K || lab == GM_OUTLIER) {
      const int b = (int)(i / HW), r = (int)(i - (uint32_t)b * HW), Y = r / W, X = r - Y * W;
      const AcTaps4 t = ac_taps4(tap_of(Y, sy, h), tap_of(X, sx, w), w);
      const float* sp = sem + (int64_t)b * (K + 1) * hw;
      float x[KMAX], mx_in, sum_in, L_in, f, pK;
      gm_samples<KMAX>(sp, hw, t, K, x);
      gm_inlier<KMAX>(x, K, mx_in, sum_in, L_in);
      gm_all(mx_in, sum_in, ac_sample(sp + (int64_t)K * hw, t), f, pK);
      const float Rv = R[i], res = pK / Rv;
      const bool out = lab == GM_OUTLIER;
      float U = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          const float a = x[k] * f + res;
          U += (out ? a >= GM_CLAMP : k == lab) ? 1.0f / a : 0.f;
        }
      d = -(pK / (Rv * Rv)) * ((out ? c_out : c_in) * U);
    }
    dR[i] = d;
  }
}

// backward (c): grad_sem [B,K+1,h,w]
template <int KMAX, int LB>
__global__ __launch_bounds__(PB_THREADS) void gm_bwd_kernel(const float* __restrict__ sem, const void* __restrict__ labels, const float* __restrict__ R,
                                                            const float* __restrict__ dr, int K, int h, int w, int H, int W, int64_t pixels,
                                                            float ood_reg, const float* __restrict__ stats, const float* __restrict__ grad_loss,
                                                            float* __restrict__ grad_sem) {
  const AcOwner o = ac_owner(PB_OWNERS, pixels, h, w, H, W);
  const int hw = h * w;
  float c_in, c_out;
  gm_factors(stats, grad_loss, K, ood_reg, c_in, c_out);
  const float* sp = sem + (int64_t)o.b * (K + 1) * hw;
  float acc[KMAX], accR = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
  for (uint32_t c = o.sub; c < o.n; c += AC_SPLIT) {
    const AcCandidate q = ac_candidate(o, c);
    const int lab = ac_label<LB>(labels, q.P);
    float e[KMAX], mx_in, sum_in, L_in;
    gm_samples<KMAX>(sp, hw, q.t, K, e);
    gm_inlier<KMAX>(e, K, mx_in, sum_in, L_in);
    // through the reward: dr(P) d (L_in^2) / d x_k = dr(P) 2 L_in e_k / sum_in, every pixel (the blur spreads a term's gradient to its neighbours)
    const float tr = q.wgt * (dr[q.P] * 2.0f * L_in / sum_in);
    if (lab < K || lab == GM_OUTLIER) {
      float f, pK;
      gm_all(mx_in, sum_in, ac_sample(sp + (int64_t)K * hw, q.t), f, pK);
      const float Rv = R[q.P], res = pK / Rv;
      const bool out = lab == GM_OUTLIER;
      const float cc = out ? c_out : c_in;
      // u_k = d term / d p_k of the live terms; U = their sum (d / d res); D = sum_m p_m d term / d p_m, the softmax's pull-back
      float U = 0.f, D = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          const float p = e[k] * f, a = p + res;
          const float u = (out ? a >= GM_CLAMP : k == lab) ? cc / a : 0.f;
          U += u;
          D = fmaf(p, u, D);
        }
      const float qK = U / Rv;
      D = fmaf(pK, qK, D);
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          const float p = e[k] * f, a = p + res;
          const float u = (out ? a >= GM_CLAMP : k == lab) ? cc / a : 0.f;
          acc[k] += q.wgt * (p * (u - D)) + tr * e[k];
        }
      accR = fmaf(q.wgt, pK * (qK - D), accR);
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc[k] = fmaf(tr, e[k], acc[k]);
    }
  }
  accR = ac_split_sum(accR);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) acc[k] = ac_split_sum(acc[k]);
  if (o.live && o.sub == 0) {
    float* gs = grad_sem + (int64_t)o.b * (K + 1) * hw + o.r;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) gs[(int64_t)k * hw] = acc[k];
    gs[(int64_t)K * hw] = accR;
  }
}

bool gm_shape_ok(int B, int K, int h, int w, int H, int W) {
  return K >= 1 && K + 1 <= 32 && h >= 1 && w >= 1 && rba_blur_planes_ok(B, H, W, GM_BLUR_K, GM_BLUR_SIGMA) && (int64_t)B * (K + 1) * h * w <= 0x7fffffffLL &&
         (int64_t)H * W <= 0x7fffffffLL && (int64_t)h * w <= 0x7fffffffLL;
}

// ---------------------------------------------------------------------------------------------------------------- K11b
// a workgroup's record = (sum of squared differences, sum of squared outlier samples, -, -)
template <int LB>
__global__ __launch_bounds__(PB_THREADS) void sr_partial_kernel(const float* __restrict__ score, const void* __restrict__ labels, int h, int w, int H,
                                                                int W, int64_t pixels, int64_t total, float* __restrict__ ws) {
  const uint32_t stride = gridDim.x * PB_THREADS, first = blockIdx.x * PB_THREADS + threadIdx.x;
  float s_sm = 0.f, s_sp = 0.f;
  const uint32_t hw = (uint32_t)h * w;
  for (uint32_t i = first; i < (uint32_t)pixels; i += stride) {
    const uint32_t r = i % hw, y = r / w, x = r - y * w;
    const float v = score[i];
    if (y + 1 < (uint32_t)h) {
      const float d = score[i + w] - v;
      s_sm = fmaf(d, d, s_sm);
    }
    if (x + 1 < (uint32_t)w) {
      const float d = score[i + 1] - v;
      s_sm = fmaf(d, d, s_sm);
    }
  }
  if (labels) {
    const float sy = ac_scale(h, H), sx = ac_scale(w, W);
    const uint32_t HW = (uint32_t)H * W;
    for (uint32_t i = first; i < (uint32_t)total; i += stride) {
      if (ac_label<LB>(labels, i) != 1) continue;
      const int b = (int)(i / HW), r = (int)(i - (uint32_t)b * HW), Y = r / W, X = r - Y * W;
      const float s = upsampled(score + (int64_t)b * hw, w, tap_of(Y, sy, h), tap_of(X, sx, w));
      s_sp = fmaf(s, s, s_sp);
    }
  }
  loss_store_partial<PB_WS>(LossSums<2, 0>{{s_sm, s_sp}}, ws);
}

__global__ __launch_bounds__(PB_THREADS) void sr_finish_kernel(const float* __restrict__ ws, int G, float* __restrict__ losses,
                                                               float* __restrict__ stats) {
  loss_finish<PB_WS, 2, 0>(ws, G, [=](const LossSums<2, 0>& t) {
    losses[0] = 0.5f * t.f[0];
    stats[0] = t.f[0];
    losses[1] = sqrtf(t.f[1]);
    stats[1] = t.f[1];
  });
}

template <int LB>
__global__ __launch_bounds__(PB_THREADS) void sr_bwd_kernel(const float* __restrict__ score, const void* __restrict__ labels, int h, int w, int H, int W,
                                                            int64_t pixels, const float* __restrict__ stats, const float* __restrict__ grad_smooth,
                                                            const float* __restrict__ grad_sparse, float* __restrict__ grad_score) {
  const int64_t i = (int64_t)blockIdx.x * PB_THREADS + threadIdx.x;
  if (i >= pixels) return;
  const int hw = h * w, b = (int)(i / hw), r = (int)(i - (int64_t)b * hw), y = r / w, x = r - y * w;
  const float g_sm = grad_smooth ? *grad_smooth : 0.f, g_sp = grad_sparse ? *grad_sparse : 0.f;
  const float* plane = score + (int64_t)b * hw;
  // d / d s[y,x] of 1/2 sum of squared forward differences: each difference this pixel ends, minus each it starts
  const float v = plane[r];
  float st = 0.f;
  if (y > 0) st += v - plane[r - w];
  if (y < h - 1) st -= plane[r + w] - v;
  if (x > 0) st += v - plane[r - 1];
  if (x < w - 1) st -= plane[r + 1] - v;
  float acc = g_sm * st;
  const float norm = sqrtf(stats[1]);
  if (labels && norm > 0.f && g_sp != 0.f) {                // torch.norm's backward: 0 where the norm is 0
    const float f = g_sp / norm;
    float sp = 0.f;
    ac_visit_naming(b, y, x, h, w, H, W, [&](const AcTap& ty, const AcTap& tx, float wgt, int64_t P) {
      if (ac_label<LB>(labels, P) == 1) sp += wgt * upsampled(plane, w, ty, tx);
    });
    acc = fmaf(f, sp, acc);
  }
  grad_score[i] = acc;
}

bool sr_shape_ok(int B, int h, int w, int H, int W) {
  return B >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)B * h * w <= 0x7fffffffLL &&
         (int64_t)H * W <= 0x7fffffffLL && (int64_t)h * w <= 0x7fffffffLL;
}

int64_t sr_span(int B, int h, int w, int H, int W) {
  const int64_t a = (int64_t)B * h * w, b = (int64_t)B * H * W;
  return a > b ? a : b;
}

}  // namespace

extern "C" int rba_gambler_loss_workspace_f32(int B, int H, int W, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL);
  *bytes = (int64_t)loss_groups((int64_t)B * H * W, 1) * PB_WS * (int64_t)sizeof(float);
  return 0;
}

// the launchers' switch: K + 1 <= 20 | K + 1 <= 32 channels, labels of 1 | 8 bytes -- no run-time selection inside the kernels
#define GM_DISPATCH(LAUNCH)                \
  do {                                     \
    if (K + 1 <= 20) {                     \
      if (label_bytes == 1) LAUNCH(20, 1); \
      else LAUNCH(20, 8);                  \
    } else {                               \
      if (label_bytes == 1) LAUNCH(32, 1); \
      else LAUNCH(32, 8);                  \
    }                                      \
  } while (0)

extern "C" int rba_gambler_loss_fwd_f32(const float* sem, const void* labels, int label_bytes, int B, int K, int h, int w, int H, int W, float ood_reg,
                                        float* workspace, float* reward, float* losses, float* stats, float* R, void* stream) {
  RBA_CHECK_ARG(gm_shape_ok(B, K, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(sem && labels && workspace && reward && losses && stats && R && reward != R && (((uintptr_t)workspace) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * H * W;
  const int G = loss_groups(total, 1);
  if (K + 1 <= 20) hipLaunchKernelGGL(gm_reward_kernel<20>, dim3(G), dim3(PB_THREADS), 0, st, sem, K, h, w, H, W, total, reward);
  else hipLaunchKernelGGL(gm_reward_kernel<32>, dim3(G), dim3(PB_THREADS), 0, st, sem, K, h, w, H, W, total, reward);
  if (const int e = rba_launch_status()) return e;
  rba_blur_planes_launch(false, reward, R, B, H, W, GM_BLUR_K, GM_BLUR_SIGMA, st);
  if (const int e = rba_launch_status()) return e;
#define GM_PARTIAL(KM, LB) \
  hipLaunchKernelGGL((gm_partial_kernel<KM, LB>), dim3(G), dim3(PB_THREADS), 0, st, sem, labels, R, K, h, w, H, W, total, workspace)
  GM_DISPATCH(GM_PARTIAL);
#undef GM_PARTIAL
  if (const int e = rba_launch_status()) return e;
  hipLaunchKernelGGL(gm_finish_kernel, dim3(1), dim3(PB_THREADS), 0, st, workspace, G, K, ood_reg, losses, stats);
  return rba_launch_status();
}

extern "C" int rba_gambler_loss_bwd_f32(const float* sem, const void* labels, int label_bytes, const float* R, int B, int K, int h, int w, int H, int W,
                                        float ood_reg, const float* stats, const float* grad_loss, float* grad_R, float* grad_reward,
                                        float* grad_sem, void* stream) {
  RBA_CHECK_ARG(gm_shape_ok(B, K, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(sem && labels && R && stats && grad_loss && grad_R && grad_reward && grad_sem && grad_R != grad_reward);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * H * W, pixels = (int64_t)B * h * w;
  const int G = loss_groups(total, 1);
#define GM_DR(KM, LB)                                                                                                                          \
  hipLaunchKernelGGL((gm_dR_kernel<KM, LB>), dim3(G), dim3(PB_THREADS), 0, st, sem, labels, R, K, h, w, H, W, total, ood_reg, stats, grad_loss, \
                     grad_R)
  GM_DISPATCH(GM_DR);
#undef GM_DR
  if (const int e = rba_launch_status()) return e;
  rba_blur_planes_launch(true, grad_R, grad_reward, B, H, W, GM_BLUR_K, GM_BLUR_SIGMA, st);
  if (const int e = rba_launch_status()) return e;
  const unsigned grid = (unsigned)((pixels + PB_OWNERS - 1) / PB_OWNERS);
#define GM_BWD(KM, LB)                                                                                                                           \
  hipLaunchKernelGGL((gm_bwd_kernel<KM, LB>), dim3(grid), dim3(PB_THREADS), 0, st, sem, labels, R, grad_reward, K, h, w, H, W, pixels, ood_reg, \
                     stats, grad_loss, grad_sem)
  GM_DISPATCH(GM_BWD);
#undef GM_BWD
  return rba_launch_status();
}

extern "C" int rba_score_reg_workspace_f32(int B, int h, int w, int H, int W, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && sr_shape_ok(B, h, w, H, W));
  *bytes = (int64_t)loss_groups(sr_span(B, h, w, H, W), 1) * PB_WS * (int64_t)sizeof(float);
  return 0;
}

extern "C" int rba_score_reg_fwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, float* workspace,
                                     float* losses, float* stats, void* stream) {
  RBA_CHECK_ARG(sr_shape_ok(B, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(score && workspace && losses && stats && (((uintptr_t)workspace) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t pixels = (int64_t)B * h * w, total = (int64_t)B * H * W;
  const int G = loss_groups(sr_span(B, h, w, H, W), 1);
  if (label_bytes == 1)
    hipLaunchKernelGGL(sr_partial_kernel<1>, dim3(G), dim3(PB_THREADS), 0, st, score, labels, h, w, H, W, pixels, total, workspace);
  else hipLaunchKernelGGL(sr_partial_kernel<8>, dim3(G), dim3(PB_THREADS), 0, st, score, labels, h, w, H, W, pixels, total, workspace);
  if (const int e = rba_launch_status()) return e;
  hipLaunchKernelGGL(sr_finish_kernel, dim3(1), dim3(PB_THREADS), 0, st, workspace, G, losses, stats);
  return rba_launch_status();
}

extern "C" int rba_score_reg_bwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, const float* stats,
                                     const float* grad_smooth, const float* grad_sparse, float* grad_score, void* stream) {
  RBA_CHECK_ARG(sr_shape_ok(B, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(score && stats && grad_score && (grad_smooth || grad_sparse));
  rba_begin();
  const int64_t pixels = (int64_t)B * h * w;
  const dim3 grid((unsigned)((pixels + PB_THREADS - 1) / PB_THREADS));
  if (label_bytes == 1)
    hipLaunchKernelGGL(sr_bwd_kernel<1>, grid, dim3(PB_THREADS), 0, (hipStream_t)stream, score, labels, h, w, H, W, pixels, stats, grad_smooth,
                       grad_sparse, grad_score);
  else
    hipLaunchKernelGGL(sr_bwd_kernel<8>, grid, dim3(PB_THREADS), 0, (hipStream_t)stream, score, labels, h, w, H, W, pixels, stats, grad_smooth,
                       grad_sparse, grad_score);
  return rba_launch_status();
}
