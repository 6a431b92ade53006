// K11 -- the PEBAL fine-tune recipe's three losses behind K1 (reference: mask2former/modeling/criterion.py:245-388): SetCriterion.gambler_loss behind
// its (K+1)-channel class map (K11a), and smoothness_loss / sparsity_loss behind their score map (K11b) -- forward and backward.  No up-sampled
// map exists in either direction: every label pixel samples its values out of the quarter-resolution map (K10's walk, bilinear_ac.h's taps).
// fp32, wave64, no MFMA, no scratch, no float atomics, nothing read back.  docs/kernels/K11.md.
//
// K11a, per label pixel P:  x_k = sample of sem[b,k] (k < K: the classes, k = K: the reservation channel),
//   L_in = logsumexp_{k<K} x_k,  L = logsumexp_{k<=K} x_k,  p_k = exp(x_k - L),  reward r(P) = L_in^2,  R = blur_{7, sigma 1}(r) per image plane
//   (torchvision's GaussianBlur as gaussian_blur.hip restates it),  res = p_K / R
//   label < K: t_in = log(p_label + res) (no clamp);   label 254: t_out = sum_{k<K} log(max(p_k + res, 1e-7));   anything else: void
//   loss = -(S_in / n_in + [n_ood > 0] ood_reg S_out / (n_ood K))                        n_in == 0: NaN, the mean of nothing, as in the reference
// forward:  (a) gm_reward_kernel: r;  (b) blur_planes_kernel: R;  (c) gm_partial_kernel + gm_finish_kernel: K10's partial / finish scheme.
// backward: (a) gm_dR_kernel: dR(P) = -(p_K / R^2) c sum 1 / (p_k + res) over P's live terms (a clamped term: 0; equality passes, as torch.clamp),
//           c = -g / n_in | -g ood_reg / (n_ood K);  (b) blur_planes_adjoint_kernel: dr = A^T dR, the adjoint of the reflect-padded blur;
//           (c) gm_bwd_kernel, K10's gather form: 16 lanes own one quarter-resolution pixel of all K + 1 channels, split the exact rectangle of
//           label pixels whose taps name it, recompute samples, L, L_in and the terms, and add
//           weight [d (direct softmax terms) / d x_k + dr(P) 2 L_in exp(x_k - L_in) [k < K]]; a fixed xor tree, plain stores.
//
// K11b:  smoothness = 1/2 (sum_{y<h-1} (s[y+1,x] - s[y,x])^2 + sum_{x<w-1} (s[y,x+1] - s[y,x])^2)   (a sum; the last row / column add 0)
//        sparsity   = sqrt(sum_{label=1} up(s)^2), up = the align_corners=True upsample to the labels' size; 0 without labels or outlier pixel
// sr_partial_kernel / sr_finish_kernel: K9's scheme;  sr_bwd_kernel: one thread per score pixel, the four-neighbour stencil of the differences
// plus K9's gather walk of w up(s)(P) / norm; 0 where the norm is 0 (torch.norm's backward).
#include "bilinear_ac.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int PB_THREADS = 256, PB_MAX_GROUPS = 2048, PB_WS = 4;    // workspace words per workgroup: two sums, two integer counts
constexpr int PB_SPLIT = 16, PB_OWNERS = PB_THREADS / PB_SPLIT;     // gather backward: lanes per owner pixel, owner pixels per workgroup
constexpr int GM_OUTLIER = 254;
constexpr int GM_BLUR_K = 7;
constexpr float GM_BLUR_SIGMA = 1.0f, GM_CLAMP = 1e-7f;

// K9's label convention: is this an outlier pixel (label 1)
template <int LB>
__device__ __forceinline__ bool sr_outlier(const void* __restrict__ labels, int64_t i) {
  if constexpr (LB == 1) return reinterpret_cast<const uint8_t*>(labels)[i] == 1;
  else return reinterpret_cast<const int64_t*>(labels)[i] == 1;
}

int pb_groups(int64_t total) {
  const int64_t g = (total + PB_THREADS - 1) / PB_THREADS;
  return (int)(g < PB_MAX_GROUPS ? g : PB_MAX_GROUPS);
}

// two float sums and two integer counts of a workgroup's 256 threads -> threads 0 .. 3 hold one each (the counts as bit patterns)
__device__ __forceinline__ float pb_block_reduce(float s0, float s1, int n0, int n1, float (*red)[4]) {
  const int tid = threadIdx.x;
  s0 = wave_reduce_sum(s0);
  s1 = wave_reduce_sum(s1);
  n0 = wave_reduce_sum_int(n0);
  n1 = wave_reduce_sum_int(n1);
  if ((tid & 63) == 0) {
    float* r = red[tid >> 6];
    r[0] = s0, r[1] = s1, r[2] = __int_as_float(n0), r[3] = __int_as_float(n1);
  }
  __syncthreads();
  float out = 0.f;
  if (tid < 2) out = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  else if (tid < 4)
    out = __int_as_float((__float_as_int(red[0][tid]) + __float_as_int(red[1][tid])) + (__float_as_int(red[2][tid]) + __float_as_int(red[3][tid])));
  return out;
}

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

// forward (c): the terms against the blurred reward R; workspace [G][4] = (S_in, S_out, n_in, n_ood)
template <int KMAX, int LB>
__global__ __launch_bounds__(PB_THREADS) void gm_partial_kernel(const float* __restrict__ sem, const void* __restrict__ labels,
                                                                const float* __restrict__ R, int K, int h, int w, int H, int W, int64_t total,
                                                                float* __restrict__ ws) {
  __shared__ float red[PB_THREADS / 64][4];
  const int tid = threadIdx.x;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int hw = h * w;
  const uint32_t HW = (uint32_t)H * W, stride = gridDim.x * PB_THREADS, end = (uint32_t)total;
  float s_in = 0.f, s_out = 0.f;
  int n_in = 0, n_ood = 0;
  for (uint32_t i = blockIdx.x * PB_THREADS + tid; i < end; i += stride) {
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
      s_in += logf(e_lab * f + res);
      ++n_in;
    } else {
      float t_out = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) t_out += logf(fmaxf(x[k] * f + res, GM_CLAMP));
      s_out += t_out;
      ++n_ood;
    }
  }
  const float v = pb_block_reduce(s_in, s_out, n_in, n_ood, red);
  if (tid < 4) ws[PB_WS * (int64_t)blockIdx.x + tid] = v;
}

// thread t takes the partials t, t + 256, ... in ascending order, then the same fixed tree
__global__ __launch_bounds__(PB_THREADS) void gm_finish_kernel(const float* __restrict__ ws, int G, int K, float ood_reg, float* __restrict__ losses,
                                                               float* __restrict__ stats) {
  __shared__ float red[PB_THREADS / 64][4];
  __shared__ float fin[4];
  const int tid = threadIdx.x;
  float s_in = 0.f, s_out = 0.f;
  int n_in = 0, n_ood = 0;
  for (int g = tid; g < G; g += PB_THREADS) {
    const float* p = ws + PB_WS * (int64_t)g;
    s_in += p[0];
    s_out += p[1];
    n_in += __float_as_int(p[2]);
    n_ood += __float_as_int(p[3]);
  }
  const float v = pb_block_reduce(s_in, s_out, n_in, n_ood, red);
  if (tid < 4) fin[tid] = v;
  __syncthreads();
  if (tid == 0) {
    const int Nood = __float_as_int(fin[3]);
    const float N_in = (float)__float_as_int(fin[2]), N_ood = (float)Nood;
    const float in_mean = fin[0] / N_in;                                  // 0 / 0 = NaN, the mean of nothing
    const float out_mean = Nood > 0 ? fin[1] / (N_ood * (float)K) : 0.f;  // the reference's `ood_mask.sum() > 0`, decided here
    losses[0] = -(in_mean + ood_reg * out_mean);
    losses[1] = in_mean;
    losses[2] = out_mean;
    stats[0] = fin[0], stats[1] = fin[1], stats[2] = N_in, stats[3] = N_ood;
  }
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
  const int sub = threadIdx.x & (PB_SPLIT - 1);
  const int64_t owner = (int64_t)blockIdx.x * PB_OWNERS + (threadIdx.x >> 4);
  const bool live = owner < pixels;
  const int64_t i = live ? owner : pixels - 1;            // a group past the end walks nothing and stores nothing, but takes part in the shuffles
  const int hw = h * w, b = (int)(i / hw), r = (int)(i - (int64_t)b * hw), y = r / w, x0 = r - y * w;
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  float c_in, c_out;
  gm_factors(stats, grad_loss, K, ood_reg, c_in, c_out);
  int Y0, Y1, X0, X1;
  ac_naming(y, sy, h, H, Y0, Y1);
  ac_naming(x0, sx, w, W, X0, X1);
  const uint32_t nX = X1 >= X0 ? X1 - X0 + 1 : 0;
  const uint32_t n = live && Y1 >= Y0 ? (uint32_t)(Y1 - Y0 + 1) * nX : 0;      // <= H W < 2^31: c + 16 stays below 2^32
  const float* sp = sem + (int64_t)b * (K + 1) * hw;
  float acc[KMAX], accR = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
  for (uint32_t c = sub; c < n; c += PB_SPLIT) {
    const uint32_t dy = c / nX;
    const int Y = Y0 + (int)dy, X = X0 + (int)(c - dy * nX);
    const AcTap ty = tap_of(Y, sy, h), tx = tap_of(X, sx, w);
    const float wgt = tap_weight(ty, y) * tap_weight(tx, x0);
    const AcTaps4 t = ac_taps4(ty, tx, w);
    const int64_t P = ((int64_t)b * H + Y) * W + X;
    const int lab = ac_label<LB>(labels, P);
    float e[KMAX], mx_in, sum_in, L_in;
    gm_samples<KMAX>(sp, hw, t, K, e);
    gm_inlier<KMAX>(e, K, mx_in, sum_in, L_in);
    // through the reward: dr(P) d (L_in^2) / d x_k = dr(P) 2 L_in e_k / sum_in, every pixel (the blur spreads a term's gradient to its neighbours)
    const float tr = wgt * (dr[P] * 2.0f * L_in / sum_in);
    if (lab < K || lab == GM_OUTLIER) {
      float f, pK;
      gm_all(mx_in, sum_in, ac_sample(sp + (int64_t)K * hw, t), f, pK);
      const float Rv = R[P], res = pK / Rv;
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
          acc[k] += wgt * (p * (u - D)) + tr * e[k];
        }
      accR = fmaf(wgt, pK * (qK - D), accR);
    } else {
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc[k] = fmaf(tr, e[k], acc[k]);
    }
  }
  // the 16 lanes of an owner, a fixed xor tree (every lane of the wave is here)
#pragma unroll
  for (int o = PB_SPLIT / 2; o > 0; o >>= 1) {
    accR += __shfl_xor(accR, o, RBA_WAVE);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) acc[k] += __shfl_xor(acc[k], o, RBA_WAVE);
  }
  if (live && sub == 0) {
    float* gs = grad_sem + (int64_t)b * (K + 1) * hw + r;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) gs[(int64_t)k * hw] = acc[k];
    gs[(int64_t)K * hw] = accR;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the blur of B planes and its adjoint
constexpr int BL_TX = 64, BL_TY = 4, BL_KMAX = 15;

__device__ __forceinline__ int bl_reflect(int i, int n) {            // torch "reflect": -1 -> 1, n -> n - 2  (gaussian_blur.hip)
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return i < 0 ? 0 : i;                                              // beyond n - 1 + pad: only read by threads outside the image
}

// torchvision's 1-D kernel: exp(-0.5 (x / sigma)^2) on linspace(-(k-1)/2, (k-1)/2, k), normalised to 1 (gaussian_blur.hip's arithmetic)
__device__ __forceinline__ void bl_weights(float* w1, int k, float sigma, int tid) {
  if (tid < k) {
    const float half = (k - 1) * 0.5f;
    float s = 0.f;
    for (int i = 0; i < k; ++i) { const float t = (-half + i) / sigma; s += expf(-0.5f * t * t); }
    const float t = (-half + tid) / sigma;
    w1[tid] = expf(-0.5f * t * t) / s;
  }
}

// gaussian_blur.hip's kernel with the plane on blockIdx.z: the same staging, weights and summation order, so one plane gives its bits
__global__ __launch_bounds__(BL_TX * BL_TY) void blur_planes_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int k,
                                                                    float sigma) {
  __shared__ float tile[BL_TY + BL_KMAX - 1][BL_TX + BL_KMAX - 1];
  __shared__ float w1[BL_KMAX];
  const int r = k >> 1, tw = BL_TX + k - 1, th = BL_TY + k - 1;
  const int x0 = blockIdx.x * BL_TX, y0 = blockIdx.y * BL_TY;
  const int tid = threadIdx.y * BL_TX + threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * H * W;
  bl_weights(w1, k, sigma, tid);
  for (int i = tid; i < tw * th; i += BL_TX * BL_TY) {
    const int ty = i / tw, tx = i - ty * tw;
    tile[ty][tx] = in[plane + (int64_t)bl_reflect(y0 + ty - r, H) * W + bl_reflect(x0 + tx - r, W)];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  float acc = 0.f;
  for (int dy = 0; dy < k; ++dy) {
    const float wy = w1[dy];
    for (int dx = 0; dx < k; ++dx) acc = fmaf(tile[threadIdx.y + dy][threadIdx.x + dx], wy * w1[dx], acc);
  }
  out[plane + (int64_t)y * W + x] = acc;
}

// The coefficient of (d out)[q] in (d in)[p] along one axis of length n.  out[q] = sum_d w[d + r] in[reflect(q + d)], so in[p] is read through
// every virtual position v that reflects onto p: v = p, v = -p (p >= 1) and v = 2 (n - 1) - p (p <= n - 2), each by the q with |v - q| <= r.
// Within r of a border the folded-back taps add; every contributing q lies in [p - r, p + r].
__device__ __forceinline__ float bl_adjoint_coef(int p, int q, int n, const float* w1, int r) {
  float c = 0.f;
  int d = p - q;
  if (d >= -r && d <= r) c += w1[d + r];
  d = -p - q;
  if (p >= 1 && d >= -r) c += w1[d + r];
  d = 2 * (n - 1) - p - q;
  if (p <= n - 2 && d <= r) c += w1[d + r];
  return c;
}

// din = A^T dout in gather form, separably: a source pixel (y, x) collects dout over [y - r, y + r] x [x - r, x + r] (zero outside the plane) with
// the outer product of the two axes' adjoint coefficients.  The tile and its halo are staged in LDS as the forward's.
__global__ __launch_bounds__(BL_TX * BL_TY) void blur_planes_adjoint_kernel(const float* __restrict__ dout, float* __restrict__ din, int H, int W,
                                                                            int k, float sigma) {
  __shared__ float tile[BL_TY + BL_KMAX - 1][BL_TX + BL_KMAX - 1];
  __shared__ float w1[BL_KMAX];
  const int r = k >> 1, tw = BL_TX + k - 1, th = BL_TY + k - 1;
  const int x0 = blockIdx.x * BL_TX, y0 = blockIdx.y * BL_TY;
  const int tid = threadIdx.y * BL_TX + threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * H * W;
  bl_weights(w1, k, sigma, tid);
  for (int i = tid; i < tw * th; i += BL_TX * BL_TY) {
    const int ty = i / tw, tx = i - ty * tw, Y = y0 + ty - r, X = x0 + tx - r;
    tile[ty][tx] = Y >= 0 && Y < H && X >= 0 && X < W ? dout[plane + (int64_t)Y * W + X] : 0.f;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  float acc = 0.f;
  for (int dy = 0; dy < k; ++dy) {
    const int Y = y + dy - r;
    if (Y < 0 || Y >= H) continue;
    const float cy = bl_adjoint_coef(y, Y, H, w1, r);
    float row = 0.f;
    for (int dx = 0; dx < k; ++dx) {
      const int X = x + dx - r;
      if (X < 0 || X >= W) continue;
      row = fmaf(tile[threadIdx.y + dy][threadIdx.x + dx], bl_adjoint_coef(x, X, W, w1, r), row);
    }
    acc = fmaf(cy, row, acc);
  }
  din[plane + (int64_t)y * W + x] = acc;
}

bool bl_ok(int B, int H, int W, int k, float sigma) {
  return B >= 1 && B <= 65535 && k >= 1 && k <= BL_KMAX && (k & 1) && sigma > 0.f && H > k / 2 && W > k / 2 && (H + BL_TY - 1) / BL_TY <= 65535 &&
         (int64_t)B * H * W <= 0x7fffffffLL;
}

void bl_launch(bool adjoint, const float* in, float* out, int B, int H, int W, int k, float sigma, hipStream_t st) {
  const dim3 grid((W + BL_TX - 1) / BL_TX, (H + BL_TY - 1) / BL_TY, B), block(BL_TX, BL_TY);
  if (adjoint) hipLaunchKernelGGL(blur_planes_adjoint_kernel, grid, block, 0, st, in, out, H, W, k, sigma);
  else hipLaunchKernelGGL(blur_planes_kernel, grid, block, 0, st, in, out, H, W, k, sigma);
}

bool gm_shape_ok(int B, int K, int h, int w, int H, int W) {
  return K >= 1 && K + 1 <= 32 && h >= 1 && w >= 1 && bl_ok(B, H, W, GM_BLUR_K, GM_BLUR_SIGMA) && (int64_t)B * (K + 1) * h * w <= 0x7fffffffLL &&
         (int64_t)H * W <= 0x7fffffffLL && (int64_t)h * w <= 0x7fffffffLL;
}

// ---------------------------------------------------------------------------------------------------------------- K11b
// workspace [G][4] = (sum of squared differences, sum of squared outlier samples, -, -)
template <int LB>
__global__ __launch_bounds__(PB_THREADS) void sr_partial_kernel(const float* __restrict__ score, const void* __restrict__ labels, int h, int w, int H,
                                                                int W, int64_t pixels, int64_t total, float* __restrict__ ws) {
  __shared__ float red[PB_THREADS / 64][4];
  const int tid = threadIdx.x;
  const uint32_t stride = gridDim.x * PB_THREADS, first = blockIdx.x * PB_THREADS + tid;
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
      if (!sr_outlier<LB>(labels, i)) continue;
      const int b = (int)(i / HW), r = (int)(i - (uint32_t)b * HW), Y = r / W, X = r - Y * W;
      const float s = upsampled(score + (int64_t)b * hw, w, tap_of(Y, sy, h), tap_of(X, sx, w));
      s_sp = fmaf(s, s, s_sp);
    }
  }
  const float v = pb_block_reduce(s_sm, s_sp, 0, 0, red);
  if (tid < 2) ws[PB_WS * (int64_t)blockIdx.x + tid] = v;
}

__global__ __launch_bounds__(PB_THREADS) void sr_finish_kernel(const float* __restrict__ ws, int G, float* __restrict__ losses,
                                                               float* __restrict__ stats) {
  __shared__ float red[PB_THREADS / 64][4];
  const int tid = threadIdx.x;
  float s_sm = 0.f, s_sp = 0.f;
  for (int g = tid; g < G; g += PB_THREADS) {
    s_sm += ws[PB_WS * (int64_t)g];
    s_sp += ws[PB_WS * (int64_t)g + 1];
  }
  const float v = pb_block_reduce(s_sm, s_sp, 0, 0, red);
  if (tid == 0) {
    losses[0] = 0.5f * v;
    stats[0] = v;
  } else if (tid == 1) {
    losses[1] = sqrtf(v);
    stats[1] = v;
  }
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
    const float sy = ac_scale(h, H), sx = ac_scale(w, W), f = g_sp / norm;
    int Y0, Y1, X0, X1;
    candidates(y, sy, H, Y0, Y1);
    candidates(x, sx, W, X0, X1);
    float sp = 0.f;
    for (int Y = Y0; Y <= Y1; ++Y) {
      const AcTap ty = tap_of(Y, sy, h);
      if (ty.i0 != y && ty.i1 != y) continue;
      const float wy = tap_weight(ty, y);
      const int64_t row = ((int64_t)b * H + Y) * W;
      for (int X = X0; X <= X1; ++X) {
        const AcTap tx = tap_of(X, sx, w);
        if (tx.i0 != x && tx.i1 != x) continue;
        if (!sr_outlier<LB>(labels, row + X)) continue;
        sp += wy * tap_weight(tx, x) * upsampled(plane, w, ty, tx);
      }
    }
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

extern "C" int rba_gaussian_blur_planes_f32(const float* in, float* out, int B, int H, int W, int kernel_size, float sigma, void* stream) {
  RBA_CHECK_ARG(bl_ok(B, H, W, kernel_size, sigma) && in && out && in != out);       // reflect padding needs pad < size
  rba_begin();
  bl_launch(false, in, out, B, H, W, kernel_size, sigma, (hipStream_t)stream);
  return rba_launch_status();
}

extern "C" int rba_gaussian_blur_planes_adjoint_f32(const float* grad_out, float* grad_in, int B, int H, int W, int kernel_size, float sigma,
                                                    void* stream) {
  RBA_CHECK_ARG(bl_ok(B, H, W, kernel_size, sigma) && grad_out && grad_in && grad_out != grad_in);
  rba_begin();
  bl_launch(true, grad_out, grad_in, B, H, W, kernel_size, sigma, (hipStream_t)stream);
  return rba_launch_status();
}

extern "C" int rba_gambler_loss_workspace_f32(int B, int H, int W, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL);
  *bytes = (int64_t)pb_groups((int64_t)B * H * W) * PB_WS * (int64_t)sizeof(float);
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
  const int G = pb_groups(total);
  if (K + 1 <= 20) hipLaunchKernelGGL(gm_reward_kernel<20>, dim3(G), dim3(PB_THREADS), 0, st, sem, K, h, w, H, W, total, reward);
  else hipLaunchKernelGGL(gm_reward_kernel<32>, dim3(G), dim3(PB_THREADS), 0, st, sem, K, h, w, H, W, total, reward);
  if (const int e = rba_launch_status()) return e;
  bl_launch(false, reward, R, B, H, W, GM_BLUR_K, GM_BLUR_SIGMA, st);
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
  const int G = pb_groups(total);
#define GM_DR(KM, LB)                                                                                                                          \
  hipLaunchKernelGGL((gm_dR_kernel<KM, LB>), dim3(G), dim3(PB_THREADS), 0, st, sem, labels, R, K, h, w, H, W, total, ood_reg, stats, grad_loss, \
                     grad_R)
  GM_DISPATCH(GM_DR);
#undef GM_DR
  if (const int e = rba_launch_status()) return e;
  bl_launch(true, grad_R, grad_reward, B, H, W, GM_BLUR_K, GM_BLUR_SIGMA, st);
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
  *bytes = (int64_t)pb_groups(sr_span(B, h, w, H, W)) * PB_WS * (int64_t)sizeof(float);
  return 0;
}

extern "C" int rba_score_reg_fwd_f32(const float* score, const void* labels, int label_bytes, int B, int h, int w, int H, int W, float* workspace,
                                     float* losses, float* stats, void* stream) {
  RBA_CHECK_ARG(sr_shape_ok(B, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(score && workspace && losses && stats && (((uintptr_t)workspace) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t pixels = (int64_t)B * h * w, total = (int64_t)B * H * W;
  const int G = pb_groups(sr_span(B, h, w, H, W));
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
