// K10 -- SetCriterion.densehybrid_loss behind its class map (reference: mask2former/modeling/criterion.py:406-431): the align_corners=True bilinear
// upsample of the K-channel class map sem [B,K,h,w] and of the two-channel ood_pred [B,2,h,w] to the labels' [B,H,W], log_softmax / logsumexp over
// the channels, get_batch_avg's global mean, the two nll_loss means -- and all of it backward.  The upsampled maps never exist: every label pixel
// samples its K + 2 values out of the quarter-resolution maps.  fp32, wave64, no MFMA, no scratch.  docs/kernels/K10.md.
//
// Per label pixel P (taps and weights: bilinear_ac.h):  x_k = sample of sem[b,k], o_c = sample of ood[b,c], L = logsumexp_k x_k.
//   label < K: class;  254: outlier;  anything else: ignored by the segmentation term (the reference maps 254 and 255 to ignore_index)
//   S_seg = sum_{label<K} (L - x_label), n_seg      S_ood = sum_{label=254} L, n_ood
//   S_th  = sum_all (logsumexp_c o_c - o_[label=254])   (void pixels are target 0, as in the reference)      S_x = sum_all sum_k x_k
//   m = S_x / (B K H W)  (get_batch_avg: detached)   loss_seg = S_seg / n_seg   loss_ood = S_ood / n_ood - m   loss_th = S_th / (B H W)
//   loss = loss_seg + beta loss_ood + 10 beta loss_th                       n_seg == 0 or n_ood == 0: NaN, the mean of nothing, as in the reference
//
// (a) dh_partial_kernel + dh_finish_kernel: the partial / finish scheme of loss_reduce.h, four sums and two counts, one pixel to a thread before the
//     cap; L goes to the [B,H,W] map `lse` for the backward.  The finish forms losses [4] and stats [8] on the device.
// (b) dh_bwd_kernel, gather form: the 16-lane walk of bilinear_ac.h (AcOwner) -- 16 lanes own one quarter-resolution pixel (b, y, x) of all K + 2
//     channels and split the rectangle of label pixels whose taps name it.  For each candidate they recompute its samples with the forward's
//     functions, p_k = exp(x_k - L) from the saved L, and add weight * d loss / d x_k; ac_split_sum, plain stores.  A pixel nobody samples gets 0.
#include "bilinear_ac.h"
#include "loss_reduce.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int DH_THREADS = LOSS_THREADS, DH_WS = 8;                 // workspace words per workgroup: S_seg S_ood S_th S_x n_seg n_ood - -
constexpr int DH_OWNERS = DH_THREADS / AC_SPLIT;                    // backward: owner pixels per workgroup
constexpr int DH_OUTLIER = 254;

template <int KMAX, int LB>
__global__ __launch_bounds__(DH_THREADS) void dh_partial_kernel(const float* __restrict__ sem, const float* __restrict__ ood,
                                                                const void* __restrict__ labels, int K, int h, int w, int H, int W, int64_t total,
                                                                float* __restrict__ ws, float* __restrict__ lse) {
  const float sy = ac_scale(h, H), sx = ac_scale(w, W);
  const int hw = h * w;
  const uint32_t HW = (uint32_t)H * W, stride = gridDim.x * DH_THREADS, end = (uint32_t)total;    // B H W < 2^31: i + stride stays below 2^32
  LossSums<4, 2> a{};                                     // f: S_seg, S_ood, S_th, S_x; n: n_seg, n_ood
  for (uint32_t i = blockIdx.x * DH_THREADS + threadIdx.x; i < end; i += stride) {
    const int lab = ac_label<LB>(labels, i);
    const int b = (int)(i / HW), r = (int)(i - (uint32_t)b * HW), Y = r / W, X = r - Y * W;
    const AcTaps4 t = ac_taps4(tap_of(Y, sy, h), tap_of(X, sx, w), w);
    const float* sp = sem + (int64_t)b * K * hw;
    float x[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) x[k] = ac_sample(sp + (int64_t)k * hw, t);
    float mx = x[0], sum_x = 0.f, x_lab = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        mx = fmaxf(mx, x[k]);
        sum_x += x[k];
        x_lab = k == lab ? x[k] : x_lab;
      }
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) e += expf(x[k] - mx);
    const float L = mx + logf(e);
    lse[i] = L;
    a.f[3] += sum_x;
    if (lab < K) {
      a.f[0] += L - x_lab;
      ++a.n[0];
    } else if (lab == DH_OUTLIER) {
      a.f[1] += L;
      ++a.n[1];
    }
    const float* op = ood + (int64_t)b * 2 * hw;
    const float o0 = ac_sample(op, t), o1 = ac_sample(op + hw, t), om = fmaxf(o0, o1);
    a.f[2] += om + logf(expf(o0 - om) + expf(o1 - om)) - (lab == DH_OUTLIER ? o1 : o0);
  }
  loss_store_partial<DH_WS>(a, ws);
}

__global__ __launch_bounds__(DH_THREADS) void dh_finish_kernel(const float* __restrict__ ws, int G, int64_t total, int K, float beta,
                                                               float* __restrict__ losses, float* __restrict__ stats) {
  loss_finish<DH_WS, 4, 2>(ws, G, [=](const LossSums<4, 2>& t) {
    const float S_seg = t.f[0], S_ood = t.f[1], S_th = t.f[2], S_x = t.f[3];
    const float N_seg = (float)t.n[0], N_ood = (float)t.n[1], N = (float)total;
    const float m = S_x / (N * (float)K);
    const float loss_seg = S_seg / N_seg;                 // 0 / 0 = NaN, the mean of nothing
    const float loss_ood = S_ood / N_ood - m;
    const float loss_th = S_th / N;
    losses[0] = loss_seg + beta * loss_ood + 10.0f * beta * loss_th;
    losses[1] = loss_seg;
    losses[2] = loss_ood;
    losses[3] = loss_th;
    stats[0] = S_seg, stats[1] = S_ood, stats[2] = S_th, stats[3] = S_x;
    stats[4] = N_seg, stats[5] = N_ood, stats[6] = N, stats[7] = m;
  });
}

template <int KMAX, int LB>
__global__ __launch_bounds__(DH_THREADS) void dh_bwd_kernel(const float* __restrict__ sem, const float* __restrict__ ood,
                                                            const void* __restrict__ labels, const float* __restrict__ lse, int K, int h, int w, int H,
                                                            int W, int64_t pixels, float beta, const float* __restrict__ stats,
                                                            const float* __restrict__ grad_loss, float* __restrict__ grad_sem,
                                                            float* __restrict__ grad_ood) {
  const AcOwner o = ac_owner(DH_OWNERS, pixels, h, w, H, W);
  const int hw = h * w;
  const float g = *grad_loss;
  // d loss / d (a pixel's term): the means' 1 / n
  const float c_seg = g / stats[4], c_ood = g * beta / stats[5], c_th = g * 10.0f * beta / stats[6];
  const float* sp = sem + (int64_t)o.b * K * hw;
  const float* op = ood + (int64_t)o.b * 2 * hw;
  float acc[KMAX], a0 = 0.f, a1 = 0.f;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
  for (uint32_t c = o.sub; c < o.n; c += AC_SPLIT) {
    const AcCandidate q = ac_candidate(o, c);
    const int lab = ac_label<LB>(labels, q.P);
    const bool out = lab == DH_OUTLIER;
    const float o0 = ac_sample(op, q.t), o1 = ac_sample(op + hw, q.t), om = fmaxf(o0, o1);
    const float e0 = expf(o0 - om), e1 = expf(o1 - om), es = e0 + e1;
    a0 = fmaf(q.wgt, e0 / es - (out ? 0.f : 1.0f), a0);
    a1 = fmaf(q.wgt, e1 / es - (out ? 1.0f : 0.f), a1);
    if (lab < K || out) {
      const float cw = q.wgt * (out ? c_ood : c_seg), L = lse[q.P];
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc[k] = fmaf(cw, expf(ac_sample(sp + (int64_t)k * hw, q.t) - L) - (k == lab ? 1.0f : 0.f), acc[k]);
    }
  }
  a0 = ac_split_sum(a0);
  a1 = ac_split_sum(a1);
#pragma unroll
  for (int k = 0; k < KMAX; ++k)
    if (k < K) acc[k] = ac_split_sum(acc[k]);
  if (o.live && o.sub == 0) {
    float* gs = grad_sem + (int64_t)o.b * K * hw + o.r;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) gs[(int64_t)k * hw] = acc[k];
    float* go = grad_ood + (int64_t)o.b * 2 * hw + o.r;
    go[0] = c_th * a0;
    go[hw] = c_th * a1;
  }
}

bool dh_shape_ok(int B, int K, int h, int w, int H, int W) {
  return B >= 1 && K >= 1 && K <= 32 && h >= 1 && w >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL &&
         (int64_t)B * K * h * w <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL && (int64_t)h * w <= 0x7fffffffLL;
}

}  // namespace

extern "C" int rba_dense_hybrid_loss_workspace_f32(int B, int H, int W, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && B >= 1 && H >= 1 && W >= 1 && (int64_t)B * H * W <= 0x7fffffffLL && (int64_t)H * W <= 0x7fffffffLL);
  *bytes = (int64_t)loss_groups((int64_t)B * H * W, 1) * DH_WS * (int64_t)sizeof(float);
  return 0;
}

// the launchers' switch: K <= 20 | K <= 32, labels of 1 | 8 bytes -- no run-time selection inside the kernels
#define DH_DISPATCH(LAUNCH)              \
  do {                                   \
    if (K <= 20) {                       \
      if (label_bytes == 1) LAUNCH(20, 1); \
      else LAUNCH(20, 8);                \
    } else {                             \
      if (label_bytes == 1) LAUNCH(32, 1); \
      else LAUNCH(32, 8);                \
    }                                    \
  } while (0)

extern "C" int rba_dense_hybrid_loss_fwd_f32(const float* sem, const float* ood, const void* labels, int label_bytes, int B, int K, int h, int w,
                                             int H, int W, float beta, float* workspace, float* losses, float* stats, float* lse, void* stream) {
  RBA_CHECK_ARG(dh_shape_ok(B, K, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(sem && ood && labels && workspace && losses && stats && lse && (((uintptr_t)workspace) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t total = (int64_t)B * H * W;
  const int G = loss_groups(total, 1);
#define DH_PARTIAL(KM, LB) \
  hipLaunchKernelGGL((dh_partial_kernel<KM, LB>), dim3(G), dim3(DH_THREADS), 0, st, sem, ood, labels, K, h, w, H, W, total, workspace, lse)
  DH_DISPATCH(DH_PARTIAL);
#undef DH_PARTIAL
  if (const int e = rba_launch_status()) return e;
  hipLaunchKernelGGL(dh_finish_kernel, dim3(1), dim3(DH_THREADS), 0, st, workspace, G, total, K, beta, losses, stats);
  return rba_launch_status();
}

extern "C" int rba_dense_hybrid_loss_bwd_f32(const float* sem, const float* ood, const void* labels, int label_bytes, const float* lse, int B, int K,
                                             int h, int w, int H, int W, float beta, const float* stats, const float* grad_loss, float* grad_sem,
                                             float* grad_ood, void* stream) {
  RBA_CHECK_ARG(dh_shape_ok(B, K, h, w, H, W) && (label_bytes == 1 || label_bytes == 8));
  RBA_CHECK_ARG(sem && ood && labels && lse && stats && grad_loss && grad_sem && grad_ood);
  rba_begin();
  const int64_t pixels = (int64_t)B * h * w;
  const unsigned grid = (unsigned)((pixels + DH_OWNERS - 1) / DH_OWNERS);
#define DH_BWD(KM, LB)                                                                                                                              \
  hipLaunchKernelGGL((dh_bwd_kernel<KM, LB>), dim3(grid), dim3(DH_THREADS), 0, (hipStream_t)stream, sem, ood, labels, lse, K, h, w, H, W, pixels, beta, \
                     stats, grad_loss, grad_sem, grad_ood)
  DH_DISPATCH(DH_BWD);
#undef DH_BWD
  return rba_launch_status();
}
