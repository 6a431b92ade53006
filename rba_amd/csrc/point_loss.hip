// K8 -- the point-sampled mask losses and the matcher's cost (reference: SetCriterion.loss_masks, mask2former/modeling/criterion.py:194-243, and
// HungarianMatcher.memory_efficient_forward, mask2former/modeling/matcher.py:95-156).  One access pattern, three uses: a bilinear gather of
// mask planes at normalised points (Detectron2's point_sample = F.grid_sample(x, 2 c - 1, align_corners=False), zero padding) followed by a
// small reduction.  fp32, wave64, no MFMA, no scratch.
//
// Sampling rule (taps_of): pixel coordinates c_x w - 0.5, c_y h - 0.5; the four taps floor / floor + 1; a tap outside the plane contributes 0
// and is never read (its offset is the plane's first pixel and its load is predicated off).  Coordinates are finite floats, nothing else is
// assumed: the pixel coordinate is clamped to [-2, size + 1] before it is converted, which keeps every tap of such a point outside.
//
// (a) point_sample_kernel: one thread per (row, point), the row's plane through an optional index vector.
// (b) the loss: loss_sums_kernel = one workgroup of 1024 threads per matched mask, every thread a fixed set of points, a fixed shuffle / LDS tree:
//     the four sums of a mask (bce, sigma t, sigma, t) are bitwise reproducible; loss_finish_kernel = one workgroup that forms both scalar losses
//     from them in a fixed order (the workgroup tree of loss_reduce.h).  loss_bwd_kernel = one thread per (mask, point): it recomputes x and sigma, forms d loss / d x from the saved
//     sums and the two upstream gradients (device pointers) and adds its four tap contributions into the zero-filled gradient tensor with float
//     atomics.  Sizing (the recipe: 2 images x ~20 targets, P = 12544): 38 x 12544 x 4 taps x 4 B = 7.6 MB of added bytes as scattered single
//     dwords against a chip-wide rate of ~1.3 TB/s for WELL-SHAPED float atomics -- a floor of 6 us that scattered dwords will not reach -- beside
//     a 26 MB zero fill of [200,128,256].  The other reasonable form, one workgroup per matched plane summing in LDS, has the same arrival-order
//     sums (LDS float atomics of different waves) and needs a second form for planes beyond 160 KB; docs/kernels/K8.md has the numbers.
// (c) match_cost: pos t + neg (1 - t) = softplus(x) - x t, so the [Q,T] cost needs sum_p softplus(x_q), sum_p sigma(x_q), sum_p t_m and the two
//     contractions sum_p x_q t_m, sum_p sigma_q t_m.  A workgroup owns one slice of the points, 32 queries and 32 targets: per step of 64 points it
//     samples both tiles into LDS (a thread keeps ONE point per step: its geometry for both resolutions is computed once and serves 8 queries and
//     8 targets), then every thread sums 4 (q, t) pairs over the 64 points.  Per-slice partial sums go to the caller's workspace with plain
//     stores, cost_finish_kernel adds them in slice order: no float atomics, bitwise reproducible, nothing in the workspace has to start from a
//     known value.  Neither [Q,P] nor [T,P] goes to memory.
#include <math.h>
#include "common.h"
#include "loss_reduce.h"
#include "../../include/rba_hip.h"

namespace {

struct Taps {
  int o[4];        // offsets inside the plane: (y0,x0) (y0,x1) (y1,x0) (y1,x1); 0 where the tap is outside
  float w[4];      // bilinear weights (of every tap, inside or not)
  bool in[4];
};

__device__ __forceinline__ Taps taps_of(float cx, float cy, int h, int w) {
  float px = cx * (float)w - 0.5f, py = cy * (float)h - 0.5f;
  px = fminf(fmaxf(px, -2.0f), (float)w + 1.0f);
  py = fminf(fmaxf(py, -2.0f), (float)h + 1.0f);
  const float fx0 = floorf(px), fy0 = floorf(py);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = x0 + 1, y1 = y0 + 1;
  const float ax = px - fx0, ay = py - fy0;
  const bool xi0 = x0 >= 0 && x0 < w, xi1 = x1 >= 0 && x1 < w, yi0 = y0 >= 0 && y0 < h, yi1 = y1 >= 0 && y1 < h;
  Taps t;
  t.w[0] = (1.0f - ax) * (1.0f - ay);
  t.w[1] = ax * (1.0f - ay);
  t.w[2] = (1.0f - ax) * ay;
  t.w[3] = ax * ay;
  t.in[0] = xi0 && yi0;
  t.in[1] = xi1 && yi0;
  t.in[2] = xi0 && yi1;
  t.in[3] = xi1 && yi1;
  t.o[0] = t.in[0] ? y0 * w + x0 : 0;
  t.o[1] = t.in[1] ? y0 * w + x1 : 0;
  t.o[2] = t.in[2] ? y1 * w + x0 : 0;
  t.o[3] = t.in[3] ? y1 * w + x1 : 0;
  return t;
}

// grid_sample's order of the four products; a tap outside is 0 and not read
__device__ __forceinline__ float sample(const float* __restrict__ plane, const Taps& t) {
  float v = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) v += (t.in[i] ? plane[t.o[i]] : 0.f) * t.w[i];
  return v;
}

__device__ __forceinline__ float sigmoid_exact(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float softplus_stable(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// the plane of row n, or -1 when the index vector names none (the row then reads and writes nothing)
__device__ __forceinline__ int64_t plane_of(const int64_t* __restrict__ index, int n, int64_t planes) {
  const int64_t p = index ? index[n] : n;
  return p >= 0 && p < planes ? p : -1;
}

__global__ __launch_bounds__(256) void point_sample_kernel(const float* __restrict__ planes, const int64_t* __restrict__ index,
                                                           const float* __restrict__ coords, float* __restrict__ out, int64_t num_planes, int h,
                                                           int w, int P, int shared) {
  const int n = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int64_t pl = plane_of(index, n, num_planes);
  const float* c = coords + ((shared ? 0 : (int64_t)n * P) + p) * 2;
  float v = __builtin_nanf("");                                   // a row whose index names no plane
  if (pl >= 0) v = sample(planes + pl * h * w, taps_of(c[0], c[1], h, w));
  out[(int64_t)n * P + p] = v;
}

// ---------------------------------------------------------------------------------------------------------------- the fused loss
constexpr int LS_THREADS = 1024;

__global__ __launch_bounds__(LS_THREADS) void loss_sums_kernel(const float* __restrict__ masks, const int64_t* __restrict__ index,
                                                               const float* __restrict__ coords, const float* __restrict__ labels,
                                                               float* __restrict__ sums, int64_t num_planes, int h, int w, int P) {
  __shared__ float red[LS_THREADS / 64][4];                 // (not loss_reduce.h's tree: 1024 threads, and the 16 waves are added in index order)
  const int n = blockIdx.x, tid = threadIdx.x;
  const int64_t pl = plane_of(index, n, num_planes);
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (pl >= 0) {
    const float* plane = masks + pl * h * w;
    for (int p = tid; p < P; p += LS_THREADS) {
      const int64_t i = (int64_t)n * P + p;
      const float x = sample(plane, taps_of(coords[2 * i], coords[2 * i + 1], h, w)), t = labels[i], sg = sigmoid_exact(x);
      s[0] += fmaxf(x, 0.f) - x * t + log1pf(expf(-fabsf(x)));
      s[1] += sg * t;
      s[2] += sg;
      s[3] += t;
    }
  } else {
    s[0] = s[1] = s[2] = s[3] = __builtin_nanf("");
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_reduce_sum(s[k]);
  if ((tid & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red[tid >> 6][k] = s[k];
  }
  __syncthreads();
  if (tid < 4) {
    float a = 0.f;
#pragma unroll
    for (int v = 0; v < LS_THREADS / 64; ++v) a += red[v][tid];
    sums[4 * (int64_t)n + tid] = a;
  }
}

// losses[0] = sum_n (bce_n / P) / num_masks, losses[1] = sum_n [1 - (2 a + 1) / (b + c + 1)] / num_masks: thread t takes masks t, t + 256, ...
// in ascending order, then loss_reduce.h's tree
__global__ __launch_bounds__(LOSS_THREADS) void loss_finish_kernel(const float* __restrict__ sums, float* __restrict__ losses, int N, int P,
                                                                   float num_masks) {
  const int tid = threadIdx.x;
  LossSums<2, 0> a{};                                       // f: the masks' bce means, their dice terms
  for (int n = tid; n < N; n += LOSS_THREADS) {
    const float* s = sums + 4 * (int64_t)n;
    a.f[0] += s[0] / (float)P;
    a.f[1] += 1.0f - (2.0f * s[1] + 1.0f) / (s[2] + s[3] + 1.0f);
  }
  const float v = loss_block_reduce(a);
  if (tid < 2) losses[tid] = v / num_masks;
}

__global__ __launch_bounds__(256) void loss_bwd_kernel(const float* __restrict__ masks, const int64_t* __restrict__ index,
                                                       const float* __restrict__ coords, const float* __restrict__ labels,
                                                       const float* __restrict__ sums, const float* __restrict__ g_mask,
                                                       const float* __restrict__ g_dice, float* __restrict__ grad, int64_t num_planes, int h, int w,
                                                       int P, float num_masks) {
  const int n = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int64_t pl = plane_of(index, n, num_planes);
  if (pl < 0) return;
  const int64_t i = (int64_t)n * P + p;
  const Taps tp = taps_of(coords[2 * i], coords[2 * i + 1], h, w);
  const float x = sample(masks + pl * h * w, tp), t = labels[i], sg = sigmoid_exact(x);
  const float a = sums[4 * (int64_t)n + 1], den = sums[4 * (int64_t)n + 2] + sums[4 * (int64_t)n + 3] + 1.0f;
  const float gm = (g_mask ? *g_mask : 0.f) / (num_masks * (float)P), gd = (g_dice ? *g_dice : 0.f) / num_masks;
  // d dice_n / d sigma_p = (2 a + 1) / den^2 - 2 t_p / den;  d sigma / d x = sigma (1 - sigma);  d bce / d x = sigma - t
  const float gx = gm * (sg - t) + gd * sg * (1.0f - sg) * ((2.0f * a + 1.0f) / (den * den) - 2.0f * t / den);
  float* gp = grad + pl * h * w;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (tp.in[k]) atomicAdd(gp + tp.o[k], gx * tp.w[k]);
}

// ---------------------------------------------------------------------------------------------------------------- the matcher's cost
constexpr int MC_QB = 32, MC_TB = 32, MC_PC = 64, MC_LD = MC_PC + 1;     // queries, targets per workgroup; points per step; LDS row (odd: rows fall in different banks)

// THE launch rule of match_cost.  A slice is a run of `len` points (a multiple of 64) summed by one workgroup per (query block, target block); the
// count aims at 512 workgroups and never cuts below 64 points.  Recipe (Q = 100, T = 19, P = 12544): 4 x 1 units, 98 slices of 128 points.
struct Slices { int len; int count; };
Slices slices_of(int Q, int T, int P) {
  const int64_t units = (int64_t)((Q + MC_QB - 1) / MC_QB) * ((T + MC_TB - 1) / MC_TB);
  const int64_t target = units >= 512 ? 1 : (512 + units - 1) / units;
  int64_t len = ((P + target - 1) / target + MC_PC - 1) / MC_PC * MC_PC;
  if (len < MC_PC) len = MC_PC;
  return {(int)len, (int)((P + len - 1) / len)};
}
// workspace, in floats: xt [S][Q][T], st [S][Q][T], sq [S][Q][2] (softplus, sigma), tt [S][T]
int64_t cost_words(int Q, int T, int P) { return (int64_t)slices_of(Q, T, P).count * (2 * (int64_t)Q * T + 2 * (int64_t)Q + T); }

__global__ __launch_bounds__(256) void cost_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, const float* __restrict__ coords,
                                                           float* __restrict__ ws, int Q, int T, int P, int h, int w, int H, int W, int len, int S) {
  __shared__ float xs[MC_QB][MC_LD], sg[MC_QB][MC_LD], sp[MC_QB][MC_LD], ts[MC_TB][MC_LD];
  const int tid = threadIdx.x, slice = blockIdx.x, q0 = blockIdx.y * MC_QB, t0 = blockIdx.z * MC_TB;
  const int p_begin = slice * len, p_end = p_begin + len < P ? p_begin + len : P;
  const int sp_pt = tid & 63, sp_row = tid >> 6;                  // staging: one point, rows sp_row + 4 j
  const int cq = tid >> 3, ct = tid & 7;                          // summing: query cq, targets ct + 8 k
  float axt[4] = {0.f, 0.f, 0.f, 0.f}, ast[4] = {0.f, 0.f, 0.f, 0.f}, att[4] = {0.f, 0.f, 0.f, 0.f}, asp = 0.f, asg = 0.f;
  for (int pb = p_begin; pb < p_end; pb += MC_PC) {
    const int p = pb + sp_pt;
    const bool live = p < p_end;
    Taps tq, tt;
    if (live) {
      const float cx = coords[2 * (int64_t)p], cy = coords[2 * (int64_t)p + 1];
      tq = taps_of(cx, cy, h, w);
      tt = taps_of(cx, cy, H, W);
    }
#pragma unroll
    for (int j = 0; j < MC_QB / 4; ++j) {
      const int r = sp_row + 4 * j;
      float x = 0.f, s = 0.f, f = 0.f, t = 0.f;                   // a point or a row past the end adds 0 to every sum
      if (live && q0 + r < Q) {
        x = sample(pred + (int64_t)(q0 + r) * h * w, tq);
        s = sigmoid_exact(x);
        f = softplus_stable(x);
      }
      if (live && t0 + r < T) t = sample(tgt + (int64_t)(t0 + r) * H * W, tt);
      xs[r][sp_pt] = x;
      sg[r][sp_pt] = s;
      sp[r][sp_pt] = f;
      ts[r][sp_pt] = t;
    }
    __syncthreads();
    for (int k = 0; k < MC_PC; ++k) {
      const float x = xs[cq][k], s = sg[cq][k];
      asp += sp[cq][k];
      asg += s;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const float t = ts[ct + 8 * u][k];
        axt[u] = fmaf(x, t, axt[u]);
        ast[u] = fmaf(s, t, ast[u]);
        att[u] += t;
      }
    }
    __syncthreads();
  }
  float* xt = ws + (int64_t)slice * Q * T;
  float* st = ws + (int64_t)S * Q * T + (int64_t)slice * Q * T;
  float* sq = ws + 2 * (int64_t)S * Q * T + (int64_t)slice * Q * 2;
  float* tsum = ws + 2 * (int64_t)S * Q * T + 2 * (int64_t)S * Q + (int64_t)slice * T;
  const int q = q0 + cq;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = t0 + ct + 8 * u;
    if (q < Q && t < T) {
      xt[(int64_t)q * T + t] = axt[u];
      st[(int64_t)q * T + t] = ast[u];
    }
    if (blockIdx.y == 0 && cq == 0 && t < T) tsum[t] = att[u];
  }
  if (blockIdx.z == 0 && ct == 0 && q < Q) {
    sq[2 * q] = asp;
    sq[2 * q + 1] = asg;
  }
}

// one thread per (q, t): every sum over the slices in ascending order
__global__ __launch_bounds__(256) void cost_finish_kernel(const float* __restrict__ ws, const float* __restrict__ cls_prob, const int64_t* __restrict__ ids,
                                                          float* __restrict__ cost, int Q, int T, int P, int K1, int S, float w_mask, float w_class,
                                                          float w_dice) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)Q * T) return;
  const int q = (int)(i / T), t = (int)(i - (int64_t)q * T);
  const float* xt = ws + i;
  const float* st = ws + (int64_t)S * Q * T + i;
  const float* sq = ws + 2 * (int64_t)S * Q * T + 2 * q;
  const float* tsum = ws + 2 * (int64_t)S * Q * T + 2 * (int64_t)S * Q + t;
  float a_xt = 0.f, a_st = 0.f, a_sp = 0.f, a_sg = 0.f, a_t = 0.f;
  for (int s = 0; s < S; ++s) {
    a_xt += xt[(int64_t)s * Q * T];
    a_st += st[(int64_t)s * Q * T];
    a_sp += sq[(int64_t)s * Q * 2];
    a_sg += sq[(int64_t)s * Q * 2 + 1];
    a_t += tsum[(int64_t)s * T];
  }
  const int64_t id = ids[t];
  const float c_class = id >= 0 && id < K1 ? -cls_prob[(int64_t)q * K1 + id] : __builtin_nanf("");
  const float c_mask = (a_sp - a_xt) / (float)P;
  const float c_dice = 1.0f - (2.0f * a_st + 1.0f) / (a_sg + a_t + 1.0f);
  cost[i] = w_mask * c_mask + w_class * c_class + w_dice * c_dice;
}

bool plane_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= 0x7fffffffLL; }
bool rows_ok(int N, int P) { return N >= 0 && P >= 0 && N <= 65535 && ((int64_t)P + 255) / 256 <= 0x7fffffffLL; }

}  // namespace

extern "C" int rba_point_sample_f32(const float* planes, const int64_t* plane_index, const float* coords, float* out, int64_t num_planes, int N,
                                    int h, int w, int P, int shared_coords, void* stream) {
  RBA_CHECK_ARG(num_planes >= 0 && plane_ok(h, w) && rows_ok(N, P) && (shared_coords == 0 || shared_coords == 1));
  RBA_CHECK_ARG(plane_index || N <= num_planes);
  if (N == 0 || P == 0) return 0;
  RBA_CHECK_ARG(planes && coords && out && num_planes >= 1);
  rba_begin();
  hipLaunchKernelGGL(point_sample_kernel, dim3((unsigned)((P + 255) / 256), N), dim3(256), 0, (hipStream_t)stream, planes, plane_index, coords, out,
                     num_planes, h, w, P, shared_coords);
  return rba_launch_status();
}

extern "C" int rba_mask_point_loss_fwd_f32(const float* pred_masks, const int64_t* plane_index, const float* coords, const float* labels, float* sums,
                                           float* losses, int64_t num_planes, int N, int h, int w, int P, float num_masks, void* stream) {
  RBA_CHECK_ARG(num_planes >= 1 && plane_ok(h, w) && rows_ok(N, P) && N >= 1 && P >= 1 && num_masks > 0.f);
  RBA_CHECK_ARG(pred_masks && plane_index && coords && labels && sums && losses);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(loss_sums_kernel, dim3(N), dim3(LS_THREADS), 0, st, pred_masks, plane_index, coords, labels, sums, num_planes, h, w, P);
  if (const int e = rba_launch_status()) return e;
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(LOSS_THREADS), 0, st, sums, losses, N, P, num_masks);
  return rba_launch_status();
}

extern "C" int rba_mask_point_loss_bwd_f32(const float* pred_masks, const int64_t* plane_index, const float* coords, const float* labels,
                                           const float* sums, const float* grad_loss_mask, const float* grad_loss_dice, float* grad_masks,
                                           int64_t num_planes, int N, int h, int w, int P, float num_masks, void* stream) {
  RBA_CHECK_ARG(num_planes >= 1 && plane_ok(h, w) && rows_ok(N, P) && N >= 1 && P >= 1 && num_masks > 0.f);
  RBA_CHECK_ARG(num_planes <= 0x7fffffffffffffffLL / ((int64_t)h * w * 4));
  RBA_CHECK_ARG(pred_masks && plane_index && coords && labels && sums && grad_masks && (grad_loss_mask || grad_loss_dice));
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(grad_masks, 0, (size_t)(num_planes * h * w) * sizeof(float), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(loss_bwd_kernel, dim3((unsigned)((P + 255) / 256), N), dim3(256), 0, st, pred_masks, plane_index, coords, labels, sums,
                     grad_loss_mask, grad_loss_dice, grad_masks, num_planes, h, w, P, num_masks);
  return rba_launch_status();
}

extern "C" int rba_match_cost_workspace_f32(int Q, int T, int P, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && Q >= 1 && T >= 1 && P >= 1);
  *bytes = cost_words(Q, T, P) * (int64_t)sizeof(float);
  return 0;
}

extern "C" int rba_match_cost_f32(const float* pred_masks, const float* tgt_masks, const float* coords, const float* cls_prob, const int64_t* tgt_ids,
                                  float* cost, int Q, int T, int P, int h, int w, int H, int W, int K1, float w_mask, float w_class, float w_dice,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  RBA_CHECK_ARG(Q >= 1 && T >= 1 && P >= 1 && K1 >= 1 && plane_ok(h, w) && plane_ok(H, W));
  RBA_CHECK_ARG((Q + MC_QB - 1) / MC_QB <= 65535 && (T + MC_TB - 1) / MC_TB <= 65535 && ((int64_t)Q * T + 255) / 256 <= 0x7fffffffLL);
  RBA_CHECK_ARG(pred_masks && tgt_masks && coords && cls_prob && tgt_ids && cost);
  RBA_CHECK_ARG(workspace && (((uintptr_t)workspace) & 3) == 0 && workspace_bytes >= cost_words(Q, T, P) * (int64_t)sizeof(float));
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const Slices sl = slices_of(Q, T, P);
  float* ws = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(cost_partial_kernel, dim3(sl.count, (Q + MC_QB - 1) / MC_QB, (T + MC_TB - 1) / MC_TB), dim3(256), 0, st, pred_masks, tgt_masks,
                     coords, ws, Q, T, P, h, w, H, W, sl.len, sl.count);
  if (const int e = rba_launch_status()) return e;
  hipLaunchKernelGGL(cost_finish_kernel, dim3((unsigned)(((int64_t)Q * T + 255) / 256)), dim3(256), 0, st, ws, cls_prob, tgt_ids, cost, Q, T, P, K1,
                     sl.count, w_mask, w_class, w_dice);
  return rba_launch_status();
}
