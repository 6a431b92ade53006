// K3 backward -- gradients of the masked multi-head cross attention core (masked_xattn.hip) with respect to q, k and v.  The mask is detached in the
// reference (mask2former_transformer_decoder.py:487) and receives no gradient.
//
// Flash-style: the [B*nH, Q, S] score / probability tensors are never written.  With s = scale q.k, p = softmax over the un-blocked keys,
// dp = dO.v, delta = sum_s p dp (= dO.O):   dv_s = sum_q p dO,   ds = p (dp - delta) scale,   dk_s = sum_q ds q,   dq = sum_s ds k.
//
// Two launches, every output with ONE writer and a fixed summation order (bitwise reproducible, no atomics, no hand-off between workgroups):
//   row pass  long rows (S >= 1024): one 512-thread workgroup per (batch, head, 4 queries); a thread takes keys t, t + 512, ... and reads each
//             k / v row ONCE for the four queries (q, dO are workgroup-uniform: scalar loads).  Short rows: one 256-thread workgroup per (batch,
//             head, query), the shape of forward v1 -- four times the workgroups and a quarter of the serial work each, which wins while the k / v
//             re-reads are cheap (measured: docs/kernels/K3.md).  A first sweep over the keys gives each row's softmax statistics (max m,
//             1 / l, delta) and its "any un-blocked key" flag (the all-masked-row rule of :433) -> workspace; a second sweep over the same keys
//             (L2-resident) sums dq.  The workgroup owns its whole rows, so dq needs no sum across key chunks at all.
//   key pass  one 256-thread workgroup per (64-key chunk, head, batch): lane = key, its k / v rows and its dk / dv accumulators in registers;
//             the four waves sweep a quarter of the queries each (q, dO and the row statistics are wave-uniform: scalar loads), then the four
//             partial sums are added in wave order through LDS.
// Exact fp32 FMA throughout (no matrix pipe): 100 queries x 32 dims x at most ~8k keys is launch- and latency-bound, docs/kernels/K3.md
// (Backward) has the count and the measured times.  A blocked (query, key) pair is skipped by a branch, so it contributes exactly nothing.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int HD = 32;
constexpr int KCH = 64;                                  // keys per workgroup of the key pass (one per lane)
constexpr int KW = 4;                                    // its waves: query quarters
constexpr int RST = 2 * HD + 1;                          // LDS row stride of the wave partials (odd: lane-indexed rows hit distinct banks)
constexpr float SCALE = 0.17677669529663687f;            // 32^-0.5

__device__ __forceinline__ float dot32(const float (&a)[HD], const float4* __restrict__ row) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < HD / 4; ++i) {
    const float4 r = row[i];
    s = fmaf(a[4 * i], r.x, s); s = fmaf(a[4 * i + 1], r.y, s);
    s = fmaf(a[4 * i + 2], r.z, s); s = fmaf(a[4 * i + 3], r.w, s);
  }
  return s;
}

// Row pass, short rows (S < RLONG): one 256-thread workgroup per (batch, head, query), the shape of forward v1 -- q, dO in registers, keys streamed.
// stats[((b * nH + h) * Q + q) * 4 + {0, 1, 2, 3}] = row max m, 1 / l, delta, use_mask (0.f | 1.f)
__global__ __launch_bounds__(256) void xattn_bwd_row1_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ mlog, const float* __restrict__ dout,
                                                            float* __restrict__ stats, float* __restrict__ dq, int Q, int S, int nH) {
  const int qi = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ float sh_any[4];
  __shared__ float sh_m[4], sh_l[4], sh_a[4], sh_acc[4][HD];

  const float* mrow = mlog ? mlog + ((int64_t)b * Q + qi) * S : nullptr;
  bool use_mask = false;
  if (mrow) {
    float any = 0.f;
    for (int s = tid; s < S; s += 256) any = fmaxf(any, rba_mask_blocked(mrow[s]) ? 0.f : 1.f);
    any = wave_reduce_max(any);
    if (lane == 0) sh_any[wave] = any;
    __syncthreads();
    use_mask = fmaxf(fmaxf(sh_any[0], sh_any[1]), fmaxf(sh_any[2], sh_any[3])) > 0.f;
  }

  const int64_t row = (((int64_t)b * Q + qi) * nH + h) * HD;      // workgroup-uniform -> scalar loads
  float qv[HD], gv[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) { qv[d] = q[row + d] * SCALE; gv[d] = dout[row + d]; }

  const int64_t rs = (int64_t)nH * HD;
  const float* kb = k + (int64_t)b * S * rs + h * HD;
  const float* vb = v + (int64_t)b * S * rs + h * HD;

  // ---- sweep 1: m, l = sum e^(s - m), a = sum e^(s - m) dp
  float m = -INFINITY, l = 0.f, a = 0.f;
  for (int s = tid; s < S; s += 256) {
    if (use_mask && rba_mask_blocked(mrow[s])) continue;
    const float sc = dot32(qv, reinterpret_cast<const float4*>(kb + s * rs));
    const float dp = dot32(gv, reinterpret_cast<const float4*>(vb + s * rs));
    if (sc > m) {
      const float f = __expf(m - sc);                   // m = -inf -> 0
      l *= f; a *= f; m = sc;
    }
    const float e = __expf(sc - m);
    l += e;
    a = fmaf(e, dp, a);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float m2 = __shfl_xor(m, o, RBA_WAVE), l2 = __shfl_xor(l, o, RBA_WAVE), a2 = __shfl_xor(a, o, RBA_WAVE);
    const float mn = fmaxf(m, m2);
    const float f1 = (m == -INFINITY) ? 0.f : __expf(m - mn), f2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
    l = l * f1 + l2 * f2;
    a = a * f1 + a2 * f2;
    m = mn;
  }
  if (lane == 0) { sh_m[wave] = m; sh_l[wave] = l; sh_a[wave] = a; }
  __syncthreads();
  const float M = fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));       // finite: S >= 1 and a row never ends with every key blocked
  float L = 0.f, A = 0.f;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float f = sh_m[w] == -INFINITY ? 0.f : __expf(sh_m[w] - M);
    L += sh_l[w] * f;
    A += sh_a[w] * f;
  }
  const float inv_l = 1.0f / L, delta = A / L;
  if (tid == 0) {
    float* st = stats + (((int64_t)b * nH + h) * Q + qi) * 4;
    st[0] = M; st[1] = inv_l; st[2] = delta; st[3] = use_mask ? 1.f : 0.f;
  }
  if (!dq) return;                                        // uniform

  // ---- sweep 2: dq = sum_s ds k_s
  float acc[HD];
#pragma unroll
  for (int d = 0; d < HD; ++d) acc[d] = 0.f;
  for (int s = tid; s < S; s += 256) {
    if (use_mask && rba_mask_blocked(mrow[s])) continue;
    const float4* kr = reinterpret_cast<const float4*>(kb + s * rs);
    const float sc = dot32(qv, kr);
    const float dp = dot32(gv, reinterpret_cast<const float4*>(vb + s * rs));
    const float ds = __expf(sc - M) * inv_l * (dp - delta) * SCALE;
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
      const float4 kk = kr[i];
      acc[4 * i] = fmaf(ds, kk.x, acc[4 * i]); acc[4 * i + 1] = fmaf(ds, kk.y, acc[4 * i + 1]);
      acc[4 * i + 2] = fmaf(ds, kk.z, acc[4 * i + 2]); acc[4 * i + 3] = fmaf(ds, kk.w, acc[4 * i + 3]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1)
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[d] += __shfl_xor(acc[d], o, RBA_WAVE);
  if (lane == 0) {
#pragma unroll
    for (int d = 0; d < HD; ++d) sh_acc[wave][d] = acc[d];
  }
  __syncthreads();
  if (tid < HD) dq[row + tid] = ((sh_acc[0][tid] + sh_acc[1][tid]) + sh_acc[2][tid]) + sh_acc[3][tid];
}

// Row pass, long rows (S >= RLONG): four queries per workgroup share every k / v row read.  Same outputs, same statistics layout.
constexpr int RLONG = 1024;
constexpr int RQ = 4;                                     // queries per workgroup of the row pass
constexpr int RT = 512, RWV = RT / 64;                    // its threads (one key each per step) and waves

// stats[((b * nH + h) * Q + q) * 4 + {0, 1, 2, 3}] = row max m, 1 / l, delta, use_mask (0.f | 1.f)
__global__ __launch_bounds__(RT) void xattn_bwd_row_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           const float* __restrict__ mlog, const float* __restrict__ dout,
                                                           float* __restrict__ stats, float* __restrict__ dq, int Q, int S, int nH) {
  const int q0 = blockIdx.x * RQ, h = blockIdx.y, b = blockIdx.z;
  const int nq = min(RQ, Q - q0);                         // workgroup-uniform, >= 1
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __shared__ float sh_any[RQ][RWV];
  __shared__ float sh_m[RQ][RWV], sh_l[RQ][RWV], sh_a[RQ][RWV];
  __shared__ float sh_acc[RWV][RQ * HD];

  // ---- which rows have an un-blocked key (blocked iff sigmoid(x) < 0.5: rba_mask_blocked); a row without one attends everywhere
  bool use_mask[RQ];
#pragma unroll
  for (int j = 0; j < RQ; ++j) use_mask[j] = false;
  if (mlog) {
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      float any = 0.f;
      if (j < nq) {
        const float* mrow = mlog + ((int64_t)b * Q + q0 + j) * S;
        for (int s = tid; s < S; s += RT) any = fmaxf(any, rba_mask_blocked(mrow[s]) ? 0.f : 1.f);
      }
      any = wave_reduce_max(any);
      if (lane == 0) sh_any[j][wave] = any;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      float any = 0.f;
#pragma unroll
      for (int w = 0; w < RWV; ++w) any = fmaxf(any, sh_any[j][w]);
      use_mask[j] = any > 0.f;
    }
  }

  const int64_t rs = (int64_t)nH * HD;
  const float* kb = k + (int64_t)b * S * rs + h * HD;
  const float* vb = v + (int64_t)b * S * rs + h * HD;
  const int64_t row0 = (((int64_t)b * Q + q0) * nH + h) * HD;          // query j of the workgroup: row0 + j * rs (workgroup-uniform -> scalar loads)

  // ---- sweep 1: per query m, l = sum e^(s - m), a = sum e^(s - m) dp; the key's k (pre-scaled) and v rows are read once for the RQ queries
  float m[RQ], l[RQ], a[RQ];
#pragma unroll
  for (int j = 0; j < RQ; ++j) { m[j] = -INFINITY; l[j] = 0.f; a[j] = 0.f; }
  for (int s = tid; s < S; s += RT) {
    float ks[HD], vv[HD];
    const float4* kr = reinterpret_cast<const float4*>(kb + s * rs);
    const float4* vr = reinterpret_cast<const float4*>(vb + s * rs);
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
      const float4 x = kr[i], y = vr[i];
      ks[4 * i] = x.x * SCALE; ks[4 * i + 1] = x.y * SCALE; ks[4 * i + 2] = x.z * SCALE; ks[4 * i + 3] = x.w * SCALE;
      vv[4 * i] = y.x; vv[4 * i + 1] = y.y; vv[4 * i + 2] = y.z; vv[4 * i + 3] = y.w;
    }
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      if (j >= nq) continue;
      if (use_mask[j] && rba_mask_blocked(mlog[((int64_t)b * Q + q0 + j) * S + s])) continue;
      const float* qr = q + row0 + j * rs;
      const float* gr = dout + row0 + j * rs;
      float sc = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) { sc = fmaf(qr[d], ks[d], sc); dp = fmaf(gr[d], vv[d], dp); }
      if (sc > m[j]) {
        const float f = __expf(m[j] - sc);                // m = -inf -> 0
        l[j] *= f; a[j] *= f; m[j] = sc;
      }
      const float e = __expf(sc - m[j]);
      l[j] += e;
      a[j] = fmaf(e, dp, a[j]);
    }
  }
  float M[RQ], inv_l[RQ], delta[RQ];
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m[j], o, RBA_WAVE), l2 = __shfl_xor(l[j], o, RBA_WAVE), a2 = __shfl_xor(a[j], o, RBA_WAVE);
      const float mn = fmaxf(m[j], m2);
      const float f1 = (m[j] == -INFINITY) ? 0.f : __expf(m[j] - mn), f2 = (m2 == -INFINITY) ? 0.f : __expf(m2 - mn);
      l[j] = l[j] * f1 + l2 * f2;
      a[j] = a[j] * f1 + a2 * f2;
      m[j] = mn;
    }
    if (lane == 0) { sh_m[j][wave] = m[j]; sh_l[j][wave] = l[j]; sh_a[j][wave] = a[j]; }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < RQ; ++j) {
    float mm = -INFINITY;
#pragma unroll
    for (int w = 0; w < RWV; ++w) mm = fmaxf(mm, sh_m[j][w]);          // finite for j < nq: S >= 1 and a row never ends with every key blocked
    float L = 0.f, A = 0.f;
#pragma unroll
    for (int w = 0; w < RWV; ++w) {
      const float f = sh_m[j][w] == -INFINITY ? 0.f : __expf(sh_m[j][w] - mm);
      L += sh_l[j][w] * f;
      A += sh_a[j][w] * f;
    }
    M[j] = mm; inv_l[j] = 1.0f / L; delta[j] = A / L;                   // (rows j >= nq: unused)
    if (tid == 0 && j < nq) {
      float* st = stats + (((int64_t)b * nH + h) * Q + q0 + j) * 4;
      st[0] = M[j]; st[1] = inv_l[j]; st[2] = delta[j]; st[3] = use_mask[j] ? 1.f : 0.f;
    }
  }
  if (!dq) return;                                        // uniform

  // ---- sweep 2: dq = sum_s ds k_s = sum_s p (dp - delta) (scale k_s)
  float acc[RQ][HD];
#pragma unroll
  for (int j = 0; j < RQ; ++j)
#pragma unroll
    for (int d = 0; d < HD; ++d) acc[j][d] = 0.f;
  for (int s = tid; s < S; s += RT) {
    float ks[HD], vv[HD];
    const float4* kr = reinterpret_cast<const float4*>(kb + s * rs);
    const float4* vr = reinterpret_cast<const float4*>(vb + s * rs);
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
      const float4 x = kr[i], y = vr[i];
      ks[4 * i] = x.x * SCALE; ks[4 * i + 1] = x.y * SCALE; ks[4 * i + 2] = x.z * SCALE; ks[4 * i + 3] = x.w * SCALE;
      vv[4 * i] = y.x; vv[4 * i + 1] = y.y; vv[4 * i + 2] = y.z; vv[4 * i + 3] = y.w;
    }
#pragma unroll
    for (int j = 0; j < RQ; ++j) {
      if (j >= nq) continue;
      if (use_mask[j] && rba_mask_blocked(mlog[((int64_t)b * Q + q0 + j) * S + s])) continue;
      const float* qr = q + row0 + j * rs;
      const float* gr = dout + row0 + j * rs;
      float sc = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) { sc = fmaf(qr[d], ks[d], sc); dp = fmaf(gr[d], vv[d], dp); }
      const float ds = __expf(sc - M[j]) * inv_l[j] * (dp - delta[j]);
#pragma unroll
      for (int d = 0; d < HD; ++d) acc[j][d] = fmaf(ds, ks[d], acc[j][d]);
    }
  }
#pragma unroll
  for (int j = 0; j < RQ; ++j)
#pragma unroll
    for (int d = 0; d < HD; ++d) {
      float x = acc[j][d];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, RBA_WAVE);
      if (lane == 0) sh_acc[wave][j * HD + d] = x;
    }
  __syncthreads();
  if (tid < nq * HD) {
    float x = sh_acc[0][tid];
#pragma unroll
    for (int w = 1; w < RWV; ++w) x += sh_acc[w][tid];                  // wave order: fixed
    dq[row0 + (tid / HD) * rs + (tid % HD)] = x;
  }
}

__global__ __launch_bounds__(64 * KW) void xattn_bwd_key_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                const float* __restrict__ mlog, const float* __restrict__ dout,
                                                                const float* __restrict__ stats, float* __restrict__ dk, float* __restrict__ dv,
                                                                int Q, int S, int nH) {
  __shared__ float red[(KW - 1) * KCH * RST];
  const int h = blockIdx.y, b = blockIdx.z;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int s = blockIdx.x * KCH + lane;
  const bool valid = s < S;
  const int64_t rs = (int64_t)nH * HD;
  const int64_t krow = ((int64_t)b * S + (valid ? s : 0)) * rs + h * HD;

  float ks[HD], vv[HD], dka[HD], dva[HD];                 // ks = k * scale: the score's operand (dq is not formed here)
  {
    const float4* kr = reinterpret_cast<const float4*>(k + krow);
    const float4* vr = reinterpret_cast<const float4*>(v + krow);
#pragma unroll
    for (int i = 0; i < HD / 4; ++i) {
      const float4 a = kr[i], c = vr[i];
      ks[4 * i] = a.x * SCALE; ks[4 * i + 1] = a.y * SCALE; ks[4 * i + 2] = a.z * SCALE; ks[4 * i + 3] = a.w * SCALE;
      vv[4 * i] = c.x; vv[4 * i + 1] = c.y; vv[4 * i + 2] = c.z; vv[4 * i + 3] = c.w;
    }
  }
#pragma unroll
  for (int d = 0; d < HD; ++d) { dka[d] = 0.f; dva[d] = 0.f; }

  const int per = (Q + KW - 1) / KW;
  const int q0 = wave * per, q1 = min(Q, q0 + per);
  for (int qi = q0; qi < q1; ++qi) {                      // wave-uniform bounds
    const float* st = stats + (((int64_t)b * nH + h) * Q + qi) * 4;
    const float M = st[0], inv_l = st[1], delta = st[2];
    const bool use_mask = mlog != nullptr && st[3] != 0.f;
    bool open = valid;
    if (use_mask && valid) open = !rba_mask_blocked(mlog[((int64_t)b * Q + qi) * S + s]);
    if (open) {
      const float* qr = q + (((int64_t)b * Q + qi) * nH + h) * HD;           // wave-uniform rows
      const float* gr = dout + (((int64_t)b * Q + qi) * nH + h) * HD;
      float sc = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) { sc = fmaf(qr[d], ks[d], sc); dp = fmaf(gr[d], vv[d], dp); }
      const float p = __expf(sc - M) * inv_l;
      const float ds = p * (dp - delta) * SCALE;
#pragma unroll
      for (int d = 0; d < HD; ++d) { dva[d] = fmaf(p, gr[d], dva[d]); dka[d] = fmaf(ds, qr[d], dka[d]); }
    }
  }
  // ---- the four query quarters, added in wave order
  if (wave > 0) {
    float* r = red + ((wave - 1) * KCH + lane) * RST;
#pragma unroll
    for (int d = 0; d < HD; ++d) { r[d] = dka[d]; r[HD + d] = dva[d]; }
  }
  __syncthreads();
  if (wave == 0 && valid) {
#pragma unroll
    for (int w = 0; w < KW - 1; ++w) {
      const float* r = red + (w * KCH + lane) * RST;
#pragma unroll
      for (int d = 0; d < HD; ++d) { dka[d] += r[d]; dva[d] += r[HD + d]; }
    }
    if (dk) {
      float4* o = reinterpret_cast<float4*>(dk + krow);
#pragma unroll
      for (int i = 0; i < HD / 4; ++i) o[i] = make_float4(dka[4 * i], dka[4 * i + 1], dka[4 * i + 2], dka[4 * i + 3]);
    }
    if (dv) {
      float4* o = reinterpret_cast<float4*>(dv + krow);
#pragma unroll
      for (int i = 0; i < HD / 4; ++i) o[i] = make_float4(dva[4 * i], dva[4 * i + 1], dva[4 * i + 2], dva[4 * i + 3]);
    }
  }
}

}  // namespace

extern "C" int64_t rba_masked_xattn_bwd_workspace_bytes(int B, int Q, int S, int nH) {
  if (B <= 0 || Q <= 0 || S <= 0 || nH <= 0) return 0;
  return (int64_t)B * nH * Q * 4 * sizeof(float);         // the row statistics; dq has one writer per row and needs no partial tiles
}

extern "C" int rba_masked_xattn_bwd_f32(const float* q, const float* k, const float* v, const float* mask_logits, const float* grad_out,
                                        float* grad_q, float* grad_k, float* grad_v, float* workspace, int B, int Q, int S, int nH, int hd,
                                        void* stream) {
  RBA_CHECK_ARG(B >= 0 && Q >= 0 && S >= 1 && nH >= 1 && hd == HD && nH <= 65535 && B <= 65535);
  RBA_CHECK_ARG((int64_t)(S + KCH - 1) / KCH <= 2147483647);
  if (B == 0 || !(grad_q || grad_k || grad_v)) return 0;
  hipStream_t st = (hipStream_t)stream;
  rba_begin();
  if (Q == 0) {                                           // an empty sum over the queries: dk = dv = 0, dq is empty
    const size_t n = (size_t)B * S * nH * HD * sizeof(float);
    if (grad_k && hipMemsetAsync(grad_k, 0, n, st) != hipSuccess) return rba_launch_status();
    if (grad_v && hipMemsetAsync(grad_v, 0, n, st) != hipSuccess) return rba_launch_status();
    return rba_launch_status();
  }
  RBA_CHECK_ARG(q && k && v && grad_out && workspace);
  RBA_CHECK_ARG((((uintptr_t)k | (uintptr_t)v | (uintptr_t)grad_k | (uintptr_t)grad_v | (uintptr_t)workspace) & 15) == 0);
  if (S >= RLONG)
    hipLaunchKernelGGL(xattn_bwd_row_kernel, dim3((Q + RQ - 1) / RQ, nH, B), dim3(RT), 0, st, q, k, v, mask_logits, grad_out, workspace, grad_q, Q, S, nH);
  else
    hipLaunchKernelGGL(xattn_bwd_row1_kernel, dim3(Q, nH, B), dim3(256), 0, st, q, k, v, mask_logits, grad_out, workspace, grad_q, Q, S, nH);
  if (grad_k || grad_v)
    hipLaunchKernelGGL(xattn_bwd_key_kernel, dim3((S + KCH - 1) / KCH, nH, B), dim3(64 * KW), 0, st, q, k, v, mask_logits, grad_out, workspace,
                       grad_k, grad_v, Q, S, nH);
  return rba_launch_status();
}
