// K19a -- the spatial-reduction attention core of the MiT (SegFormer) block (mask2former/modeling/backbone/mix_transformer.py:113-117):
//
//   out[b,n,h,:] = softmax_s(q[b,n,h,:] . k[b,s,h,:] * scale) v[b,s,h,:]        N queries against S = N / sr^2 keys, no windows, no mask
//
// q [B,N,nH*hd] is the q Linear's output, kv [B,S,2*nH*hd] the kv Linear's output as it lies (k = kv[..., :C], v = kv[..., C:], head-major inside), out
// [B,N,nH*hd] head-major: the three reshapes / permutes of the reference are index arithmetic here.  docs/kernels/K19.md has the design and the floors.
//
// Flash-style, exact fp32 products on v_mfma_f32_32x32x2_f32.  One workgroup of four waves per (batch, head, block of 128 queries), 32 queries per wave.
// Per tile of 32 keys the workgroup stages K [32 x hd] and V [32 x hd] once in LDS (rows of hd + 4 floats; loads of tile t + 1 are in flight during the
// MFMAs of tile t).  A wave computes the TRANSPOSED score tile S^T = K Q^T: the key is the MFMA's row, the query its column, so a lane (q = lane % 32,
// half = lane / 32) holds the scores of ITS query against 16 keys {(r % 4) + 8 (r / 4) + 4 half} in its 16 accumulator registers.  The online softmax
// is then a reduction over a lane's own registers plus one exchange with lane ^ 32, and the probabilities P^T[key][q] sit exactly where the B operand
// of O^T = V^T P^T wants them (register r of the two halves = the key pair {kr, kr + 4} = the two k-slices of one MFMA): P never moves between
// lanes and never touches LDS.  O^T comes out with the query on the lane and four consecutive channels per register quad: 16-byte stores.
//
// Tails: keys >= S are staged as zeros and their scores set to -inf (exp = 0); query rows >= N are loaded as zeros, computed and not stored.
// One fixed summation order per output: bitwise reproducible.  No atomics, no scratch, no workspace.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

typedef float k19_f32x16 __attribute__((ext_vector_type(16)));

constexpr int SA_QW = 32, SA_WAVES = 4, SA_QB = SA_QW * SA_WAVES, SA_KT = 32;     // queries per wave, waves, queries per workgroup, keys per tile

template <int HD>
__global__ __launch_bounds__(256) void k19_sr_attn_kernel(const float* __restrict__ q, const float* __restrict__ kv, float* __restrict__ out,
                                                          int N, int S, int nH, float scale) {
  constexpr int LD = HD + 4, F4 = HD / 4, DT = HD / 32, QT = HD / 8, NLD = HD / 16;
  __shared__ __attribute__((aligned(16))) float kl[SA_KT * LD];
  __shared__ __attribute__((aligned(16))) float vl[SA_KT * LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, half = lane >> 5;
  const int b = blockIdx.z, head = blockIdx.y, C = nH * HD;
  const int64_t q0 = (int64_t)blockIdx.x * SA_QB + wave * SA_QW, qrow = q0 + l31;
  const bool wave_live = q0 < N, qvalid = qrow < N;            // a wave past the last query only helps staging K and V
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  // B operand of S^T = K Q^T: lane (q, half) holds Q[q][8 t + 4 half + i] in qr[t][i]; the k-slices of MFMA (t, i) are d = 8 t + i and 8 t + 4 + i
  f32x4 qr[QT];
  {
    const float* qp = q + ((int64_t)b * N + (qvalid ? qrow : 0)) * C + head * HD + 4 * half;
#pragma unroll
    for (int t = 0; t < QT; ++t) qr[t] = qvalid ? *reinterpret_cast<const f32x4*>(qp + 8 * t) : zero;
  }

  const float* kvb = kv + (int64_t)b * S * 2 * C + head * HD;
  f32x4 stage[NLD];
  auto load = [&](int k0) {                                     // 2 x 32 x hd / 4 float4 over 256 threads: a row's 128 or 256 bytes on consecutive lanes
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = tid + 256 * j, which = idx / (SA_KT * F4), rem = idx - which * (SA_KT * F4), row = rem / F4, c4 = rem - row * F4;
      const int key = k0 + row;
      stage[j] = key < S ? *reinterpret_cast<const f32x4*>(kvb + (int64_t)key * 2 * C + which * C + 4 * c4) : zero;
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int j = 0; j < NLD; ++j) {
      const int idx = tid + 256 * j, which = idx / (SA_KT * F4), rem = idx - which * (SA_KT * F4), row = rem / F4, c4 = rem - row * F4;
      *reinterpret_cast<f32x4*>((which ? vl : kl) + row * LD + 4 * c4) = stage[j];
    }
  };

  k19_f32x16 o[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float m = -INFINITY, l = 0.f;                                 // running maximum of the query's scores (both halves agree), this half's share of the sum

  load(0);
  for (int k0 = 0; k0 < S; k0 += SA_KT) {
    if (k0) __syncthreads();                                    // every wave has read the previous tile
    store();
    __syncthreads();
    if (k0 + SA_KT < S) load(k0 + SA_KT);
    if (!wave_live) continue;

    k19_f32x16 s;
#pragma unroll
    for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
    for (int t = 0; t < QT; ++t) {
      const f32x4 kf = *reinterpret_cast<const f32x4*>(kl + l31 * LD + 8 * t + 4 * half);
#pragma unroll
      for (int i = 0; i < 4; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[i], qr[t][i], s, 0, 0, 0);
    }
    // lane holds score[key = k0 + (r % 4) + 8 (r / 4) + 4 half][q] in s[r]
    float mt = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + (r & 3) + 8 * (r >> 2) + 4 * half;
      s[r] = key < S ? s[r] * scale : -INFINITY;
      mt = fmaxf(mt, s[r]);
    }
    mt = fmaxf(mt, __shfl_xor(mt, 32));                         // key k0 < S is in every tile: finite for finite inputs
    const float m_new = fmaxf(m, mt), alpha = __expf(m - m_new);
    m = m_new;
    float ls = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      s[r] = __expf(s[r] - m_new);                              // exp(-inf) = 0 for the keys >= S
      ls += s[r];
    }
    l = fmaf(l, alpha, ls);
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
    // O^T += V^T P^T: A = V[key pair of register r][d = 32 dt + lane % 32] out of LDS, B = s[r] where it is
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* vp = vl + ((r & 3) + 8 * (r >> 2) + 4 * half) * LD + l31;
#pragma unroll
      for (int d = 0; d < DT; ++d) o[d] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32 * d], s[r], o[d], 0, 0, 0);
    }
  }
  // lane holds O[q][d = 32 dt + (r % 4) + 8 (r / 4) + 4 half] in o[dt][r]
  if (!qvalid) return;
  const float inv = 1.0f / (l + __shfl_xor(l, 32));
  float* op = out + ((int64_t)b * N + qrow) * C + head * HD + 4 * half;
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<f32x4*>(op + 32 * d + 8 * g) = (f32x4){o[d][4 * g] * inv, o[d][4 * g + 1] * inv, o[d][4 * g + 2] * inv, o[d][4 * g + 3] * inv};
}

}  // namespace

extern "C" int rba_sr_attn_f32(const float* q, const float* kv, float* out, int B, int N, int S, int nH, int hd, float scale, void* stream) {
  RBA_CHECK_ARG(B >= 0 && N >= 1 && S >= 1 && nH >= 1 && (hd == 32 || hd == 64));
  if (B == 0) return 0;
  RBA_CHECK_ARG(q && kv && out && ((((uintptr_t)q) | ((uintptr_t)kv) | ((uintptr_t)out)) & 15) == 0);
  RBA_CHECK_ARG(B <= 65535 && nH <= 65535 && S <= (1 << 30) && (int64_t)nH * hd <= (1 << 24));
  rba_begin();
  const dim3 grid((unsigned)(((int64_t)N + SA_QB - 1) / SA_QB), nH, B);
  if (hd == 32)
    hipLaunchKernelGGL(k19_sr_attn_kernel<32>, grid, dim3(256), 0, (hipStream_t)stream, q, kv, out, N, S, nH, scale);
  else
    hipLaunchKernelGGL(k19_sr_attn_kernel<64>, grid, dim3(256), 0, (hipStream_t)stream, q, kv, out, N, S, nH, scale);
  return rba_launch_status();
}
