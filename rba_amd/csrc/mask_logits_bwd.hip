// K4 backward -- the two gradients of the mask-logit contraction out[b,q,n] = sum_c E[b,q,c] F[b,c,n] (mask_logits.hip; reference:
// torch.einsum("bqc,bchw->bqhw"), mask2former_transformer_decoder.py:479 under autograd).  With G = d loss / d out [B,Q,N]:
//
//   grad_embed[b,q,c] = sum_n G[b,q,n] F[b,c,n]          grad_feat[b,c,n] = sum_q E[b,q,c] G[b,q,n]
//
// Both run in exact fp32 on the matrix pipe (v_mfma_f32_16x16x4_f32, the instruction of the forward's exact path): G is the gradient of a mean
// over 10^4 .. 10^6 pixels, far below f16's smallest normal number, so an f16 split would lose it.  Scaling G by a power of two scales both
// results by exactly that power (tests/test_mask_logits_backward_gpu.py holds this).
//
// grad_embed -- a tiny [Q x C] output with a long reduction over n, both operands contiguous along n.  The pixel axis is cut into slices
// (rule: slices_of below); one workgroup of four waves owns one slice, one block of 112 queries and one block of 64 channels, 16 channels per
// wave: 7 accumulator tiles of 16 x 16 (28 registers).  Per step of 32 pixels the workgroup stages its G rows [112 x 32] once for all four
// waves through LDS (coalesced 128-byte row pieces; double-buffered, one barrier per step; rows >= Q are zeros), every wave loads its own 16
// rows of F in operand order (lane (j = lane % 16, kk = lane / 16) reads F[c0 + j][n + 4 kk .. + 3] and F[c0 + j][n + 16 + 4 kk .. + 3]: the whole
// 128-byte line of a row is consumed by the same wave in two back-to-back loads), and component i of those float4 is the k-slice {n + 4 kk + i}
// of one MFMA -- the same pixels for A (G out of LDS, ds_read_b128 at row stride 36: conflict-free) and B.  Loads of step s + 1 are in flight
// during the 56 MFMAs of step s.  The partial tile goes to the caller's workspace [slice][b][q][c] with plain stores and a second small launch
// sums the slices in a fixed order: no float atomics, bitwise reproducible, nothing in the workspace has to start from a known value.
//
// grad_feat -- the forward's shape class (M = C rows, K = Q, long N).  One wave owns 64 pixel columns and 64 channels: per k-step of 4
// queries it loads ONE float4 of G per lane (lane (j, kk) reads G[4 s + kk][n0 + 4 j .. + 3], 256 B contiguous per query row), the B operand of
// four column tiles {n0 + 4 j + i} as in the forward; the A operand E[q][c] in its native [q][c] layout is already the [k][m] image: LDS rows of
// 80 floats (64 + 16: the four kk groups of a read land 16 banks apart, conflict-free), filled per chunk of 128 queries so that LDS stays at
// 40 KiB for every Q (no dynamic-LDS cap to raise), rows >= Q and channels >= C zero.  4 x 4 accumulator tiles = 64 registers.  Each output is
// one fixed chain: bitwise reproducible by construction.
//
// Outside N % 4 == 0 and 16-byte aligned pointers both gradients take plain fp32 VALU kernels (same slices, same workspace, same sum).
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

typedef float k4b_f32x4 __attribute__((ext_vector_type(4)));

constexpr int GE_QB = 112, GE_QT = 7, GE_CB = 64, GE_KC = 32, GE_LD = GE_KC + 4;       // grad_embed: query block, its tiles, channel block, pixels per step
constexpr int GF_CB = 64, GF_LD = GF_CB + 16, GF_QC = 128, GF_COLS = 256;               // grad_feat: channel block, LDS row, query chunk, columns per workgroup

// THE launch rule of grad_embed.  A slice is a run of `len` pixels (a multiple of 32, at least 512) summed by one workgroup per (image, query
// block, channel block); the count aims at 512 workgroups -- two per CU of the 256 -- and never cuts below 512 pixels, which bounds the partial
// traffic: count * Q C * 8 bytes written and read back against 4 (C + Q) N bytes of input is 2 Q C / ((C + Q) * 512) <= 0.28 at Q = 100, C = 256.
// Training crop (1 x 100 x 256 x 32768): 64 slices of 512 x 4 channel blocks = 256 workgroups, one per CU; N = 131072: 128 slices of 1024 = 512.
struct Slices { int64_t len; int64_t count; };
Slices slices_of(int B, int Q, int C, int64_t N) {
  const int64_t units = (int64_t)B * ((Q + GE_QB - 1) / GE_QB) * ((C + GE_CB - 1) / GE_CB);
  const int64_t target = units >= 512 ? 1 : (512 + units - 1) / units;
  int64_t len = ((N + target - 1) / target + 31) / 32 * 32;
  if (len < 512) len = 512;
  return {len, (N + len - 1) / len};
}

__global__ __launch_bounds__(256) void k4_bwd_embed_kernel(const float* __restrict__ gout, const float* __restrict__ feat, float* __restrict__ part,
                                                           int B, int Q, int C, int64_t N, int64_t len, int cblocks) {
  __shared__ __attribute__((aligned(16))) float gl[2][GE_QB * GE_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kk = lane >> 4;
  const int b = blockIdx.z, qb = blockIdx.x / cblocks, cbk = blockIdx.x - qb * cblocks;
  const int q0 = qb * GE_QB, c0 = cbk * GE_CB + wave * 16;
  const int64_t n_begin = (int64_t)blockIdx.y * len, n_end = n_begin + len < N ? n_begin + len : N;     // N % 4 == 0: a float4 is wholly in or out
  const int64_t steps = (n_end - n_begin + GE_KC - 1) / GE_KC;
  const float* gb = gout + (int64_t)b * Q * N;
  const float* fb = feat + (int64_t)b * C * N;
  const bool wave_live = c0 < C;                                  // a wave past the last channel only helps staging G
  const int fc = c0 + l15;
  const k4b_f32x4 zero = {0.f, 0.f, 0.f, 0.f};

  k4b_f32x4 greg[4], freg[2];
  auto load = [&](int64_t step) {
    const int64_t n = n_begin + step * GE_KC;
#pragma unroll
    for (int j = 0; j < 4; ++j) {                                 // 896 float4 of the G tile over 256 threads: 8 lanes = 128 B of one row
      const int idx = tid + 256 * j, row = idx >> 3;
      const int64_t col = n + 4 * (idx & 7);
      greg[j] = (idx < GE_QB * 8 && q0 + row < Q && col < n_end) ? *reinterpret_cast<const k4b_f32x4*>(gb + (int64_t)(q0 + row) * N + col) : zero;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int64_t col = n + 16 * h + 4 * kk;
      freg[h] = (fc < C && col < n_end) ? *reinterpret_cast<const k4b_f32x4*>(fb + (int64_t)fc * N + col) : zero;
    }
  };

  k4b_f32x4 acc[GE_QT];
#pragma unroll
  for (int t = 0; t < GE_QT; ++t) acc[t] = zero;
  load(0);
  for (int64_t s = 0; s < steps; ++s) {
    float* buf = gl[s & 1];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int idx = tid + 256 * j;
      if (idx < GE_QB * 8) *reinterpret_cast<k4b_f32x4*>(buf + (idx >> 3) * GE_LD + 4 * (idx & 7)) = greg[j];
    }
    const k4b_f32x4 f0 = freg[0], f1 = freg[1];
    __syncthreads();                 // one barrier per step: the buffer written now was last read two steps ago, before the previous barrier
    if (s + 1 < steps) load(s + 1);
    if (wave_live) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const k4b_f32x4 f4 = h ? f1 : f0;
        k4b_f32x4 a[GE_QT];
#pragma unroll
        for (int t = 0; t < GE_QT; ++t) a[t] = *reinterpret_cast<const k4b_f32x4*>(buf + (16 * t + l15) * GE_LD + 16 * h + 4 * kk);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int t = 0; t < GE_QT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t][i], f4[i], acc[t], 0, 0, 0);
      }
    }
  }
  // lane holds grad_embed[q = q0 + 16 t + 4 kk + r][c = c0 + l15] in acc[t][r]
  if (fc >= C) return;
  float* pb = part + (((int64_t)blockIdx.y * B + b) * Q) * C + fc;
#pragma unroll
  for (int t = 0; t < GE_QT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 16 * t + 4 * kk + r;
      if (q < Q) pb[(int64_t)q * C] = acc[t][r];
    }
}

// The same slices on the VALU, for N % 4 != 0 or unaligned pointers: one workgroup = one slice and 16 x 16 outputs, 32 pixels per step through LDS
__global__ __launch_bounds__(256) void k4_bwd_embed_valu_kernel(const float* __restrict__ gout, const float* __restrict__ feat, float* __restrict__ part,
                                                                int B, int Q, int C, int64_t N, int64_t len, int ctiles) {
  __shared__ float gs[16][33], fs[16][33];
  const int tid = threadIdx.x, tq = tid >> 4, tc = tid & 15;
  const int b = blockIdx.z, qt = blockIdx.x / ctiles, q0 = qt * 16, c0 = (blockIdx.x - qt * ctiles) * 16;
  const int64_t n_begin = (int64_t)blockIdx.y * len, n_end = n_begin + len < N ? n_begin + len : N;
  const float* gb = gout + (int64_t)b * Q * N;
  const float* fb = feat + (int64_t)b * C * N;
  float acc = 0.f;
  for (int64_t n = n_begin; n < n_end; n += 32) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + 256 * j, row = idx >> 5, col = idx & 31;
      const bool in = n + col < n_end;
      gs[row][col] = (in && q0 + row < Q) ? gb[(int64_t)(q0 + row) * N + n + col] : 0.f;
      fs[row][col] = (in && c0 + row < C) ? fb[(int64_t)(c0 + row) * N + n + col] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 32; ++k) acc = fmaf(gs[tq][k], fs[tc][k], acc);
    __syncthreads();
  }
  if (q0 + tq < Q && c0 + tc < C) part[(((int64_t)blockIdx.y * B + b) * Q + q0 + tq) * C + c0 + tc] = acc;
}

// grad_embed[i] = sum over the slices of part[slice][i]: four interleaved runs in ascending order, then ((0 + 1) + (2 + 3))
__global__ __launch_bounds__(256) void k4_bwd_embed_sum_kernel(const float* __restrict__ part, float* __restrict__ gembed, int64_t total, int64_t slices) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  const float* p = part + i;
  int64_t t = 0;
  for (; t + 4 <= slices; t += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) s[u] += p[(t + u) * total];
  }
  if (t < slices) s[0] += p[t * total];
  if (t + 1 < slices) s[1] += p[(t + 1) * total];
  if (t + 2 < slices) s[2] += p[(t + 2) * total];
  gembed[i] = (s[0] + s[1]) + (s[2] + s[3]);
}

__global__ __launch_bounds__(256) void k4_bwd_feat_kernel(const float* __restrict__ embed, const float* __restrict__ gout, float* __restrict__ gfeat,
                                                          int Q, int C, int64_t N) {
  __shared__ float el[GF_QC * GF_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, kk = lane >> 4;
  const int b = blockIdx.z, c0 = blockIdx.y * GF_CB;
  const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * 64;
  const bool wave_live = n0 < N;                                  // a wave past the last column only helps filling LDS
  const int64_t ncol = n0 + 4 * l15;                              // this lane's 4 columns (N % 4 == 0)
  const bool cvalid = ncol < N;
  const float* eb = embed + (int64_t)b * Q * C;
  const float* gb = gout + (int64_t)b * Q * N + (cvalid ? ncol : 0);
  const k4b_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  k4b_f32x4 acc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[t][i] = zero;

  for (int qc0 = 0; qc0 < Q; qc0 += GF_QC) {
    const int qn = Q - qc0 < GF_QC ? Q - qc0 : GF_QC;
    if (qc0) __syncthreads();                                     // the previous chunk has been read
    for (int idx = tid; idx < GF_QC * GF_CB; idx += 256) {
      const int r = idx >> 6, cc = idx & 63;
      el[r * GF_LD + cc] = (r < qn && c0 + cc < C) ? eb[(int64_t)(qc0 + r) * C + c0 + cc] : 0.f;
    }
    __syncthreads();
    if (!wave_live) continue;
    const int steps = (qn + 3) >> 2;
    auto load = [&](int st) {                                     // rows >= Q carry zeros: the A operand's zero padding must not meet a NaN
      const int q = qc0 + 4 * st + kk;
      return (st < steps && q < Q) ? *reinterpret_cast<const k4b_f32x4*>(gb + (int64_t)q * N) : zero;
    };
    k4b_f32x4 gcur[4], gnxt[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) gcur[u] = load(u);
    for (int s0 = 0; s0 < steps; s0 += 4) {
#pragma unroll
      for (int u = 0; u < 4; ++u) gnxt[u] = load(s0 + 4 + u);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (s0 + u < steps) {
          const float* ea = el + (4 * (s0 + u) + kk) * GF_LD + l15;
          float a[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) a[t] = ea[16 * t];
#pragma unroll
          for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[t][i] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[t], gcur[u][i], acc[t][i], 0, 0, 0);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) gcur[u] = gnxt[u];
    }
  }
  // lane holds grad_feat[c = c0 + 16 t + 4 kk + r][n = ncol + i] in acc[t][i][r]
  if (!wave_live || !cvalid) return;
  float* ob = gfeat + (int64_t)b * C * N + ncol;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = c0 + 16 * t + 4 * kk + r;
      if (c < C) *reinterpret_cast<k4b_f32x4*>(ob + (int64_t)c * N) = (k4b_f32x4){acc[t][0][r], acc[t][1][r], acc[t][2][r], acc[t][3][r]};
    }
}

// one thread = one pixel column, channels walked by blockIdx.y: E[q][c] is wave-uniform, G rows are read coalesced
__global__ __launch_bounds__(256) void k4_bwd_feat_valu_kernel(const float* __restrict__ embed, const float* __restrict__ gout, float* __restrict__ gfeat,
                                                               int Q, int C, int64_t N) {
  const int b = blockIdx.z;
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float* eb = embed + (int64_t)b * Q * C;
  const float* gb = gout + (int64_t)b * Q * N + n;
  for (int c = blockIdx.y; c < C; c += gridDim.y) {
    float acc = 0.f;
    for (int q = 0; q < Q; ++q) acc = fmaf(eb[(int64_t)q * C + c], gb[(int64_t)q * N], acc);
    gfeat[((int64_t)b * C + c) * N + n] = acc;
  }
}

bool domain_ok(int B, int Q, int C, int64_t N) { return B >= 0 && Q >= 0 && C >= 1 && N >= 0 && B <= 65535; }
int64_t part_bytes(int B, int Q, int C, int64_t N) { return slices_of(B, Q, C, N).count * B * Q * C * (int64_t)sizeof(float); }
// every grid dimension below stays inside HIP's limits (x < 2^31, y and z <= 65535) and the partial sums' element count inside int64
bool sizes_ok(int B, int Q, int C, int64_t N) {
  const int64_t tiles16 = (int64_t)((Q + 15) / 16) * ((C + 15) / 16);
  return tiles16 <= 0x7fffffffLL && ((int64_t)B * Q * C + 255) / 256 <= 0x7fffffffLL && (N + 255) / 256 <= 0x7fffffffLL && (C + GF_CB - 1) / GF_CB <= 65535;
}

}  // namespace

extern "C" int rba_mask_logits_bwd_workspace_f32(int B, int Q, int C, int64_t N, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && domain_ok(B, Q, C, N));
  if (B == 0 || Q == 0 || N == 0) {
    *bytes = 0;
    return 0;
  }
  RBA_CHECK_ARG(sizes_ok(B, Q, C, N));
  *bytes = part_bytes(B, Q, C, N);
  return 0;
}

extern "C" int rba_mask_logits_bwd_f32(const float* embed, const float* feat, const float* grad_out, float* grad_embed, float* grad_feat,
                                       int B, int Q, int C, int64_t N, void* workspace, int64_t workspace_bytes, void* stream) {
  RBA_CHECK_ARG(domain_ok(B, Q, C, N));
  if (B == 0 || Q == 0 || N == 0) return 0;
  RBA_CHECK_ARG(sizes_ok(B, Q, C, N));
  RBA_CHECK_ARG(grad_out && (grad_embed || grad_feat) && (!grad_embed || feat) && (!grad_feat || embed));
  if (grad_embed) RBA_CHECK_ARG(workspace && (((uintptr_t)workspace) & 3) == 0 && workspace_bytes >= part_bytes(B, Q, C, N));
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const bool g16 = N % 4 == 0 && (((uintptr_t)grad_out) & 15) == 0;
  if (grad_embed) {
    const Slices sl = slices_of(B, Q, C, N);
    float* part = reinterpret_cast<float*>(workspace);
    if (g16 && (((uintptr_t)feat) & 15) == 0) {
      const int cblocks = (C + GE_CB - 1) / GE_CB;
      hipLaunchKernelGGL(k4_bwd_embed_kernel, dim3((unsigned)(((Q + GE_QB - 1) / GE_QB) * (int64_t)cblocks), (unsigned)sl.count, B), dim3(256), 0, st,
                         grad_out, feat, part, B, Q, C, N, sl.len, cblocks);
    } else {
      const int ctiles = (C + 15) / 16;
      hipLaunchKernelGGL(k4_bwd_embed_valu_kernel, dim3((unsigned)(((Q + 15) / 16) * (int64_t)ctiles), (unsigned)sl.count, B), dim3(256), 0, st,
                         grad_out, feat, part, B, Q, C, N, sl.len, ctiles);
    }
    if (const int e = rba_launch_status()) return e;
    const int64_t total = (int64_t)B * Q * C;
    hipLaunchKernelGGL(k4_bwd_embed_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, part, grad_embed, total, sl.count);
    if (const int e = rba_launch_status()) return e;
  }
  if (grad_feat) {
    if (g16 && (((uintptr_t)grad_feat) & 15) == 0)
      hipLaunchKernelGGL(k4_bwd_feat_kernel, dim3((unsigned)((N + GF_COLS - 1) / GF_COLS), (C + GF_CB - 1) / GF_CB, B), dim3(256), 0, st,
                         embed, grad_out, grad_feat, Q, C, N);
    else
      hipLaunchKernelGGL(k4_bwd_feat_valu_kernel, dim3((unsigned)((N + 255) / 256), C < 65535 ? C : 65535, B), dim3(256), 0, st,
                         embed, grad_out, grad_feat, Q, C, N);
    return rba_launch_status();
  }
  return 0;
}
