// K1 backward -- gradients of the RbA score (rba_reduce.hip) with respect to the mask logits and the class probabilities: the heavy
// differentiable piece of the reference's outlier-supervised fine-tune (SetCriterion.outlier_loss, mask2former/modeling/criterion.py:449-463).
//
//   sig = sigmoid(m);  s[k,n] = sum_q p[q,k] sig[q,n]                                     (recomputed here: the forward saves nothing)
//   t[k,n] = d score[n] / d s[k,n] = -(1 - tanh^2 s) | -softmax_k(s) | -1                 (score_mode 0 | 1 | 2)
//   u[k,n] = g[n] t[k,n]
//   grad_m[q,n] = sig (1 - sig) sum_k p[q,k] u[k,n]          grad_p[q,k] = sum_n sig[q,n] u[k,n]
//
// One workgroup of TILE = 128 lanes owns TILE consecutive pixels, one pixel per lane:
//   phase 1  every mask plane of the tile is read once (coalesced), sig goes to the lane's own LDS column, the K sums s[k] live in registers
//            (class probabilities are wave-uniform: scalar loads, SGPR operands of the FMAs -- the forward's scheme);
//   phase 2  s[k] -> u[k] in place (accurate expf and division: the gradient bar is fp32 autograd's own error), u also to LDS;
//   phase 3  per query: sig back from the lane's LDS column, K FMAs, one coalesced store of grad_m;
//   phase 4  the tile's share of grad_p, a [Q x TILE] x [TILE x K] product out of LDS, 4 x 4 outputs per lane, 16-byte LDS reads, ascending
//            pixel order; plain stores into the tile's slice of the workspace.
// A second kernel sums the slices over the tiles in a fixed order (four interleaved runs, then ((0+1)+(2+3))): no float atomics, grad_p is
// bitwise reproducible, and nothing in the workspace has to start from a known value.
// LDS rows are TILE + 4 floats.  While (Q + K) rows fit 64 KiB (Q = 100, K = 19: 61 KiB, two workgroups per CU) the whole sig tile stays
// resident; beyond that the kernel walks the queries in chunks of QC rows and phase 3 reloads the mask tile (L2 / MALL resident by then)
// and recomputes sig -- the same arithmetic, so both forms give the same bits.
//
// PER_CLASS = the adjoint of the class map itself (rba_sem_seg_bwd_f32; sem[k,n] = s[k,n] is K10's input): u[k,n] = grad_sem[k,n] is LOADED in
// phase 2 instead of derived from a one-channel gradient, so phase 1 keeps only the sigmoids.  Same tiling, workspace and fixed-order sum.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int TILE = 128, LDW = TILE + 4, ROWS_64K = 65536 / (LDW * 4);   // 124 rows of LDS without raising the kernel's dynamic limit

// 1 / (1 + e^-x) with the accurate expf and a true division: x -> -inf gives 1 / inf = 0, x -> +inf gives 1 / 1 = 1, never NaN for finite x
__device__ __forceinline__ float sigmoid_acc(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int KMAX, bool PER_CLASS>
__global__ __launch_bounds__(TILE) void rba_reduce_bwd_kernel(const float* __restrict__ mask, const float* __restrict__ prob,
                                                              const float* __restrict__ gscore /* PER_CLASS: grad_sem [K,HW] */, float* __restrict__ gmask,
                                                              float* __restrict__ part, int Q, int K, int64_t HW, int mode, int QC) {
  extern __shared__ __attribute__((aligned(16))) float k1b_lds[];
  float* sh_u = k1b_lds;                 // [K][LDW]
  float* sh_s = k1b_lds + K * LDW;       // [QC][LDW]
  const int tid = threadIdx.x;
  const int64_t n = (int64_t)blockIdx.x * TILE + tid;
  const bool live = n < HW;
  const int64_t nc = live ? n : HW - 1;  // a lane past the end reads the last pixel and carries g = 0: it adds exactly 0 to grad_p and stores nothing
  const bool resident = QC >= Q;
  const float* mp = mask + nc;

  // ---- phase 1
  float acc[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) acc[k] = 0.f;
  if constexpr (PER_CLASS) {
    if (resident) {
#pragma unroll 4
      for (int q = 0; q < Q; ++q) sh_s[q * LDW + tid] = sigmoid_acc(mp[(int64_t)q * HW]);
    }
  } else {
#pragma unroll 4
    for (int q = 0; q < Q; ++q) {
      const float s = sigmoid_acc(mp[(int64_t)q * HW]);
      if (resident) sh_s[q * LDW + tid] = s;
      const float* pq = prob + q * K;      // wave-uniform
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) acc[k] = fmaf(pq[k], s, acc[k]);
    }
  }

  // ---- phase 2: acc[k] = u[k]
  const float g = PER_CLASS || !live ? 0.f : gscore[n];
  if constexpr (PER_CLASS) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) acc[k] = live ? gscore[(int64_t)k * HW + n] : 0.f;
  } else if (mode == 0) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {       // 1 - tanh^2 s = 4 E / (1 + E)^2 with E = e^(-2|s|): no cancellation where tanh s is within an ulp of 1
        const float e = expf(-2.0f * fabsf(acc[k])), d = 1.0f + e;
        acc[k] = -g * (4.0f * e / (d * d));
      }
  } else if (mode == 2) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k) acc[k] = -g;
  } else {
    float mx = acc[0], sum = 0.f;
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
      if (k < K) mx = fmaxf(mx, acc[k]);
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) {
        acc[k] = expf(acc[k] - mx);
        sum += acc[k];
      }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) acc[k] = -g * (acc[k] / sum);
  }
  if (part) {
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) sh_u[k * LDW + tid] = acc[k];
  }

  for (int q0 = 0; q0 < Q; q0 += QC) {
    const int qn = min(QC, Q - q0);
    // ---- phase 3
    if (gmask || !resident) {
#pragma unroll 2
      for (int j = 0; j < qn; ++j) {
        const int q = q0 + j;
        float s;
        if (resident) {
          s = sh_s[j * LDW + tid];
        } else {
          s = sigmoid_acc(mp[(int64_t)q * HW]);
          if (part) sh_s[j * LDW + tid] = s;
        }
        if (gmask) {
          const float* pq = prob + q * K;
          float d = 0.f;
#pragma unroll
          for (int k = 0; k < KMAX; ++k)
            if (k < K) d = fmaf(pq[k], acc[k], d);
          if (live) gmask[(int64_t)q * HW + n] = s * (1.0f - s) * d;
        }
      }
    }
    if (!part) continue;               // workgroup-uniform
    __syncthreads();
    // ---- phase 4: rows q0 .. q0 + qn of the tile's grad_p slice
    const int nkb = (K + 3) >> 2, nqb = (qn + 3) >> 2;
    float* slice = part + (int64_t)blockIdx.x * Q * K;
    for (int b = tid; b < nqb * nkb; b += TILE) {
      const int qb = b / nkb, kb = b - qb * nkb;
      const float *sr[4], *ur[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {      // rows past the edge alias the last valid row; their sums are not stored
        sr[i] = sh_s + min(qb * 4 + i, qn - 1) * LDW;
        ur[i] = sh_u + min(kb * 4 + i, K - 1) * LDW;
      }
      float c[4][4];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) c[i][j] = 0.f;
#pragma unroll 2
      for (int x = 0; x < TILE; x += 4) {
        f32x4 a[4], u[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[i] = *reinterpret_cast<const f32x4*>(sr[i] + x);
          u[i] = *reinterpret_cast<const f32x4*>(ur[i] + x);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) c[i][j] = fmaf(a[i][e], u[j][e], c[i][j]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (qb * 4 + i < qn && kb * 4 + j < K) slice[(int64_t)(q0 + qb * 4 + i) * K + kb * 4 + j] = c[i][j];
    }
    __syncthreads();                   // the next chunk overwrites sh_s
  }
}

// grad_p[i] = sum over tiles of part[tile][i]: lane column x owns element i, row y sums tiles y, y + 4, ... in ascending order, then ((0+1)+(2+3))
__global__ __launch_bounds__(256) void rba_reduce_bwd_sum_kernel(const float* __restrict__ part, float* __restrict__ gprob, int QK, int64_t tiles) {
  __shared__ float red[4][64];
  const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + x;
  float s = 0.f;
  if (i < QK) {
    const float* p = part + i;
#pragma unroll 4
    for (int64_t t = y; t < tiles; t += 4) s += p[t * QK];
  }
  red[y][x] = s;
  __syncthreads();
  if (y == 0 && i < QK) gprob[i] = (red[0][x] + red[1][x]) + (red[2][x] + red[3][x]);
}

int64_t tiles_of(int64_t HW) { return (HW + TILE - 1) / TILE; }

template <int KMAX, bool PER_CLASS>
int launch_bwd(const float* mask, const float* prob, const float* gscore, float* gmask, float* part, int Q, int K, int64_t HW, int mode,
               hipStream_t st) {
  const int QC = Q + K <= ROWS_64K ? Q : min(Q, max(16, ROWS_64K - K));
  const size_t shm = (size_t)(K + QC) * LDW * sizeof(float);
  // beyond 64 KiB (K > 108) the size varies with K: raise the kernel's dynamic-LDS cap once per instantiation and device to the LARGEST size
  // any legal call can ask for, (160 + 16) rows = 92 928 bytes, so that no later call depends on which one came first
  constexpr size_t SHM_MAX = (size_t)(160 + 16) * LDW * sizeof(float);
  if (shm > SHM_MAX) return (int)hipErrorInvalidValue;
  if (shm > 65536) {
    static size_t lds_enabled[64];
    if (const int rc = rba_dynamic_lds(rba_reduce_bwd_kernel<KMAX, PER_CLASS>, SHM_MAX, lds_enabled)) return rc;
  }
  hipLaunchKernelGGL((rba_reduce_bwd_kernel<KMAX, PER_CLASS>), dim3((unsigned)tiles_of(HW)), dim3(TILE), shm, st, mask, prob, gscore, gmask, part, Q, K, HW,
                     mode, QC);
  return rba_launch_status();
}

bool domain_ok(int Q, int K, int64_t HW) {
  // 32-bit q * K and slice offsets inside the kernels, one workgroup per tile
  return Q >= 1 && K >= 1 && K <= 160 && HW >= 1 && (int64_t)Q * K <= 0x7fffffffLL && tiles_of(HW) <= 0x7fffffffLL &&
         tiles_of(HW) <= INT64_MAX / 4 / ((int64_t)Q * K);
}

// the body of both entry points: `grad` is grad_score [HW] (PER_CLASS false) or grad_sem [K,HW] (true, where `score_mode` is not read)
template <bool PER_CLASS>
int reduce_bwd(const float* mask, const float* cls_prob, const float* grad, float* grad_mask, float* grad_prob, int Q, int K, int64_t HW, int score_mode,
               void* workspace, int64_t workspace_bytes, void* stream) {
  RBA_CHECK_ARG(domain_ok(Q, K, HW) && score_mode >= 0 && score_mode <= 2);
  RBA_CHECK_ARG(mask && cls_prob && grad && (grad_mask || grad_prob));
  const int64_t tiles = tiles_of(HW);
  float* part = nullptr;
  if (grad_prob) {
    RBA_CHECK_ARG(workspace && (((uintptr_t)workspace) & 3) == 0 && workspace_bytes >= tiles * Q * K * (int64_t)sizeof(float));
    part = reinterpret_cast<float*>(workspace);
  }
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  int e;
  if (K <= 20) e = launch_bwd<20, PER_CLASS>(mask, cls_prob, grad, grad_mask, part, Q, K, HW, score_mode, st);
  else if (K <= 32) e = launch_bwd<32, PER_CLASS>(mask, cls_prob, grad, grad_mask, part, Q, K, HW, score_mode, st);
  else if (K <= 80) e = launch_bwd<80, PER_CLASS>(mask, cls_prob, grad, grad_mask, part, Q, K, HW, score_mode, st);
  else e = launch_bwd<160, PER_CLASS>(mask, cls_prob, grad, grad_mask, part, Q, K, HW, score_mode, st);
  if (e != 0 || !grad_prob) return e;
  const int QK = Q * K;
  hipLaunchKernelGGL(rba_reduce_bwd_sum_kernel, dim3((unsigned)((QK + 63) / 64)), dim3(256), 0, st, part, grad_prob, QK, tiles);
  return rba_launch_status();
}

}  // namespace

extern "C" int rba_reduce_bwd_workspace_f32(int Q, int K, int64_t HW, int64_t* bytes) {
  RBA_CHECK_ARG(bytes && domain_ok(Q, K, HW));
  *bytes = tiles_of(HW) * Q * K * (int64_t)sizeof(float);
  return 0;
}

extern "C" int rba_reduce_bwd_f32(const float* mask, const float* cls_prob, const float* grad_score, float* grad_mask, float* grad_prob,
                                  int Q, int K, int64_t HW, int score_mode, void* workspace, int64_t workspace_bytes, void* stream) {
  return reduce_bwd<false>(mask, cls_prob, grad_score, grad_mask, grad_prob, Q, K, HW, score_mode, workspace, workspace_bytes, stream);
}

extern "C" int rba_sem_seg_bwd_f32(const float* mask, const float* cls_prob, const float* grad_sem, float* grad_mask, float* grad_prob,
                                   int Q, int K, int64_t HW, void* workspace, int64_t workspace_bytes, void* stream) {
  return reduce_bwd<true>(mask, cls_prob, grad_sem, grad_mask, grad_prob, Q, K, HW, 0, workspace, workspace_bytes, stream);
}
