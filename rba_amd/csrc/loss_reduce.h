// The deterministic reduction of the fine-tune loss kernels -- K8's loss_finish_kernel (point_loss.hip), K9 (outlier_tail.hip), K10
// (dense_hybrid_loss.hip), K11 (pebal_loss.hip) -- written once.  A loss is NF float sums and NI integer counts over the label pixels:
//   partial kernel:  G = loss_groups(...) workgroups of 256 threads; thread `tid` of workgroup `wg` walks pixels wg 256 + tid + k G 256 in ascending order
//                    (the walk and its per-pixel arithmetic are the kernel's own), then loss_store_partial: the wave's xor tree, (r0 + r1) + (r2 + r3)
//                    over the four waves, and the group's record (sums, then counts as bit patterns) into the caller's workspace with plain stores;
//   finish kernel:   one workgroup, loss_finish: thread t adds the records t, t + 256, ... in ascending order, the same tree, and thread 0 hands the
//                    NF + NI totals to the loss's epilogue.
// No float atomics, no word of the workspace has to start from a known value, and every order is fixed: a loss is bitwise reproducible from launch to launch.
#pragma once
#include "common.h"

constexpr int LOSS_THREADS = 256, LOSS_WAVES = LOSS_THREADS / RBA_WAVE, LOSS_MAX_GROUPS = 2048;
static_assert(LOSS_WAVES == 4, "loss_block_reduce adds exactly four waves as (r0 + r1) + (r2 + r3): another count is another order, and other bits");

// the number of partial workgroups for `total` pixels, `per_thread` of them to a thread before the cap makes it more
inline int loss_groups(int64_t total, int per_thread) {
  const int64_t per_group = (int64_t)LOSS_THREADS * per_thread, g = (total + per_group - 1) / per_group;
  return (int)(g < LOSS_MAX_GROUPS ? g : LOSS_MAX_GROUPS);
}

template <int NF, int NI>
struct LossSums {          // `LossSums<NF, NI> a{};` starts every sum and count at 0
  float f[NF];
  int n[NI > 0 ? NI : 1];
};

// the sums and counts of a workgroup's 256 threads -> threads 0 .. NF + NI - 1 hold one each (the counts as bit patterns); every thread must call it
template <int NF, int NI>
__device__ __forceinline__ float loss_block_reduce(LossSums<NF, NI> a) {
  __shared__ float red[LOSS_WAVES][NF + NI];
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NF; ++k) a.f[k] = wave_reduce_sum(a.f[k]);
#pragma unroll
  for (int k = 0; k < NI; ++k) a.n[k] = wave_reduce_sum_int(a.n[k]);
  if ((tid & (RBA_WAVE - 1)) == 0) {
    float* r = red[tid / RBA_WAVE];
#pragma unroll
    for (int k = 0; k < NF; ++k) r[k] = a.f[k];
#pragma unroll
    for (int k = 0; k < NI; ++k) r[NF + k] = __int_as_float(a.n[k]);
  }
  __syncthreads();
  float out = 0.f;
  if (tid < NF) out = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
  else if (tid < NF + NI)
    out = __int_as_float((__float_as_int(red[0][tid]) + __float_as_int(red[1][tid])) + (__float_as_int(red[2][tid]) + __float_as_int(red[3][tid])));
  return out;
}

// the end of a partial kernel: this workgroup's record, WORDS words apart from its neighbours'
template <int WORDS, int NF, int NI>
__device__ __forceinline__ void loss_store_partial(const LossSums<NF, NI>& a, float* __restrict__ ws) {
  static_assert(NF + NI <= WORDS, "a record holds every sum and count");
  const float v = loss_block_reduce(a);
  if (threadIdx.x < NF + NI) ws[WORDS * (int64_t)blockIdx.x + threadIdx.x] = v;
}

// the finish kernel: the G records -> totals, and `epilogue(totals)` in thread 0 alone
template <int WORDS, int NF, int NI, class Epilogue>
__device__ __forceinline__ void loss_finish(const float* __restrict__ ws, int G, Epilogue epilogue) {
  __shared__ float fin[NF + NI];
  const int tid = threadIdx.x;
  LossSums<NF, NI> a{};
  for (int g = tid; g < G; g += LOSS_THREADS) {
    const float* p = ws + WORDS * (int64_t)g;
#pragma unroll
    for (int k = 0; k < NF; ++k) a.f[k] += p[k];
#pragma unroll
    for (int k = 0; k < NI; ++k) a.n[k] += __float_as_int(p[NF + k]);
  }
  const float v = loss_block_reduce(a);
  if (tid < NF + NI) fin[tid] = v;
  __syncthreads();
  if (tid == 0) {
    LossSums<NF, NI> t{};
#pragma unroll
    for (int k = 0; k < NF; ++k) t.f[k] = fin[k];
#pragma unroll
    for (int k = 0; k < NI; ++k) t.n[k] = __float_as_int(fin[NF + k]);
    epilogue(t);
  }
}
