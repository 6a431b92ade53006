// K16: the closed-set panoptic merge of MaskFormer.panoptic_inference (mask2former/maskformer_model.py:394-452) and the segment-pair histogram of the
// open-set PQ evaluation (mask2former/evaluation/evaluation.py:152-159).  docs/kernels/K16.md.
//
// K16a  rba_panoptic_merge_f32 / rba_panoptic_merge_up4_f32: per pixel, over the kept queries in ascending q, s = sigmoid(mask[q,p]), v = score[q] * s;
//       best = the first q that attains the largest v; winner[p] = best where sigmoid(mask[best,p]) >= 0.5, else 0xFF; counts[0][q] = pixels q won,
//       counts[1][q] = pixels with sigmoid(mask[q,p]) >= 0.5, counts[2][q] = pixels q won and is >= 0.5 on.  The reference's per-query
//       `cur_mask_ids == k`, `cur_masks[k] >= 0.5` and their conjunction (:420-427) for every kept k in ONE pass over the mask planes: no sigmoid plane,
//       no product plane, no argmax plane, and the 3 Q numbers the host loop needs come back in one copy.  The up4 form reads the quarter-resolution
//       logits and interpolates on the fly (K1's up4 arithmetic), so the full-resolution planes need not exist either.
// K16b  rba_panoptic_assign_i32: panoptic[p] = seg_of_query[winner[p]] (0 for 0xFF) -- the reference's `panoptic_seg[mask] = id` writes, which touch
//       disjoint pixels, as one gather.
// K16c  rba_segment_pairs_accum: counts[gt[p] * P + pred[p]] += 1 on dense segment ids, K13's design (docs/kernels/K13.md) on two int32 maps.
//
// Every counter is an integer added with integer atomics: all outputs are bitwise reproducible whatever the arrival order.  Nothing is allocated,
// synchronised or read back here; every entry point is capturable.  Plain C++, LDS atomics and vector global atomics.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int K16_THREADS = 256;                        // four waves
constexpr int K16_WAVES = K16_THREADS / RBA_WAVE;
constexpr int K16_MAX_Q = 255;                          // 0xFF is the "nobody" byte of `winner`
constexpr int K16_SLOTS = 256;                          // LDS slots per counter row (>= K16_MAX_Q)
constexpr int K16_GRID_CAP = 1024;                      // four workgroups per CU: 16 waves with four 16-byte loads in flight each
constexpr uint32_t K16_NOBODY = 0xFFu;

struct MergeLds {
  int q[K16_SLOTS];                                     // the kept queries, ascending
  float score[K16_SLOTS];
  uint32_t cnt[K16_WAVES][3][K16_SLOTS];                // per wave: won / own >= 0.5 area / intersection, indexed by position in the kept list
  int wave_kept[K16_WAVES];
};

// The kept list (ascending q) and zeroed counters -> number of kept queries.  Q <= 255 < K16_THREADS: thread t looks at query t.
__device__ __forceinline__ int merge_begin(MergeLds& L, const float* __restrict__ score, const uint8_t* __restrict__ keep, int Q) {
  const int t = threadIdx.x, lane = t & (RBA_WAVE - 1), wave = t / RBA_WAVE;
  for (int i = t; i < K16_WAVES * 3 * K16_SLOTS; i += K16_THREADS) (&L.cnt[0][0][0])[i] = 0u;
  const bool kept = t < Q && keep[t] != 0;
  const unsigned long long m = __ballot(kept);
  if (lane == 0) L.wave_kept[wave] = __popcll(m);
  __syncthreads();
  int at = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
  for (int w = 0; w < K16_WAVES; ++w) {
    if (w < wave) at += L.wave_kept[w];
    total += L.wave_kept[w];
  }
  if (kept) {
    L.q[at] = t;
    L.score[at] = score[t];
  }
  __syncthreads();
  return total;
}

// The workgroup's counters -> counts [3,Q], non-zero ones only
__device__ __forceinline__ void merge_end(MergeLds& L, int nk, int Q, int32_t* __restrict__ counts) {
  __syncthreads();
  for (int k = threadIdx.x; k < nk; k += K16_THREADS) {
    const int q = L.q[k];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t v = 0;
#pragma unroll
      for (int w = 0; w < K16_WAVES; ++w) v += L.cnt[w][c][k];
      if (v) atomicAdd(&counts[c * Q + q], (int)v);
    }
  }
}

// The per-pixel body on N pixels of one thread.  `load(q, x)` gives the N logits of query q; `valid[i]` masks pixels that do not exist (their loads are
// made on clamped addresses and their results dropped).  Every lane of the wave runs every step: the ballots count whole waves.
template <int N, int U, typename Load>
__device__ __forceinline__ void merge_pixels(MergeLds& L, int nk, const bool (&valid)[N], const Load& load, uint32_t (&win)[N]) {
  const int lane = threadIdx.x & (RBA_WAVE - 1), wave = threadIdx.x / RBA_WAVE;
  float bv[N];
  int bk[N];
  bool bsolid[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    bv[i] = -INFINITY;
    bk[i] = -1;
    bsolid[i] = false;
  }
  // U kept queries per step, unrolled by hand (the ballots are convergent: the compiler does not unroll a loop of run-time length around them): the
  // loads of all U planes are issued before the first is used; behind the end of the list the last plane is loaded again and dropped.
  for (int k0 = 0; k0 < nk; k0 += U) {
    float x[U][N];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int ku = k0 + u < nk ? k0 + u : nk - 1;
      load(__builtin_amdgcn_readfirstlane(L.q[ku]), x[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + u;
      if (k >= nk) break;                               // the same in every lane
      const float sc = L.score[k];
      int own = 0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const float s = rba_sigmoid(x[u][i]);
        const float v = sc * s;
        const bool solid = valid[i] && s >= 0.5f;
        own += __popcll(__ballot(solid));
        if (v > bv[i]) {                                // strict: the first q that attains the maximum stays
          bv[i] = v;
          bk[i] = k;
          bsolid[i] = solid;
        }
      }
      if (lane == 0 && own) L.cnt[wave][1][k] += (uint32_t)own;    // this wave's row: lane 0 is its only writer
    }
  }
  // won / intersection: equal consecutive winners of the thread are merged before they reach LDS
  int run_k = -1;
  uint32_t run_won = 0, run_inter = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const bool has = valid[i] && bk[i] >= 0;
    win[i] = has && bsolid[i] ? (uint32_t)L.q[bk[i]] : K16_NOBODY;
    if (!has) continue;
    if (bk[i] != run_k) {
      if (run_won) {
        atomicAdd(&L.cnt[wave][0][run_k], run_won);
        if (run_inter) atomicAdd(&L.cnt[wave][2][run_k], run_inter);
      }
      run_k = bk[i];
      run_won = run_inter = 0;
    }
    ++run_won;
    run_inter += bsolid[i] ? 1u : 0u;
  }
  if (run_won) {
    atomicAdd(&L.cnt[wave][0][run_k], run_won);
    if (run_inter) atomicAdd(&L.cnt[wave][2][run_k], run_inter);
  }
}

// Full-resolution form.  Pixels [head, head + VEC * groups) are taken VEC per thread in a capped grid-stride loop -- VEC = 4: one 16-byte load per
// plane on a 16-byte aligned address (every plane starts at the same phase: HW % 4 == 0) -- and the at most 3 + 3 pixels in front of and behind them by
// workgroup 0, one per thread with element accesses.  VEC = 1 (HW % 4 != 0: the planes' phases differ): element accesses throughout, head = 0.
template <int VEC>
__global__ __launch_bounds__(K16_THREADS) void panoptic_merge_kernel(const float* __restrict__ mask, const float* __restrict__ score,
                                                                     const uint8_t* __restrict__ keep, uint8_t* __restrict__ winner,
                                                                     int32_t* __restrict__ counts, int Q, int64_t HW, int64_t head, int64_t groups,
                                                                     int winner_dword) {
  __shared__ MergeLds L;
  const int nk = merge_begin(L, score, keep, Q);
  for (int64_t g0 = (int64_t)blockIdx.x * K16_THREADS; g0 < groups; g0 += (int64_t)gridDim.x * K16_THREADS) {
    const int64_t g = g0 + threadIdx.x;
    const bool ok = g < groups;
    const int64_t p0 = head + (ok ? g : groups - 1) * VEC;
    bool valid[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) valid[i] = ok;
    uint32_t win[VEC];
    merge_pixels<VEC, 4>(L, nk, valid, [&](int q, float (&x)[VEC]) {
      const float* at = mask + (int64_t)q * HW + p0;
      if constexpr (VEC == 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(at);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
      } else {
        x[0] = at[0];
      }
    }, win);
    if (ok) {
      if (VEC == 4 && winner_dword) {
        *reinterpret_cast<uint32_t*>(winner + p0) = win[0] | win[1 % VEC] << 8 | win[2 % VEC] << 16 | win[3 % VEC] << 24;
      } else {
#pragma unroll
        for (int i = 0; i < VEC; ++i) winner[p0 + i] = (uint8_t)win[i];
      }
    }
  }
  const int64_t tail = head + groups * VEC;               // VEC = 1: head = 0 and tail = HW, nothing left
  if (blockIdx.x == 0 && (head > 0 || tail < HW)) {
    const int64_t t = threadIdx.x;
    const int64_t p = t < head ? t : tail + (t - head);
    const bool valid[1] = {p < HW};
    const int64_t pc = valid[0] ? p : 0;
    uint32_t win[1];
    merge_pixels<1, 4>(L, nk, valid, [&](int q, float (&x)[1]) { x[0] = mask[(int64_t)q * HW + pc]; }, win);
    if (valid[0]) winner[p] = (uint8_t)win[0];
  }
  merge_end(L, nk, Q, counts);
}

// x4 upsample fused in front (rba_reduce_up4_kernel's taps and arithmetic, rba_reduce_kernels.h): a thread owns output columns 4j .. 4j+3 of one output
// row of the cropped [crop_h, crop_w] window of the virtual [Q,4h,4w] map; (row, j) pairs are handed out in a capped grid-stride loop.
__global__ __launch_bounds__(K16_THREADS) void panoptic_merge_up4_kernel(const float* __restrict__ low, const float* __restrict__ score,
                                                                         const uint8_t* __restrict__ keep, uint8_t* __restrict__ winner,
                                                                         int32_t* __restrict__ counts, int Q, int h, int w, int crop_h, int crop_w,
                                                                         int wq /* ceil(crop_w / 4) */, int winner_dword) {
  __shared__ MergeLds L;
  const int nk = merge_begin(L, score, keep, Q);
  const int64_t total = (int64_t)crop_h * wq;
  const int64_t plane = (int64_t)h * w;
  for (int64_t t0 = (int64_t)blockIdx.x * K16_THREADS; t0 < total; t0 += (int64_t)gridDim.x * K16_THREADS) {
    const int64_t t = t0 + threadIdx.x;
    const bool ok = t < total;
    const int64_t tc = ok ? t : total - 1;
    const int y = (int)(tc / wq), j = (int)(tc - (int64_t)y * wq);
    const BilinearTap ty = bilinear_tap(y, 0.25f, h);
    BilinearTap tx[4];
    bool valid[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      tx[r] = bilinear_tap(4 * j + r, 0.25f, w);
      valid[r] = ok && 4 * j + r < crop_w;
    }
    const int jm = j > 0 ? j - 1 : 0, jp = j < w - 1 ? j + 1 : w - 1;
    const float* r0 = low + (int64_t)ty.i0 * w;
    const float* r1 = low + (int64_t)ty.i1 * w;
    uint32_t win[4];
    merge_pixels<4, 2>(L, nk, valid, [&](int q, float (&x)[4]) {
      const float* a = r0 + (int64_t)q * plane;
      const float* b = r1 + (int64_t)q * plane;
      const float a0 = a[jm], a1 = a[j], a2 = a[jp];
      const float b0 = b[jm], b1 = b[j], b2 = b[jp];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        // ATen order: l0h*(l0w*v00 + l1w*v01) + l1h*(l0w*v10 + l1w*v11); columns r < 2 -> (j-1, j), r >= 2 -> (j, j+1)
        const float v00 = r < 2 ? a0 : a1, v01 = r < 2 ? a1 : a2;
        const float v10 = r < 2 ? b0 : b1, v11 = r < 2 ? b1 : b2;
        const float top = tx[r].l0 * v00 + tx[r].l1 * v01;
        const float bot = tx[r].l0 * v10 + tx[r].l1 * v11;
        x[r] = ty.l0 * top + ty.l1 * bot;
      }
    }, win);
    if (ok) {
      const int64_t p0 = (int64_t)y * crop_w + 4 * j;
      if (winner_dword && valid[3]) {
        *reinterpret_cast<uint32_t*>(winner + p0) = win[0] | win[1] << 8 | win[2] << 16 | win[3] << 24;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (valid[r]) winner[p0 + r] = (uint8_t)win[r];
      }
    }
  }
  merge_end(L, nk, Q, counts);
}

__global__ __launch_bounds__(K16_THREADS) void panoptic_assign_kernel(const uint8_t* __restrict__ winner, const int32_t* __restrict__ seg_of_query,
                                                                      int32_t* __restrict__ panoptic, int Q, int64_t HW) {
  for (int64_t p = (int64_t)blockIdx.x * K16_THREADS + threadIdx.x; p < HW; p += (int64_t)gridDim.x * K16_THREADS) {
    const int q = winner[p];
    panoptic[p] = q < Q ? seg_of_query[q] : 0;            // 0xFF (and any byte >= Q) is nobody
  }
}

unsigned capped_grid(int64_t items, int cap) {
  const int64_t wanted = (items + K16_THREADS - 1) / K16_THREADS;
  return (unsigned)(wanted < 1 ? 1 : (wanted > cap ? cap : wanted));
}

// ---------------------------------------------------------------------------------------------------------------- K16c
constexpr int K16C_GRID_CAP = 512;                      // K13's: two workgroups per CU, what two 64 KiB histograms leave room for
constexpr int K16C_LDS_WORDS = 16384;                   // the 64 KiB a kernel gets without asking for more
constexpr int64_t K16C_MAX_PAIRS = 1LL << 24;
constexpr int64_t K16C_MAX_PIXELS = 1LL << 40;
// a workgroup's share of one launch stays below 2^32 pixels, so no uint32 counter (LDS or a thread's run length) can wrap
static_assert(K16C_MAX_PIXELS / K16C_GRID_CAP + K16_THREADS * 4 + 32 < (1LL << 32), "uint32 counters cannot wrap");

struct PairRule {
  int G, P;
  uint32_t bad_key;                                     // G * P: either id out of range
};
__device__ __forceinline__ uint32_t pair_key(int g, int p, const PairRule& r) {
  if ((uint32_t)g >= (uint32_t)r.G || (uint32_t)p >= (uint32_t)r.P) return r.bad_key;
  return (uint32_t)g * (uint32_t)r.P + (uint32_t)p;
}
struct PairLdsSink {
  uint32_t* hist;                                       // this wave's copy
  __device__ __forceinline__ void add(uint32_t key, uint32_t n, const PairRule&) const { atomicAdd(&hist[key], n); }
};
struct PairGlobalSink {
  unsigned long long *counts, *bad;
  __device__ __forceinline__ void add(uint32_t key, uint32_t n, const PairRule& r) const {
    atomicAdd(key < r.bad_key ? counts + key : bad, (unsigned long long)n);
  }
};
struct PairRun {                                        // the open run of equal keys (they need not be adjacent pixels)
  uint32_t key = 0, n = 0;
  template <typename Sink>
  __device__ __forceinline__ void push(uint32_t k, const Sink& s, const PairRule& r) {
    if (k == key) {
      ++n;
    } else {
      if (n) s.add(key, n, r);
      key = k;
      n = 1;
    }
  }
  template <typename Sink>
  __device__ __forceinline__ void close(const Sink& s, const PairRule& r) {
    if (n) s.add(key, n, r);
    n = 0;
  }
};

// VEC = 4: both maps share their 16-byte phase; a thread takes one 16-byte load of each per step, lane i at base + 16 i (whole lines per wave), pixels
// [0, head) and [head + 4 groups, n) go to workgroup 0 one per thread.  VEC = 1: the phases differ, one pixel per thread and step with element accesses
// (consecutive lanes, consecutive pixels), head = 0.  The run is carried across the steps.
template <int VEC, typename Sink>
__device__ __forceinline__ void pairs_accumulate(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, int64_t n, int64_t head, int64_t groups,
                                                 const PairRule& r, const Sink& sink) {
  PairRun run;
  const int64_t tail = head + groups * VEC;
  if (blockIdx.x == 0 && (head > 0 || tail < n)) {
    const int64_t t = threadIdx.x;
    const int64_t p = t < head ? t : tail + (t - head);
    if (p < n) run.push(pair_key(gt[p], pred[p], r), sink, r);
  }
#pragma unroll 4
  for (int64_t g = (int64_t)blockIdx.x * K16_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * K16_THREADS) {
    const int64_t p0 = head + g * VEC;
    if constexpr (VEC == 4) {
      const rba_u32x4 a = *reinterpret_cast<const rba_u32x4*>(gt + p0);
      const rba_u32x4 b = *reinterpret_cast<const rba_u32x4*>(pred + p0);
#pragma unroll
      for (int i = 0; i < 4; ++i) run.push(pair_key((int)a[i], (int)b[i], r), sink, r);
    } else {
      run.push(pair_key(gt[p0], pred[p0], r), sink, r);
    }
  }
  run.close(sink, r);
}

template <int VEC>
__global__ __launch_bounds__(K16_THREADS) void segment_pairs_lds_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, int64_t n,
                                                                        int64_t head, int64_t groups, PairRule r, int copies,
                                                                        unsigned long long* __restrict__ counts, unsigned long long* __restrict__ bad) {
  extern __shared__ uint32_t pair_lds[];                // [copies][G * P + 1] counters: sized by the launch
  const int counters = (int)r.bad_key + 1;
  for (int i = threadIdx.x; i < copies * counters; i += K16_THREADS) pair_lds[i] = 0u;
  __syncthreads();
  pairs_accumulate<VEC>(gt, pred, n, head, groups, r, PairLdsSink{pair_lds + (copies > 1 ? (threadIdx.x / RBA_WAVE) * counters : 0)});
  __syncthreads();
  for (int i = threadIdx.x; i < counters; i += K16_THREADS) {
    uint32_t v = pair_lds[i];
    for (int c = 1; c < copies; ++c) v += pair_lds[c * counters + i];
    if (v) atomicAdd((uint32_t)i < r.bad_key ? counts + i : bad, (unsigned long long)v);
  }
}

template <int VEC>
__global__ __launch_bounds__(K16_THREADS) void segment_pairs_global_kernel(const int32_t* __restrict__ gt, const int32_t* __restrict__ pred, int64_t n,
                                                                           int64_t head, int64_t groups, PairRule r,
                                                                           unsigned long long* __restrict__ counts, unsigned long long* __restrict__ bad) {
  pairs_accumulate<VEC>(gt, pred, n, head, groups, r, PairGlobalSink{counts, bad});
}

template <int VEC>
int launch_pairs(const int32_t* gt, const int32_t* pred, int64_t n, int64_t head, int64_t groups, const PairRule& r, int64_t* counts, int64_t* bad,
                 hipStream_t st) {
  const unsigned grid = capped_grid(groups, K16C_GRID_CAP);                     // workgroup 0 also takes head and tail
  unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
  unsigned long long* b = reinterpret_cast<unsigned long long*>(bad);
  const int64_t counters = (int64_t)r.bad_key + 1;
  if (counters <= K16C_LDS_WORDS) {
    const int copies = K16_WAVES * counters <= K16C_LDS_WORDS ? K16_WAVES : 1;
    hipLaunchKernelGGL((segment_pairs_lds_kernel<VEC>), dim3(grid), dim3(K16_THREADS), sizeof(uint32_t) * (size_t)(copies * counters), st, gt, pred, n,
                       head, groups, r, copies, c, b);
  } else {
    hipLaunchKernelGGL((segment_pairs_global_kernel<VEC>), dim3(grid), dim3(K16_THREADS), 0, st, gt, pred, n, head, groups, r, c, b);
  }
  return rba_launch_status();
}

}  // namespace

extern "C" int rba_panoptic_merge_f32(const float* mask, const float* score, const uint8_t* keep, uint8_t* winner, int32_t* counts, int Q, int64_t HW,
                                      void* stream) {
  RBA_CHECK_ARG(mask && score && keep && winner && counts && Q >= 1 && Q <= K16_MAX_Q && HW >= 1 && HW < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)mask | (uintptr_t)score | (uintptr_t)counts) & 3) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  if (HW % 4 == 0) {
    int64_t head = (4 - (int64_t)(((uintptr_t)mask >> 2) & 3)) & 3;            // pixels in front of the first 16-byte aligned one (the same in every plane)
    if (head > HW) head = HW;
    const int64_t groups = (HW - head) / 4;
    hipLaunchKernelGGL(panoptic_merge_kernel<4>, dim3(capped_grid(groups, K16_GRID_CAP)), dim3(K16_THREADS), 0, st, mask, score, keep, winner, counts, Q,
                       HW, head, groups, (int)((((uintptr_t)winner + (uintptr_t)head) & 3) == 0));
  } else {
    hipLaunchKernelGGL(panoptic_merge_kernel<1>, dim3(capped_grid(HW, K16_GRID_CAP)), dim3(K16_THREADS), 0, st, mask, score, keep, winner, counts, Q, HW,
                       (int64_t)0, HW, 0);
  }
  return rba_launch_status();
}

extern "C" int rba_panoptic_merge_up4_f32(const float* mask_lowres, const float* score, const uint8_t* keep, uint8_t* winner, int32_t* counts, int Q,
                                          int h, int w, int crop_h, int crop_w, void* stream) {
  RBA_CHECK_ARG(mask_lowres && score && keep && winner && counts && Q >= 1 && Q <= K16_MAX_Q && h >= 1 && w >= 1);
  RBA_CHECK_ARG(crop_h >= 1 && crop_w >= 1 && crop_h <= 4 * (int64_t)h && crop_w <= 4 * (int64_t)w && (int64_t)crop_h * crop_w < (1LL << 31) &&
                (int64_t)h * w < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)mask_lowres | (uintptr_t)score | (uintptr_t)counts) & 3) == 0);
  rba_begin();
  const int wq = (crop_w + 3) / 4;
  hipLaunchKernelGGL(panoptic_merge_up4_kernel, dim3(capped_grid((int64_t)crop_h * wq, K16_GRID_CAP)), dim3(K16_THREADS), 0, (hipStream_t)stream,
                     mask_lowres, score, keep, winner, counts, Q, h, w, crop_h, crop_w, wq, (int)((((uintptr_t)winner) & 3) == 0 && (crop_w & 3) == 0));
  return rba_launch_status();
}

extern "C" int rba_panoptic_assign_i32(const uint8_t* winner, const int32_t* seg_of_query, int32_t* panoptic, int Q, int64_t HW, void* stream) {
  RBA_CHECK_ARG(winner && seg_of_query && panoptic && Q >= 1 && Q <= K16_MAX_Q && HW >= 1 && HW < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)seg_of_query | (uintptr_t)panoptic) & 3) == 0);
  rba_begin();
  hipLaunchKernelGGL(panoptic_assign_kernel, dim3(capped_grid(HW, 2048)), dim3(K16_THREADS), 0, (hipStream_t)stream, winner, seg_of_query, panoptic, Q, HW);
  return rba_launch_status();
}

extern "C" int rba_segment_pairs_accum(const int32_t* gt, const int32_t* pred, int64_t n, int G, int P, int64_t* counts, int64_t* bad, void* stream) {
  RBA_CHECK_ARG(gt && pred && counts && bad && n >= 1 && n <= K16C_MAX_PIXELS && G >= 1 && P >= 1 && (int64_t)G * P <= K16C_MAX_PAIRS);
  RBA_CHECK_ARG((((uintptr_t)gt | (uintptr_t)pred) & 3) == 0 && ((((uintptr_t)counts) | ((uintptr_t)bad)) & 7) == 0);
  const PairRule r{G, P, (uint32_t)((int64_t)G * P)};
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  if (((((uintptr_t)gt) ^ ((uintptr_t)pred)) & 15) == 0) {                     // one head aligns both
    int64_t head = (4 - (int64_t)(((uintptr_t)gt >> 2) & 3)) & 3;
    if (head > n) head = n;
    return launch_pairs<4>(gt, pred, n, head, (n - head) / 4, r, counts, bad, st);
  }
  return launch_pairs<1>(gt, pred, n, 0, n, r, counts, bad, st);
}
