// K13: the confusion matrix of closed-set segmentation evaluation (Detectron2's SemSegEvaluator.process: np.bincount((K + 1) * pred + gt) per image on
// the host, after copying the argmax map back).  Here: (int32 argmax map, uint8 | int64 label map) -> += into an int64 [(K+1), (K+1)] matrix on the
// device, rows = predictions, columns = ground truth, column K = ignored; nothing is read back and nothing synchronises.  docs/kernels/K13.md.
//
// One thread owns TILE = 16 consecutive pixels per step of a capped grid-stride loop (four 16-byte loads of predictions, one 16-byte load of uint8
// labels), turns each pixel into a key (pred * (K+1) + gt, or one of the two "bad" keys behind the matrix) and merges equal consecutive keys in registers:
// a segmentation map is spatially coherent, so a thread usually leaves its whole share with a handful of (key, count) runs, and only a run's end touches
// a histogram.  The run is carried across the loop's steps.
//   LDS form    (K <= K13_LDS_MAX_K): uint32 histograms in LDS, one private copy per wave while four copies fit; the workgroup adds its non-zero
//                counters to the matrix with 64-bit global atomics once, at its end.
//   global form (K >  K13_LDS_MAX_K): a run's end is one 64-bit global atomic on the matrix itself.
// Integer adds commute: every output is bitwise reproducible whatever the arrival order.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int K13_THREADS = 256;                       // four waves
constexpr int K13_WAVES = K13_THREADS / RBA_WAVE;
constexpr int K13_TILE = 16;                           // pixels per thread and step: one 16-byte load of uint8 labels
constexpr int K13_GRID_CAP = 512;                      // two workgroups per CU: what two histograms of the largest LDS-form K (64 KiB each) leave room for
constexpr int K13_LDS_WORDS = 16384;                   // the 64 KiB a kernel gets without asking for more
constexpr int K13_LUT_WORDS = 64;                      // the 256-entry label table, held in the same array
constexpr int K13_HIST_WORDS = K13_LDS_WORDS - K13_LUT_WORDS;
// THE threshold between the two forms: the largest K whose (K+1)^2 + 2 counters (the matrix and the two bad counters) fit in LDS once.
constexpr int K13_LDS_MAX_K = 126;
constexpr int k13_counters(int K) { return (K + 1) * (K + 1) + 2; }
static_assert(k13_counters(K13_LDS_MAX_K) <= K13_HIST_WORDS && k13_counters(K13_LDS_MAX_K + 1) > K13_HIST_WORDS, "K13_LDS_MAX_K is the LDS budget's");
// a workgroup's share of one launch stays below 2^32 pixels, so no uint32 counter (LDS or a thread's run length) can wrap
constexpr int64_t K13_MAX_PIXELS = 1LL << 40;
static_assert(K13_MAX_PIXELS / K13_GRID_CAP + K13_THREADS * K13_TILE + 32 < (1LL << 32), "uint32 counters cannot wrap");

struct Rule {                                          // the per-pixel rule's constants
  int K, ignore_label;
  uint32_t bad_key;                                    // (K+1)^2: bad label; bad_key + 1: bad prediction
};

// label -> column: through the table (0..255 only), ignore_label -> K; a negative result stands for "out of range"
template <bool LUT>
__device__ __forceinline__ int label_of(int64_t g, const Rule& r, const uint8_t* lut) {
  if (LUT) {
    if ((uint64_t)g > 255u) return -1;
    g = lut[(int)g];
  }
  if (r.ignore_label >= 0 && g == (int64_t)r.ignore_label) return r.K;
  return (uint64_t)g <= (uint64_t)r.K ? (int)g : -1;
}
__device__ __forceinline__ uint32_t key_of(int pred, int label, const Rule& r) {
  if (label < 0) return r.bad_key;                     // both out of range counts as a label
  if ((uint32_t)pred >= (uint32_t)r.K) return r.bad_key + 1u;
  return (uint32_t)pred * (uint32_t)(r.K + 1) + (uint32_t)label;
}

// where a finished run goes
struct LdsSink {
  uint32_t* hist;                                      // this wave's copy
  __device__ __forceinline__ void add(uint32_t key, uint32_t n, const Rule&) const { atomicAdd(&hist[key], n); }
};
struct GlobalSink {
  unsigned long long *conf, *bad;
  __device__ __forceinline__ void add(uint32_t key, uint32_t n, const Rule& r) const {
    atomicAdd(key < r.bad_key ? conf + key : bad + (key - r.bad_key), (unsigned long long)n);
  }
};

struct Run {                                           // the open run of equal consecutive keys
  uint32_t key = 0, n = 0;
  template <typename Sink>
  __device__ __forceinline__ void push(uint32_t k, const Sink& s, const Rule& r) {
    if (k == key) {
      ++n;
    } else {
      if (n) s.add(key, n, r);
      key = k;
      n = 1;
    }
  }
  template <typename Sink>
  __device__ __forceinline__ void close(const Sink& s, const Rule& r) {
    if (n) s.add(key, n, r);
    n = 0;
  }
};

// 16 labels of type GT from an address aligned to GA bytes, in loads of GA bytes (GA = 16: the vector loads; GA = sizeof(GT): element accesses)
template <typename GT, int GA>
__device__ __forceinline__ void load_labels(const GT* __restrict__ p, int64_t (&g)[K13_TILE]) {
  if constexpr (sizeof(GT) == 1 && GA == 16) {
    const rba_u32x4 v = *reinterpret_cast<const rba_u32x4*>(p);
#pragma unroll
    for (int i = 0; i < K13_TILE; ++i) g[i] = (v[i >> 2] >> (8 * (i & 3))) & 0xffu;
  } else if constexpr (sizeof(GT) == 8 && GA == 16) {
    typedef int64_t i64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int i = 0; i < K13_TILE / 2; ++i) {
      const i64x2 v = reinterpret_cast<const i64x2*>(p)[i];
      g[2 * i] = v.x;
      g[2 * i + 1] = v.y;
    }
  } else {
    // Element accesses that STAY element accesses: sixteen plain reads of p[i] are merged back into one 16-byte load by the compiler's load-store
    // vectoriser (the target tolerates unaligned global loads), on an address that is only GA-byte aligned.  The empty asm makes every index an
    // opaque value, so no two reads are provably adjacent and none can be merged: sixteen global loads of sizeof(GT) bytes each (the pointer
    // itself is left alone: it keeps its global address space).
    static_assert(GA == (int)sizeof(GT), "element accesses");
#pragma unroll
    for (int i = 0; i < K13_TILE; ++i) {
      int at = i;
      asm volatile("" : "+v"(at));
      g[i] = (int64_t)p[at];
    }
  }
}

// The body both forms share.  Pixels [0, head) and [tail, n) are taken one per thread with element accesses by workgroup 0 (at most 15 + 15 of them);
// [head, tail) is whole tiles whose predictions are 16-byte aligned and whose labels are GA-byte aligned.
template <typename GT, int GA, bool LUT, typename Sink>
__device__ __forceinline__ void accumulate(const int32_t* __restrict__ pred, const GT* __restrict__ gt, int64_t n, int64_t head, int64_t tiles,
                                           const Rule& r, const uint8_t* lut, const Sink& sink) {
  Run run;
  if (blockIdx.x == 0) {
    const int64_t tail = head + tiles * K13_TILE;
    const int64_t p = (int64_t)threadIdx.x < head ? (int64_t)threadIdx.x : tail + ((int64_t)threadIdx.x - head);
    if (p < n) run.push(key_of(pred[p], label_of<LUT>((int64_t)gt[p], r, lut), r), sink, r);
  }
  for (int64_t t = (int64_t)blockIdx.x * K13_THREADS + threadIdx.x; t < tiles; t += (int64_t)gridDim.x * K13_THREADS) {
    const int64_t p0 = head + t * K13_TILE;
    rba_u32x4 pv[K13_TILE / 4];
#pragma unroll
    for (int i = 0; i < K13_TILE / 4; ++i) pv[i] = reinterpret_cast<const rba_u32x4*>(pred + p0)[i];
    int64_t g[K13_TILE];
    load_labels<GT, GA>(gt + p0, g);
#pragma unroll
    for (int i = 0; i < K13_TILE; ++i) run.push(key_of((int)pv[i >> 2][i & 3], label_of<LUT>(g[i], r, lut), r), sink, r);
  }
  run.close(sink, r);
}

template <typename GT, int GA, bool LUT>
__global__ __launch_bounds__(K13_THREADS) void confusion_lds_kernel(const int32_t* __restrict__ pred, const GT* __restrict__ gt, int64_t n, int64_t head,
                                                                    int64_t tiles, Rule r, const uint8_t* __restrict__ lut_g, int copies,
                                                                    unsigned long long* __restrict__ conf, unsigned long long* __restrict__ bad) {
  extern __shared__ uint32_t lds[];                    // [copies][(K+1)^2 + 2] counters, then the 64 words of the label table: sized by the launch
  const int counters = k13_counters(r.K);
  uint32_t* lut_s = lds + copies * counters;
  for (int i = threadIdx.x; i < copies * counters; i += K13_THREADS) lds[i] = 0u;
  if (LUT && threadIdx.x < K13_LUT_WORDS)
    lut_s[threadIdx.x] = (uint32_t)lut_g[4 * threadIdx.x] | (uint32_t)lut_g[4 * threadIdx.x + 1] << 8 |
                         (uint32_t)lut_g[4 * threadIdx.x + 2] << 16 | (uint32_t)lut_g[4 * threadIdx.x + 3] << 24;
  __syncthreads();
  const LdsSink sink{lds + (copies > 1 ? (threadIdx.x / RBA_WAVE) * counters : 0)};
  accumulate<GT, GA, LUT>(pred, gt, n, head, tiles, r, reinterpret_cast<const uint8_t*>(lut_s), sink);
  __syncthreads();
  for (int i = threadIdx.x; i < counters; i += K13_THREADS) {
    uint32_t v = lds[i];
    for (int c = 1; c < copies; ++c) v += lds[c * counters + i];
    if (v) atomicAdd((uint32_t)i < r.bad_key ? conf + i : bad + (i - (int)r.bad_key), (unsigned long long)v);
  }
}

template <typename GT, int GA, bool LUT>
__global__ __launch_bounds__(K13_THREADS) void confusion_global_kernel(const int32_t* __restrict__ pred, const GT* __restrict__ gt, int64_t n,
                                                                       int64_t head, int64_t tiles, Rule r, const uint8_t* __restrict__ lut_g,
                                                                       unsigned long long* __restrict__ conf, unsigned long long* __restrict__ bad) {
  __shared__ uint32_t lut_s[K13_LUT_WORDS];
  if (LUT) {
    if (threadIdx.x < K13_LUT_WORDS)
      lut_s[threadIdx.x] = (uint32_t)lut_g[4 * threadIdx.x] | (uint32_t)lut_g[4 * threadIdx.x + 1] << 8 | (uint32_t)lut_g[4 * threadIdx.x + 2] << 16 |
                           (uint32_t)lut_g[4 * threadIdx.x + 3] << 24;
    __syncthreads();
  }
  accumulate<GT, GA, LUT>(pred, gt, n, head, tiles, r, reinterpret_cast<const uint8_t*>(lut_s), GlobalSink{conf, bad});
}

template <typename GT, int GA, bool LUT>
int launch(const int32_t* pred, const GT* gt, int64_t n, int64_t head, int64_t tiles, const Rule& r, const uint8_t* lut, int64_t* conf, int64_t* bad,
           hipStream_t st) {
  const int64_t wanted = (tiles + K13_THREADS - 1) / K13_THREADS;
  const unsigned grid = (unsigned)(wanted < 1 ? 1 : (wanted > K13_GRID_CAP ? K13_GRID_CAP : wanted));      // workgroup 0 also takes head and tail
  unsigned long long* c = reinterpret_cast<unsigned long long*>(conf);
  unsigned long long* b = reinterpret_cast<unsigned long long*>(bad);
  if (r.K <= K13_LDS_MAX_K) {
    const int copies = K13_WAVES * k13_counters(r.K) <= K13_HIST_WORDS ? K13_WAVES : 1;
    const size_t lds_bytes = sizeof(uint32_t) * (size_t)(copies * k13_counters(r.K) + K13_LUT_WORDS);      // <= 64 KiB: 7.1 KiB at K = 19
    hipLaunchKernelGGL((confusion_lds_kernel<GT, GA, LUT>), dim3(grid), dim3(K13_THREADS), lds_bytes, st, pred, gt, n, head, tiles, r, lut, copies, c, b);
  } else {
    hipLaunchKernelGGL((confusion_global_kernel<GT, GA, LUT>), dim3(grid), dim3(K13_THREADS), 0, st, pred, gt, n, head, tiles, r, lut, c, b);
  }
  return rba_launch_status();
}

template <typename GT>
int dispatch(const int32_t* pred, const GT* gt, int64_t n, const Rule& r, const uint8_t* lut, int64_t* conf, int64_t* bad, hipStream_t st) {
  // head: the fewest pixels after which the predictions are 16-byte aligned and, where the two pointers allow it at all, the labels too
  int64_t head = (4 - (int64_t)(((uintptr_t)pred >> 2) & 3)) & 3;
  bool vec = false;
  for (int k = 0; k < 4 && !vec; ++k)
    if ((((uintptr_t)(gt + head + 4 * k)) & 15) == 0) {
      head += 4 * k;
      vec = true;
    }
  if (head > n) head = n;
  const int64_t tiles = (n - head) / K13_TILE;
  if (vec) return lut ? launch<GT, 16, true>(pred, gt, n, head, tiles, r, lut, conf, bad, st) : launch<GT, 16, false>(pred, gt, n, head, tiles, r, lut, conf, bad, st);
  return lut ? launch<GT, (int)sizeof(GT), true>(pred, gt, n, head, tiles, r, lut, conf, bad, st)
             : launch<GT, (int)sizeof(GT), false>(pred, gt, n, head, tiles, r, lut, conf, bad, st);
}

}  // namespace

extern "C" int rba_confusion_accum(const int32_t* pred, const void* gt, int gt_bytes, int64_t n_pixels, int K, int ignore_label, const uint8_t* lut,
                                   int64_t* conf, int64_t* bad, void* stream) {
  RBA_CHECK_ARG(pred && gt && conf && bad && (gt_bytes == 1 || gt_bytes == 8) && n_pixels >= 1 && n_pixels <= K13_MAX_PIXELS && K >= 1 && K <= 255);
  RBA_CHECK_ARG((((uintptr_t)pred) & 3) == 0 && (((uintptr_t)gt) & (uintptr_t)(gt_bytes - 1)) == 0 && ((((uintptr_t)conf) | ((uintptr_t)bad)) & 7) == 0);
  const Rule r{K, ignore_label, (uint32_t)((K + 1) * (K + 1))};
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  if (gt_bytes == 1) return dispatch<uint8_t>(pred, (const uint8_t*)gt, n_pixels, r, lut, conf, bad, st);
  return dispatch<int64_t>(pred, (const int64_t*)gt, n_pixels, r, lut, conf, bad, st);
}
