// K17: MaskFormer.instance_inference (mask2former/maskformer_model.py:488-527) on the mask logits.  docs/kernels/K17.md.
//
// K17a  rba_instance_stats_f32 / rba_instance_stats_up4_f32: for every kept query q and every pixel with logit m > 0: count[q] += 1,
//       ssum[q] += sigmoid(m) * 2^32 (an integer, see below), box[q] = min / max of x and y.  The reference's `(mask_pred > 0).float()`, `.sigmoid()`,
//       their product and the two sums (:517-524) -- and BitMasks.get_bounding_boxes, which it leaves commented out as slow (:520) -- for every query of
//       the top-k in ONE pass over the kept planes.  The up4 form reads the quarter-resolution logits and interpolates on the fly (K1's up4 arithmetic).
// K17b  rba_instance_masks_{f32,u8} / rba_instance_masks_up4_{f32,u8}: out[n,p] = mask[qidx[n],p] > 0 (:503, :517), the result planes, written once.
//
// The sum of the sigmoids is a FIXED-POINT sum: a sigmoid of a positive logit is an fp32 value s in [~0.5, 1], whose ulp is at least 2^-25, so s * 2^31 is
// an integer below 2^32 that v_cvt_u32_f32 gives exactly.  Threads add these in 64 bits, the flush doubles the workgroup's sum (-> units of 2^-32) and adds it
// with one 64-bit integer atomic: ssum is the EXACT sum of the fp32 sigmoids, independent of arrival order and bitwise reproducible, with no float atomics
// and no partial-sum workspace.  count <= HW < 2^31 keeps it below 2^63.
//
// Nothing is allocated, synchronised or read back here; every entry point is capturable.  Plain C++, LDS atomics and vector global atomics.
#include <limits.h>
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int K17_THREADS = 256;                        // four waves
constexpr int K17_WAVES = K17_THREADS / RBA_WAVE;
constexpr int K17_MAX_Q = 255;                          // K16's limit: the kept list is built by thread q
constexpr int K17_SLOTS = 256;
constexpr int K17_GRID_CAP = 1024;                      // K16a's: four workgroups per CU
constexpr int K17B_GRID_CAP = 512;                      // per result plane
constexpr int K17B_MAX_N = 65535;                       // one grid row per result plane

struct StatLds {
  int q[K17_SLOTS];                                     // the kept queries, ascending
  uint32_t cnt[K17_SLOTS];                              // the workgroup's sums, indexed by position in the kept list
  unsigned long long ss[K17_SLOTS];                     // in units of 2^-31
  int box[4][K17_SLOTS];                                // xmin, ymin, xmax, ymax
  int wave_kept[K17_WAVES];
};

// The kept list (ascending q, K16a's merge_begin) and neutral sums -> number of kept queries.  Q <= 255 < K17_THREADS: thread t looks at query t.
__device__ __forceinline__ int stats_begin(StatLds& L, const uint8_t* __restrict__ keep, int Q) {
  const int t = threadIdx.x, lane = t & (RBA_WAVE - 1), wave = t / RBA_WAVE;
  for (int i = t; i < K17_SLOTS; i += K17_THREADS) {
    L.cnt[i] = 0u;
    L.ss[i] = 0ull;
    L.box[0][i] = L.box[1][i] = INT_MAX;
    L.box[2][i] = L.box[3][i] = -1;
  }
  const bool kept = t < Q && keep[t] != 0;
  const unsigned long long m = __ballot(kept);
  if (lane == 0) L.wave_kept[wave] = __popcll(m);
  __syncthreads();
  int at = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
  for (int w = 0; w < K17_WAVES; ++w) {
    if (w < wave) at += L.wave_kept[w];
    total += L.wave_kept[w];
  }
  if (kept) L.q[at] = t;
  __syncthreads();
  return total;
}

// One thread's sums for one kept query
struct StatAcc {
  uint32_t cnt = 0;
  unsigned long long ss = 0;
  int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
  __device__ __forceinline__ void add(float m, bool ok, int x, int y) {
    const bool pos = ok && m > 0.0f;                                   // a NaN logit is not > 0
    const uint32_t u = (uint32_t)(rba_sigmoid(m) * 2147483648.0f);     // exact: see the head of the file
    cnt += pos ? 1u : 0u;
    ss += pos ? u : 0u;
    x0 = pos && x < x0 ? x : x0;
    y0 = pos && y < y0 ? y : y0;
    x1 = pos && x > x1 ? x : x1;
    y1 = pos && y > y1 ? y : y1;
  }
  // four pixels of ONE row, columns x .. x + 3: the box moves once per call, by the first and the last positive pixel of the four
  __device__ __forceinline__ void add_row4(const float (&m)[4], const bool (&ok)[4], int x, int y) {
    uint32_t bits = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool pos = ok[i] && m[i] > 0.0f;
      const uint32_t u = (uint32_t)(rba_sigmoid(m[i]) * 2147483648.0f);
      ss += pos ? u : 0u;
      bits |= pos ? 1u << i : 0u;
    }
    if (bits) {
      cnt += (uint32_t)__popc(bits);
      x0 = min(x0, x + __ffs(bits) - 1);
      x1 = max(x1, x + 31 - __clz(bits));
      y0 = min(y0, y);
      y1 = max(y1, y);
    }
  }
};

// The wave's sums for kept query k -> the workgroup's row in LDS.  Every lane of the wave calls it.
__device__ __forceinline__ void stats_commit(StatLds& L, int k, StatAcc a) {
#pragma unroll
  for (int o = RBA_WAVE / 2; o > 0; o >>= 1) {
    a.cnt += __shfl_xor(a.cnt, o, RBA_WAVE);
    a.ss += __shfl_xor(a.ss, o, RBA_WAVE);
    a.x0 = min(a.x0, __shfl_xor(a.x0, o, RBA_WAVE));
    a.y0 = min(a.y0, __shfl_xor(a.y0, o, RBA_WAVE));
    a.x1 = max(a.x1, __shfl_xor(a.x1, o, RBA_WAVE));
    a.y1 = max(a.y1, __shfl_xor(a.y1, o, RBA_WAVE));
  }
  if ((threadIdx.x & (RBA_WAVE - 1)) == 0 && a.cnt) {
    atomicAdd(&L.cnt[k], a.cnt);
    atomicAdd(&L.ss[k], a.ss);
    atomicMin(&L.box[0][k], a.x0);
    atomicMin(&L.box[1][k], a.y0);
    atomicMax(&L.box[2][k], a.x1);
    atomicMax(&L.box[3][k], a.y1);
  }
}

// The workgroup's sums -> count / ssum / box, one flush per kept query that met a positive pixel
__device__ __forceinline__ void stats_end(StatLds& L, int nk, int32_t* __restrict__ count, unsigned long long* __restrict__ ssum,
                                          int32_t* __restrict__ box) {
  __syncthreads();
  for (int k = threadIdx.x; k < nk; k += K17_THREADS) {
    if (!L.cnt[k]) continue;
    const int q = L.q[k];
    atomicAdd(&count[q], (int)L.cnt[k]);
    atomicAdd(&ssum[q], L.ss[k] * 2ull);                               // 2^-31 -> 2^-32
    atomicMin(&box[4 * q + 0], L.box[0][k]);
    atomicMin(&box[4 * q + 1], L.box[1][k]);
    atomicMax(&box[4 * q + 2], L.box[2][k]);
    atomicMax(&box[4 * q + 3], L.box[3][k]);
  }
}

// Full-resolution form.  The kept queries are taken U at a time (the loads of all U planes are issued before the first is used; behind the end of the list
// the last plane is read again and dropped); for each such set the workgroup walks its pixels in a capped grid-stride loop with the sums in registers, so a
// wave reduces once per kept query, not once per step.  Pixels [head, head + VEC * groups) are taken VEC per thread -- VEC = 4: one 16-byte load per plane on
// a 16-byte aligned address (every plane starts at the same phase: HW % 4 == 0) -- and the at most 3 + 3 pixels in front of and behind them by workgroup 0,
// one per thread with element loads.  VEC = 1 (HW % 4 != 0: the planes' phases differ): element loads throughout, head = 0.
template <int VEC>
__global__ __launch_bounds__(K17_THREADS) void instance_stats_kernel(const float* __restrict__ mask, const uint8_t* __restrict__ keep,
                                                                     int32_t* __restrict__ count, unsigned long long* __restrict__ ssum,
                                                                     int32_t* __restrict__ box, int Q, int64_t HW, int W, int64_t head, int64_t groups) {
  constexpr int U = 4;
  __shared__ StatLds L;
  const int nk = stats_begin(L, keep, Q);
  const int64_t tail = head + groups * VEC;               // VEC = 1: head = 0 and tail = HW, nothing left
  const bool edges = blockIdx.x == 0 && (head > 0 || tail < HW);
  const int64_t te = threadIdx.x;
  const int64_t pe = te < head ? te : tail + (te - head);
  const bool edge_ok = edges && pe < HW;
  const int64_t pec = edge_ok ? pe : 0;
  const int ye = (int)((uint32_t)pec / (uint32_t)W), xe = (int)((uint32_t)pec - (uint32_t)ye * (uint32_t)W);
  for (int k0 = 0; k0 < nk; k0 += U) {
    const float* plane[U];
#pragma unroll
    for (int u = 0; u < U; ++u) plane[u] = mask + (int64_t)__builtin_amdgcn_readfirstlane(L.q[k0 + u < nk ? k0 + u : nk - 1]) * HW;
    StatAcc acc[U];
    for (int64_t g0 = (int64_t)blockIdx.x * K17_THREADS; g0 < groups; g0 += (int64_t)gridDim.x * K17_THREADS) {
      const int64_t g = g0 + threadIdx.x;
      const bool ok = g < groups;
      const int64_t p0 = head + (ok ? g : groups - 1) * VEC;
      int y = (int)((uint32_t)p0 / (uint32_t)W), x = (int)((uint32_t)p0 - (uint32_t)y * (uint32_t)W);      // p0 < 2^31
      int xs[VEC], ys[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        xs[i] = x;
        ys[i] = y;
        if (++x == W) {
          x = 0;
          ++y;
        }
      }
      float v[U][VEC];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (VEC == 4) {
          const f32x4 t = *reinterpret_cast<const f32x4*>(plane[u] + p0);
          v[u][0] = t.x; v[u][1] = t.y; v[u][2] = t.z; v[u][3] = t.w;
        } else {
          v[u][0] = plane[u][p0];
        }
      }
      if constexpr (VEC == 4) {
        if (ys[3] == ys[0]) {                               // the four pixels lie in one row (always, where W % 4 == 0 and the head is 0)
          const bool oks[4] = {ok, ok, ok, ok};
#pragma unroll
          for (int u = 0; u < U; ++u) acc[u].add_row4(v[u], oks, xs[0], ys[0]);
          continue;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int i = 0; i < VEC; ++i) acc[u].add(v[u][i], ok, xs[i], ys[i]);
    }
    if (edges) {
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u].add(plane[u][pec], edge_ok, xe, ye);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (k0 + u < nk) stats_commit(L, k0 + u, acc[u]);   // the same in every lane
  }
  stats_end(L, nk, count, ssum, box);
}

// The four x4-upsampled logits of output columns 4j .. 4j+3 of one output row (rba_reduce_up4_kernel's taps and expression, rba_reduce_kernels.h; the same
// lines as K16a's up4 form): a, b = the two source rows of the plane.
__device__ __forceinline__ void up4_quad(const float* __restrict__ a, const float* __restrict__ b, int jm, int j, int jp, const BilinearTap& ty,
                                         const BilinearTap (&tx)[4], float (&x)[4]) {
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
}

// x4 upsample fused in front: a thread owns output columns 4j .. 4j+3 of one output row of the cropped [crop_h, crop_w] window of the virtual [Q,4h,4w]
// map; (row, j) pairs are handed out in a capped grid-stride loop, per set of U kept queries as above.
__global__ __launch_bounds__(K17_THREADS) void instance_stats_up4_kernel(const float* __restrict__ low, const uint8_t* __restrict__ keep,
                                                                         int32_t* __restrict__ count, unsigned long long* __restrict__ ssum,
                                                                         int32_t* __restrict__ box, int Q, int h, int w, int crop_h, int crop_w,
                                                                         int wq /* ceil(crop_w / 4) */) {
  constexpr int U = 2;
  __shared__ StatLds L;
  const int nk = stats_begin(L, keep, Q);
  const int64_t total = (int64_t)crop_h * wq;
  const int64_t plane_size = (int64_t)h * w;
  for (int k0 = 0; k0 < nk; k0 += U) {
    const float* plane[U];
#pragma unroll
    for (int u = 0; u < U; ++u) plane[u] = low + (int64_t)__builtin_amdgcn_readfirstlane(L.q[k0 + u < nk ? k0 + u : nk - 1]) * plane_size;
    StatAcc acc[U];
    for (int64_t t0 = (int64_t)blockIdx.x * K17_THREADS; t0 < total; t0 += (int64_t)gridDim.x * K17_THREADS) {
      const int64_t t = t0 + threadIdx.x;
      const bool ok = t < total;
      const int64_t tc = ok ? t : total - 1;
      const int y = (int)((uint32_t)tc / (uint32_t)wq), j = (int)((uint32_t)tc - (uint32_t)y * (uint32_t)wq);       // total < 2^31
      const BilinearTap ty = bilinear_tap(y, 0.25f, h);
      BilinearTap tx[4];
      bool oks[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        tx[r] = bilinear_tap(4 * j + r, 0.25f, w);
        oks[r] = ok && 4 * j + r < crop_w;
      }
      const int jm = j > 0 ? j - 1 : 0, jp = j < w - 1 ? j + 1 : w - 1;
      const int64_t r0 = (int64_t)ty.i0 * w, r1 = (int64_t)ty.i1 * w;
      float v[U][4];
#pragma unroll
      for (int u = 0; u < U; ++u) up4_quad(plane[u] + r0, plane[u] + r1, jm, j, jp, ty, tx, v[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) acc[u].add_row4(v[u], oks, 4 * j, y);
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (k0 + u < nk) stats_commit(L, k0 + u, acc[u]);
  }
  stats_end(L, nk, count, ssum, box);
}

unsigned capped_grid(int64_t items, int cap) {
  const int64_t wanted = (items + K17_THREADS - 1) / K17_THREADS;
  return (unsigned)(wanted < 1 ? 1 : (wanted > cap ? cap : wanted));
}

// ---------------------------------------------------------------------------------------------------------------- K17b
// four results as one store: 16 bytes of float, 4 bytes of uint8
__device__ __forceinline__ void store4(float* at, const bool (&b)[4]) {
  *reinterpret_cast<f32x4*>(at) = (f32x4){b[0] ? 1.0f : 0.0f, b[1] ? 1.0f : 0.0f, b[2] ? 1.0f : 0.0f, b[3] ? 1.0f : 0.0f};
}
__device__ __forceinline__ void store4(uint8_t* at, const bool (&b)[4]) {
  *reinterpret_cast<uint32_t*>(at) = (b[0] ? 1u : 0u) | (b[1] ? 1u << 8 : 0u) | (b[2] ? 1u << 16 : 0u) | (b[3] ? 1u << 24 : 0u);
}

// Workgroup row n writes result plane n.  A write-bound stream: the plane's pixels [head, head + 4 groups) go four per thread as ONE store on an address
// aligned to four elements of T (head: the 0..3 elements in front of the first such address of THIS plane, so HW % 4 != 0 and an `out` that is 1-3
// elements off are served alike), read by one 16-byte load where the logits happen to share that phase and by four element loads where they do not; the
// at most 3 + 3 pixels beside them by workgroup column 0 with element accesses.  A qidx outside [0, Q) writes zeros.
template <typename T>
__global__ __launch_bounds__(K17_THREADS) void instance_masks_kernel(const float* __restrict__ mask, const int32_t* __restrict__ qidx, T* __restrict__ out,
                                                                     int Q, int64_t HW) {
  const int n = blockIdx.y;
  const int q = qidx[n];
  const bool known = (uint32_t)q < (uint32_t)Q;
  const float* __restrict__ m = mask + (int64_t)(known ? q : 0) * HW;
  T* __restrict__ o = out + (int64_t)n * HW;
  int64_t head = (int64_t)((4 - (((uintptr_t)o / sizeof(T)) & 3)) & 3);
  if (head > HW) head = HW;
  const int64_t groups = (HW - head) / 4;
  const bool wide_load = (((uintptr_t)(m + head)) & 15) == 0;
  for (int64_t g = (int64_t)blockIdx.x * K17_THREADS + threadIdx.x; g < groups; g += (int64_t)gridDim.x * K17_THREADS) {
    const int64_t p0 = head + g * 4;
    float v[4];
    if (wide_load) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(m + p0);
      v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) v[i] = m[p0 + i];
    }
    const bool b[4] = {known && v[0] > 0.0f, known && v[1] > 0.0f, known && v[2] > 0.0f, known && v[3] > 0.0f};
    store4(o + p0, b);
  }
  const int64_t tail = head + groups * 4;
  if (blockIdx.x == 0 && (head > 0 || tail < HW)) {
    const int64_t t = threadIdx.x;
    const int64_t p = t < head ? t : tail + (t - head);
    if (p < HW) o[p] = (T)(known && m[p] > 0.0f ? 1 : 0);
  }
}

// The same planes from the quarter-resolution logits: thread = output columns 4j .. 4j+3 of one row of result plane n; one store where `wide` (crop_w % 4 == 0
// and `out` aligned to four elements: then every row of every plane starts on such an address), element stores otherwise.
template <typename T>
__global__ __launch_bounds__(K17_THREADS) void instance_masks_up4_kernel(const float* __restrict__ low, const int32_t* __restrict__ qidx,
                                                                         T* __restrict__ out, int Q, int h, int w, int crop_h, int crop_w, int wq,
                                                                         int wide) {
  const int n = blockIdx.y;
  const int q = qidx[n];
  const bool known = (uint32_t)q < (uint32_t)Q;
  const float* __restrict__ plane = low + (int64_t)(known ? q : 0) * h * w;
  T* __restrict__ o = out + (int64_t)n * crop_h * crop_w;
  const int64_t total = (int64_t)crop_h * wq;
  for (int64_t t = (int64_t)blockIdx.x * K17_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * K17_THREADS) {
    const int y = (int)(t / wq), j = (int)(t - (int64_t)y * wq);
    const BilinearTap ty = bilinear_tap(y, 0.25f, h);
    BilinearTap tx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) tx[r] = bilinear_tap(4 * j + r, 0.25f, w);
    const int jm = j > 0 ? j - 1 : 0, jp = j < w - 1 ? j + 1 : w - 1;
    float v[4];
    up4_quad(plane + (int64_t)ty.i0 * w, plane + (int64_t)ty.i1 * w, jm, j, jp, ty, tx, v);
    const bool b[4] = {known && v[0] > 0.0f, known && v[1] > 0.0f, known && v[2] > 0.0f, known && v[3] > 0.0f};
    T* at = o + (int64_t)y * crop_w + 4 * j;
    if (wide) {
      store4(at, b);
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * j + r < crop_w) at[r] = (T)(b[r] ? 1 : 0);
    }
  }
}

template <typename T>
int launch_masks(const float* mask, const int32_t* qidx, T* out, int Q, int N, int64_t HW, void* stream) {
  RBA_CHECK_ARG(mask && qidx && out && Q >= 1 && N >= 1 && N <= K17B_MAX_N && HW >= 1 && HW < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)mask | (uintptr_t)qidx) & 3) == 0 && ((uintptr_t)out & (sizeof(T) - 1)) == 0);
  rba_begin();
  hipLaunchKernelGGL((instance_masks_kernel<T>), dim3(capped_grid(HW / 4, K17B_GRID_CAP), (unsigned)N), dim3(K17_THREADS), 0, (hipStream_t)stream, mask,
                     qidx, out, Q, HW);
  return rba_launch_status();
}

template <typename T>
int launch_masks_up4(const float* low, const int32_t* qidx, T* out, int Q, int N, int h, int w, int crop_h, int crop_w, void* stream) {
  RBA_CHECK_ARG(low && qidx && out && Q >= 1 && N >= 1 && N <= K17B_MAX_N && h >= 1 && w >= 1);
  RBA_CHECK_ARG(crop_h >= 1 && crop_w >= 1 && crop_h <= 4 * (int64_t)h && crop_w <= 4 * (int64_t)w && (int64_t)crop_h * crop_w < (1LL << 31) &&
                (int64_t)h * w < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)low | (uintptr_t)qidx) & 3) == 0 && ((uintptr_t)out & (sizeof(T) - 1)) == 0);
  rba_begin();
  const int wq = (crop_w + 3) / 4;
  const int wide = (crop_w & 3) == 0 && ((uintptr_t)out & (4 * sizeof(T) - 1)) == 0;
  hipLaunchKernelGGL((instance_masks_up4_kernel<T>), dim3(capped_grid((int64_t)crop_h * wq, K17B_GRID_CAP), (unsigned)N), dim3(K17_THREADS), 0,
                     (hipStream_t)stream, low, qidx, out, Q, h, w, crop_h, crop_w, wq, wide);
  return rba_launch_status();
}

}  // namespace

extern "C" int rba_instance_stats_f32(const float* mask, const uint8_t* keep, int32_t* count, int64_t* ssum, int32_t* box, int Q, int H, int W,
                                      void* stream) {
  RBA_CHECK_ARG(mask && keep && count && ssum && box && Q >= 1 && Q <= K17_MAX_Q && H >= 1 && W >= 1 && (int64_t)H * W < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)mask | (uintptr_t)count | (uintptr_t)box) & 3) == 0 && ((uintptr_t)ssum & 7) == 0);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const int64_t HW = (int64_t)H * W;
  unsigned long long* ss = reinterpret_cast<unsigned long long*>(ssum);
  if (HW % 4 == 0) {
    int64_t head = (4 - (int64_t)(((uintptr_t)mask >> 2) & 3)) & 3;            // pixels in front of the first 16-byte aligned one (the same in every plane)
    if (head > HW) head = HW;
    const int64_t groups = (HW - head) / 4;
    hipLaunchKernelGGL(instance_stats_kernel<4>, dim3(capped_grid(groups, K17_GRID_CAP)), dim3(K17_THREADS), 0, st, mask, keep, count, ss, box, Q, HW, W,
                       head, groups);
  } else {
    hipLaunchKernelGGL(instance_stats_kernel<1>, dim3(capped_grid(HW, K17_GRID_CAP)), dim3(K17_THREADS), 0, st, mask, keep, count, ss, box, Q, HW, W,
                       (int64_t)0, HW);
  }
  return rba_launch_status();
}

extern "C" int rba_instance_stats_up4_f32(const float* mask_lowres, const uint8_t* keep, int32_t* count, int64_t* ssum, int32_t* box, int Q, int h, int w,
                                          int crop_h, int crop_w, void* stream) {
  RBA_CHECK_ARG(mask_lowres && keep && count && ssum && box && Q >= 1 && Q <= K17_MAX_Q && h >= 1 && w >= 1);
  RBA_CHECK_ARG(crop_h >= 1 && crop_w >= 1 && crop_h <= 4 * (int64_t)h && crop_w <= 4 * (int64_t)w && (int64_t)crop_h * crop_w < (1LL << 31) &&
                (int64_t)h * w < (1LL << 31));
  RBA_CHECK_ARG((((uintptr_t)mask_lowres | (uintptr_t)count | (uintptr_t)box) & 3) == 0 && ((uintptr_t)ssum & 7) == 0);
  rba_begin();
  const int wq = (crop_w + 3) / 4;
  hipLaunchKernelGGL(instance_stats_up4_kernel, dim3(capped_grid((int64_t)crop_h * wq, K17_GRID_CAP)), dim3(K17_THREADS), 0, (hipStream_t)stream,
                     mask_lowres, keep, count, reinterpret_cast<unsigned long long*>(ssum), box, Q, h, w, crop_h, crop_w, wq);
  return rba_launch_status();
}

extern "C" int rba_instance_masks_f32(const float* mask, const int32_t* qidx, float* out, int Q, int N, int64_t HW, void* stream) {
  return launch_masks<float>(mask, qidx, out, Q, N, HW, stream);
}

extern "C" int rba_instance_masks_u8(const float* mask, const int32_t* qidx, uint8_t* out, int Q, int N, int64_t HW, void* stream) {
  return launch_masks<uint8_t>(mask, qidx, out, Q, N, HW, stream);
}

extern "C" int rba_instance_masks_up4_f32(const float* mask_lowres, const int32_t* qidx, float* out, int Q, int N, int h, int w, int crop_h, int crop_w,
                                          void* stream) {
  return launch_masks_up4<float>(mask_lowres, qidx, out, Q, N, h, w, crop_h, crop_w, stream);
}

extern "C" int rba_instance_masks_up4_u8(const float* mask_lowres, const int32_t* qidx, uint8_t* out, int Q, int N, int h, int w, int crop_h, int crop_w,
                                         void* stream) {
  return launch_masks_up4<uint8_t>(mask_lowres, qidx, out, Q, N, h, w, crop_h, crop_w, stream);
}
