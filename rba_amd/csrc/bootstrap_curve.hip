// K18: the ROC and precision-recall curves of up to 64 image subsets (the trials of OODEvaluator.evaluate_ood_bootstrapped, support.py:305-351) from ONE
// globally sorted pixel list.  docs/kernels/K18.md.
//
// After the one descending sort of the pooled metric, the sorted order of any subset of images is a filter of the global order: a trial's curve is the
// global walk with the pixels of foreign images skipped.  Here a WAVE walks a chunk of the list in batches of 64 pixels and LANE t IS TRIAL t: the batch is
// loaded one pixel per lane and transposed (one ballot and one select per trial), after which lane t holds a 64-bit word with the batch's pixels
// of its trial.  Counting is then two population counts per lane, and labels and run ends (score[i] != score[i + 1]) are wave-uniform masks: the run ends
// are visited by a scalar loop, the step of all 64 curves is taken at once, and the fp64 division of the precision only by the lanes whose trial gained a
// positive in the run.
//
//   rba_subset_curves_totals   pass 1: per chunk and trial the member pixels' (tp, cnt), the same up to the chunk's last run end, and whether it has one
//   (torch)                    the prefix of those [T, 2, chunks] integers: `base` (counts in front of a chunk), `prev` (counts at the last run end in
//                              front of it -- a run may span any number of chunks), `ends` (inclusive)
//   rba_subset_curves_walk     pass 2: the curve steps at the run ends inside each chunk: auroc2 (exact, integer atomics), ap_part (float64 per chunk)
//   rba_subset_curves_finish   one workgroup per trial: ap = the chunks' partials added in chunk order; the first ROC point with tpr > 0.95 that
//                              survives scikit-learn's drop_intermediate, by a forward walk from the chunk the prefix places the crossing in
//   rba_labelled_tags_i32      the list's producer: (score, (image << 1) | label) of an image's pixels labelled 0 or 1, appended at a device cursor
//
// Counts are uint32 in registers (n < 2^31), int64 in memory.  No float atomics, no scratch, nothing allocated, synchronised or read back.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int K18_MIN_CHUNK = 64;
constexpr int K18_MAX_CHUNK = 1 << 20;
constexpr int K18_MAX_IMAGES = 1 << 30;
constexpr int K18_TAG_THREADS = 256;
constexpr int K18_TAG_WAVES = K18_TAG_THREADS / RBA_WAVE;
constexpr int K18_TAG_ITEMS = 4;                                   // pixels per thread
constexpr int K18_TAG_TILE = K18_TAG_THREADS * K18_TAG_ITEMS;

__device__ __forceinline__ uint32_t lane_value(uint32_t v, int j) { return (uint32_t)__builtin_amdgcn_readlane((int)v, j); }
__device__ __forceinline__ double lane_value(double v, int j) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned long long r = (unsigned long long)lane_value((uint32_t)u, j) | ((unsigned long long)lane_value((uint32_t)(u >> 32), j) << 32);
  return __builtin_bit_cast(double, r);
}

// 64 consecutive pixels of the sorted list, TRANSPOSED: the pixels are loaded one per lane (pixel i0 + lane in lane `lane`), then lane t receives the
// 64-bit word whose bit j says that pixel i0 + j belongs to trial t.  Labels and run ends are wave-uniform 64-bit masks.  Pixels at or past `lim` are
// no pixels (no membership, no run end).
struct Batch {
  unsigned long long mine;             // lane t: bit j = pixel i0 + j is a pixel of trial t
  unsigned long long positive;         // wave-uniform: bit j = pixel i0 + j is labelled 1
  unsigned long long ends;             // wave-uniform: bit j = pixel i0 + j is the last of its run of equal scores
};

// The membership word is fetched once per run of equal image index inside the batch (the lanes at the head of a run load it, a segmented copy
// hands it down the run): neighbours in score are often neighbours in the image.  An index outside the table has no membership.
// The transposition is one ballot per trial: lane = pixel tests bit t of its word, and lane t keeps the 64 answers.
__device__ __forceinline__ Batch load_batch(const float* __restrict__ score, const int32_t* __restrict__ tag, const uint64_t* __restrict__ member,
                                            int64_t n, int n_images, int T, int64_t i0, int64_t lim, int lane) {
  const int64_t i = i0 + lane;
  const bool ok = i < lim;
  const float sc = ok ? score[i] : 0.0f;
  const bool last = i + 1 >= n;
  const float nx = (ok && !last) ? score[i + 1] : sc;
  Batch b;
  b.ends = __ballot(ok && (last || sc != nx));
  const uint32_t tg = ok ? (uint32_t)tag[i] : 0u;
  b.positive = __ballot(ok && (tg & 1u));
  const uint32_t img = tg >> 1;
  const uint32_t before = (uint32_t)__shfl_up((int)img, 1, RBA_WAVE);
  const bool head = ok && (lane == 0 || img != before);
  unsigned long long m = (head && img < (uint32_t)n_images) ? member[img] : 0ull;
  int have = (head || !ok) ? 1 : 0;
#pragma unroll
  for (int d = 1; d < RBA_WAVE; d <<= 1) {                            // before step d every lane less than d behind its head has the word
    const unsigned long long om = __shfl_up(m, d, RBA_WAVE);
    const int oh = __shfl_up(have, d, RBA_WAVE);
    if (!have && lane >= d) {
      m = om;
      have = oh;
    }
  }
  const uint32_t m_lo = (uint32_t)m, m_hi = (uint32_t)(m >> 32);
  b.mine = 0ull;
  for (int t = 0; t < (T < 32 ? T : 32); ++t) {
    const unsigned long long answers = __ballot((m_lo >> t) & 1u);
    b.mine = lane == t ? answers : b.mine;
  }
  for (int t = 32; t < T; ++t) {
    const unsigned long long answers = __ballot((m_hi >> (t - 32)) & 1u);
    b.mine = lane == t ? answers : b.mine;
  }
  return b;
}

// The per-chunk integers are laid out [T][2][chunks] -- (tp, cnt) planes of each trial with the chunk index innermost, so that their prefix over chunks
// is a scan along the contiguous dimension: element (t, 0, c); the cnt plane is `chunks` further on.
__device__ __forceinline__ int64_t k18_at(int t, int64_t chunks, int64_t c) { return (int64_t)t * 2 * chunks + c; }

__device__ __forceinline__ unsigned long long bits_upto(int j) { return j >= 63 ? ~0ull : (1ull << (j + 1)) - 1ull; }

// Passes 1 and 2 share the batches: lane = trial.  Pass 1 needs two population counts per batch (and two more up to the batch's last run end);
// pass 2 visits the run ends of the batch, a wave-uniform loop, and takes the step of all 64 curves there.
template <bool WALK>
__global__ __launch_bounds__(RBA_WAVE) void k18_chunk_kernel(const float* __restrict__ score, const int32_t* __restrict__ tag,
                                                             const uint64_t* __restrict__ member, int64_t n, int n_images, int T, int chunk,
                                                             int32_t* __restrict__ totals, int32_t* __restrict__ upto_end, int32_t* __restrict__ has_end,
                                                             const int64_t* __restrict__ base, const int64_t* __restrict__ prev,
                                                             unsigned long long* __restrict__ auroc2, double* __restrict__ ap_part) {
  const int lane = threadIdx.x;
  const int64_t c = blockIdx.x, chunks = gridDim.x;
  const int64_t begin = c * chunk, lim = begin + chunk < n ? begin + chunk : n;
  const bool mine = lane < T;
  uint32_t tp = 0, cnt = 0;            // the trial's counts in front of the batch
  uint32_t ptp = 0, pcnt = 0;          // WALK: at the last run end; totals: at the chunk's last run end
  int any_end = 0;
  unsigned long long au = 0;
  double ap = 0.0;
  if (WALK && mine) {
    const int64_t at = k18_at(lane, chunks, c);
    tp = (uint32_t)base[at], cnt = (uint32_t)base[at + chunks];
    ptp = (uint32_t)prev[at], pcnt = (uint32_t)prev[at + chunks];
  }
  for (int64_t i0 = begin; i0 < lim; i0 += RBA_WAVE) {
    const Batch b = load_batch(score, tag, member, n, n_images, T, i0, lim, lane);
    const unsigned long long pos = b.mine & b.positive;
    if (WALK) {
      for (unsigned long long e = b.ends; e; e &= e - 1ull) {
        const unsigned long long upto = bits_upto(__builtin_ctzll(e));
        const uint32_t ntp = tp + (uint32_t)__popcll(pos & upto), ncnt = cnt + (uint32_t)__popcll(b.mine & upto);
        const uint32_t dtp = ntp - ptp, dfp = (ncnt - ntp) - (pcnt - ptp);
        au += (unsigned long long)dfp * (unsigned long long)(ptp + ntp);           // ptp + ntp < 2^32: n < 2^31
        if (dtp) ap += (double)dtp * ((double)ntp / (double)ncnt);
        ptp = ntp;
        pcnt = ncnt;
      }
    } else if (b.ends) {
      const unsigned long long upto = bits_upto(63 - __builtin_clzll(b.ends));
      ptp = tp + (uint32_t)__popcll(pos & upto);
      pcnt = cnt + (uint32_t)__popcll(b.mine & upto);
      any_end = 1;
    }
    tp += (uint32_t)__popcll(pos);
    cnt += (uint32_t)__popcll(b.mine);
  }
  if (!mine) return;
  if (WALK) {
    ap_part[(int64_t)lane * chunks + c] = ap;
    if (au) atomicAdd(auroc2 + lane, au);
  } else {
    const int64_t at = k18_at(lane, chunks, c);
    totals[at] = (int32_t)tp, totals[at + chunks] = (int32_t)cnt;
    upto_end[at] = (int32_t)ptp, upto_end[at + chunks] = (int32_t)pcnt;
    if (lane == 0) has_end[c] = any_end;
  }
}

// One trial per workgroup (one wave; here lane = pixel and everything after the ballots is wave-uniform).
__global__ __launch_bounds__(RBA_WAVE) void k18_finish_kernel(const float* __restrict__ score, const int32_t* __restrict__ tag,
                                                              const uint64_t* __restrict__ member, int64_t n, int n_images, int T, int chunk,
                                                              int64_t chunks, const int64_t* __restrict__ base, const int64_t* __restrict__ prev,
                                                              const int64_t* __restrict__ ends, const double* __restrict__ ap_part,
                                                              double* __restrict__ ap, int64_t* __restrict__ at95) {
  const int lane = threadIdx.x, t = blockIdx.x;
  // ---- average precision: the chunks' partial sums, strictly in chunk order
  double acc = 0.0;
  for (int64_t c0 = 0; c0 < chunks; c0 += RBA_WAVE) {
    const double v = c0 + lane < chunks ? ap_part[(int64_t)t * chunks + c0 + lane] : 0.0;
    const int valid = chunks - c0 < RBA_WAVE ? (int)(chunks - c0) : RBA_WAVE;
    for (int j = 0; j < valid; ++j) acc += lane_value(v, j);
  }
  // ---- the first kept ROC point with tpr > 0.95
  const int64_t P = ends[k18_at(t, chunks, chunks - 1)], total = ends[k18_at(t, chunks, chunks - 1) + chunks];
  int64_t ctp = 0, ccnt = 0;                      // the candidate point
  if (P > 0) {
    // K: the smallest count with (double)K / (double)P > 0.95, the comparison metrics.ood_metrics makes
    const double Pd = (double)P;
    int64_t K = (int64_t)(0.95 * Pd);
    K = K < 1 ? 1 : K;
    while (K > 1 && (double)(K - 1) / Pd > 0.95) --K;
    while (!((double)K / Pd > 0.95)) ++K;                               // ends at K = P at the latest
    int64_t lo = 0, hi = chunks - 1;                                    // the first chunk at whose end tp >= K
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (ends[k18_at(t, chunks, mid)] >= K) hi = mid; else lo = mid + 1;
    }
    const int64_t at = k18_at(t, chunks, lo);
    int64_t tp = base[at], cnt = base[at + chunks];                                // in front of the batch
    int64_t ptp = prev[at], pcnt = prev[at + chunks];                              // at the trial's last curve point
    int64_t sdtp = 0, sdcnt = 0;                                                   // the step into the candidate
    bool have = false, done = false;
    for (int64_t i0 = lo * chunk; i0 < n && !done; i0 += RBA_WAVE) {
      const int64_t i = i0 + lane;
      const bool ok = i < n;
      const float sc = ok ? score[i] : 0.0f;
      const bool last = i + 1 >= n;
      const float nx = (ok && !last) ? score[i + 1] : sc;
      const uint32_t tg = ok ? (uint32_t)tag[i] : 0u;
      const uint32_t img = tg >> 1;
      const bool listed = ok && img < (uint32_t)n_images;
      const bool in = listed && ((member[listed ? img : 0u] >> t) & 1ull);
      const unsigned long long mbits = __ballot(in), pbits = __ballot(in && (tg & 1u));
      unsigned long long e = __ballot(ok && (last || sc != nx));
      if (!(mbits == 0ull && tp == ptp && cnt == pcnt)) {               // (no member pixel and no open step: no curve point ends here)
        while (e && !done) {
          const int j = __builtin_ctzll(e);
          e &= e - 1ull;
          const unsigned long long upto = bits_upto(j);
          const int64_t ntp = tp + __popcll(pbits & upto), ncnt = cnt + __popcll(mbits & upto);
          if (ntp == ptp && ncnt == pcnt) continue;                      // a run without a pixel of the trial is no point of its curve
          const int64_t dtp = ntp - ptp, dcnt = ncnt - pcnt;
          if (have) {
            if (dtp != sdtp || dcnt != sdcnt) {
              done = true;                                               // the step out differs from the step in: the candidate stays
            } else {
              ctp = ntp, ccnt = ncnt;                                    // collinear: dropped, the next point with the same step in is the candidate
            }
          } else if (ntp >= K) {
            have = true;
            ctp = ntp, ccnt = ncnt, sdtp = dtp, sdcnt = dcnt;
            done = ptp == 0 && pcnt == 0;                                // the curve's first point always stays
          }
          done = done || (have && ctp == P && ccnt == total);            // and so does its last
          ptp = ntp, pcnt = ncnt;
        }
      }
      tp += __popcll(pbits);
      cnt += __popcll(mbits);
    }
  }
  if (lane == 0) {
    ap[t] = acc;
    at95[t * 2] = ccnt - ctp;
    at95[t * 2 + 1] = ctp;
  }
}

template <typename L>
__global__ __launch_bounds__(K18_TAG_THREADS) void k18_tags_kernel(const float* __restrict__ score, const L* __restrict__ labels, int64_t n,
                                                                   int image_index, float* __restrict__ out_score, int32_t* __restrict__ out_tag,
                                                                   int64_t capacity, unsigned long long* __restrict__ cursor) {
  __shared__ uint32_t wave_count[K18_TAG_WAVES];
  __shared__ unsigned long long block_at;
  const int t = threadIdx.x, lane = t & (RBA_WAVE - 1), wave = t / RBA_WAVE;
  const int64_t tile = (int64_t)blockIdx.x * K18_TAG_TILE;
  float s[K18_TAG_ITEMS];
  uint32_t lab[K18_TAG_ITEMS], rank[K18_TAG_ITEMS];
  bool keep[K18_TAG_ITEMS];
  uint32_t in_wave = 0;
#pragma unroll
  for (int k = 0; k < K18_TAG_ITEMS; ++k) {
    const int64_t i = tile + k * K18_TAG_THREADS + t;
    const bool ok = i < n;
    const L l = ok ? labels[i] : (L)255;
    s[k] = ok ? score[i] : 0.0f;
    keep[k] = l == (L)0 || l == (L)1;
    lab[k] = (uint32_t)l & 1u;
    const unsigned long long bal = __ballot(keep[k]);
    rank[k] = in_wave + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
    in_wave += (uint32_t)__popcll(bal);
  }
  if (lane == 0) wave_count[wave] = in_wave;
  __syncthreads();
  if (t == 0) {
    uint32_t total = 0;
#pragma unroll
    for (int w = 0; w < K18_TAG_WAVES; ++w) total += wave_count[w];
    unsigned long long at = 0;
    if (total) {
      at = atomicAdd(cursor, (unsigned long long)total);
      if (at + total > (unsigned long long)capacity) atomicOr(cursor + 1, 1ull);
    }
    block_at = at;
  }
  __syncthreads();
  unsigned long long at = block_at;
#pragma unroll
  for (int w = 0; w < K18_TAG_WAVES; ++w) at += w < wave ? wave_count[w] : 0u;
#pragma unroll
  for (int k = 0; k < K18_TAG_ITEMS; ++k) {
    const unsigned long long slot = at + rank[k];
    if (keep[k] && slot < (unsigned long long)capacity) {
      out_score[slot] = s[k];
      out_tag[slot] = (int32_t)(((uint32_t)image_index << 1) | lab[k]);
    }
  }
}

bool curves_ok(const void* score, const void* tag, const void* member, int64_t n, int n_images, int T, int chunk) {
  return score && tag && member && n >= 1 && n < (1ll << 31) && n_images >= 1 && n_images <= K18_MAX_IMAGES && T >= 1 && T <= 64 &&
         chunk >= K18_MIN_CHUNK && chunk <= K18_MAX_CHUNK && chunk % RBA_WAVE == 0;
}

}  // namespace

extern "C" int rba_subset_curves_totals(const float* score, const int32_t* tag, const uint64_t* member, int64_t n, int n_images, int T, int chunk,
                                        int32_t* totals, int32_t* upto_end, int32_t* has_end, void* stream) {
  RBA_CHECK_ARG(curves_ok(score, tag, member, n, n_images, T, chunk) && totals && upto_end && has_end);
  rba_begin();
  const int64_t chunks = (n + chunk - 1) / chunk;
  hipLaunchKernelGGL(k18_chunk_kernel<false>, dim3((unsigned)chunks), dim3(RBA_WAVE), 0, (hipStream_t)stream, score, tag, member, n, n_images, T, chunk,
                     totals, upto_end, has_end, (const int64_t*)nullptr, (const int64_t*)nullptr, (unsigned long long*)nullptr, (double*)nullptr);
  return rba_launch_status();
}

extern "C" int rba_subset_curves_walk(const float* score, const int32_t* tag, const uint64_t* member, int64_t n, int n_images, int T, int chunk,
                                      const int64_t* base, const int64_t* prev, int64_t* auroc2, double* ap_part, void* stream) {
  RBA_CHECK_ARG(curves_ok(score, tag, member, n, n_images, T, chunk) && base && prev && auroc2 && ap_part);
  rba_begin();
  const int64_t chunks = (n + chunk - 1) / chunk;
  hipLaunchKernelGGL(k18_chunk_kernel<true>, dim3((unsigned)chunks), dim3(RBA_WAVE), 0, (hipStream_t)stream, score, tag, member, n, n_images, T, chunk,
                     (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, base, prev, (unsigned long long*)auroc2, ap_part);
  return rba_launch_status();
}

extern "C" int rba_subset_curves_finish(const float* score, const int32_t* tag, const uint64_t* member, int64_t n, int n_images, int T, int chunk,
                                        const int64_t* base, const int64_t* prev, const int64_t* ends, const double* ap_part, double* ap,
                                        int64_t* at95, void* stream) {
  RBA_CHECK_ARG(curves_ok(score, tag, member, n, n_images, T, chunk) && base && prev && ends && ap_part && ap && at95);
  rba_begin();
  const int64_t chunks = (n + chunk - 1) / chunk;
  hipLaunchKernelGGL(k18_finish_kernel, dim3((unsigned)T), dim3(RBA_WAVE), 0, (hipStream_t)stream, score, tag, member, n, n_images, T, chunk, chunks,
                     base, prev, ends, ap_part, ap, at95);
  return rba_launch_status();
}

extern "C" int rba_labelled_tags_i32(const float* score, const void* labels, int label_bytes, int64_t n, int image_index, float* out_score,
                                     int32_t* out_tag, int64_t capacity, int64_t* cursor, void* stream) {
  RBA_CHECK_ARG(score && labels && out_score && out_tag && cursor && (label_bytes == 1 || label_bytes == 8) && n >= 1 && n < (1ll << 31) &&
                image_index >= 0 && image_index < K18_MAX_IMAGES && capacity >= 0);
  rba_begin();
  const unsigned grid = (unsigned)((n + K18_TAG_TILE - 1) / K18_TAG_TILE);
  if (label_bytes == 1)
    hipLaunchKernelGGL(k18_tags_kernel<uint8_t>, dim3(grid), dim3(K18_TAG_THREADS), 0, (hipStream_t)stream, score, (const uint8_t*)labels, n,
                       image_index, out_score, out_tag, capacity, (unsigned long long*)cursor);
  else
    hipLaunchKernelGGL(k18_tags_kernel<int64_t>, dim3(grid), dim3(K18_TAG_THREADS), 0, (hipStream_t)stream, score, (const int64_t*)labels, n,
                       image_index, out_score, out_tag, capacity, (unsigned long long*)cursor);
  return rba_launch_status();
}
