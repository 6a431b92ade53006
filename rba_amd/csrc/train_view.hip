// K14: the training view of the COCO-mix fine-tune mapper (mask2former/data/dataset_mappers/mask_former_semantic_coco_mix_dataset_mapper.py over
// Detectron2's ResizeShortestEdge, RandomCrop, ColorAugSSDTransform and RandomFlip).  One launch per image writes the finished view -- image, sem_seg,
// outlier_mask and the label histogram of the crop -- from the source frame: the pasted frame, the resized frame and the intermediate of Pillow's two
// passes never exist in memory; only the crop's pixels are computed.  Every output is an integer and equals the host composition in every element.
// docs/kernels/K14.md.
//
// A workgroup owns a tile of 16 output rows x 64 output columns; one thread owns four consecutive output columns of one row and all three channels
// (the colour legs need the triple).  Pillow's horizontal pass of the tile's source rows is staged in LDS as rounded uint8 (neighbouring output rows
// share them); a tile whose source rows do not fit (K14_MAX_SROWS) computes each Hrow value where it is used (the unstaged form), as does an image
// without a vertical pass.  The paste of the out-of-distribution object is folded into the source fetch.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int K14_THREADS = 256;                       // four waves
constexpr int K14_WAVES = K14_THREADS / RBA_WAVE;
constexpr int K14_TILE_ROWS = 16;
constexpr int K14_TILE_COLS = 64;                      // 16 threads of four columns
constexpr int K14_QUADS = K14_TILE_COLS / 4;
constexpr int K14_MAX_SROWS = 40;                      // staged source rows: 16 output rows at scale 2 with ksize 5 need 36
constexpr int K14_STAGE_BYTES = 3 * K14_MAX_SROWS * K14_TILE_COLS;
constexpr int PRECISION_BITS = 32 - 8 - 2;             // Pillow's
static_assert(K14_THREADS == K14_TILE_ROWS * K14_QUADS, "one thread per row and column quad");

typedef int64_t i64x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int clip8(int v) {
  v >>= PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// mix_object folded into the fetch: (r, col) of the frame reads the object where it lies in the box and the object's mask says ood_label there
__device__ __forceinline__ bool pasted(const rba_train_view& a, int r, int col, int& at) {
  const unsigned dr = (unsigned)(r - a.py), dc = (unsigned)(col - a.px);
  if (dr < (unsigned)a.bh && dc < (unsigned)a.bw) {
    at = (int)(dr * (unsigned)a.bw + dc);
    return a.objmask[at] == (uint8_t)a.ood_label;
  }
  return false;
}

__device__ __forceinline__ void pixel3(const rba_train_view& a, int r, int col, int (&p)[3]) {
  int at;
  if (pasted(a, r, col, at)) {
    const int plane = a.bh * a.bw;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = a.obj[c * plane + at];
  } else {
    const int plane = a.h * a.w;
    at = r * a.w + col;
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = a.img[c * plane + at];
  }
}

// Pillow's horizontal pass of source row r at resized column X, all three channels (the pixel itself where the width does not change)
__device__ __forceinline__ void hrow3(const rba_train_view& a, int r, int X, int (&v)[3]) {
  if (a.new_w == a.w) {
    pixel3(a, r, X, v);
    return;
  }
  const int lo = a.bx[2 * X], n = a.bx[2 * X + 1];
  const int32_t* k = a.kx + (int64_t)X * a.ksize_x;
  int ss[3] = {1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1), 1 << (PRECISION_BITS - 1)};
  for (int j = 0; j < n; ++j) {
    int p[3];
    pixel3(a, r, lo + j, p);
    const int kj = k[j];
#pragma unroll
    for (int c = 0; c < 3; ++c) ss[c] += p[c] * kj;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = clip8(ss[c]);
}

// the labels' nearest source index along one axis: the table ATen's upsample_nearest itself gave the host (rba_amd.ops.nearest_index_tables), or the
// index itself on an axis whose size does not change; a value outside the axis is brought back into it
__device__ __forceinline__ int nearest(const int32_t* table, int dst, int n_in) {
  if (!table) return dst;
  const unsigned s = (unsigned)table[dst];
  return (int)(s < (unsigned)n_in ? s : (unsigned)(n_in - 1));
}

// ---------------------------------------------------------------------------------------------------------------- ColorAugSSDTransform, on BGR order
// Every product below is rounded to fp32 on its own before anything is added to it.  The library is built with -ffp-contract=fast, under which a
// multiply and the add or subtract behind it become one fused multiply-add (pragmas and the plain-operator __fmul_rn of the HIP headers included),
// and a fused result differs from the two-step one in truncated and rounded bytes: the empty asm makes the product an opaque value.
__device__ __forceinline__ float mul_rn(float a, float b) {
  float m = a * b;
  asm volatile("" : "+v"(m));
  return m;
}

// one fp32 multiply, rounded, then one fp32 add, rounded (never fused), clip, truncate
__device__ __forceinline__ int convert(int p, float alpha, float beta) {
  float v = mul_rn((float)p, alpha) + beta;
  v = v < 0.f ? 0.f : (v > 255.f ? 255.f : v);
  return (int)v;
}

__device__ __forceinline__ void bgr2hsv(int b, int g, int r, const int* sdiv, const int* hdiv, int& H, int& S, int& V) {
  const int v = max(b, max(g, r)), diff = v - min(b, min(g, r));
  S = (diff * sdiv[v] + 2048) >> 12;
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * hdiv[diff] + 2048) >> 12;
  H = h < 0 ? h + 180 : h;
  V = v;
}

__device__ __forceinline__ int round8(float x) {
  const float y = rintf(mul_rn(x, 255.f));
  return y < 0.f ? 0 : (y > 255.f ? 255 : (int)y);
}

__device__ __forceinline__ void hsv2bgr(int H, int S, int V, int& b, int& g, int& r) {
  const float s = mul_rn((float)S, 1.f / 255.f), v = mul_rn((float)V, 1.f / 255.f);
  float fb = v, fg = v, fr = v;
  if (S != 0) {
    float hh = mul_rn((float)H, 6.f / 180.f);
    if (hh < 0.f) hh = (hh + 6.f);
    if (hh >= 6.f) hh = (hh - 6.f);
    const float fl = floorf(hh);
    const int sector = (int)fl;
    const float f = (hh - fl);
    const float t0 = v;
    const float t1 = mul_rn(v, (1.f - s));
    const float t2 = mul_rn(v, (1.f - mul_rn(s, f)));
    const float t3 = mul_rn(v, (1.f - mul_rn(s, (1.f - f))));
    // (b, g, r) = t[{{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}}[sector]], as selects
    fb = sector == 0 || sector == 1 ? t1 : (sector == 2 ? t3 : (sector == 5 ? t2 : t0));
    fg = sector == 0 ? t3 : (sector == 1 || sector == 2 ? t0 : (sector == 3 ? t2 : t1));
    fr = sector == 0 || sector == 5 ? t0 : (sector == 1 ? t2 : (sector == 4 ? t3 : t1));
  }
  b = round8(fb);
  g = round8(fg);
  r = round8(fr);
}

__device__ __forceinline__ void color_legs(const rba_train_view_color& k, const int* sdiv, const int* hdiv, int& b, int& g, int& r) {
  if (k.brightness) {
    b = convert(b, 1.f, k.beta);
    g = convert(g, 1.f, k.beta);
    r = convert(r, 1.f, k.beta);
  }
#pragma unroll
  for (int leg = 0; leg < 3; ++leg) {
    // order set: contrast, saturation, hue; otherwise saturation, hue, contrast
    const int what = k.order ? leg : (leg + 1) % 3;                 // 0 contrast, 1 saturation, 2 hue
    if (what == 0) {
      if (k.contrast) {
        b = convert(b, k.contrast_alpha, 0.f);
        g = convert(g, k.contrast_alpha, 0.f);
        r = convert(r, k.contrast_alpha, 0.f);
      }
    } else if (what == 1 ? k.saturation : k.hue) {
      int H, S, V;
      bgr2hsv(b, g, r, sdiv, hdiv, H, S, V);
      if (what == 1) {
        S = convert(S, k.saturation_alpha, 0.f);
      } else {
        H = (H + k.hue_delta) % 180;
        if (H < 0) H += 180;
      }
      hsv2bgr(H, S, V, b, g, r);
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(K14_THREADS) void train_view_kernel(const rba_train_view a, const int col_tiles) {
  __shared__ uint32_t stage_words[K14_STAGE_BYTES / 4];               // [3][K14_MAX_SROWS][64] bytes: the horizontal pass of the tile's source rows
  __shared__ uint32_t hist_s[K14_WAVES * 256];                        // one histogram per wave
  __shared__ int hsv_div[512];                                        // sdiv, hdiv
  uint8_t* stage = reinterpret_cast<uint8_t*>(stage_words);
  const int tid = threadIdx.x;
  const int row_tile = (int)(blockIdx.x / (unsigned)col_tiles);
  const int yb = row_tile * K14_TILE_ROWS, xb = (int)(blockIdx.x - (unsigned)row_tile * (unsigned)col_tiles) * K14_TILE_COLS;
  const bool vert = a.new_h != a.h;
  const bool colour = a.color.enabled != 0;

  for (int i = tid; i < K14_WAVES * 256; i += K14_THREADS) hist_s[i] = 0u;
  if (colour && (a.color.saturation || a.color.hue)) {               // OpenCV's tables: cvRound of a double quotient
    hsv_div[tid] = tid ? (int)rint((double)(255 << 12) / (double)tid) : 0;
    hsv_div[256 + tid] = tid ? (int)rint((double)(180 << 12) / (6.0 * (double)tid)) : 0;
  }

  // the tile's share of the crop: rows [yb, yend) and columns [xb, xb + ncols)
  const int yend = min(yb + K14_TILE_ROWS, a.ch);
  const int ncols = min(K14_TILE_COLS, a.cw - xb);
  bool staged = false;
  int rbase = 0;
  if (vert && yb < a.ch && ncols > 0) {                               // workgroup-uniform
    rbase = a.by[2 * (a.y0 + yb)];
    const int srows = a.by[2 * (a.y0 + yend - 1)] + a.by[2 * (a.y0 + yend - 1) + 1] - rbase;
    staged = srows >= 0 && srows <= K14_MAX_SROWS;
    if (staged) {
      for (int i = tid; i < srows * K14_TILE_COLS; i += K14_THREADS) {
        const int sr = i / K14_TILE_COLS, t = i - sr * K14_TILE_COLS;
        if (t < ncols) {
          const int x = xb + t;
          int v[3];
          hrow3(a, rbase + sr, a.x0 + (a.flip ? a.cw - 1 - x : x), v);
#pragma unroll
          for (int c = 0; c < 3; ++c) stage[(c * K14_MAX_SROWS + sr) * K14_TILE_COLS + t] = (uint8_t)v[c];
        }
      }
    }
  }
  __syncthreads();

  const int y = yb + tid / K14_QUADS, tq = tid % K14_QUADS, x = xb + 4 * tq;
  if (y < a.pad_h && x < a.pad_w) {
    const bool row_in = y < a.ch;
    uint32_t word[3] = {0x80808080u, 0x80808080u, 0x80808080u};       // the image's pad value
    int64_t sem[4], outl[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) sem[q] = a.ignore_label, outl[q] = 0;
    if (row_in && x < a.cw) {
      const int Y = a.y0 + y;
      int px[4][3];
      if (vert) {
        const int lo = a.by[2 * Y], n = a.by[2 * Y + 1];
        const int32_t* k = a.ky + (int64_t)Y * a.ksize_y;
        int ss[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int c = 0; c < 3; ++c) ss[q][c] = 1 << (PRECISION_BITS - 1);
        if (staged) {
          // lo - rbase + i lies in [0, srows) for tables that grow with Y (Pillow's do); an index outside only reads other LDS bytes
          for (int i = 0; i < n; ++i) {
            const int ki = k[i];
            const unsigned sr = min((unsigned)(lo - rbase + i), (unsigned)(K14_MAX_SROWS - 1));
#pragma unroll
            for (int c = 0; c < 3; ++c) {
              const uint32_t p = stage_words[((c * K14_MAX_SROWS + (int)sr) * K14_TILE_COLS) / 4 + tq];
#pragma unroll
              for (int q = 0; q < 4; ++q) ss[q][c] += (int)((p >> (8 * q)) & 0xffu) * ki;
            }
          }
        } else {
          for (int i = 0; i < n; ++i) {
            const int ki = k[i];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const int xq = min(x + q, a.cw - 1);
              int v[3];
              hrow3(a, lo + i, a.x0 + (a.flip ? a.cw - 1 - xq : xq), v);
#pragma unroll
              for (int c = 0; c < 3; ++c) ss[q][c] += v[c] * ki;
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int c = 0; c < 3; ++c) px[q][c] = clip8(ss[q][c]);
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int xq = min(x + q, a.cw - 1);
          hrow3(a, Y, a.x0 + (a.flip ? a.cw - 1 - xq : xq), px[q]);
        }
      }
      if (colour) {
#pragma unroll
        for (int q = 0; q < 4; ++q) color_legs(a.color, hsv_div, hsv_div + 256, px[q][2], px[q][1], px[q][0]);      // channels are R, G, B
      }
      // labels: nearest source pixel of the pasted frame, through the table
      const int sy = nearest(a.ny, Y, a.h);
      uint32_t* hist_w = hist_s + (tid / RBA_WAVE) * 256;
      int run_label = -1;
      uint32_t run_n = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (x + q < a.cw) {
          const int xq = x + q;
          const int sx = nearest(a.nx, a.x0 + (a.flip ? a.cw - 1 - xq : xq), a.w);
          int at, l;
          if (pasted(a, sy, sx, at)) {
            l = a.ood_label;
          } else {
            l = a.lab[sy * a.w + sx];
            if (a.lut) l = a.lut[l];
          }
          sem[q] = l;
          outl[q] = l == a.ignore_label ? (int64_t)a.ignore_label : (l == a.ood_label ? 1 : 0);
          if (l == run_label) {
            ++run_n;
          } else {
            if (run_n) atomicAdd(&hist_w[run_label], run_n);
            run_label = l;
            run_n = 1;
          }
#pragma unroll
          for (int c = 0; c < 3; ++c) word[c] = (word[c] & ~(0xffu << (8 * q))) | ((uint32_t)px[q][c] << (8 * q));
        }
      }
      if (run_n) atomicAdd(&hist_w[run_label], run_n);
    }
    const int64_t at = (int64_t)y * a.pad_w + x;
    const int64_t plane = (int64_t)a.pad_h * a.pad_w;
    if (VEC) {                                                        // pad_w % 4 == 0 and cw % 4 == 0: a quad is whole, inside the crop or outside
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(a.image + c * plane + at) = word[c];
      i64x2* s2 = reinterpret_cast<i64x2*>(a.sem_seg + at);
      s2[0] = (i64x2){sem[0], sem[1]};
      s2[1] = (i64x2){sem[2], sem[3]};
      if (row_in && x < a.cw) {
        i64x2* o2 = reinterpret_cast<i64x2*>(a.outlier_mask + (int64_t)y * a.cw + x);
        o2[0] = (i64x2){outl[0], outl[1]};
        o2[1] = (i64x2){outl[2], outl[3]};
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (x + q < a.pad_w) {
#pragma unroll
          for (int c = 0; c < 3; ++c) a.image[c * plane + at + q] = (uint8_t)(word[c] >> (8 * q));
          a.sem_seg[at + q] = sem[q];
          if (row_in && x + q < a.cw) a.outlier_mask[(int64_t)y * a.cw + x + q] = outl[q];
        }
      }
    }
  }
  __syncthreads();
  {
    uint32_t v = 0;
#pragma unroll
    for (int wv = 0; wv < K14_WAVES; ++wv) v += hist_s[wv * 256 + tid];
    if (v) atomicAdd(a.hist + tid, (int)v);
  }
}

}  // namespace

extern "C" int rba_train_view_u8(const rba_train_view* view, void* stream) {
  RBA_CHECK_ARG(view != nullptr);
  const rba_train_view a = *view;
  RBA_CHECK_ARG(a.img && a.lab && a.image && a.sem_seg && a.outlier_mask && a.hist);
  RBA_CHECK_ARG(a.h >= 1 && a.w >= 1 && a.new_h >= 1 && a.new_w >= 1 && a.ch >= 1 && a.cw >= 1);
  RBA_CHECK_ARG(a.y0 >= 0 && a.x0 >= 0 && (int64_t)a.y0 + a.ch <= a.new_h && (int64_t)a.x0 + a.cw <= a.new_w);
  RBA_CHECK_ARG(a.pad_h >= a.ch && a.pad_w >= a.cw);
  RBA_CHECK_ARG(3LL * a.h * a.w < (1LL << 31) && 3LL * a.pad_h * a.pad_w < (1LL << 31) && (int64_t)a.new_h * a.new_w < (1LL << 40));
  RBA_CHECK_ARG(a.ood_label >= 0 && a.ood_label <= 255);
  RBA_CHECK_ARG(a.bh >= 0 && a.bw >= 0 && (a.bh == 0) == (a.bw == 0));
  if (a.bh > 0) {                                                     // the box lies inside the source, or is absent
    RBA_CHECK_ARG(a.obj && a.objmask && a.py >= 0 && a.px >= 0 && (int64_t)a.py + a.bh <= a.h && (int64_t)a.px + a.bw <= a.w);
  }
  RBA_CHECK_ARG(a.new_w == a.w || (a.kx && a.bx && a.nx && a.ksize_x >= 1));   // an axis whose size does not change has no pass
  RBA_CHECK_ARG(a.new_h == a.h || (a.ky && a.by && a.ny && a.ksize_y >= 1));
  RBA_CHECK_ARG((((uintptr_t)a.sem_seg | (uintptr_t)a.outlier_mask) & 7) == 0 && (((uintptr_t)a.hist) & 3) == 0);
  const int col_tiles = (a.pad_w + K14_TILE_COLS - 1) / K14_TILE_COLS;
  const int64_t blocks = (int64_t)((a.pad_h + K14_TILE_ROWS - 1) / K14_TILE_ROWS) * col_tiles;
  RBA_CHECK_ARG(blocks <= 0x7fffffffLL);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const hipError_t e = hipMemsetAsync(a.hist, 0, 256 * sizeof(int32_t), st);                     // hist is owned: prior contents do not matter
  if (e != hipSuccess) return (int)e;
  const bool vec = (a.pad_w & 3) == 0 && (a.cw & 3) == 0 && (((uintptr_t)a.image) & 3) == 0 &&
                   ((((uintptr_t)a.sem_seg) | ((uintptr_t)a.outlier_mask)) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(train_view_kernel<true>, dim3((unsigned)blocks), dim3(K14_THREADS), 0, st, a, col_tiles);
  else
    hipLaunchKernelGGL(train_view_kernel<false>, dim3((unsigned)blocks), dim3(K14_THREADS), 0, st, a, col_tiles);
  return rba_launch_status();
}
