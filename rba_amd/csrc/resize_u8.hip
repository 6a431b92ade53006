// K12b: the view images of test-time augmentation.  Detectron2's ResizeTransform sends a uint8 image through Pillow's Image.resize(BILINEAR)
// (detectron2/data/transforms/transform.py), which is not ATen's bilinear: a triangle filter whose support widens when down-scaling, in 22-bit
// fixed point, the horizontal pass first and the vertical pass behind it with a rounded uint8 image in between (Pillow: src/libImaging/Resample.c,
// ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc).  The host builds the two coefficient tables in double, as Pillow does
// (rba_amd.ops.pil_bilinear_coeffs); the kernels here are the two integer passes on a CHW image:
//   out = clip8(((1 << 21) + sum_{j < n} kk[j] * pixel[lo + j]) >> 22)
// One thread owns four consecutive output columns of one row of one channel and stores them as one 32-bit word where the row offset allows.  The
// horizontal flip of a flipped view is folded into the store of the last pass.  docs/kernels/K12.md.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int PRECISION_BITS = 32 - 8 - 2;                                         // Pillow's

__device__ __forceinline__ uint32_t clip8(int v) {
  v >>= PRECISION_BITS;
  return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// four output bytes of row `row` (of the [rows, W] output plane) at columns x0 .. x0 + 3, or columns W - 1 - x0 .. W - 4 - x0 when flipped
template <bool VEC4>
__device__ __forceinline__ void store4(uint8_t* __restrict__ out, int64_t row, int W, int x0, int flip, const uint32_t (&b)[4]) {
  if (VEC4) {                                                                       // W % 4 == 0, 4-byte aligned plane: x0 + 3 < W, and W - 4 - x0 is a multiple of 4 too
    const uint32_t word = flip ? (b[3] | (b[2] << 8) | (b[1] << 16) | (b[0] << 24)) : (b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24));
    *reinterpret_cast<uint32_t*>(out + row * W + (flip ? W - 4 - x0 : x0)) = word;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (x0 + r < W) out[row * W + (flip ? W - 1 - (x0 + r) : x0 + r)] = (uint8_t)b[r];
  }
}

// in [C*h, w] -> out [C*h, W]: output column x sums bounds[2 x + 1] pixels from column bounds[2 x] on with the weights kk[x * ksize ..]
template <bool VEC4>
__global__ __launch_bounds__(256) void resize_h_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ kk,
                                                       const int32_t* __restrict__ bounds, int ksize, int w, int W, int wq, int xblocks, int flip) {
  const int64_t row = blockIdx.x / xblocks;                                        // channel * h + y
  const int xg = (int)(blockIdx.x - row * xblocks) * blockDim.x + threadIdx.x;
  if (xg >= wq) return;
  const int x0 = xg * 4;
  const uint8_t* src = in + row * w;
  uint32_t b[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int x = x0 + r < W ? x0 + r : W - 1;
    const int lo = bounds[2 * x], n = bounds[2 * x + 1];
    const int32_t* k = kk + (int64_t)x * ksize;
    int ss = 1 << (PRECISION_BITS - 1);
    for (int j = 0; j < n; ++j) ss += (int)src[lo + j] * k[j];
    b[r] = clip8(ss);
  }
  store4<VEC4>(out, row, W, x0, flip, b);
}

// in [C, h, W] -> out [C, H, W]: output row y sums bounds[2 y + 1] rows from row bounds[2 y] on
template <bool VEC4>
__global__ __launch_bounds__(256) void resize_v_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, const int32_t* __restrict__ kk,
                                                       const int32_t* __restrict__ bounds, int ksize, int h, int H, int W, int wq, int xblocks, int flip) {
  const int64_t row = blockIdx.x / xblocks;                                        // channel * H + y
  const int xg = (int)(blockIdx.x - row * xblocks) * blockDim.x + threadIdx.x;
  if (xg >= wq) return;
  const int x0 = xg * 4;
  const int c = (int)(row / H), y = (int)(row - (int64_t)c * H);
  const int lo = bounds[2 * y], n = bounds[2 * y + 1];                             // workgroup-uniform
  const int32_t* k = kk + (int64_t)y * ksize;
  const uint8_t* src = in + ((int64_t)c * h + lo) * W;
  int ss[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) ss[r] = 1 << (PRECISION_BITS - 1);
  for (int j = 0; j < n; ++j) {
    const int kj = k[j];
    if (VEC4) {
      const uint32_t p = *reinterpret_cast<const uint32_t*>(src + (int64_t)j * W + x0);
#pragma unroll
      for (int r = 0; r < 4; ++r) ss[r] += (int)((p >> (8 * r)) & 0xffu) * kj;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) ss[r] += (int)src[(int64_t)j * W + (x0 + r < W ? x0 + r : W - 1)] * kj;
    }
  }
  uint32_t b[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) b[r] = clip8(ss[r]);
  store4<VEC4>(out, row, W, x0, flip, b);
}

// neither axis changes: the copy, or the flip alone
template <bool VEC4>
__global__ __launch_bounds__(256) void copy_flip_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int W, int wq, int xblocks, int flip) {
  const int64_t row = blockIdx.x / xblocks;
  const int xg = (int)(blockIdx.x - row * xblocks) * blockDim.x + threadIdx.x;
  if (xg >= wq) return;
  const int x0 = xg * 4;
  uint32_t b[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) b[r] = in[row * W + (x0 + r < W ? x0 + r : W - 1)];
  store4<VEC4>(out, row, W, x0, flip, b);
}

struct Grid {
  int wq, threads, xblocks;
  int64_t blocks;
};
Grid grid_of(int64_t rows, int W) {
  Grid g;
  g.wq = (W + 3) / 4;
  g.threads = g.wq >= 256 ? 256 : (g.wq >= 128 ? 128 : 64);
  g.xblocks = (g.wq + g.threads - 1) / g.threads;
  g.blocks = rows * g.xblocks;
  return g;
}

}  // namespace

extern "C" int rba_resize_u8_pil_bilinear(const uint8_t* in, uint8_t* out, uint8_t* tmp, int C, int h, int w, int H, int W, const int32_t* kx,
                                          const int32_t* bx, int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, int flip, void* stream) {
  RBA_CHECK_ARG(in && out && in != out && C >= 1 && h >= 1 && w >= 1 && H >= 1 && W >= 1);
  RBA_CHECK_ARG((int64_t)C * h * w < (1LL << 31) && (int64_t)C * H * W < (1LL << 31) && (int64_t)C * h * W < (1LL << 31));
  const bool horiz = w != W, vert = h != H;                                        // Pillow skips an axis whose size does not change
  RBA_CHECK_ARG(!horiz || (kx && bx && ksize_x >= 1));
  RBA_CHECK_ARG(!vert || (ky && by && ksize_y >= 1));
  RBA_CHECK_ARG(!(horiz && vert) || (tmp && tmp != in && tmp != out));
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const bool wide = (W & 3) == 0;
  auto aligned = [&](const void* a, const void* b) { return wide && ((((uintptr_t)a | (uintptr_t)b) & 3) == 0); };
  if (horiz) {
    uint8_t* dst = vert ? tmp : out;
    const Grid g = grid_of((int64_t)C * h, W);
    RBA_CHECK_ARG(g.blocks <= 0x7fffffffLL);
    const int f = vert ? 0 : flip;
    if (aligned(dst, dst))
      hipLaunchKernelGGL(resize_h_kernel<true>, dim3((unsigned)g.blocks), dim3(g.threads), 0, st, in, dst, kx, bx, ksize_x, w, W, g.wq, g.xblocks, f);
    else
      hipLaunchKernelGGL(resize_h_kernel<false>, dim3((unsigned)g.blocks), dim3(g.threads), 0, st, in, dst, kx, bx, ksize_x, w, W, g.wq, g.xblocks, f);
  }
  if (vert) {
    const uint8_t* src = horiz ? tmp : in;
    const Grid g = grid_of((int64_t)C * H, W);
    RBA_CHECK_ARG(g.blocks <= 0x7fffffffLL);
    if (aligned(src, out))
      hipLaunchKernelGGL(resize_v_kernel<true>, dim3((unsigned)g.blocks), dim3(g.threads), 0, st, src, out, ky, by, ksize_y, h, H, W, g.wq, g.xblocks, flip);
    else
      hipLaunchKernelGGL(resize_v_kernel<false>, dim3((unsigned)g.blocks), dim3(g.threads), 0, st, src, out, ky, by, ksize_y, h, H, W, g.wq, g.xblocks, flip);
  }
  if (!horiz && !vert) {
    const Grid g = grid_of((int64_t)C * H, W);
    RBA_CHECK_ARG(g.blocks <= 0x7fffffffLL);
    if (aligned(out, out))
      hipLaunchKernelGGL(copy_flip_kernel<true>, dim3((unsigned)g.blocks), dim3(g.threads), 0, st, in, out, W, g.wq, g.xblocks, flip);
    else
      hipLaunchKernelGGL(copy_flip_kernel<false>, dim3((unsigned)g.blocks), dim3(g.threads), 0, st, in, out, W, g.wq, g.xblocks, flip);
  }
  return rba_launch_status();
}
