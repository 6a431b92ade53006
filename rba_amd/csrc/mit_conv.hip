// K19b / K19c -- the two convolution-shaped pieces of the MiT (SegFormer) block that are not GEMMs (mask2former/modeling/backbone/mix_transformer.py):
//
// K19b  y = GELU(depthwise3x3(x) + bias) on channels-last tokens [B, H*W, C] (Mlp.forward :53-55 through DWConv :384-390: the reference transposes to
//       NCHW, calls the grouped convolution, transposes back and applies nn.GELU; here it is one pass).  A thread owns four channels of one pixel: nine
//       16-byte loads of x (rows y - 1 .. y + 1 of ITS image only: a row of image b + 1 never feeds the bottom padding of image b), nine of the tap-major
//       weight w9 [9][C], one 16-byte store.  Neighbouring pixels' loads hit the same lines, so HBM sees x once: 4 M C bytes in, 4 M C out.
//
// K19c  cols[(b, oy, ox)][(ky, kx, c)] = x[b][oy * stride - pad + ky][ox * stride - pad + kx][c], zero outside the image and in columns k * k * C .. Kp - 1:
//       the operand of the strided / overlapping convolutions (OverlapPatchEmbed 7x7 / 4 and 3x3 / 2 :177-178, Attention.sr sr x sr / sr :80) as a GEMM
//       over Kp.  x is channels-last tokens, or (nchw_in) the normalised [B,C,H,W] image batch.  A thread writes four consecutive columns with one 16-byte
//       store; where C % 4 == 0 and x is channels-last they are one 16-byte load.  Ho = floor((H + 2 pad - k) / stride) + 1: rows the stride leaves over
//       are dropped, as the convolution drops them.
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

__global__ __launch_bounds__(256) void k19_dwconv3x3_gelu_kernel(const float* __restrict__ x, const float* __restrict__ w9, const float* __restrict__ bias,
                                                                 float* __restrict__ y, int H, int W, int C, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int C4 = C >> 2, c = 4 * (int)(i % C4);
  const int64_t pix = i / C4, t = pix / W;
  const int px = (int)(pix - t * W), py = (int)(t % H);
  const float* xp = x + pix * C + c;
  f32x4 acc = *reinterpret_cast<const f32x4*>(bias + c);
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    if (py + dy < 0 || py + dy >= H) continue;
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      if (px + dx < 0 || px + dx >= W) continue;
      const f32x4 v = *reinterpret_cast<const f32x4*>(xp + ((int64_t)dy * W + dx) * C);
      const f32x4 w = *reinterpret_cast<const f32x4*>(w9 + ((dy + 1) * 3 + dx + 1) * C + c);
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = fmaf(v[e], w[e], acc[e]);
    }
  }
  *reinterpret_cast<f32x4*>(y + pix * C + c) = (f32x4){gelu_erf(acc[0]), gelu_erf(acc[1]), gelu_erf(acc[2]), gelu_erf(acc[3])};
}

template <bool VEC>
__global__ __launch_bounds__(256) void k19_im2col_kernel(const float* __restrict__ x, float* __restrict__ cols, int H, int W, int C, int k, int stride, int pad,
                                                         int Ho, int Wo, int Kp, int nchw_in, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int K4 = Kp >> 2, col0 = 4 * (int)(i % K4), KK = k * k * C;
  const int64_t row = i / K4, t = row / Wo;
  const int ox = (int)(row - t * Wo), oy = (int)(t % Ho);
  const int64_t b = t / Ho;
  const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (VEC) {                                                   // C % 4 == 0, channels-last, 16-byte aligned: the four columns are four channels of one tap
    if (col0 < KK) {
      const int tap = col0 / C, c = col0 - tap * C, ky = tap / k, kx = tap - ky * k, iy = iy0 + ky, ix = ix0 + kx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *reinterpret_cast<const f32x4*>(x + ((b * H + iy) * W + ix) * C + c);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int col = col0 + e;
      if (col >= KK) continue;
      const int tap = col / C, c = col - tap * C, ky = tap / k, kx = tap - ky * k, iy = iy0 + ky, ix = ix0 + kx;
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v[e] = nchw_in ? x[((b * C + c) * H + iy) * W + ix] : x[((b * H + iy) * W + ix) * C + c];
    }
  }
  *reinterpret_cast<f32x4*>(cols + row * Kp + col0) = v;
}

}  // namespace

extern "C" int rba_dwconv3x3_gelu_nhwc_f32(const float* x, const float* w9, const float* bias, float* y, int B, int H, int W, int C, void* stream) {
  RBA_CHECK_ARG(B >= 0 && H >= 0 && W >= 0 && C >= 4 && C % 4 == 0);
  const int64_t total = (int64_t)B * H * W * (C / 4);
  if (total == 0) return 0;
  RBA_CHECK_ARG(x && w9 && bias && y && ((((uintptr_t)x) | ((uintptr_t)w9) | ((uintptr_t)bias) | ((uintptr_t)y)) & 15) == 0);
  RBA_CHECK_ARG((int64_t)H * W < (1LL << 31) && (total + 255) / 256 <= 0x7fffffffLL);
  rba_begin();
  hipLaunchKernelGGL(k19_dwconv3x3_gelu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, w9, bias, y, H, W, C, total);
  return rba_launch_status();
}

extern "C" int rba_im2col_nhwc_f32(const float* x, float* cols, int B, int H, int W, int C, int k, int stride, int pad, int Kp, int nchw_in, void* stream) {
  RBA_CHECK_ARG(B >= 0 && H >= 1 && W >= 1 && C >= 1 && k >= 1 && k <= 64 && stride >= 1 && pad >= 0 && pad < k);
  RBA_CHECK_ARG((int64_t)k * k * C <= Kp && Kp % 4 == 0 && Kp <= (1 << 24) && (int64_t)H * W < (1LL << 31));
  const int Ho = H + 2 * pad < k ? 0 : (H + 2 * pad - k) / stride + 1, Wo = W + 2 * pad < k ? 0 : (W + 2 * pad - k) / stride + 1;    // no window fits: no rows
  const int64_t total = (int64_t)B * Ho * Wo * (Kp / 4);
  if (total == 0) return 0;
  RBA_CHECK_ARG(x && cols && (((uintptr_t)x) & 3) == 0 && (((uintptr_t)cols) & 15) == 0 && (total + 255) / 256 <= 0x7fffffffLL);
  rba_begin();
  const dim3 grid((unsigned)((total + 255) / 256));
  if (!nchw_in && C % 4 == 0 && (((uintptr_t)x) & 15) == 0)
    hipLaunchKernelGGL(k19_im2col_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, cols, H, W, C, k, stride, pad, Ho, Wo, Kp, 0, total);
  else
    hipLaunchKernelGGL(k19_im2col_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, cols, H, W, C, k, stride, pad, Ho, Wo, Kp, nchw_in ? 1 : 0, total);
  return rba_launch_status();
}
