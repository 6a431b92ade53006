// Gaussian smoothing of [H,W] planes: the reference evaluator's optional transforms.GaussianBlur(7, sigma=1) of the anomaly-score map
// (support.py:366-383) and the blur of K11a's reward map (criterion.py:337-388), with its adjoint for the backward.  torchvision semantics: 1-D kernel
// exp(-0.5 (x/sigma)^2) on linspace(-(k-1)/2, (k-1)/2, k) normalised to 1, 2-D kernel = outer product, reflect padding.  One thread per output pixel,
// the plane on blockIdx.z, the tile and its halo staged in LDS, k*k fused multiply-adds in the order of the 2-D correlation.  Pure bandwidth (one read
// + one write of the map).  ONE kernel for the evaluator's single map and the loss's B planes: a plane's bits do not depend on how many travel with it.
#include "common.h"
#include "gaussian_blur.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int TX = 64, TY = 4, KMAX = 15;

__device__ __forceinline__ int reflect(int i, int n) {            // torch "reflect": -1 -> 1, n -> n - 2
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return i < 0 ? 0 : i;                                           // beyond n - 1 + pad: only read by threads outside the image
}

// torchvision's 1-D kernel, one weight per thread tid < k
__device__ __forceinline__ void weights(float* w1, int k, float sigma, int tid) {
  if (tid < k) {
    const float half = (k - 1) * 0.5f;
    float s = 0.f;
    for (int i = 0; i < k; ++i) { const float t = (-half + i) / sigma; s += expf(-0.5f * t * t); }
    const float t = (-half + tid) / sigma;
    w1[tid] = expf(-0.5f * t * t) / s;
  }
}

__global__ __launch_bounds__(TX * TY) void blur_planes_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int k, float sigma) {
  __shared__ float tile[TY + KMAX - 1][TX + KMAX - 1];
  __shared__ float w1[KMAX];
  const int r = k >> 1, tw = TX + k - 1, th = TY + k - 1;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const int tid = threadIdx.y * TX + threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * H * W;
  weights(w1, k, sigma, tid);
  for (int i = tid; i < tw * th; i += TX * TY) {
    const int ty = i / tw, tx = i - ty * tw;
    tile[ty][tx] = in[plane + (int64_t)reflect(y0 + ty - r, H) * W + reflect(x0 + tx - r, W)];
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  float acc = 0.f;
  for (int dy = 0; dy < k; ++dy) {
    const float wy = w1[dy];
    for (int dx = 0; dx < k; ++dx) acc = fmaf(tile[threadIdx.y + dy][threadIdx.x + dx], wy * w1[dx], acc);
  }
  out[plane + (int64_t)y * W + x] = acc;
}

// The coefficient of (d out)[q] in (d in)[p] along one axis of length n.  out[q] = sum_d w[d + r] in[reflect(q + d)], so in[p] is read through
// every virtual position v that reflects onto p: v = p, v = -p (p >= 1) and v = 2 (n - 1) - p (p <= n - 2), each by the q with |v - q| <= r.
// Within r of a border the folded-back taps add; every contributing q lies in [p - r, p + r].
__device__ __forceinline__ float adjoint_coef(int p, int q, int n, const float* w1, int r) {
  float c = 0.f;
  int d = p - q;
  if (d >= -r && d <= r) c += w1[d + r];
  d = -p - q;
  if (p >= 1 && d >= -r) c += w1[d + r];
  d = 2 * (n - 1) - p - q;
  if (p <= n - 2 && d <= r) c += w1[d + r];
  return c;
}

// din = A^T dout in gather form, separably: a source pixel (y, x) collects dout over [y - r, y + r] x [x - r, x + r] (zero outside the plane) with
// the outer product of the two axes' adjoint coefficients.  The tile and its halo are staged in LDS as the forward's.
__global__ __launch_bounds__(TX * TY) void blur_planes_adjoint_kernel(const float* __restrict__ dout, float* __restrict__ din, int H, int W,
                                                                            int k, float sigma) {
  __shared__ float tile[TY + KMAX - 1][TX + KMAX - 1];
  __shared__ float w1[KMAX];
  const int r = k >> 1, tw = TX + k - 1, th = TY + k - 1;
  const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
  const int tid = threadIdx.y * TX + threadIdx.x;
  const int64_t plane = (int64_t)blockIdx.z * H * W;
  weights(w1, k, sigma, tid);
  for (int i = tid; i < tw * th; i += TX * TY) {
    const int ty = i / tw, tx = i - ty * tw, Y = y0 + ty - r, X = x0 + tx - r;
    tile[ty][tx] = Y >= 0 && Y < H && X >= 0 && X < W ? dout[plane + (int64_t)Y * W + X] : 0.f;
  }
  __syncthreads();
  const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
  if (x >= W || y >= H) return;
  float acc = 0.f;
  for (int dy = 0; dy < k; ++dy) {
    const int Y = y + dy - r;
    if (Y < 0 || Y >= H) continue;
    const float cy = adjoint_coef(y, Y, H, w1, r);
    float row = 0.f;
    for (int dx = 0; dx < k; ++dx) {
      const int X = x + dx - r;
      if (X < 0 || X >= W) continue;
      row = fmaf(tile[threadIdx.y + dy][threadIdx.x + dx], adjoint_coef(x, X, W, w1, r), row);
    }
    acc = fmaf(cy, row, acc);
  }
  din[plane + (int64_t)y * W + x] = acc;
}

}  // namespace

bool rba_blur_planes_ok(int B, int H, int W, int k, float sigma) {
  return B >= 1 && B <= 65535 && k >= 1 && k <= KMAX && (k & 1) && sigma > 0.f && H > k / 2 && W > k / 2 && (H + TY - 1) / TY <= 65535 &&
         (int64_t)B * H * W <= 0x7fffffffLL;
}

void rba_blur_planes_launch(bool adjoint, const float* in, float* out, int B, int H, int W, int k, float sigma, hipStream_t st) {
  const dim3 grid((W + TX - 1) / TX, (H + TY - 1) / TY, B), block(TX, TY);
  if (adjoint) hipLaunchKernelGGL(blur_planes_adjoint_kernel, grid, block, 0, st, in, out, H, W, k, sigma);
  else hipLaunchKernelGGL(blur_planes_kernel, grid, block, 0, st, in, out, H, W, k, sigma);
}

extern "C" int rba_gaussian_blur_f32(const float* in, float* out, int H, int W, int kernel_size, float sigma, void* stream) {
  RBA_CHECK_ARG(H >= 0 && W >= 0 && kernel_size >= 1 && kernel_size <= KMAX && (kernel_size & 1) && sigma > 0.f);
  if (H == 0 || W == 0) return 0;
  RBA_CHECK_ARG(in && out && in != out && H > kernel_size / 2 && W > kernel_size / 2);      // reflect padding needs pad < size
  RBA_CHECK_ARG((H + TY - 1) / TY <= 65535);
  rba_begin();
  rba_blur_planes_launch(false, in, out, 1, H, W, kernel_size, sigma, (hipStream_t)stream);
  return rba_launch_status();
}

extern "C" int rba_gaussian_blur_planes_f32(const float* in, float* out, int B, int H, int W, int kernel_size, float sigma, void* stream) {
  RBA_CHECK_ARG(rba_blur_planes_ok(B, H, W, kernel_size, sigma) && in && out && in != out);       // reflect padding needs pad < size
  rba_begin();
  rba_blur_planes_launch(false, in, out, B, H, W, kernel_size, sigma, (hipStream_t)stream);
  return rba_launch_status();
}

extern "C" int rba_gaussian_blur_planes_adjoint_f32(const float* grad_out, float* grad_in, int B, int H, int W, int kernel_size, float sigma,
                                                    void* stream) {
  RBA_CHECK_ARG(rba_blur_planes_ok(B, H, W, kernel_size, sigma) && grad_out && grad_in && grad_out != grad_in);
  rba_begin();
  rba_blur_planes_launch(true, grad_out, grad_in, B, H, W, kernel_size, sigma, (hipStream_t)stream);
  return rba_launch_status();
}
