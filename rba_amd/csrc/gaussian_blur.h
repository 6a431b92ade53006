// The reflect-padded Gaussian blur of B planes and its adjoint (gaussian_blur.hip), for a launcher of another file that needs one between its own kernels:
// K11a's reward blur and its backward (pebal_loss.hip).  Library-internal: neither name is exported.
#pragma once
#include <hip/hip_runtime.h>

// what rba_blur_planes_launch needs: 1 <= B <= 65535 planes [H, W] with B H W < 2^31, an odd k <= 15, sigma > 0, and the reflect padding's k / 2 < H, W
__attribute__((visibility("hidden"))) bool rba_blur_planes_ok(int B, int H, int W, int k, float sigma);
// one launch on `st`: out = blur(in), or with `adjoint` out = A^T in.  The caller has checked rba_blur_planes_ok and reads rba_launch_status() after it.
__attribute__((visibility("hidden"))) void rba_blur_planes_launch(bool adjoint, const float* in, float* out, int B, int H, int W, int k, float sigma,
                                                                  hipStream_t st);
