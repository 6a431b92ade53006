// K1 -- the RbA "rejected by all" reduction (reference: mask2former/maskformer_model.py:381-386 +
// evaluate_ood.py:143-150 + support.py:385-388), and its variant fused with the x4 mask upsample.
//
//   sem[k,p] = sum_q P[q,k] * sigmoid(mask[q,p]);  rba[p] = -sum_k tanh(sem[k,p]);  argmax[p] = argmax_k sem
//
// Scan/reduce priced against the HBM roofline: every mask plane is read exactly once with 16 B/lane coalesced
// loads, the Q x K class probabilities are wave-uniform (scalar loads -> SGPR operands of the FMAs), K accumulators
// per pixel live in VGPRs, nothing but rba (and optionally sem_seg / argmax) is written.  Algorithmic bytes per
// launch: 4*Q*HW + 4*Q*K + 4*HW (+ 4*K*HW with sem_seg, + 4*HW with argmax).  Measured: ~170 us = 62 % of 8 TB/s at
// Q=100, K=19, 1024x2048, HBM traffic 1.005x algorithmic; the remaining gap to the 128 us of the load pattern is VALU
// time (see DESIGN.md and profiles/r01_k1_bandwidth_probes.txt).  The kernels launched here live in rba_reduce_kernels.h; probes and
// experimental variants in tune/ (rba_reduce_experiments.h, rba_reduce_tune.hip: built into librba_tune.so for tools/, not into this library).
#include "rba_reduce_kernels.h"

using namespace rba_k1;

extern "C" int rba_hip_version(void) { return 191; }

// tools / tests only: which fused kernel rba_reduce_up4_f32 runs for K = 19 / 20 (up4_form below)
RBA_KNOB(rba_k1_up4_variant, 0);

// The class counts with kernels of their own (Cityscapes without / with void): f(std::integral_constant<int, K>) for K = 19 / 20.
static bool fixed_k(int K) { return K == 19 || K == 20; }
template <class F>
static int with_fixed_k(int K, F&& f) {
  if (K == 19) return f(std::integral_constant<int, 19>{});
  return f(std::integral_constant<int, 20>{});
}

static int reduce_impl(const float* mask, const float* cls_prob, float* rba, float* sem_seg, int32_t* argmax, int Q, int K, int64_t HW,
                       int score_mode, unsigned int* counters, void* stream) {
  RBA_CHECK_ARG(Q >= 1 && K >= 1 && K <= 160 && HW >= 0 && score_mode >= 0 && score_mode <= 2);
  const int mode = score_mode;
  if (HW == 0) return 0;
  RBA_CHECK_ARG(mask && cls_prob && rba);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  const bool vec4 = (HW % 4 == 0) && ((((uintptr_t)mask | (uintptr_t)rba | (uintptr_t)sem_seg) & 15) == 0);
  // K = 19 / 20: compile-time K, packed FMAs, 2-deep prefetch ring, 4 workgroups per CU
  if (fixed_k(K) && vec4)
    return with_fixed_k(K, [&](auto KC) { return launch_reduce_pk<KC.value, 2, 4>(mask, cls_prob, rba, sem_seg, argmax, Q, HW, mode, counters, st); });
  if (K <= 32 && vec4) return launch_reduce<32, 4>(mask, cls_prob, rba, sem_seg, argmax, Q, K, HW, st, mode);
  if (K <= 32) return launch_reduce<32, 1>(mask, cls_prob, rba, sem_seg, argmax, Q, K, HW, st, mode);
  if (K <= 80) return launch_reduce<80, 1>(mask, cls_prob, rba, sem_seg, argmax, Q, K, HW, st, mode);
  return launch_reduce<160, 1>(mask, cls_prob, rba, sem_seg, argmax, Q, K, HW, st, mode);
}

extern "C" int rba_reduce_f32(const float* mask, const float* cls_prob, float* rba, float* sem_seg, int32_t* argmax,
                              int Q, int K, int64_t HW, int score_mode, void* stream) {
  return reduce_impl(mask, cls_prob, rba, sem_seg, argmax, Q, K, HW, score_mode, nullptr, stream);
}

extern "C" int rba_reduce_ws_f32(const float* mask, const float* cls_prob, float* rba, float* sem_seg, int32_t* argmax,
                                 int Q, int K, int64_t HW, int score_mode, void* workspace, void* stream) {
  RBA_CHECK_ARG(workspace && (((uintptr_t)workspace) & 3) == 0);
  return reduce_impl(mask, cls_prob, rba, sem_seg, argmax, Q, K, HW, score_mode, reinterpret_cast<unsigned int*>(workspace), stream);
}

// Which fused kernel a K = 19 / 20 call gets.  rba_k1_up4_variant (tools / tests): 0 = the product's choice, 1 = the generic kernel, 2 = never the
// matrix pipe, 3 = the matrix pipe for score-only calls only (the round-3 dispatch).
enum class Up4Form { MatrixPipe, PackedValu, Generic };
static Up4Form up4_form(int variant, bool extra_outputs, int crop_w, int Q, bool offsets_fit_32_bits, bool argmax_aligned) {
  // rows a multiple of four wide, at most 512 queries: the class contraction on the matrix pipe (since round 4 also with sem_seg / argmax outputs)
  const bool mx_wanted = variant == 0 || (variant == 3 && !extra_outputs);
  if (mx_wanted && (crop_w & 3) == 0 && Q <= 512 && offsets_fit_32_bits && argmax_aligned) return Up4Form::MatrixPipe;
  return variant != 1 ? Up4Form::PackedValu : Up4Form::Generic;
}

extern "C" int rba_reduce_up4_f32(const float* mask_lowres, const float* cls_prob, float* rba, float* sem_seg,
                                  int32_t* argmax, int Q, int K, int h, int w, int crop_h, int crop_w, int score_mode,
                                  void* stream) {
  RBA_CHECK_ARG(Q >= 1 && K >= 1 && K <= 32 && h >= 1 && w >= 1 && score_mode >= 0 && score_mode <= 2);
  RBA_CHECK_ARG(crop_h >= 0 && crop_w >= 0 && crop_h <= 4 * h && crop_w <= 4 * w && crop_h <= 65535);
  if (crop_h == 0 || crop_w == 0) return 0;
  RBA_CHECK_ARG(mask_lowres && cls_prob && rba);
  rba_begin();
  hipStream_t st = (hipStream_t)stream;
  // vector stores need 16 B aligned rows; the kernel falls back to scalar stores when crop_w % 4 != 0
  RBA_CHECK_ARG((((uintptr_t)rba | (uintptr_t)sem_seg) & 15) == 0);
  if (fixed_k(K)) {
    switch (up4_form(rba_k1_up4_variant, sem_seg || argmax, crop_w, Q, (int64_t)(Q + 8) * h * w < (1LL << 29), (((uintptr_t)argmax) & 15) == 0)) {
      case Up4Form::MatrixPipe:
        return with_fixed_k(K, [&](auto KC) { return launch_up4_mx<KC.value>(mask_lowres, cls_prob, rba, sem_seg, argmax, Q, h, w, crop_h, crop_w, st, score_mode); });
      case Up4Form::PackedValu:
        return with_fixed_k(K, [&](auto KC) { return launch_up4_pk<KC.value>(mask_lowres, cls_prob, rba, sem_seg, argmax, Q, h, w, crop_h, crop_w, st, score_mode); });
      case Up4Form::Generic:
        break;
    }
  }
  // the generic kernel: every other class count, and K = 19 / 20 under variant 1 (K = 19 with its own bound, the round 1-2 instantiation)
  if (K == 19) return launch_up4<19>(mask_lowres, cls_prob, rba, sem_seg, argmax, Q, K, h, w, crop_h, crop_w, st, score_mode);
  return launch_up4<32>(mask_lowres, cls_prob, rba, sem_seg, argmax, Q, K, h, w, crop_h, crop_w, st, score_mode);
}

