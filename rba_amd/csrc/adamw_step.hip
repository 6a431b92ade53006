// K15: the optimizer step of the head fine-tune -- torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.AdamW(amsgrad=False).step()
// (train_net.py:303-328 of the reference: FullModelGradientClippingOptimizer over AdamW) in two launches over flat fp32 state.  docs/kernels/K15.md.
//
// The gradients of all trained tensors live in ONE flat buffer (each parameter's .grad is a view of its slice, slices start on multiples of four
// elements, the gaps stay zero), exp_avg and exp_avg_sq in two more of the same layout.  The parameters stay where the model has them and are reached
// through a device table of descriptors; a second table names, for every workgroup of K15b, its (tensor, chunk).
//   K15a  grad_sqnorm_kernel:  workgroup b sums (grad * grad_scale)^2 over its fixed share of the flat buffer and writes partials[b].  No atomics.
//   K15b  clip_adamw_kernel:   EVERY workgroup sums the partials itself in one fixed order (so all hold the same bits: no hand-over between
//                              workgroups, no third launch), forms the clip coefficient and steps its chunk.  Workgroup 0 writes the norm to stats[0].
// Both reductions are a fixed lane order, a wave shuffle tree and a fixed walk over the waves' LDS slots: bitwise reproducible.
// 16-byte accesses are written on 16-byte aligned addresses only: the flat buffers always (the entry points require it), a parameter where its pointer
// allows it; a parameter that is a view starting anywhere is read and written element by element (global accesses of this target need element
// alignment only, whatever width the compiler merges neighbours to).
#include "common.h"
#include "../../include/rba_hip.h"

namespace {

constexpr int K15_THREADS = 256;                       // four waves
constexpr int K15_WAVES = K15_THREADS / RBA_WAVE;
constexpr int K15_MAX_PARTIALS = 1024;                 // RBA_ADAMW_MAX_PARTIALS: four per thread of K15b
static_assert(K15_MAX_PARTIALS == RBA_ADAMW_MAX_PARTIALS && K15_MAX_PARTIALS == 4 * K15_THREADS, "K15b reads at most four partials per thread");

// the workgroup's sum, the same bits in every thread: xor-shuffle tree per wave, then the waves' slots in index order
// (not loss_reduce.h's loss_block_reduce: ((s0 + s1) + s2) + s3 is another order than its (s0 + s1) + (s2 + s3), and the order is the bits)
__device__ __forceinline__ float block_sum(float v, float* slots /* [K15_WAVES] LDS */) {
  v = wave_reduce_sum(v);
  if ((threadIdx.x & (RBA_WAVE - 1)) == 0) slots[threadIdx.x / RBA_WAVE] = v;
  __syncthreads();
  float s = slots[0];
#pragma unroll
  for (int w = 1; w < K15_WAVES; ++w) s += slots[w];
  return s;
}

// K15a.  Workgroup b owns flat elements [b * per, min((b + 1) * per, n)); per is a multiple of 4 and grad is 16-byte aligned.
__global__ __launch_bounds__(K15_THREADS) void grad_sqnorm_kernel(const float* __restrict__ grad, int64_t n, int64_t per, float grad_scale,
                                                                  float* __restrict__ partials) {
  __shared__ float slots[K15_WAVES];
  const int64_t begin = (int64_t)blockIdx.x * per;
  int64_t end = begin + per;
  if (end > n) end = n;
  float acc = 0.f;
  if (begin < end) {
    const int64_t quads = (end - begin) >> 2;
    const f32x4* g4 = reinterpret_cast<const f32x4*>(grad + begin);
    for (int64_t q = threadIdx.x; q < quads; q += K15_THREADS) {
      const f32x4 g = g4[q] * grad_scale;
      acc = fmaf(g.x, g.x, acc);
      acc = fmaf(g.y, g.y, acc);
      acc = fmaf(g.z, g.z, acc);
      acc = fmaf(g.w, g.w, acc);
    }
    const int64_t t = begin + 4 * quads + threadIdx.x;   // the last workgroup's n % 4 elements
    if (t < end) {
      const float g = grad[t] * grad_scale;
      acc = fmaf(g, g, acc);
    }
  }
  const float s = block_sum(acc, slots);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

struct Hyper {                                         // one step's scalars, as torch.optim.AdamW's single-tensor path forms them on the host
  double lr;                                           // the scheduled learning rate of a group with multiplier 1
  double bc1;                                          // 1 - beta1^step
  float bc2_sqrt;                                      // sqrt(1 - beta2^step)
  float one_minus_beta1, beta2, one_minus_beta2, eps;
  float grad_scale, max_norm;
};

__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, float decay, float step_size, const Hyper& h) {
  p *= decay;                                          // param.mul_(1 - lr * weight_decay)
  m += (g - m) * h.one_minus_beta1;                    // exp_avg.lerp_(grad, 1 - beta1)
  v = h.beta2 * v + h.one_minus_beta2 * g * g;         // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;   // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p -= step_size * (m / denom);                        // param.addcdiv_(exp_avg, denom, value = -step_size)
}

__device__ __forceinline__ void adamw_quad(f32x4& p, f32x4 g, f32x4& m, f32x4& v, float decay, float step_size, const Hyper& h) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float pk = p[k], mk = m[k], vk = v[k];
    adamw_element(pk, g[k], mk, vk, decay, step_size, h);
    p[k] = pk;
    m[k] = mk;
    v[k] = vk;
  }
}

// K15b.  Workgroup b steps elements [c * chunk, min((c + 1) * chunk, n)) of tensor t, (t, c) = blocks[b]; chunk is a multiple of 4.
__global__ __launch_bounds__(K15_THREADS) void clip_adamw_kernel(const rba_adamw_tensor* __restrict__ tensors, const int32_t* __restrict__ blocks,
                                                                 int chunk, const float* __restrict__ grad, float* __restrict__ exp_avg,
                                                                 float* __restrict__ exp_avg_sq, const float* __restrict__ partials, int n_partials,
                                                                 Hyper h, float* __restrict__ stats) {
  __shared__ float slots[K15_WAVES];
  float acc = 0.f;
#pragma unroll
  for (int k = 0; k < K15_MAX_PARTIALS / K15_THREADS; ++k) {
    const int i = k * K15_THREADS + threadIdx.x;
    if (i < n_partials) acc += partials[i];
  }
  const float total = sqrtf(block_sum(acc, slots));
  if (blockIdx.x == 0 && threadIdx.x == 0) stats[0] = total;
  float coef = 1.f;
  if (h.max_norm > 0.f) {
    coef = h.max_norm / (total + 1e-6f);
    coef = coef > 1.f ? 1.f : coef;                    // NOT fminf: a NaN norm must stay NaN and poison the step, as torch's clamp does
  }

  const rba_adamw_tensor t = tensors[blocks[2 * blockIdx.x]];
  const int64_t first = (int64_t)blocks[2 * blockIdx.x + 1] * chunk;
  if (first >= t.n) return;                            // (never, with the tables the wrapper builds)
  const int64_t count = t.n - first < chunk ? t.n - first : (int64_t)chunk;
  const double lr = h.lr * t.lr_mult;                  // the group's lr, and torch's two host scalars of it, in double as torch forms them
  const float decay = (float)(1.0 - lr * t.weight_decay);
  const float step_size = (float)(lr / h.bc1);
  float* __restrict__ p = t.param + first;
  const float* __restrict__ g = grad + t.offset + first;
  float* __restrict__ m = exp_avg + t.offset + first;
  float* __restrict__ v = exp_avg_sq + t.offset + first;

  const int64_t quads = count >> 2;
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    for (int64_t q = threadIdx.x; q < quads; q += K15_THREADS) {
      f32x4 pp = reinterpret_cast<f32x4*>(p)[q], mm = reinterpret_cast<f32x4*>(m)[q], vv = reinterpret_cast<f32x4*>(v)[q];
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[q] * h.grad_scale * coef;
      adamw_quad(pp, gg, mm, vv, decay, step_size, h);
      reinterpret_cast<f32x4*>(p)[q] = pp;
      reinterpret_cast<f32x4*>(m)[q] = mm;
      reinterpret_cast<f32x4*>(v)[q] = vv;
    }
  } else {                                             // the parameter is element-aligned only: its four values one by one, the flat state in quads
    for (int64_t q = threadIdx.x; q < quads; q += K15_THREADS) {
      f32x4 mm = reinterpret_cast<f32x4*>(m)[q], vv = reinterpret_cast<f32x4*>(v)[q];
      const f32x4 gg = reinterpret_cast<const f32x4*>(g)[q] * h.grad_scale * coef;
      f32x4 pp = {p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]};
      adamw_quad(pp, gg, mm, vv, decay, step_size, h);
      p[4 * q] = pp.x;
      p[4 * q + 1] = pp.y;
      p[4 * q + 2] = pp.z;
      p[4 * q + 3] = pp.w;
      reinterpret_cast<f32x4*>(m)[q] = mm;
      reinterpret_cast<f32x4*>(v)[q] = vv;
    }
  }
  const int64_t i = 4 * quads + threadIdx.x;            // the tensor's last n % 4 elements
  if (i < count) {
    float pp = p[i], mm = m[i], vv = v[i];
    adamw_element(pp, g[i] * h.grad_scale * coef, mm, vv, decay, step_size, h);
    p[i] = pp;
    m[i] = mm;
    v[i] = vv;
  }
}

}  // namespace

extern "C" int rba_grad_sqnorm_f32(const float* grad, int64_t n, float grad_scale, float* partials, int n_partials, void* stream) {
  RBA_CHECK_ARG(grad && partials && n >= 1 && n_partials >= 1 && n_partials <= K15_MAX_PARTIALS);
  RBA_CHECK_ARG((reinterpret_cast<uintptr_t>(grad) & 15) == 0 && (reinterpret_cast<uintptr_t>(partials) & 3) == 0);
  const int64_t share = (n + n_partials - 1) / n_partials;
  const int64_t per = (share + 3) & ~(int64_t)3;        // shares start on 16-byte boundaries; the last ones may be empty and write 0
  rba_begin();
  hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)n_partials), dim3(K15_THREADS), 0, (hipStream_t)stream, grad, n, per, grad_scale, partials);
  return rba_launch_status();
}

extern "C" int rba_clip_adamw_step_f32(const rba_adamw_tensor* tensors, const int32_t* blocks, int n_blocks, int chunk, const float* grad,
                                       float* exp_avg, float* exp_avg_sq, const float* partials, int n_partials, const rba_adamw_hyper* hyper,
                                       float* stats, void* stream) {
  RBA_CHECK_ARG(tensors && blocks && grad && exp_avg && exp_avg_sq && partials && hyper && stats && n_blocks >= 1 && chunk >= 4 && chunk % 4 == 0);
  RBA_CHECK_ARG(n_partials >= 1 && n_partials <= K15_MAX_PARTIALS);
  RBA_CHECK_ARG(((reinterpret_cast<uintptr_t>(grad) | reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq)) & 15) == 0);
  RBA_CHECK_ARG(((reinterpret_cast<uintptr_t>(tensors) & 7) | (reinterpret_cast<uintptr_t>(blocks) & 3) | (reinterpret_cast<uintptr_t>(partials) & 3) |
                 (reinterpret_cast<uintptr_t>(stats) & 3)) == 0);
  const rba_adamw_hyper& y = *hyper;
  RBA_CHECK_ARG(y.bias_correction1 > 0.0 && y.bias_correction2_sqrt > 0.0 && y.beta1 >= 0.0 && y.beta1 < 1.0 && y.beta2 >= 0.0 && y.beta2 < 1.0 && y.eps >= 0.0);
  Hyper h;
  h.lr = y.lr;
  h.bc1 = y.bias_correction1;
  h.bc2_sqrt = (float)y.bias_correction2_sqrt;
  h.one_minus_beta1 = (float)(1.0 - y.beta1);
  h.beta2 = (float)y.beta2;
  h.one_minus_beta2 = (float)(1.0 - y.beta2);
  h.eps = (float)y.eps;
  h.grad_scale = y.grad_scale;
  h.max_norm = y.max_norm;
  rba_begin();
  hipLaunchKernelGGL(clip_adamw_kernel, dim3((unsigned)n_blocks), dim3(K15_THREADS), 0, (hipStream_t)stream, tensors, blocks, chunk, grad, exp_avg,
                     exp_avg_sq, partials, n_partials, h, stats);
  return rba_launch_status();
}
