// K2 backward -- gradients of multi-scale deformable attention (the second export of the reference's native op:
// MultiScaleDeformableAttention.ms_deform_attn_backward, pixel_decoder/ops/src/vision.cpp:20, ops/src/ms_deform_attn.h:46-66,
// ops/src/cuda/ms_deform_attn_cuda.cu:88-158).  Written from the mathematics of the forward kernel in ms_deform_attn.hip:
//
//   sample (n, q, m, l, p):  h = y H_l - 0.5, w = x W_l - 0.5, taken iff -1 < h < H_l and -1 < w < W_l; lh, lw the fractions, hh = 1 - lh,
//   hw = 1 - lw; v00 v01 v10 v11 the four taps (0 outside the map); g[d] the output gradient of (n, q, m); A the attention weight.
//     grad_value[tap][d]  += g[d] A tapweight                                      (summed across workgroups: float atomics)
//     grad_attn_weight     = sum_d g[d] (hh hw v00 + hh lw v01 + lh hw v10 + lh lw v11)[d]
//     grad_sampling_loc.x  = W_l A sum_d g[d] (-hh v00 + hh v01 - lh v10 + lh v11)[d]
//     grad_sampling_loc.y  = H_l A sum_d g[d] (-hw v00 - lw v01 + hw v10 + lw v11)[d]
//   a sample outside the window adds nothing to grad_value and its other two gradients are exactly 0.
//
// grad_value is zero-filled by the entry point and receives no-return global_atomic_add_f32 / _f64 (plain atomicAdd): its last bits
// depend on arrival order.  grad_sampling_loc and grad_attn_weight are written with plain stores, each element by exactly one lane, from
// reductions of a fixed order: bitwise reproducible, no zero-fill needed.
#include "common.h"
#include "../../include/rba_hip.h"

// tools / tests only (not part of the ABI contract): 1 = rba_ms_deform_attn_bwd_f32 always runs the generic kernel
RBA_KNOB(rba_k2_bwd_variant, 0);

namespace {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, RBA_WAVE);
  return v;
}

// ---- generic form: any D, L, P; float or double.  One wave per (n, q, m); lanes stride over the D channels; per sample each lane keeps
// three partial sums (attn, x, y), reduced across the wave by shuffles; lane 0 stores.  The sample geometry is wave-uniform, so every
// branch around the shuffles is taken by the whole wave.  Correct first, not tuned.
template <typename T>
__global__ __launch_bounds__(256) void msda_bwd_kernel(const T* __restrict__ value, const int64_t* __restrict__ shapes,
                                                       const int64_t* __restrict__ lsi, const T* __restrict__ loc,
                                                       const T* __restrict__ attw, const T* __restrict__ gout, T* __restrict__ gvalue,
                                                       T* __restrict__ gloc, T* __restrict__ gattw, int S, int M, int D, int L, int Lq,
                                                       int P, int64_t total) {
  const int lane = threadIdx.x & (RBA_WAVE - 1);
  const int64_t nqm = (int64_t)blockIdx.x * (blockDim.x / RBA_WAVE) + (threadIdx.x / RBA_WAVE);   // (n*Lq + q)*M + m
  if (nqm >= total) return;                                                                       // a whole wave leaves
  const int m = (int)(nqm % M);
  const int64_t n = nqm / ((int64_t)M * Lq);
  const int64_t hbase = (n * S * M + m) * (int64_t)D;        // channel 0 of head m at spatial position 0 of image n
  const int64_t vstride = (int64_t)M * D;
  const T* lp = loc + nqm * L * P * 2;
  const T* wp = attw + nqm * L * P;
  const T* gp = gout + nqm * D;
  T* glp = gloc + nqm * L * P * 2;
  T* gwp = gattw + nqm * L * P;
  for (int l = 0; l < L; ++l) {
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    const int64_t lbase = hbase + lsi[l] * vstride;
    for (int p = 0; p < P; ++p) {
      const int i = l * P + p;
      const T x = lp[2 * i], y = lp[2 * i + 1];
      const T A = wp[i];
      const T h_im = y * H - (T)0.5, w_im = x * W - (T)0.5;
      T sa = (T)0, sx = (T)0, sy = (T)0;
      if (h_im > (T)-1 && w_im > (T)-1 && h_im < (T)H && w_im < (T)W) {
        const T hf = floor(h_im), wf = floor(w_im);
        const int h0 = (int)hf, w0 = (int)wf;
        const T lh = h_im - hf, lw = w_im - wf, hh = (T)1 - lh, hw = (T)1 - lw;
        const bool h0ok = h0 >= 0, h1ok = h0 + 1 <= H - 1, w0ok = w0 >= 0, w1ok = w0 + 1 <= W - 1;
        const bool k00 = h0ok && w0ok, k01 = h0ok && w1ok, k10 = h1ok && w0ok, k11 = h1ok && w1ok;
        const int64_t o00 = lbase + ((int64_t)h0 * W + w0) * vstride;
        const int64_t o01 = o00 + vstride, o10 = o00 + (int64_t)W * vstride, o11 = o10 + vstride;
        const T t00 = hh * hw, t01 = hh * lw, t10 = lh * hw, t11 = lh * lw;
        T pa = (T)0, px = (T)0, py = (T)0;
        for (int c = lane; c < D; c += RBA_WAVE) {
          const T g = gp[c];
          const T ga = g * A;
          const T v00 = k00 ? value[o00 + c] : (T)0, v01 = k01 ? value[o01 + c] : (T)0;
          const T v10 = k10 ? value[o10 + c] : (T)0, v11 = k11 ? value[o11 + c] : (T)0;
          if (k00) atomicAdd(gvalue + o00 + c, ga * t00);
          if (k01) atomicAdd(gvalue + o01 + c, ga * t01);
          if (k10) atomicAdd(gvalue + o10 + c, ga * t10);
          if (k11) atomicAdd(gvalue + o11 + c, ga * t11);
          pa += g * (t00 * v00 + t01 * v01 + t10 * v10 + t11 * v11);
          px += g * (hh * (v01 - v00) + lh * (v11 - v10));
          py += g * (hw * (v10 - v00) + lw * (v11 - v01));
        }
        sa = wave_sum(pa);
        sx = (T)W * A * wave_sum(px);
        sy = (T)H * A * wave_sum(py);
      }
      if (lane == 0) {
        gwp[i] = sa;
        glp[2 * i] = sx;
        glp[2 * i + 1] = sy;
      }
    }
  }
}

// ---- model form: fp32, head_dim 32, P = 4, L = 1 or 3 (what every released config runs).  The kernel is priced by its atomics: global float
// atomic adds run at one chip-wide byte rate when each wave-instruction covers 256 contiguous bytes or two 128-byte row segments.  One tap
// of one (query, head) is 32 channels x 4 B = 128 B, so
//   * 32 lanes x ONE dword per (query, head), two (query, head) pairs per wave: every atomic wave-instruction is two 128-byte segments
//     (the forward's 8 lanes x 16 B would give 32-byte segments);
//   * a workgroup is 8 consecutive (query, head) pairs in memory order -- the 8 heads of one query at M = 8: the sampling parameters, the
//     output gradient and the three outputs of a workgroup are contiguous, and its atomics spread over the heads' disjoint channel slices.
//     (Measured against the forward's mapping, 8 consecutive queries of ONE head, whose adds land on the same addresses together: 707 vs
//     781 us at the C5 encoder shape, docs/kernels/K2.md);
//   * the geometry of sample i (four clamped 32-bit tap offsets, lh, lw, A, the four in-map bits) is computed once, by lane i of the group,
//     and shared through LDS, as the forward does; an out-of-map tap is loaded from a clamped (valid) address and selected to 0, and its
//     atomic is predicated off: no atomic bandwidth for a tap that adds nothing;
//   * the three sums of a sample are reduced over the group's 32 lanes with five xor shuffles (fixed order); lane i keeps sample i's results
//     and stores them: contiguous plain stores, each output element written by exactly one lane.
template <int L, int P>
__global__ __launch_bounds__(256) void msda_bwd_lp_kernel(const float* __restrict__ value, const int64_t* __restrict__ shapes,
                                                          const int64_t* __restrict__ lsi, const float* __restrict__ loc,
                                                          const float* __restrict__ attw, const float* __restrict__ gout,
                                                          float* __restrict__ gvalue, float* __restrict__ gloc, float* __restrict__ gattw,
                                                          int S, int M, int Lq) {
  constexpr int D = 32, LP = L * P, G = 8;                   // G (query, head) groups of 32 lanes per workgroup
  static_assert(LP <= 32, "one lane of a group per sample");
  __shared__ __attribute__((aligned(16))) uint32_t sh_off[G][LP][4];
  __shared__ __attribute__((aligned(16))) float sh_prm[G][LP][4];   // lh, lw, A, in-map bits (0 for a sample outside the window)
  const int g = threadIdx.x >> 5, c = threadIdx.x & 31;
  const int pair = blockIdx.x * G + g, q = pair / M, m = pair - q * M, n = blockIdx.y;
  if (q >= Lq) return;                                       // a whole group leaves; the shuffles below stay inside a group
  const int64_t nqm = ((int64_t)n * Lq + q) * M + m;
  const uint32_t vstride_b = (uint32_t)M * D * 4;            // bytes between spatial positions

  // ---- phase A: lane i < LP of the group computes sample i
  float Wl = 0.f, Hl = 0.f;
  if (c < LP) {
    const int l = c / P;
    const int H = (int)shapes[2 * l], W = (int)shapes[2 * l + 1];
    Hl = (float)H;
    Wl = (float)W;
    const float2 xy = *reinterpret_cast<const float2*>(loc + (nqm * LP + c) * 2);
    const float A = attw[nqm * LP + c];
    const float h_im = xy.y * H - 0.5f, w_im = xy.x * W - 0.5f;
    const bool inside = h_im > -1.f && w_im > -1.f && h_im < (float)H && w_im < (float)W;
    const float hf = floorf(h_im), wf = floorf(w_im);
    const int h0 = inside ? (int)hf : 0, w0 = inside ? (int)wf : 0;
    const float lh = h_im - hf, lw = w_im - wf;
    const bool h0ok = inside && h0 >= 0, h1ok = inside && h0 + 1 <= H - 1, w0ok = w0 >= 0, w1ok = w0 + 1 <= W - 1;
    const int hc0 = min(max(h0, 0), H - 1), hc1 = min(max(h0 + 1, 0), H - 1), wc0 = min(max(w0, 0), W - 1), wc1 = min(max(w0 + 1, 0), W - 1);
    const uint32_t base = (uint32_t)lsi[l];
    const rba_u32x4 o4 = {(base + (uint32_t)(hc0 * W + wc0)) * vstride_b, (base + (uint32_t)(hc0 * W + wc1)) * vstride_b,
                          (base + (uint32_t)(hc1 * W + wc0)) * vstride_b, (base + (uint32_t)(hc1 * W + wc1)) * vstride_b};
    const uint32_t bits = (h0ok && w0ok ? 1u : 0u) | (h0ok && w1ok ? 2u : 0u) | (h1ok && w0ok ? 4u : 0u) | (h1ok && w1ok ? 8u : 0u);
    const f32x4 prm = {lh, lw, A, __uint_as_float(bits)};
    *reinterpret_cast<rba_u32x4*>(&sh_off[g][c][0]) = o4;
    *reinterpret_cast<f32x4*>(&sh_prm[g][c][0]) = prm;
  }
  __builtin_amdgcn_wave_barrier();                           // a group lives inside one wave; LDS operations of a wave are in order

  // ---- phase B: lane c owns channel c of this (query, head)
  const int64_t hoff = ((int64_t)n * S * M + m) * D + c;
  const char* vb = reinterpret_cast<const char*>(value + hoff);
  char* gb = reinterpret_cast<char*>(gvalue + hoff);
  const float go = gout[nqm * D + c];
  float ra = 0.f, rx = 0.f, ry = 0.f;                        // lane i < LP ends up with sample i's three sums
#pragma unroll 4                                             // one level per trip: 61 instead of 125 registers, and 1 % faster at C5 than fully unrolled
  for (int i = 0; i < LP; ++i) {
    const rba_u32x4 o4 = *reinterpret_cast<const rba_u32x4*>(&sh_off[g][i][0]);
    const f32x4 prm = *reinterpret_cast<const f32x4*>(&sh_prm[g][i][0]);
    const float lh = prm.x, lw = prm.y, A = prm.z, hh = 1.f - lh, hw = 1.f - lw;
    const uint32_t bits = __float_as_uint(prm.w);
    float v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float ld = *reinterpret_cast<const float*>(vb + o4[t]);
      v[t] = (bits >> t & 1u) ? ld : 0.f;
    }
    const float tw[4] = {hh * hw, hh * lw, lh * hw, lh * lw};
    const float ga = go * A;
#pragma unroll
    for (int t = 0; t < 4; ++t)
      if (bits >> t & 1u) atomicAdd(reinterpret_cast<float*>(gb + o4[t]), ga * tw[t]);
    float pa = go * (tw[0] * v[0] + tw[1] * v[1] + tw[2] * v[2] + tw[3] * v[3]);
    float px = go * (hh * (v[1] - v[0]) + lh * (v[3] - v[2]));
    float py = go * (hw * (v[2] - v[0]) + lw * (v[3] - v[1]));
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
      pa += __shfl_xor(pa, o, 32);
      px += __shfl_xor(px, o, 32);
      py += __shfl_xor(py, o, 32);
    }
    if (c == i) {
      const bool any = bits != 0u;                           // a sample outside the window: exactly 0
      ra = any ? pa : 0.f;
      rx = any ? A * px : 0.f;
      ry = any ? A * py : 0.f;
    }
  }
  if (c < LP) {
    gattw[nqm * LP + c] = ra;
    *reinterpret_cast<float2*>(gloc + (nqm * LP + c) * 2) = make_float2(Wl * rx, Hl * ry);
  }
}

static int launch_msda_bwd_lp(const float* value, const int64_t* shapes, const int64_t* lsi, const float* loc, const float* attw,
                              const float* gout, float* gvalue, float* gloc, float* gattw, int N, int S, int M, int L, int Lq, int P,
                              hipStream_t st) {
  if (P != 4 || (L != 1 && L != 3) || N > 65535 || (int64_t)Lq * M > 0x7fffffffLL - 8) return -1;
  if ((int64_t)S * M * 128 >= ((int64_t)1 << 32)) return -1;     // 32-bit byte offsets into one image's [S, M, 32] fp32, as launch_msda_lp
  const dim3 grid((unsigned)(((int64_t)Lq * M + 7) / 8), (unsigned)N);
  if (L == 1)
    hipLaunchKernelGGL((msda_bwd_lp_kernel<1, 4>), grid, dim3(256), 0, st, value, shapes, lsi, loc, attw, gout, gvalue, gloc, gattw, S, M, Lq);
  else
    hipLaunchKernelGGL((msda_bwd_lp_kernel<3, 4>), grid, dim3(256), 0, st, value, shapes, lsi, loc, attw, gout, gvalue, gloc, gattw, S, M, Lq);
  return 0;
}

template <typename T>
static int msda_bwd(const T* value, const int64_t* shapes, const int64_t* lsi, const T* loc, const T* attw, const T* gout, T* gvalue, T* gloc,
                    T* gattw, int N, int S, int M, int D, int L, int Lq, int P, hipStream_t st, bool model_form_ok) {
  RBA_CHECK_ARG(N >= 0 && S >= 1 && M >= 1 && D >= 1 && L >= 1 && Lq >= 0 && P >= 1);
  rba_begin();
  const int64_t vbytes = (int64_t)N * S * M * D * (int64_t)sizeof(T);
  if (vbytes > 0) {
    RBA_CHECK_ARG(gvalue != nullptr);
    const hipError_t e = hipMemsetAsync(gvalue, 0, (size_t)vbytes, st);
    if (e != hipSuccess) return (int)e;
  }
  if (N == 0 || Lq == 0) return 0;
  RBA_CHECK_ARG(value && shapes && lsi && loc && attw && gout && gloc && gattw);
  if constexpr (sizeof(T) == 4) {
    if (model_form_ok && D == 32 && ((((uintptr_t)loc | (uintptr_t)gloc) & 7) == 0) &&
        launch_msda_bwd_lp(value, shapes, lsi, loc, attw, gout, gvalue, gloc, gattw, N, S, M, L, Lq, P, st) == 0)
      return rba_launch_status();
  }
  const int64_t total = (int64_t)N * Lq * M;                  // one wave each
  const int64_t blocks = (total + 3) / 4;
  RBA_CHECK_ARG(blocks <= 0x7fffffffLL);
  hipLaunchKernelGGL((msda_bwd_kernel<T>), dim3((unsigned)blocks), dim3(256), 0, st, value, shapes, lsi, loc, attw, gout, gvalue, gloc, gattw,
                     S, M, D, L, Lq, P, total);
  return rba_launch_status();
}

}  // namespace

extern "C" int rba_ms_deform_attn_bwd_f32(const float* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                          const float* sampling_loc, const float* attn_weight, const float* grad_out, float* grad_value,
                                          float* grad_sampling_loc, float* grad_attn_weight, int N, int S, int M, int D, int L, int Lq, int P,
                                          void* stream) {
  return msda_bwd<float>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, grad_value, grad_sampling_loc,
                         grad_attn_weight, N, S, M, D, L, Lq, P, (hipStream_t)stream, rba_k2_bwd_variant == 0);
}

// The double-precision entry: the reference dispatches float and double, and its own gradient test (ops/test.py:66-89) runs in double.
extern "C" int rba_ms_deform_attn_bwd_f64(const double* value, const int64_t* spatial_shapes, const int64_t* level_start_index,
                                          const double* sampling_loc, const double* attn_weight, const double* grad_out, double* grad_value,
                                          double* grad_sampling_loc, double* grad_attn_weight, int N, int S, int M, int D, int L, int Lq, int P,
                                          void* stream) {
  return msda_bwd<double>(value, spatial_shapes, level_start_index, sampling_loc, attn_weight, grad_out, grad_value, grad_sampling_loc,
                          grad_attn_weight, N, S, M, D, L, Lq, P, (hipStream_t)stream, false);
}
