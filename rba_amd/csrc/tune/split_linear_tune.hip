// Tuning entry points of K6's LDS-DMA kernels (tools/gemm_v4_sweep.py, tools/gemm_v5_timing.py): every tile configuration,
// the ablation builds and the persistent variant.  Built into librba_tune.so (python -m rba_amd.csrc.build --tune); the product
// library contains only the configurations rba_split_linear_f32 dispatches to.
#include "split_linear_experiments.h"
#include "../split_linear_h3.h"
extern "C" int rba_k6_occ = 1;              // (this library is always built with -DRBA_TUNE_KNOBS: the knobs are variables here, with their own defaults)
extern "C" int rba_k6_rs = 1;
extern "C" int rba_k6_rs_min_k = 0;
extern "C" int rba_k6_ks = 1;
extern "C" int rba_k6_stagger = 0;
extern "C" int rba_concurrent_streams_hint = 1;
#include "../mlp_fused_h3.h"

// Timing build of one v5 configuration (tools only): dbg[8 wg + {0..3}] = MFMA wave 0 {barrier wait, compute, epilogue, total}
// cycles, dbg[8 wg + {4..7}] = loader wave 0 {vmcnt wait, barrier wait, issue, total} (s_memtime ticks).
extern "C" int rba_split_linear_v5_timing(const float* x, const void* weight_planes, const float* bias, float* out, int64_t M, int N,
                                          int K, int cfg, unsigned long long* dbg, void* stream) {
  rba_begin();
  const u32x4_t* wp = reinterpret_cast<const u32x4_t*>(weight_planes);
#define RBA_T(RT, CT, G, D, L, WPC, MW)                                                                                              \
  {                                                                                                                              \
    constexpr int BM = 32 * RT * MW, BN = 32 * CT;                                                                               \
    constexpr size_t dyn = (size_t)(D + 1) * G * (BM * 4 + 6 * BN) * 16;                                                         \
    const int64_t MT = (M + BM - 1) / BM;                                                                                        \
    const int NT = (N + BN - 1) / BN;                                                                                            \
    (void)hipFuncSetAttribute((const void*)split_linear_v5_kernel<0, RT, CT, G, D, L, true, MW>,                                     \
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);                                            \
    int64_t grid = 256 * WPC;                                                                                                    \
    grid = MT * NT < grid ? MT * NT : grid;                                                                                      \
    if (((MT * NT) & 7) == 0 && grid >= 8) grid &= ~(int64_t)7;                                                                 \
    hipLaunchKernelGGL((split_linear_v5_kernel<0, RT, CT, G, D, L, true, MW>), dim3((unsigned)grid), dim3(64 * (MW + L)), dyn,  \
                       (hipStream_t)stream, x, wp, bias, out, (int)M, N, K, (int)MT, NT, dbg);                                   \
  }
  if (cfg == 5401421) RBA_T(1, 4, 2, 1, 4, 2, 4)
  else if (cfg == 5401413) RBA_T(1, 4, 1, 3, 4, 2, 4)
  else if (cfg == 6402421) RBA_T(2, 4, 2, 1, 4, 1, 4)
  else if (cfg == 8401421) RBA_T(1, 4, 2, 1, 4, 1, 8)
  else if (cfg == 8801421) RBA_T(1, 4, 2, 1, 8, 1, 8)
  else return (int)hipErrorInvalidValue;
#undef RBA_T
  return rba_launch_status();
}

// cfg = 100000 L + 1000 RT + 100 CT + 10 G + D (+ 10000 PROBE for the ablation builds)
extern "C" int rba_split_linear_v4_f32(const float* x, const void* weight_planes, const float* bias, float* out, int64_t M, int N,
                                       int K, int act, int cfg, void* stream) {
  RBA_CHECK_ARG(M >= 0 && N >= 1 && K >= 32 && (K % 32) == 0 && act >= 0 && act <= 2);
  if (M == 0) return 0;
  RBA_CHECK_ARG(x && weight_planes && out && M < (int64_t)1 << 31);
  RBA_CHECK_ARG((((uintptr_t)x | (uintptr_t)weight_planes | (uintptr_t)out) & 15) == 0);
  rba_begin();
  const u32x4_t* wp = reinterpret_cast<const u32x4_t*>(weight_planes);
  hipStream_t st = (hipStream_t)stream;
  int rc;
  switch (cfg) {
    case 1421: rc = launch_v4_act<1, 4, 2, 1>(act, x, wp, bias, out, M, N, K, st); break;
    case 1412: rc = launch_v4_act<1, 4, 1, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 1413: rc = launch_v4_act<1, 4, 1, 3>(act, x, wp, bias, out, M, N, K, st); break;
    case 1221: rc = launch_v4_act<1, 2, 2, 1>(act, x, wp, bias, out, M, N, K, st); break;
    case 1222: rc = launch_v4_act<1, 2, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 1612: rc = launch_v4_act<1, 6, 1, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 2411: rc = launch_v4_act<2, 4, 1, 1>(act, x, wp, bias, out, M, N, K, st); break;
    case 201421: rc = launch_v4_act<1, 4, 2, 1, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 401421: rc = launch_v4_act<1, 4, 2, 1, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 201412: rc = launch_v4_act<1, 4, 1, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 201413: rc = launch_v4_act<1, 4, 1, 3, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 401413: rc = launch_v4_act<1, 4, 1, 3, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 101413: rc = launch_v4_act<1, 4, 1, 3, 1>(act, x, wp, bias, out, M, N, K, st); break;
    case 201612: rc = launch_v4_act<1, 6, 1, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 201222: rc = launch_v4_act<1, 2, 2, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 202411: rc = launch_v4_act<2, 4, 1, 1, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 402411: rc = launch_v4_act<2, 4, 1, 1, 4>(act, x, wp, bias, out, M, N, K, st); break;
    // persistent (v5): 5000000 + 100000 L + ...; 6000000 + ...: one workgroup per CU
    case 5201421: rc = launch_v5_act<1, 4, 2, 1, 2>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5401421: rc = launch_v5_act<1, 4, 2, 1, 4>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5201413: rc = launch_v5_act<1, 4, 1, 3, 2>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5401413: rc = launch_v5_act<1, 4, 1, 3, 4>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5401412: rc = launch_v5_act<1, 4, 1, 2, 4>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5201612: rc = launch_v5_act<1, 6, 1, 2, 2>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5401222: rc = launch_v5_act<1, 2, 2, 2, 4>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 5201222: rc = launch_v5_act<1, 2, 2, 2, 2>(act, x, wp, bias, out, M, N, K, 2, st); break;
    case 7401421: rc = launch_v5_act<1, 4, 2, 1, 4, 4, true>(act, x, wp, bias, out, M, N, K, 2, st); break;    // 16-byte stores
    case 8801421: rc = launch_v5_act<1, 4, 2, 1, 8, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;          // 8 + 8 waves
    case 8801413: rc = launch_v5_act<1, 4, 1, 3, 8, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 8801621: rc = launch_v5_act<1, 6, 2, 1, 8, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 5801421: rc = launch_v5_act<1, 4, 2, 1, 8, 4>(act, x, wp, bias, out, M, N, K, 1, st); break;          // 4 + 8 waves, 1 per CU
    case 5401422: rc = launch_v5_act<1, 4, 2, 2, 4, 4>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 8401421: rc = launch_v5_act<1, 4, 2, 1, 4, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;          // 8 MFMA waves, 256 x 128
    case 8401413: rc = launch_v5_act<1, 4, 1, 3, 4, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 8401412: rc = launch_v5_act<1, 4, 1, 2, 4, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 8201421: rc = launch_v5_act<1, 4, 2, 1, 2, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 8401621: rc = launch_v5_act<1, 6, 2, 1, 4, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;          // 256 x 192
    case 8401821: rc = launch_v5_act<1, 8, 2, 1, 4, 8>(act, x, wp, bias, out, M, N, K, 1, st); break;          // 256 x 256
    case 6402412: rc = launch_v5_act<2, 4, 1, 2, 4>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 6402421: rc = launch_v5_act<2, 4, 2, 1, 4>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 6401422: rc = launch_v5_act<1, 4, 2, 2, 4>(act, x, wp, bias, out, M, N, K, 1, st); break;
    case 9990032: rc = launch_v4<0, 1, 4, 1, 2, 32, 4>(x, wp, bias, out, M, N, K, st); break;   // 401412 + s_setprio 1 in the MFMA waves
    case 9990064: rc = launch_v4<0, 1, 4, 1, 2, 64, 4>(x, wp, bias, out, M, N, K, st); break;   // 401412 + s_setprio 1 in the loader waves
    case 401412: rc = launch_v4_act<1, 4, 1, 2, 4>(act, x, wp, bias, out, M, N, K, st); break;
    // v8 (A direct, flag-synchronised ring, no barrier): 9500000 + 100 CT + 10 R + L
    case 9500432: rc = launch_v8_act<4, 3, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9500434: rc = launch_v8_act<4, 3, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 9500422: rc = launch_v8_act<4, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9500424: rc = launch_v8_act<4, 2, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 9500232: rc = launch_v8_act<2, 3, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9500234: rc = launch_v8_act<2, 3, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 9500431: rc = launch_v8_act<4, 3, 1>(act, x, wp, bias, out, M, N, K, st); break;
    // v7 (A direct to registers): 9000000 + 100 CT + 10 D + L
    case 9000412: rc = launch_v7_act<4, 1, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000414: rc = launch_v7_act<4, 1, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000422: rc = launch_v7_act<4, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000424: rc = launch_v7_act<4, 2, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000222: rc = launch_v7_act<2, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000224: rc = launch_v7_act<2, 2, 4>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000622: rc = launch_v7_act<6, 2, 2>(act, x, wp, bias, out, M, N, K, st); break;
    case 9000822: rc = launch_v7_act<8, 1, 2>(act, x, wp, bias, out, M, N, K, st); break;
#define RBA_PROBE(P) case 1421 + 10000 * P: rc = launch_v4<0, 1, 4, 2, 1, P>(x, wp, bias, out, M, N, K, st); break;
    RBA_PROBE(1) RBA_PROBE(2) RBA_PROBE(3) RBA_PROBE(4) RBA_PROBE(7) RBA_PROBE(8) RBA_PROBE(9) RBA_PROBE(15) RBA_PROBE(31) RBA_PROBE(16) RBA_PROBE(17)
#undef RBA_PROBE
    default: return (int)hipErrorInvalidValue;
  }
  if (rc) return rc;
  return rba_launch_status();
}

// f16x3 kernel with an explicit tile width and the ablation builds: cfg = CT + 10 PROBE
extern "C" int rba_split_linear_h3_tune(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                                        int act, int cfg, void* stream) {
  RBA_CHECK_ARG(M >= 1 && N >= 1 && K >= 32 && (K % 32) == 0 && act >= 0 && act <= 2);
  rba_begin();
  const H3Args a{x, reinterpret_cast<const u32x4_t*>(weight_packed), bias, out, M, N, K, (hipStream_t)stream};
  int rc;
  switch (cfg) {
    case 4: rc = h3_with_act(act, [&](auto ACT) { return launch_h3<ACT, 4>(a); }); break;
    case 1004: rc = h3_with_act(act, [&](auto ACT) { return launch_h3l<ACT, 4>(a); }); break;
    case 1002: rc = h3_with_act(act, [&](auto ACT) { return launch_h3l<ACT, 2>(a); }); break;
    case 1014: rc = launch_h3l<1, 4, h3_probe(1)>(a); break;
    case 1044: rc = launch_h3l<1, 4, h3_probe(4)>(a); break;
    case 1054: rc = launch_h3l<1, 4, h3_probe(5)>(a); break;
    case 1164: rc = launch_h3l<1, 4, h3_probe(16)>(a); break;
    case 1324: rc = launch_h3l<1, 4, h3_probe(32)>(a); break;
    case 1644: rc = launch_h3l<1, 4, h3_probe(64)>(a); break;
    case 2284: rc = launch_h3l<1, 4, h3_probe(128)>(a); break;
    case 4004: rc = h3_with_act(act, [&](auto ACT) { return launch_h3p_by_shape<ACT, 0, H3_OCC1>(a); }); break;
    case 5004: rc = h3_with_act(act, [&](auto ACT) { return launch_h3p<ACT, H3_OCC1>(a); }); break;
    case 6004: rc = h3_with_act(act, [&](auto ACT) { return launch_h3p<ACT, H3_OCC1 | H3_KS2>(a); }); break;
    case 6104: rc = launch_h3p<0, H3_PRE | H3_OCC1 | H3_KS2>(a); break;              // timing only: x read as if it were a split image
    // round 4: the product's launch forms on split-image operands (timing only: x is read as if it were a split image), one 128 x 128 tile per
    // workgroup, two workgroups per CU (5204: fp32 rows out = qkv; 5214: GELU + split image out = fc1) -- and the 256 x 128 / 8-wave / shared weight
    // ring form RS = 2 of the same two launches (7104, 7114)
    case 5204: rc = launch_h3p<0, H3_PRE>(a); break;
    case 5214: rc = launch_h3p<1, H3_PRE | H3_FOUT>(a); break;
    case 7104: rc = launch_h3p<0, H3_PRE | H3_RS2>(a); break;
    case 7114: rc = launch_h3p<1, H3_PRE | H3_FOUT | H3_RS2>(a); break;
    case 7004: rc = act == 1 ? launch_h3p<1, H3_RS2>(a) : launch_h3p<0, H3_RS2>(a); break;   // RS = 2 on fp32 rows (results checked by tools/gemm_h3_sweep.py)
    case 5104: rc = launch_h3p<0, H3_PRE | H3_OCC1>(a); break;
    case 4044: rc = launch_h3p<1, h3_probe(4)>(a); break;
    case 4014: rc = launch_h3p<1, h3_probe(1)>(a); break;
    case 4024: rc = launch_h3p<1, h3_probe(2)>(a); break;
    case 4034: rc = launch_h3p<1, h3_probe(3)>(a); break;
    case 4644: rc = launch_h3p<1, h3_probe(64)>(a); break;
    case 4674: rc = launch_h3p<1, h3_probe(67)>(a); break;
    case 2: rc = h3_with_act(act, [&](auto ACT) { return launch_h3<ACT, 2>(a); }); break;
    case 1: rc = h3_with_act(act, [&](auto ACT) { return launch_h3<ACT, 1>(a); }); break;
    case 14: rc = launch_h3<1, 4, h3_probe(1)>(a); break;
    case 24: rc = launch_h3<1, 4, h3_probe(2)>(a); break;
    case 34: rc = launch_h3<1, 4, h3_probe(3)>(a); break;
    case 44: rc = launch_h3<1, 4, h3_probe(4)>(a); break;
    case 74: rc = launch_h3<1, 4, h3_probe(7)>(a); break;
    case 154: rc = launch_h3<1, 4, h3_probe(15)>(a); break;
    case 234: rc = launch_h3<1, 4, h3_probe(23)>(a); break;
    case 394: rc = launch_h3<1, 4, h3_probe(39)>(a); break;
    case 634: rc = launch_h3<1, 4, h3_probe(63)>(a); break;
    case 1274: rc = launch_h3<1, 4, h3_probe(127)>(a); break;
    case 84: rc = launch_h3<1, 4, h3_probe(8)>(a); break;
    case 164: rc = launch_h3<1, 4, h3_probe(16)>(a); break;
    case 644: rc = launch_h3<1, 4, h3_probe(64)>(a); break;
    default: return (int)hipErrorInvalidValue;
  }
  return rba_gemm_status(rc);
}

// Timing build of the f16x3 kernel: dbg[6 wg + {0..3}] = s_memrealtime (100 MHz) at entry / loop start / loop end / exit,
// [4] XCC_ID, [5] HW_ID
extern "C" int rba_split_linear_h3_timing(const float* x, const void* weight_packed, const float* bias, float* out, int64_t M, int N, int K,
                                          int probe, unsigned long long* dbg, void* stream) {
  rba_begin();
  H3Args a{x, reinterpret_cast<const u32x4_t*>(weight_packed), bias, out, M, N, K, (hipStream_t)stream};
  a.dbg = dbg;
  int rc;
  if (probe == 0) rc = launch_h3<1, 4, H3_TIMING>(a);
  else if (probe == 1000) rc = launch_h3p<1, H3_TIMING>(a);
#define RBA_H3P_T(P) else if (probe == 1100 + P) rc = launch_h3p<0, H3_TIMING | h3_probe(P)>(a);
  RBA_H3P_T(0) RBA_H3P_T(1) RBA_H3P_T(2) RBA_H3P_T(3) RBA_H3P_T(64) RBA_H3P_T(67) RBA_H3P_T(2048) RBA_H3P_T(2560)
#undef RBA_H3P_T
#define RBA_H3P_T(P) else if (probe == 1200 + P) rc = launch_h3p<0, H3_TIMING | H3_OCC1 | h3_probe(P)>(a);
  RBA_H3P_T(0) RBA_H3P_T(3) RBA_H3P_T(67) RBA_H3P_T(323) RBA_H3P_T(579) RBA_H3P_T(1091) RBA_H3P_T(1859) RBA_H3P_T(2048) RBA_H3P_T(2560) RBA_H3P_T(1) RBA_H3P_T(2) RBA_H3P_T(64) RBA_H3P_T(1795) RBA_H3P_T(768) RBA_H3P_T(512) RBA_H3P_T(256)
#undef RBA_H3P_T
  else if (probe == 1300) rc = launch_h3p<0, H3_TIMING | H3_PRE>(a);
  else if (probe == 1400) rc = launch_h3p<0, H3_TIMING | H3_PRE | H3_OCC1>(a);
  else if (probe == 1500) rc = launch_h3p<1, H3_TIMING | H3_PRE | H3_FOUT>(a);            // round 4: the fc1 launch form (GELU, split image in and out), 128 x 128 tiles
  else if (probe == 1600) rc = launch_h3p<1, H3_TIMING | H3_PRE | H3_FOUT | H3_RS2>(a);   // ... and its 256 x 128 / 8-wave form (RS = 2)
  else if (probe == 1700) rc = launch_h3p<0, H3_TIMING | H3_PRE | H3_RS2>(a);             // RS = 2, fp32 rows out, no activation (the qkv launch form)
  else if (probe == 1310 || probe == 1710) {                                              // the proj / fc2 launch forms: residual epilogue, in place over `out`
    a.res = out;
    rc = probe == 1310 ? launch_h3p<0, H3_TIMING | H3_PRE | H3_RES>(a) : launch_h3p<0, H3_TIMING | H3_PRE | H3_RES | H3_RS2>(a);
  } else if (probe == 1800 || probe == 1810) {                                            // the FPN 3 x 3 convolution on a split image: ONE image of width 512, M = H * 512 rows, K = 9 Cin
    if (M % 512) return (int)hipErrorInvalidValue;
    a.cs = ConvShape{(int)(M / 512), 512, K / 9};
    rc = probe == 1800 ? launch_h3p<0, H3_TIMING | H3_PRE | H3_CONVP | H3_RS2>(a) : launch_h3p<0, H3_TIMING | H3_PRE | H3_CONVP>(a);
  }
  else if (probe == 1001) rc = launch_h3l<1, 4, H3_TIMING>(a);
  else rc = launch_h3<1, 4, H3_TIMING | h3_probe(127)>(a);
  return rba_gemm_status(rc);
}

// ablations of the fused Swin MLP (mlp_fused_h3.h PROBE bits); timing only
extern "C" int rba_mlp_fused_probe(const float* x, const void* w1p, const float* b1, const void* w2p, const float* b2, const float* res, float* out,
                                   int64_t M, int HID, int probe, void* stream) {
  rba_begin();
  const u32x4_t* a = reinterpret_cast<const u32x4_t*>(w1p);
  const u32x4_t* b = reinterpret_cast<const u32x4_t*>(w2p);
  const dim3 grid((unsigned)((M + 127) / 128));
  hipStream_t st = (hipStream_t)stream;
#define RBA_P(P) case P: hipLaunchKernelGGL((mlp_fused_h3_kernel<P>), grid, dim3(256), 0, st, x, a, b1, b, b2, res, out, (int)M, HID); break;
  switch (probe) {
    RBA_P(0) RBA_P(1) RBA_P(2) RBA_P(4) RBA_P(6) RBA_P(7) RBA_P(8) RBA_P(9) RBA_P(15) RBA_P(14)
    default: return (int)hipErrorInvalidValue;
  }
#undef RBA_P
  return rba_launch_status();
}
