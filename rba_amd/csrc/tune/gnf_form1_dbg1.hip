// Probe build of the GroupNorm-folded mask-feature projection (split_linear_h3l_kernel<NCHW, GNF>), tools/gnfold_probe2.py: RBA_GNF_FORM = 1
// (0 = the product's max + poison, 1 = max(y, f) + (y - y), the form that goes wrong on MI355X), debug dump of the staged values on.  Tools only (librba_tune.so).
#define RBA_GNF_FORM 1
#define RBA_GNF_DEBUG 1
#include "../split_linear_h3.h"

extern "C" int rba_gnf_probe_form1_dbg1(const float* x, const float* mr, const float* gamma, const float* beta, int G, int relu, const void* weight_packed,
                                       const float* bias, float* out, int64_t M, int N, int K, int rows_per_image, unsigned long long* dbg, void* stream) {
  H3Args a{x, reinterpret_cast<const u32x4_t*>(weight_packed), bias, out, M, N, K, (hipStream_t)stream};
  a.dbg = dbg;
  a.rows_per_image = rows_per_image;
  a.gn = GnFold{mr, gamma, beta, G, K / G, relu ? 1 : 0};
  const int rc = launch_h3l<0, 4, H3_NCHW | H3_GNF>(a);
  return rc ? rc : (int)hipGetLastError();
}
