// The order="linear" instances of the fused autoregressive kernels (made_ar_r16.h): named here,
// instantiated in made_ar_linear.hip — a translation unit, and so a code object, of their own —
// and launched from made_ar.hip's dispatch through explicit instantiation declarations.
#pragma once
#include "made_ar_r16.h"

namespace naz {
using ArLin4x2 = CfgARLin<CfgAR<4, 2, 128, 8>>;  // naz's own nsa shape
using ArLin8x0 = CfgARLin<CfgAR<8, 0, 128, 8>>;  // the no-context layout
}  // namespace naz

// the four kernels of one instance; EXT = extern (declaration) or empty (definition)
#define NAZ_AR_LIN_KERNELS(EXT, CF)                                                                              \
  EXT template __global__ void made_ar_r16_kernel<CF>(const float*, int, const float*, int64_t, const float*,     \
                                                      int64_t, const float*, const float*, float*, int64_t, float, \
                                                      int64_t, int64_t, int64_t, int, float*);                    \
  EXT template __global__ void made_ar_fwd_kernel<CfgARF<CF>>(const float*, int, const float*, int64_t,           \
                                                              const float*, int64_t, const float*, const float*,  \
                                                              float*, int64_t, float*, int64_t, float, int64_t,   \
                                                              int64_t, int64_t, int64_t);                         \
  EXT template __global__ void made_ar_pack_kernel<CF>(const float*, int64_t, const int*, float*, int64_t,        \
                                                       const float*, int64_t, const float*);                      \
  EXT template __global__ void made_ar_pack_fwd_kernel<CfgARF<CF>>(const float*, int64_t, float*, int64_t,        \
                                                                   const float*);
