// The unconditional paper maf (D=2 | C=0, H=[150]x3: naz examples/papers/2506.05657/
// train_mle_unsupervised.py) on the fused autoregressive kernels: named here, instantiated in
// made_ar_uncond.hip — a translation unit, and so a code object, of their own — and launched from
// the dispatch of made_ar.hip and made_ar_bwd.hip through explicit instantiation declarations.
// Without a context every hidden unit has degree 1 (pyro's round(linspace(1, D - 1, H))), so pass 0
// of the inverse has no hidden block (its (mean, log_scale) are the output biases) and pass 1 holds
// every block: its hidden layers 2 and 3 exceed a ring slot and are cut in two (CfgAR::make_layout).
#pragma once
#include "made_ar_bwd.h"
#include "made_ar_linear.h"  // NAZ_AR_LIN_KERNELS: the four log_prob / sample / packer kernels of an instance

namespace naz {
using ArMaf2x0 = CfgAR<2, 0, 150, 8, 3, true>;
static_assert(ArMaf2x0::CUT && ArMaf2x0::nb(0) == 0 && ArMaf2x0::nb(1) == ArMaf2x0::HB,
              "one degree class: an empty pass 0, every block in pass 1, cut sub-layers");
}  // namespace naz

// the backward's two kernels of one affine instance; EXT = extern (declaration) or empty (definition)
#define NAZ_AR_BWD_KERNELS(EXT, CF)                                                                              \
  EXT template __global__ void made_ar_bwd_kernel<CfgARB<CF>>(const float*, const float*, const int*,            \
                                                              const float*, const float*, int64_t, const float*, \
                                                              const float*, ArBwdOut, int64_t, int);             \
  EXT template __global__ void made_ar_pack_bwd_kernel<CfgARB<CF>>(const float*, const float*, float*);
