// The order="linear" instances of the fused autoregressive kernels (made_ar_linear.h).
#include "made_ar_linear.h"

namespace naz {
NAZ_AR_LIN_KERNELS(, ArLin4x2)
NAZ_AR_LIN_KERNELS(, ArLin8x0)
}  // namespace naz
