// The unconditional paper maf's instances of the fused autoregressive kernels (made_ar_uncond.h).
#include "made_ar_uncond.h"

namespace naz {
NAZ_AR_LIN_KERNELS(, ArMaf2x0)
NAZ_AR_BWD_KERNELS(, ArMaf2x0)
}  // namespace naz
