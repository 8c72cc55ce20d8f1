// The MC-dropout sampler's instances (made_ar_dropout.h) and their host dispatch: a translation
// unit, and so a code object, of their own — the other fused autoregressive kernels keep their code.
#include "made_ar_dropout.h"
#include "naz_internal.h"

namespace naz {

template <class FW>
static int drop_sample(const float* packed, int L, const float* z, int64_t ldz, int64_t sz, const float* ctx,
                       int64_t ldc, const float* low, const float* high, float* y, int64_t ldy, int64_t sy,
                       float* out_ld, int64_t sld, int64_t B, int64_t P, float bound, float p, const uint64_t* seeds,
                       int64_t row_offset, hipStream_t s) {
  const int64_t rows = 16 * FW::NW, grid = (B + rows - 1) / rows;
  const size_t lds = (size_t)2 * FW::STG * 4;
  hipLaunchKernelGGL((made_ar_fwd_drop_kernel<FW>), dim3((unsigned)grid, (unsigned)P), dim3(64 * FW::NW), lds, s,
                     packed, L, z, ldz, sz, ctx, ldc, low, high, y, ldy, sy, out_ld, sld, B, bound, seeds, row_offset,
                     drop_threshold(p), drop_scale(p));
  return check_launch("made_ar_fwd_drop_kernel");
}

template <class F>
static int drop_dispatch(const naz_ar_desc* d, F&& f) {
  if (d == nullptr || d->act != NAZ_ACT_TANH || d->L < 0) return -2;
  if (d->kind == NAZ_AR_SPLINE) {
    if (d->K == 8 && d->H == 128 && d->n_hidden == 2 && d->bound > 0.f && d->D == 4 && d->C == 2)
      return f(ArDropNsa4x2{});
    return -2;
  }
  if (d->kind == NAZ_AR_AFFINE && d->C == 2 && d->H == 150 && d->n_hidden == 3) {
    if (d->D == 2) return f(ArDropMaf2x2{});
    if (d->D == 4) return f(ArDropMaf4x2{});
  }
  if (d->kind == NAZ_AR_AFFINE && d->D == 2 && d->C == 0 && d->H == 150 && d->n_hidden == 3) return f(ArDropMaf2x0{});
  return -2;
}

int ar_flow_sample_dropout_supported(const naz_ar_desc* d) {
  return drop_dispatch(d, [](auto) { return 1; }) == 1 ? 1 : 0;
}

int ar_flow_sample_dropout(const naz_ar_desc* d, const void* packed, const float* z, int64_t ldz, int64_t sz,
                           const float* ctx, int64_t ldc, const float* low, const float* high, float* y, int64_t ldy,
                           int64_t sy, float* out_ld, int64_t sld, int64_t B, int64_t P, float p,
                           const uint64_t* seeds, int64_t row_offset, hipStream_t s) {
  if (drop_scale(p) > kDropMaxScale)
    return set_error("naz_ar_flow_sample_dropout: p = %.9g scales the kept activations by more than %g, beyond the "
                     "f16 pieces of the fused kernel (use the per-layer path)", (double)p, (double)kDropMaxScale);
  const int rc = drop_dispatch(d, [&](auto fw) {
    return drop_sample<decltype(fw)>(static_cast<const float*>(packed), d->L, z, ldz, sz, ctx, ldc, low, high, y, ldy,
                                     sy, out_ld, sld, B, P, d->bound, p, seeds, row_offset, s);
  });
  if (rc != -2) return rc;
  return set_error("naz_ar_flow_sample_dropout: no dropout sampler for kind=%d D=%d C=%d H=%d x %d K=%d act=%d",
                   d->kind, d->D, d->C, d->H, d->n_hidden, d->K, d->act);
}

}  // namespace naz
