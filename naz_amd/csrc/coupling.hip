// Host dispatch of the fused spline-coupling flows (naz "nsc"): the coupling_* entry points over
// the compiled instantiations of the exact-FP32 kernel (coupling_f32.h), the bf16x6 kernel
// (coupling_x6.h), the 32-row f16x3 kernel (coupling_w32.h), the 16-row f16x3 kernel
// (coupling_r16.h) and the NLL training backward (coupling_train.h).  The autoregressive flows are
// made_ar.hip and made_ar_bwd.hip.
#include "coupling_f32.h"
#include "coupling_r16.h"
#include "coupling_train.h"
#include "coupling_w32.h"
#include "coupling_x6.h"
#include "naz_internal.h"

#include <algorithm>
#include <type_traits>

namespace naz {

// the NAZ_DEBUG_NONFINITE record (coupling_r16.h: debug_nonfinite_probe), defined in this
// translation unit alone
__device__ int64_t g_nonfinite[5];

extern "C" int naz_debug_nonfinite(int64_t* out5, int clear) {
#ifndef NAZ_DEBUG_NONFINITE
  (void)out5;
  (void)clear;
  return naz::set_error("naz_debug_nonfinite: library not built with -DNAZ_DEBUG_NONFINITE");
#else
  if (out5 == nullptr) return naz::set_error("naz_debug_nonfinite: null output");
  if (hipDeviceSynchronize() != hipSuccess ||
      hipMemcpyFromSymbol(out5, HIP_SYMBOL(naz::g_nonfinite), 5 * sizeof(int64_t)) != hipSuccess)
    return naz::set_error("naz_debug_nonfinite: reading the record failed");
  if (clear) {
    const int64_t zero[5] = {0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(naz::g_nonfinite), zero, sizeof(zero)) != hipSuccess)
      return naz::set_error("naz_debug_nonfinite: clearing the record failed");
  }
  return 0;
#endif
}

// ---------------------------------------------------------------------------
// Host dispatch over the compiled instantiations
// ---------------------------------------------------------------------------
template <class CF, class CX, class CH, class CR, bool R16OK>
struct CouplingOps {
  static bool supports(int mode) { return mode != NAZ_MFMA_F16X3_R16 || R16OK; }
  static int64_t layer_floats(int mode) {
    if (mode == NAZ_MFMA_F16X3_R16) return CR::LAYER;
    return mode == NAZ_MFMA_F32 ? CF::LAYER : (mode == NAZ_MFMA_BF16X6 ? CX::LAYER : CH::LAYER);
  }
  static int64_t packed_bytes(int L, int mode) { return (int64_t)L * layer_floats(mode) * 4; }
  static int64_t param_count(int L) { return (int64_t)L * CF::FLAT; }
  static int pack(const float* flat, void* packed, int L, float bound, int mode, hipStream_t s) {
    const int64_t n = (int64_t)L * layer_floats(mode);
    int64_t grid = (n + 255) / 256;
    if (grid > 8192) grid = 8192;
    float* pk = reinterpret_cast<float*>(packed);
    if (mode == NAZ_MFMA_F16X3_R16)
      hipLaunchKernelGGL((coupling_pack_r16_kernel<CR>), dim3((unsigned)grid), dim3(256), 0, s, flat, pk, L, bound);
    else if (mode == NAZ_MFMA_F32)
      hipLaunchKernelGGL((coupling_pack_kernel<CF>), dim3((unsigned)grid), dim3(256), 0, s, flat, pk, L, bound);
    else if (mode == NAZ_MFMA_BF16X6)
      hipLaunchKernelGGL((coupling_pack_x6_kernel<CX>), dim3((unsigned)grid), dim3(256), 0, s, flat, pk, L, bound);
    else
      hipLaunchKernelGGL((coupling_pack_x6_kernel<CH>), dim3((unsigned)grid), dim3(256), 0, s, flat, pk, L, bound);
    return check_launch("coupling_pack_kernel");
  }
  template <class G, bool INV, int X6>
  static void launch(const float* pk, int L, const float* x, int64_t ldx, const float* ctx, int64_t ldc,
                     const float* low, const float* high, float* out_lp, float* y, int64_t ldy, int64_t B, float bound,
                     hipStream_t s) {
    const size_t lds = (size_t)G::MAXSTAGE * 4;
    if constexpr (X6 == 2) {
      const int64_t grid = (B + kR16Rows - 1) / kR16Rows;
      hipLaunchKernelGGL((coupling_r16_kernel<G, INV>), dim3((unsigned)grid), dim3(kR16Rows * 4), lds, s, pk, L, x,
                         ldx, ctx, ldc, low, high, out_lp, y, ldy, B, bound);
    } else if constexpr (X6 == 3) {  // f16x3 image: the 32-row-wave kernel (coupling_w32.h)
      const int64_t grid = (B + kX6Rows - 1) / kX6Rows;
      hipLaunchKernelGGL((coupling_w32_kernel<G, INV>), dim3((unsigned)grid), dim3(kX6Rows * 2), lds, s, pk, L, x,
                         ldx, ctx, ldc, low, high, out_lp, y, ldy, B, bound);
    } else if constexpr (X6 == 1) {
      const int64_t grid = (B + kX6Rows - 1) / kX6Rows;
      hipLaunchKernelGGL((coupling_x6_kernel<G, INV>), dim3((unsigned)grid), dim3(kX6Rows * 2), lds, s, pk, L, x,
                         ldx, ctx, ldc, low, high, out_lp, y, ldy, B, bound);
    } else {
      const int64_t grid = (B + kRowsPerWG - 1) / kRowsPerWG;
      hipLaunchKernelGGL((coupling_flow_kernel<G, INV>), dim3((unsigned)grid), dim3(256), lds, s, pk, L, x, ldx,
                         ctx, ldc, low, high, out_lp, y, ldy, B, bound);
    }
  }
  // ---- NLL training path (r16 instantiations only; the packed image must be F16X3_R16)
  static int64_t bwd_layer_floats() {
    if constexpr (R16OK) return BwdR16<CR>::LAYER;
    else return -1;
  }
  static int pack_bwd(const float* flat, void* packed, int L, hipStream_t s) {
    if constexpr (R16OK) {
      const int64_t n = (int64_t)L * BwdR16<CR>::LAYER;
      const int64_t grid = std::min<int64_t>((n + 255) / 256, 8192);
      hipLaunchKernelGGL((coupling_pack_bwd_r16_kernel<CR>), dim3((unsigned)grid), dim3(256), 0, s, flat,
                         reinterpret_cast<float*>(packed), L);
      return check_launch("coupling_pack_bwd_r16_kernel");
    } else {
      return -2;
    }
  }
  static int log_prob_train(const void* packed, int L, const float* x, int64_t ldx, const float* ctx, int64_t ldc,
                            const float* low, const float* high, float* out_lp, float* states, int64_t B, float bound,
                            hipStream_t s) {
    if constexpr (R16OK) {
      if (B == 0) return 0;
      const int64_t grid = (B + kR16Rows - 1) / kR16Rows;
      hipLaunchKernelGGL((coupling_r16_kernel<CR, true, 1>), dim3((unsigned)grid), dim3(kR16Rows * 4),
                         (size_t)CR::MAXSTAGE * 4, s, reinterpret_cast<const float*>(packed), L, x, ldx, ctx, ldc, low,
                         high, out_lp, nullptr, 0, B, bound, states);
      return check_launch("coupling_r16_kernel<train>");
    } else {
      return -2;
    }
  }
  static int bwd_layer(const void* packed, const void* bwd, const float* flat, int l, const float* state,
                       const float* ctx, int64_t ldc, const float* g_in, const float* g_lp, const BwdOut& o, int64_t B,
                       float bound, hipStream_t s) {
    if constexpr (R16OK) {
      if (B == 0) return 0;
      const int64_t ntiles = (B + 16 * kBwdWaves - 1) / (16 * kBwdWaves);
      const int64_t grid = std::min<int64_t>(ntiles, 2048);
      const size_t lds = (size_t)(2 * BwdSlot<CR>::v + 2 * CR::S * (3 * CR::K - 1)) * 4;  // ring, glow, lowp
      hipLaunchKernelGGL((coupling_bwd_r16_kernel<CR>), dim3((unsigned)grid), dim3(kBwdWaves * 64), lds, s,
                         reinterpret_cast<const float*>(packed), reinterpret_cast<const float*>(bwd), flat, l, state,
                         ctx, ldc, g_in, g_lp, o, B, bound);
      return check_launch("coupling_bwd_r16_kernel");
    } else {
      return -2;
    }
  }
  // naz_coupling_layer_{fwd,inv}: one layer of the r16 image
  static int layer(bool inv, int mode, const void* packed, int l, int L, const float* x, int64_t ldx, const float* ctx,
                   int64_t ldc, float* y, int64_t ldy, float* ld, int ld_mode, int64_t B, float bound, hipStream_t s) {
    if constexpr (R16OK) {
      if (mode != NAZ_MFMA_F16X3_R16)
        return set_error("naz_coupling_layer: the packed image must be NAZ_MFMA_F16X3_R16 (mode %d)", mode);
      if (B == 0) return 0;
      (void)L;
      const float* pk = reinterpret_cast<const float*>(packed) + (int64_t)l * CR::LAYER;
      const int64_t grid = (B + kR16Rows - 1) / kR16Rows;
      const size_t lds = (size_t)CR::MAXSTAGE * 4;
      if (inv)
        hipLaunchKernelGGL((coupling_r16_kernel<CR, true, 2>), dim3((unsigned)grid), dim3(kR16Rows * 4), lds, s, pk,
                           1, x, ldx, ctx, ldc, nullptr, nullptr, ld, y, ldy, B, bound, nullptr, ld_mode);
      else
        hipLaunchKernelGGL((coupling_r16_kernel<CR, false, 2>), dim3((unsigned)grid), dim3(kR16Rows * 4), lds, s, pk,
                           1, x, ldx, ctx, ldc, nullptr, nullptr, ld, y, ldy, B, bound, nullptr, ld_mode);
      return check_launch("coupling_r16_kernel<layer>");
    } else {
      return set_error("naz_coupling_layer: no 16-row instantiation for this shape");
    }
  }
  static int dp3_columns(int* rows) {
    if constexpr (R16OK) {
      using BW = BwdR16<CR>;
      if (rows != nullptr)
        for (int q = 0; q < 4; ++q)
          for (int sl = 0; sl < BW::NS3; ++sl) rows[q * BW::NS3 + sl] = BW::slot_row(q, sl);
      return 4 * BW::NS3;
    } else {
      return -2;
    }
  }
  static int run(bool inv, int mode, const void* packed, int L, const float* x, int64_t ldx, const float* ctx,
                 int64_t ldc, const float* low, const float* high, float* out_lp, float* y, int64_t ldy, int64_t B,
                 float bound, hipStream_t s) {
    if (B == 0) return 0;
    const float* pk = reinterpret_cast<const float*>(packed);
#define NAZ_RUN(G, X6)                                                                                   \
  (inv ? launch<G, true, X6>(pk, L, x, ldx, ctx, ldc, low, high, out_lp, y, ldy, B, bound, s)            \
       : launch<G, false, X6>(pk, L, x, ldx, ctx, ldc, low, high, out_lp, y, ldy, B, bound, s))
    if (mode == NAZ_MFMA_F32) NAZ_RUN(CF, 0);
    else if (mode == NAZ_MFMA_BF16X6) NAZ_RUN(CX, 1);
    else if (mode == NAZ_MFMA_F16X3_R16) {
      if constexpr (R16OK) NAZ_RUN(CR, 2);
      else return -2;
    } else {
      NAZ_RUN(CH, 3);
    }
#undef NAZ_RUN
    return check_launch("coupling_flow_kernel");
  }
};

// Instantiation table: (D, C, S, K, H, lower).  Bench configs first (BASELINE.json
// configs 2 and 3), then small shapes used by the parity tests.
#define NAZ_COUPLING_CONFIGS(X)   \
  X(16, 32, 8, 8, 128, true)      \
  X(16, 32, 8, 8, 128, false)     \
  X(8, 0, 4, 8, 128, true)        \
  X(8, 0, 4, 8, 128, false)       \
  X(16, 0, 8, 8, 128, true)       \
  X(4, 3, 2, 8, 64, true)         \
  X(6, 2, 2, 4, 32, true)         \
  X(6, 2, 2, 4, 32, false)

template <class F>
static int coupling_dispatch(const naz_coupling_desc* d, F&& f) {
  if (d == nullptr) return set_error("naz_coupling: null descriptor");
  if (d->act != NAZ_ACT_TANH) return -2;
  if (d->mfma_mode != NAZ_MFMA_BF16X6 && d->mfma_mode != NAZ_MFMA_F32 && d->mfma_mode != NAZ_MFMA_F16X3 &&
      d->mfma_mode != NAZ_MFMA_F16X3_R16)
    return -2;
#define NAZ_R16OK(D_, S_, H_) ((S_) % 4 == 0 && ((D_) - (S_)) % 4 == 0 && (S_) / 4 <= 8 && (H_) % 32 == 0 && (H_) <= 128)
#define NAZ_TRY(D_, C_, S_, K_, H_, LOW_)                                                                  \
  if (d->D == D_ && d->C == C_ && d->S == S_ && d->K == K_ && d->H == H_ && (d->has_lower != 0) == LOW_) {  \
    using Ops = CouplingOps<CouplingCfg<D_, C_, S_, K_, H_, LOW_>, CfgX6<D_, C_, S_, K_, H_, LOW_, 3>,         \
                            CfgX6<D_, C_, S_, K_, H_, LOW_, 2>,                                                \
                            std::conditional_t<NAZ_R16OK(D_, S_, H_), CfgR16<D_, C_, S_, K_, H_, LOW_>,        \
                                               CfgR16<8, 0, 4, 8, 128, true>>,                                 \
                            NAZ_R16OK(D_, S_, H_)>;                                                            \
    if (!Ops::supports(d->mfma_mode)) return -2;                                                               \
    return f(Ops{});                                                                                           \
  }
  NAZ_COUPLING_CONFIGS(NAZ_TRY)
#undef NAZ_TRY
  return -2;
}

int coupling_supported(const naz_coupling_desc* d) {
  return coupling_dispatch(d, [](auto) { return 1; }) == 1 ? 1 : 0;
}

int64_t coupling_param_count(const naz_coupling_desc* d) {
  int64_t v = -1;
  coupling_dispatch(d, [&](auto ops) { v = decltype(ops)::param_count(d->L); return 0; });
  return v;
}

int64_t coupling_packed_bytes(const naz_coupling_desc* d) {
  int64_t v = -1;
  coupling_dispatch(d, [&](auto ops) { v = decltype(ops)::packed_bytes(d->L, d->mfma_mode); return 0; });
  return v;
}

static int unsupported(const naz_coupling_desc* d) {
  return set_error("naz_coupling: no fused instantiation for D=%d C=%d S=%d K=%d H=%d act=%d lower=%d mode=%d", d->D,
                   d->C, d->S, d->K, d->H, d->act, d->has_lower, d->mfma_mode);
}

int coupling_pack(const naz_coupling_desc* d, const float* flat, void* packed, hipStream_t s) {
  int rc = coupling_dispatch(d, [&](auto ops) { return decltype(ops)::pack(flat, packed, d->L, d->bound, d->mfma_mode, s); });
  return rc == -2 ? unsupported(d) : rc;
}

int coupling_log_prob(const naz_coupling_desc* d, const void* packed, const float* x, int64_t ldx, const float* ctx,
                      int64_t ldc, const float* low, const float* high, float* out_lp, int64_t B, hipStream_t s) {
  if ((low == nullptr) != (high == nullptr)) return set_error("naz_coupling_log_prob: low/high must both be set");
  int rc = coupling_dispatch(d, [&](auto ops) {
    return decltype(ops)::run(true, d->mfma_mode, packed, d->L, x, ldx, ctx, ldc, low, high, out_lp, nullptr, 0, B,
                              d->bound, s);
  });
  return rc == -2 ? unsupported(d) : rc;
}

int coupling_sample(const naz_coupling_desc* d, const void* packed, const float* z, int64_t ldz, const float* ctx,
                    int64_t ldc, const float* low, const float* high, float* y, int64_t ldy, float* out_ld, int64_t B,
                    hipStream_t s) {
  if ((low == nullptr) != (high == nullptr)) return set_error("naz_coupling_sample: low/high must both be set");
  int rc = coupling_dispatch(d, [&](auto ops) {
    return decltype(ops)::run(false, d->mfma_mode, packed, d->L, z, ldz, ctx, ldc, low, high, out_ld, y, ldy, B,
                              d->bound, s);
  });
  return rc == -2 ? unsupported(d) : rc;
}

// ---- NLL training path (coupling_train.h) ----------------------------------------------
static int train_mode_ok(const naz_coupling_desc* d) {
  if (d == nullptr) return set_error("naz_coupling: null descriptor");
  if (d->mfma_mode != NAZ_MFMA_F16X3_R16)
    return set_error("naz_coupling training path: the packed image must be NAZ_MFMA_F16X3_R16 (mode %d)", d->mfma_mode);
  return 0;
}

int64_t coupling_bwd_packed_bytes(const naz_coupling_desc* d) {
  int64_t v = -1;
  coupling_dispatch(d, [&](auto ops) {
    const int64_t f = decltype(ops)::bwd_layer_floats();
    v = f < 0 ? -1 : f * d->L * 4;
    return 0;
  });
  return v;
}

int coupling_pack_bwd(const naz_coupling_desc* d, const float* flat, void* packed, hipStream_t s) {
  if (int rc = train_mode_ok(d)) return rc;
  int rc = coupling_dispatch(d, [&](auto ops) { return decltype(ops)::pack_bwd(flat, packed, d->L, s); });
  return rc == -2 ? unsupported(d) : rc;
}

int coupling_log_prob_train(const naz_coupling_desc* d, const void* packed, const float* x, int64_t ldx,
                            const float* ctx, int64_t ldc, const float* low, const float* high, float* out_lp,
                            float* states, int64_t B, hipStream_t s) {
  if (int rc = train_mode_ok(d)) return rc;
  if ((low == nullptr) != (high == nullptr)) return set_error("naz_coupling_log_prob_train: low/high must both be set");
  if (states == nullptr) return set_error("naz_coupling_log_prob_train: states buffer required");
  int rc = coupling_dispatch(d, [&](auto ops) {
    return decltype(ops)::log_prob_train(packed, d->L, x, ldx, ctx, ldc, low, high, out_lp, states, B, d->bound, s);
  });
  return rc == -2 ? unsupported(d) : rc;
}

int coupling_bwd_layer(const naz_coupling_desc* d, const void* packed, const void* packed_bwd, const float* flat,
                       int layer, const float* state, const float* ctx, int64_t ldc, const float* g_in,
                       const float* g_lp, float* h1, float* h2, float* dp1, float* dp2, float* dp3, float* x0,
                       float* g_out, float* g_low, int64_t B, hipStream_t s) {
  if (int rc = train_mode_ok(d)) return rc;
  if (layer < 0 || layer >= d->L) return set_error("naz_coupling_bwd_layer: layer %d out of range", layer);
  if (d->has_lower && g_low == nullptr) return set_error("naz_coupling_bwd_layer: g_low required with a lower spline");
  const BwdOut o{h1, h2, dp1, dp2, dp3, x0, g_out, g_low};
  int rc = coupling_dispatch(d, [&](auto ops) {
    return decltype(ops)::bwd_layer(packed, packed_bwd, flat, layer, state, ctx, ldc, g_in, g_lp, o, B, d->bound, s);
  });
  return rc == -2 ? unsupported(d) : rc;
}

int coupling_layer(const naz_coupling_desc* d, int inv, const void* packed, int layer, const float* x, int64_t ldx,
                   const float* ctx, int64_t ldc, float* y, int64_t ldy, float* ld, int ld_mode, int64_t B,
                   hipStream_t s) {
  if (d == nullptr) return set_error("naz_coupling_layer: null descriptor");
  if (layer < 0 || layer >= d->L) return set_error("naz_coupling_layer: layer %d out of range", layer);
  if (ld_mode != NAZ_LD_ROWSUM && ld_mode != NAZ_LD_ROWSUM_ADD && ld_mode != NAZ_LD_ROWSUM_SUB)
    return set_error("naz_coupling_layer: ld_mode must be NAZ_LD_ROWSUM, _ADD or _SUB");
  int rc = coupling_dispatch(d, [&](auto ops) {
    return decltype(ops)::layer(inv != 0, d->mfma_mode, packed, layer, d->L, x, ldx, ctx, ldc, y, ldy, ld, ld_mode, B,
                                d->bound, s);
  });
  return rc == -2 ? unsupported(d) : rc;
}

int coupling_dp3_columns(const naz_coupling_desc* d, int* rows) {
  int rc = coupling_dispatch(d, [&](auto ops) { return decltype(ops)::dp3_columns(rows); });
  return rc == -2 ? unsupported(d) : rc;
}

}  // namespace naz
