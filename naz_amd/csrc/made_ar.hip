// Host dispatch of the fused autoregressive flows (naz "nsa" / "maf"): the ar_flow_* entry points
// over made_ar_r16.h (log_prob and sample) and made_ar_wide.h (the wide production MAFs).
#include "made_ar_linear.h"
#include "made_ar_r16.h"
#include "made_ar_uncond.h"
#include "made_ar_wide.h"
#include "naz_internal.h"

#include <algorithm>
#include <type_traits>

namespace naz {

// the linear-order instances' kernels are compiled in made_ar_linear.hip
NAZ_AR_LIN_KERNELS(extern, ArLin4x2)
NAZ_AR_LIN_KERNELS(extern, ArLin8x0)
// ... and the unconditional paper maf's in made_ar_uncond.hip
NAZ_AR_LIN_KERNELS(extern, ArMaf2x0)

// ---- forward (sample) direction, shared by AROps and AROpsW: made_ar_fwd_kernel over CfgARF<G>'s
// per-layer image
template <class G>
struct ARFwdOps {
  using FW = CfgARF<G>;
  // flat per layer: W0m [H][C + D] | b0 [H] | {Wim [H][H] | bi [H]} x (NHID - 1) | Woutm [D P][H] | bout [D P]
  static constexpr int64_t flat_floats() {
    constexpr int H = G::H, D = G::D, C = G::C, P = G::P;
    return (int64_t)H * (C + D) + H + (int64_t)(G::NHID - 1) * (H * H + H) + (int64_t)D * P * H + D * P;
  }
  static int64_t fwd_layer_floats() { return FW::LAYER; }
  static int pack_fwd_host(const float* flat, int L, float* out) {
    for (int l = 0; l < L; ++l) made_ar_pack_fwd_layer<FW>(flat + l * flat_floats(), out + (int64_t)l * FW::LAYER);
    return 0;
  }
  static int sample(const float* packed, int L, const float* z, int64_t ldz, const float* ctx, int64_t ldc,
                    const float* low, const float* high, float* y, int64_t ldy, float* out_ld, int64_t B, float bound,
                    hipStream_t s, int64_t P = 1, int64_t spk = 0, int64_t sz = 0, int64_t sy = 0, int64_t sld = 0) {
    if (B == 0 || P == 0) return 0;
    if (P > 65535) return set_error("naz_ar_flow_sample_batched: at most 65535 draws per call");
    const int64_t rows = 16 * FW::NW, grid = (B + rows - 1) / rows;
    const size_t lds = (size_t)2 * FW::STG * 4;
    hipLaunchKernelGGL((made_ar_fwd_kernel<FW>), dim3((unsigned)grid, (unsigned)P), dim3(64 * FW::NW), lds, s, packed,
                       L, z, ldz, ctx, ldc, low, high, y, ldy, out_ld, B, bound, spk, sz, sy, sld);
    return check_launch("made_ar_fwd_kernel");
  }
  static int pack_fwd_device(const float* flat, int64_t sflat, float* packed, int64_t spk, int L, int64_t P,
                             hipStream_t s, const float* mask = nullptr) {
    if (L == 0 || P == 0) return 0;
    if (P > 65535 || L > 65535) return set_error("naz_ar_flow_pack_fwd: at most 65535 draws / layers per call");
    const dim3 grid((unsigned)((FW::LAYER + 255) / 256), (unsigned)L, (unsigned)P);
    hipLaunchKernelGGL((made_ar_pack_fwd_kernel<FW>), grid, dim3(256), 0, s, flat, sflat, packed, spk, mask);
    return check_launch("made_ar_pack_fwd_kernel");
  }
};

// ---- fused autoregressive inverse (made_ar_r16.h): naz nsa / maf log_prob -------------
template <class CF>
struct AROps : ARFwdOps<CF> {
  static int64_t layer_floats() { return CF::LAYER; }
  static int degrees(int* deg) {
    for (int u = 0; u < CF::H; ++u) deg[u] = CF::deg(u);
    return 0;
  }
  static int pack_host(const float* flat, const int* perm, int L, float* out) {
    constexpr int D = CF::D;
    constexpr int64_t per = ARFwdOps<CF>::flat_floats();
    for (int l = 0; l < L; ++l) {
      bool seen[32] = {};
      for (int p = 0; p < D; ++p) {
        const int v = perm[l * D + p];
        if (v < 0 || v >= D || seen[v]) return set_error("naz_ar_flow_pack: layer %d: bad permutation", l);
        seen[v] = true;
      }
      made_ar_pack_layer<CF>(flat + l * per, perm + l * D, out + (int64_t)l * CF::LAYER);
    }
    return 0;
  }
  static int log_prob(const float* packed, int L, const float* x, int64_t ldx, const float* ctx, int64_t ldc,
                      const float* low, const float* high, float* out_lp, int64_t B, float bound, hipStream_t s,
                      int64_t P = 1, int64_t spk = 0, int64_t sx = 0, int64_t slp = 0, int c0mode = 0,
                      float* states = nullptr, void* = nullptr, int64_t = 0) {
    static_assert(2 * CF::STG * 4 <= 160 * 1024, "two weight stages exceed the LDS");
    if (c0mode && CF::LINEAR) return set_error("naz_ar_flow: the linear-order spline has no pass-0 constants form");
    if (c0mode && CF::CUT) return set_error("naz_ar_flow: D=%d C=%d H=%d x %d: no pass-0 constants form", CF::D, CF::C,
                                            CF::H, CF::NHID);
    if (B == 0 || L == 0 || P == 0) return 0;
    if (P > 65535) return set_error("naz_ar_flow_log_prob_batched: at most 65535 draws per call");
    const int64_t rows = 16 * CF::NW, grid = (B + rows - 1) / rows;
    const size_t lds = (size_t)2 * CF::STG * 4;
    hipLaunchKernelGGL((made_ar_r16_kernel<CF>), dim3((unsigned)grid, (unsigned)P), dim3(64 * CF::NW), lds, s, packed,
                       L, x, ldx, ctx, ldc, low, high, out_lp, B, bound, spk, sx, slp, c0mode, states);
    return check_launch("made_ar_r16_kernel");
  }
  static int64_t workspace_bytes(int64_t, int64_t) { return 0; }  // every intermediate stays on chip
  // (a layout with cut sub-layers has none either: the one such shape has no context to fold)
  static int64_t pass0_floats() { return CF::LINEAR || CF::CUT ? -1 : CF::C0; }
  static int pack_device(const float* flat, int64_t sflat, const int* perm, float* packed, int64_t spk, int L,
                         int64_t P, hipStream_t s, const float* c0 = nullptr, int64_t sc0 = 0,
                         const float* mask = nullptr) {
    if (c0 != nullptr && CF::LINEAR)
      return set_error("naz_ar_flow_pack: the linear-order spline has no pass-0 constants form");
    if (c0 != nullptr && CF::CUT)
      return set_error("naz_ar_flow_pack: D=%d C=%d H=%d x %d: no pass-0 constants form", CF::D, CF::C, CF::H, CF::NHID);
    if (L == 0 || P == 0) return 0;
    if (P > 65535 || L > 65535) return set_error("naz_ar_flow_pack: at most 65535 draws / layers per call");
    const dim3 grid((unsigned)((CF::LAYER + 255) / 256), (unsigned)L, (unsigned)P);
    hipLaunchKernelGGL((made_ar_pack_kernel<CF>), grid, dim3(256), 0, s, flat, sflat, perm, packed, spk, c0, sc0,
                       mask);
    return check_launch("made_ar_pack_kernel");
  }
};

// wide affine MADE (CfgARW): the sampler over CfgARF's image, log_prob over CfgARIW's
// (made_ar_wide.h: the persistent-grid inverse with hidden layers 2.. in per-wave scratch)
static int device_cu_count() { return device_cus(); }

template <class CW>
struct AROpsW : ARFwdOps<CW> {
  using IW = CfgARIW<CW>;
  static int64_t layer_floats() { return IW::LAYER; }
  static int degrees(int* deg) {
    for (int u = 0; u < CW::H; ++u) deg[u] = CW::deg(u);
    return 0;
  }
  static constexpr int64_t per() { return ARIWFlat<IW>::per(); }
  static_assert(per() == ARFwdOps<CW>::flat_floats(), "the wide packer and the sampler read one flat layout");
  static int pack_host(const float* flat, const int* perm, int L, float* out) {
    for (int l = 0; l < L; ++l) {
      bool seen[32] = {};
      for (int p = 0; p < CW::D; ++p) {
        const int v = perm[l * CW::D + p];
        if (v < 0 || v >= CW::D || seen[v]) return set_error("naz_ar_flow_pack: layer %d: bad permutation", l);
        seen[v] = true;
      }
      made_ar_pack_wide_layer<IW>(flat + l * per(), perm + l * CW::D, out + (int64_t)l * IW::LAYER);
    }
    return 0;
  }
  static int log_prob(const float* packed, int L, const float* x, int64_t ldx, const float* ctx, int64_t ldc,
                      const float* low, const float* high, float* out_lp, int64_t B, float, hipStream_t s,
                      int64_t P = 1, int64_t spk = 0, int64_t sx = 0, int64_t slp = 0, int c0mode = 0,
                      float* states = nullptr, void* ws = nullptr, int64_t ws_bytes = 0) {
    if (c0mode) return set_error("naz_ar_flow: D=%d H=%d x %d: no pass-0 constants form", CW::D, CW::H, CW::NHID);
    if (states != nullptr && (P != 1 || low != nullptr))
      return set_error("naz_ar_flow_log_prob_train: one draw, no bounds");
    if (B == 0 || L == 0 || P == 0) return 0;
    const int64_t grid = grid_size(B, P);
    // the hidden layers 2.. of every resident wave persist in caller-owned workspace (no allocation
    // inside a call: a captured HIP graph replays one fixed address)
    const int64_t need = workspace_bytes(B, P);
    if (ws == nullptr || ws_bytes < need || (reinterpret_cast<uintptr_t>(ws) & 15) != 0)
      return set_error("naz_ar_flow_log_prob: D=%d H=%d x %d needs %lld B of 16-byte aligned workspace "
                       "(naz_ar_flow_workspace_bytes), got %lld B at %p", CW::D, CW::H, CW::NHID, (long long)need,
                       (long long)ws_bytes, ws);
    const size_t lds = (size_t)2 * IW::STG * 4;
    hipLaunchKernelGGL((made_ar_inv_wide_kernel<IW>), dim3((unsigned)grid), dim3(64 * IW::NW), lds, s, packed, L, x,
                       ldx, ctx, ldc, low, high, out_lp, B, P, spk, sx, slp, static_cast<u32x4*>(ws), states);
    return check_launch("made_ar_inv_wide_kernel");
  }
  // the persistent grid: one 4-wave workgroup per CU (at most one per (draw, row tile))
  static int64_t grid_size(int64_t B, int64_t P) {
    const int64_t tiles = (B + 16 * IW::NW - 1) / (16 * IW::NW) * P;
    return std::min<int64_t>(tiles, device_cu_count());
  }
  static int64_t workspace_bytes(int64_t B, int64_t P) {
    if (B <= 0 || P <= 0) return 0;
    return grid_size(B, P) * IW::NW * IW::SCRATCH_U4 * (int64_t)sizeof(u32x4);
  }
  static int64_t pass0_floats() { return -1; }
  static int pack_device(const float* flat, int64_t sflat, const int* perm, float* packed, int64_t spk, int L,
                         int64_t P, hipStream_t s, const float* c0 = nullptr, int64_t = 0,
                         const float* mask = nullptr) {
    if (c0 != nullptr) return set_error("naz_ar_flow_pack: D=%d H=%d x %d: no pass-0 constants form", CW::D, CW::H,
                                        CW::NHID);
    if (L == 0 || P == 0) return 0;
    if (P > 65535 || L > 65535) return set_error("naz_ar_flow_pack: at most 65535 draws / layers per call");
    const dim3 grid((unsigned)((IW::LAYER + 255) / 256), (unsigned)L, (unsigned)P);
    hipLaunchKernelGGL((made_ar_pack_wide_kernel<IW>), grid, dim3(256), 0, s, flat, sflat, perm, packed, spk, mask);
    return check_launch("made_ar_pack_wide_kernel");
  }
};

template <class F>
static int ar_dispatch(const naz_ar_desc* d, F&& f) {
  if (d == nullptr || d->act != NAZ_ACT_TANH || d->L < 0) return -2;
  if (d->kind == NAZ_AR_SPLINE) {
    if (d->K != 8 || d->H != 128 || d->n_hidden != 2 || !(d->bound > 0.f)) return -2;
    if (d->D == 16 && d->C == 32) return f(AROps<CfgAR<16, 32, 128, 8>>{});
    if (d->D == 16 && d->C == 0) return f(AROps<CfgAR<16, 0, 128, 8>>{});
    if (d->D == 8 && d->C == 0) return f(AROps<CfgAR<8, 0, 128, 8>>{});
    if (d->D == 4 && d->C == 2) return f(AROps<CfgAR<4, 2, 128, 8>>{});  // naz nsa bench shape
    return -2;
  }
  if (d->kind == NAZ_AR_SPLINE_LINEAR) {
    // order="linear" (pyro's default): naz's own nsa shape and the no-context layout; log_prob and
    // sample only (the training step and the D = 16 shapes keep the per-kernel chain)
    if (d->K != 8 || d->H != 128 || d->n_hidden != 2 || !(d->bound > 0.f)) return -2;
    if (d->D == 8 && d->C == 0) return f(AROps<ArLin8x0>{});
    if (d->D == 4 && d->C == 2) return f(AROps<ArLin4x2>{});
    return -2;
  }
  if (d->kind == NAZ_AR_AFFINE) {
    // K is unused (the instances carry 8); the maf paper shape (train_mle_all_data.py:62-70) and
    // SURVEY §8d's config-3 AR variant
    if (d->D == 2 && d->C == 2 && d->H == 150 && d->n_hidden == 3) return f(AROps<CfgAR<2, 2, 150, 8, 3, true>>{});
    // the unconditional paper maf (train_mle_unsupervised.py)
    if (d->D == 2 && d->C == 0 && d->H == 150 && d->n_hidden == 3) return f(AROps<ArMaf2x0>{});
    // the 4-parameter Bayesian MAF (calibrate_4p.py:75,90-96; hmc_maf_exact.py:101-133)
    if (d->D == 4 && d->C == 2 && d->H == 150 && d->n_hidden == 3) return f(AROps<CfgAR<4, 2, 150, 8, 3, true>>{});
    if (d->D == 16 && d->C == 32 && d->H == 128 && d->n_hidden == 2) return f(AROps<CfgAR<16, 32, 128, 8, 2, true>>{});
    // naz's production MAFs (4-parameter MLE, POSYDON; AROpsW: the wide sampler and inverse)
    if (d->D == 4 && d->C == 2 && d->H == 512 && d->n_hidden == 5) return f(AROpsW<CfgARW<4, 2, 512, 5>>{});
    return -2;
  }
  return -2;
}

// 1: both directions fused; 2: the forward (sample) direction only (AROpsW); 0: neither
int ar_flow_supported(const naz_ar_desc* d) {
  const int r = ar_dispatch(d, [](auto ops) { return decltype(ops)::layer_floats() < 0 ? 2 : 1; });
  return r > 0 ? r : 0;
}

int64_t ar_flow_packed_bytes(const naz_ar_desc* d) {
  int64_t v = -1;
  ar_dispatch(d, [&](auto ops) {
    v = decltype(ops)::layer_floats() * d->L * 4;
    return 0;
  });
  return v;
}

static int ar_unsupported(const naz_ar_desc* d) {
  if (d == nullptr) return set_error("naz_ar_flow: null descriptor");
  return set_error("naz_ar_flow: no fused instantiation for kind=%d D=%d C=%d H=%d x %d K=%d act=%d", d->kind, d->D,
                   d->C, d->H, d->n_hidden, d->K, d->act);
}

int ar_flow_degrees(const naz_ar_desc* d, int* deg) {
  if (deg == nullptr) return set_error("naz_ar_flow_degrees: null output");
  const int rc = ar_dispatch(d, [&](auto ops) { return decltype(ops)::degrees(deg); });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int ar_flow_pack_host(const naz_ar_desc* d, const float* flat, const int* perm, void* packed) {
  if (flat == nullptr || perm == nullptr || packed == nullptr) return set_error("naz_ar_flow_pack_host: null pointer");
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::pack_host(flat, perm, d->L, static_cast<float*>(packed));
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int64_t ar_flow_fwd_packed_bytes(const naz_ar_desc* d) {
  int64_t v = -1;
  ar_dispatch(d, [&](auto ops) {
    v = decltype(ops)::fwd_layer_floats() * d->L * 4;
    return 0;
  });
  return v;
}

int ar_flow_pack_fwd_host(const naz_ar_desc* d, const float* flat, void* packed) {
  if (flat == nullptr || packed == nullptr) return set_error("naz_ar_flow_pack_fwd_host: null pointer");
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::pack_fwd_host(flat, d->L, static_cast<float*>(packed));
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int ar_flow_sample(const naz_ar_desc* d, const void* packed, const float* z, int64_t ldz, const float* ctx, int64_t ldc,
                   const float* low, const float* high, float* y, int64_t ldy, float* out_ld, int64_t B, hipStream_t s) {
  if ((low == nullptr) != (high == nullptr)) return set_error("naz_ar_flow_sample: low/high must both be set");
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::sample(static_cast<const float*>(packed), d->L, z, ldz, ctx, ldc, low, high, y, ldy, out_ld,
                                 B, d->bound, s);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int ar_flow_pack_fwd(const naz_ar_desc* d, const float* flat, int64_t sflat, void* packed, int64_t spk, int64_t P,
                     const float* mask, hipStream_t s) {
  if (flat == nullptr || packed == nullptr) return set_error("naz_ar_flow_pack_fwd: null pointer");
  const int rc = ar_dispatch(d, [&](auto ops) {
    using O = decltype(ops);
    if (sflat < O::flat_floats() * d->L || spk < O::fwd_layer_floats() * d->L)
      return set_error("naz_ar_flow_pack_fwd: draw strides shorter than one flow");
    return O::pack_fwd_device(flat, sflat, static_cast<float*>(packed), spk, d->L, P, s, mask);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int ar_flow_sample_batched(const naz_ar_desc* d, const void* packed, int64_t spk, const float* z, int64_t ldz,
                           int64_t sz, const float* ctx, int64_t ldc, float* y, int64_t ldy, int64_t sy, float* out_ld,
                           int64_t sld, int64_t B, int64_t P, hipStream_t s) {
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::sample(static_cast<const float*>(packed), d->L, z, ldz, ctx, ldc, nullptr, nullptr, y, ldy,
                                 out_ld, B, d->bound, s, P, spk, sz, sy, sld);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int64_t ar_flow_pass0_floats(const naz_ar_desc* d) {
  int64_t v = -1;
  ar_dispatch(d, [&](auto ops) {
    v = decltype(ops)::pass0_floats() * d->L;
    return 0;
  });
  return v;
}

int ar_flow_pack(const naz_ar_desc* d, const float* flat, int64_t sflat, const int* perm, void* packed, int64_t spk,
                 int64_t P, const float* pass0, int64_t sp0, const float* mask, hipStream_t s) {
  if (flat == nullptr || perm == nullptr || packed == nullptr) return set_error("naz_ar_flow_pack: null pointer");
  if (pass0 != nullptr && (d == nullptr || d->C <= 0))
    return set_error("naz_ar_flow_pack: pass-0 constants need a conditional flow");
  const int rc = ar_dispatch(d, [&](auto ops) {
    using O = decltype(ops);
    if (sflat < O::flat_floats() * d->L || spk < O::layer_floats() * d->L)
      return set_error("naz_ar_flow_pack: draw strides shorter than one flow");
    if (pass0 != nullptr && sp0 < O::pass0_floats() * d->L)
      return set_error("naz_ar_flow_pack: pass-0 stride shorter than one flow");
    return O::pack_device(flat, sflat, perm, static_cast<float*>(packed), spk, d->L, P, s, pass0, sp0, mask);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int64_t ar_flow_workspace_bytes(const naz_ar_desc* d, int64_t B, int64_t P) {
  int64_t v = -1;
  ar_dispatch(d, [&](auto ops) {
    v = decltype(ops)::workspace_bytes(B, P);
    return 0;
  });
  return v;
}

int ar_flow_log_prob_batched(const naz_ar_desc* d, const void* packed, int64_t spk, const float* x, int64_t ldx,
                             int64_t sx, const float* ctx, int64_t ldc, float* out_lp, int64_t slp, int64_t B, int64_t P,
                             int pass0_const, void* ws, int64_t ws_bytes, hipStream_t s) {
  if (pass0_const && (d == nullptr || d->C <= 0 || ldc != 0))
    return set_error("naz_ar_flow_log_prob_batched: pass-0 constants need one context vector (ldc = 0)");
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::log_prob(static_cast<const float*>(packed), d->L, x, ldx, ctx, ldc, nullptr, nullptr, out_lp,
                                   B, d->bound, s, P, spk, sx, slp, pass0_const ? 1 : 0, nullptr, ws, ws_bytes);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int ar_flow_log_prob(const naz_ar_desc* d, const void* packed, const float* x, int64_t ldx, const float* ctx,
                     int64_t ldc, const float* low, const float* high, float* out_lp, int64_t B, void* ws,
                     int64_t ws_bytes, hipStream_t s) {
  if ((low == nullptr) != (high == nullptr)) return set_error("naz_ar_flow_log_prob: low/high must both be set");
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::log_prob(static_cast<const float*>(packed), d->L, x, ldx, ctx, ldc, low, high, out_lp, B,
                                   d->bound, s, 1, 0, 0, 0, 0, nullptr, ws, ws_bytes);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

int ar_flow_log_prob_train(const naz_ar_desc* d, const void* packed, const float* x, int64_t ldx, const float* ctx,
                           int64_t ldc, float* out_lp, float* states, int64_t B, void* ws, int64_t ws_bytes,
                           hipStream_t s) {
  if (states == nullptr) return set_error("naz_ar_flow_log_prob_train: null states");
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::log_prob(static_cast<const float*>(packed), d->L, x, ldx, ctx, ldc, nullptr, nullptr, out_lp,
                                   B, d->bound, s, 1, 0, 0, 0, 0, states, ws, ws_bytes);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

// the nsa training forward: the spline instances of made_ar_r16_kernel with their per-layer outputs saved
int spline_ar_flow_log_prob_train(const naz_ar_desc* d, const void* packed, const float* x, int64_t ldx,
                                  const float* ctx, int64_t ldc, float* out_lp, float* states, int64_t B,
                                  hipStream_t s) {
  if (states == nullptr) return set_error("naz_spline_ar_flow_log_prob_train: null states");
  if (d == nullptr || d->kind != NAZ_AR_SPLINE) return ar_unsupported(d);
  const int rc = ar_dispatch(d, [&](auto ops) {
    return decltype(ops)::log_prob(static_cast<const float*>(packed), d->L, x, ldx, ctx, ldc, nullptr, nullptr, out_lp,
                                   B, d->bound, s, 1, 0, 0, 0, 0, states, nullptr, 0);
  });
  return rc == -2 ? ar_unsupported(d) : rc;
}

}  // namespace naz
