// Host dispatch of the fused maf backward (made_ar_bwd.h): the NUTS potential's gradient / the
// maf NLL step, ar_flow_bwd_* and ar_flow_pack_bwd; and of its spline instance, the nsa NLL step,
// spline_ar_flow_bwd_* and spline_ar_flow_pack_bwd.
#include "made_ar_bwd.h"
#include "made_ar_uncond.h"
#include "naz_internal.h"

#include <algorithm>
#include <type_traits>

namespace naz {

// the unconditional paper maf's kernels are compiled in made_ar_uncond.hip
NAZ_AR_BWD_KERNELS(extern, ArMaf2x0)

// Both families over one CfgARB image: the affine ("maf") instances launch made_ar_bwd_kernel, the
// spline ("nsa") ones made_ar_spline_bwd_kernel.  ENTRY prefixes the messages with the family's entries.
template <class CF>
struct ARBwdOps {
  using CB = CfgARB<CF>;
  static constexpr const char* ENTRY = CB::AFFINE ? "naz_ar_flow" : "naz_spline_ar_flow";
  static int64_t layer_floats() { return CB::LAYER; }
  static int dims(int* w) {  // operand widths: n_hidden, HP, XA, XB, X0W, (spline: GOW,) rows per tile
    int n = 0;
    w[n++] = CB::NHID;
    w[n++] = CB::HP;
    w[n++] = CB::XA;
    w[n++] = CB::XB;
    w[n++] = CB::X0W;
    if constexpr (!CB::AFFINE) w[n++] = CB::GOW;
    w[n] = 16 * CB::NW;
    return 0;
  }
  static int pack(const float* flat, const float* mask, float* packed, int L, hipStream_t s) {
    if (L == 0) return 0;
    if (L > 65535) return set_error("%s_pack_bwd: at most 65535 layers", ENTRY);
    const dim3 grid((unsigned)((CB::LAYER + 255) / 256), (unsigned)L);
    hipLaunchKernelGGL((made_ar_pack_bwd_kernel<CB>), grid, dim3(256), 0, s, flat, mask, packed);
    return check_launch("made_ar_pack_bwd_kernel");
  }
  // B rows of one layer through `kernel`: one workgroup per CU at a time (160 KB ring)
  template <class K, class... A>
  static int launch(K kernel, const char* what, int64_t B, hipStream_t s, A... args) {
    if (B == 0) return 0;
    const int64_t grid = (B + 16 * CB::NW - 1) / (16 * CB::NW);
    if (grid > 0x7fffffff) return set_error("%s_bwd_layer: batch too large for one launch", ENTRY);
    const size_t lds = (size_t)2 * CB::SLOT * 4;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(64 * CB::NW), lds, s, args...);
    return check_launch(what);
  }
  static int layer(const float* fimg, const float* bimg, const int* perm, const float* s_in, const float* ctx,
                   int64_t ldc, const float* g_in, const float* g_lp, const ArBwdOut& o, int64_t B, int clip_zero,
                   hipStream_t s) {
    return launch(made_ar_bwd_kernel<CB>, "made_ar_bwd_kernel", B, s, fimg, bimg, perm, s_in, ctx, ldc, g_in, g_lp, o,
                  B, clip_zero);
  }
  static int layer(const float* fimg, const float* bimg, const int* perm, const float* s_out, const float* s_in,
                   const float* ctx, int64_t ldc, const float* g_in, const float* g_lp, const ArBwdOut& o, int64_t B,
                   float bound, hipStream_t s) {
    return launch(made_ar_spline_bwd_kernel<CB>, "made_ar_spline_bwd_kernel", B, s, fimg, bimg, perm, s_out, s_in, ctx,
                  ldc, g_in, g_lp, o, B, bound);
  }
  // bufs (x0, then per hidden layer i (ha_i, hb_i), then dp_i, then gout) and g_out bound into `o`;
  // nonzero, with the message, when an operand this shape writes is null
  static int bind(float* const* bufs, float* g_out, ArBwdOut& o) {
    for (int k = 0; k < 2 + 3 * CB::NHID; ++k)
      if (bufs[k] == nullptr && !(k >= 1 && k <= 2 * CB::NHID && (k & 1) == 0 && CB::XB == 0))
        return set_error("%s_bwd_layer: null operand buffer %d", ENTRY, k);
    o.x0 = bufs[0];
    for (int i = 0; i < CB::NHID; ++i) {
      o.ha[i] = bufs[1 + 2 * i];
      o.hb[i] = bufs[2 + 2 * i];
      o.dp[i] = bufs[1 + 2 * CB::NHID + i];
    }
    o.gout = bufs[1 + 3 * CB::NHID];
    o.g_next = g_out;
    return 0;
  }
  // layer `layer`'s forward and backward image
  static const float* fimg(const void* packed_fwd, int layer) {
    return static_cast<const float*>(packed_fwd) + (int64_t)layer * CB::FW::LAYER;
  }
  static const float* bimg(const void* packed_bwd, int layer) {
    return static_cast<const float*>(packed_bwd) + (int64_t)layer * CB::LAYER;
  }
};

template <class F>
static int ar_bwd_dispatch(const naz_ar_desc* d, F&& f) {
  if (d == nullptr || d->act != NAZ_ACT_TANH || d->L < 0 || d->kind != NAZ_AR_AFFINE) return -2;
  // the maf paper shape (train_mle_all_data.py:62-70; the NUTS potential of hmc_maf_exact.py)
  if (d->D == 2 && d->C == 2 && d->H == 150 && d->n_hidden == 3) return f(ARBwdOps<CfgAR<2, 2, 150, 8, 3, true>>{});
  // the 4-parameter Bayesian MAF's NUTS potential (calibrate_4p.py:75,90-96; hmc_maf_exact.py:101-133)
  if (d->D == 4 && d->C == 2 && d->H == 150 && d->n_hidden == 3) return f(ARBwdOps<CfgAR<4, 2, 150, 8, 3, true>>{});
  // the unconditional paper maf's NLL step (train_mle_unsupervised.py)
  if (d->D == 2 && d->C == 0 && d->H == 150 && d->n_hidden == 3) return f(ARBwdOps<ArMaf2x0>{});
  return -2;
}

static int ar_bwd_unsupported(const naz_ar_desc* d) {
  if (d == nullptr) return set_error("naz_ar_flow_bwd: null descriptor");
  return set_error("naz_ar_flow_bwd: no fused backward for kind=%d D=%d C=%d H=%d x %d act=%d", d->kind, d->D, d->C,
                   d->H, d->n_hidden, d->act);
}

int64_t ar_flow_bwd_packed_bytes(const naz_ar_desc* d) {
  int64_t v = -1;
  ar_bwd_dispatch(d, [&](auto ops) {
    v = decltype(ops)::layer_floats() * d->L * 4;
    return 0;
  });
  return v;
}

int ar_flow_bwd_dims(const naz_ar_desc* d, int* dims) {
  if (dims == nullptr) return set_error("naz_ar_flow_bwd_dims: null output");
  const int rc = ar_bwd_dispatch(d, [&](auto ops) { return decltype(ops)::dims(dims); });
  return rc == -2 ? ar_bwd_unsupported(d) : rc;
}

int ar_flow_pack_bwd(const naz_ar_desc* d, const float* flat, const float* mask, void* packed, hipStream_t s) {
  if (flat == nullptr || packed == nullptr) return set_error("naz_ar_flow_pack_bwd: null pointer");
  const int rc = ar_bwd_dispatch(d, [&](auto ops) {
    return decltype(ops)::pack(flat, mask, static_cast<float*>(packed), d->L, s);
  });
  return rc == -2 ? ar_bwd_unsupported(d) : rc;
}

int ar_flow_bwd_layer(const naz_ar_desc* d, const void* packed_fwd, const void* packed_bwd, const int* perm, int layer,
                      const float* state, const float* ctx, int64_t ldc, const float* g_in, const float* g_lp,
                      float* const* bufs, float* g_out, int64_t B, hipStream_t s) {
  if (d == nullptr || layer < 0 || layer >= d->L) return set_error("naz_ar_flow_bwd_layer: layer out of range");
  const int rc = ar_bwd_dispatch(d, [&](auto ops) {
    using O = decltype(ops);
    ArBwdOut o{};
    if (const int e = O::bind(bufs, g_out, o)) return e;
    return O::layer(O::fimg(packed_fwd, layer), O::bimg(packed_bwd, layer), perm + (int64_t)layer * O::CB::D, state,
                    ctx, ldc, g_in, g_lp, o, B, (d->flags & NAZ_AR_CLIP_ZERO_GRAD) ? 1 : 0, s);
  });
  return rc == -2 ? ar_bwd_unsupported(d) : rc;
}

// the spline ("nsa") family
template <class F>
static int spline_ar_bwd_dispatch(const naz_ar_desc* d, F&& f) {
  if (d == nullptr || d->act != NAZ_ACT_TANH || d->L < 0 || d->kind != NAZ_AR_SPLINE) return -2;
  if (d->K != 8 || d->H != 128 || d->n_hidden != 2 || !(d->bound > 0.f)) return -2;
  // naz's own nsa shape (the `--flow nsa` bench case)
  if (d->D == 4 && d->C == 2) return f(ARBwdOps<CfgAR<4, 2, 128, 8>>{});
  return -2;
}

static int spline_ar_bwd_unsupported(const naz_ar_desc* d) {
  if (d == nullptr) return set_error("naz_spline_ar_flow_bwd: null descriptor");
  return set_error("naz_spline_ar_flow_bwd: no fused backward for kind=%d D=%d C=%d H=%d x %d K=%d act=%d", d->kind,
                   d->D, d->C, d->H, d->n_hidden, d->K, d->act);
}

int64_t spline_ar_flow_bwd_packed_bytes(const naz_ar_desc* d) {
  int64_t v = -1;
  spline_ar_bwd_dispatch(d, [&](auto ops) {
    v = decltype(ops)::layer_floats() * d->L * 4;
    return 0;
  });
  return v;
}

int spline_ar_flow_bwd_dims(const naz_ar_desc* d, int* dims) {
  if (dims == nullptr) return set_error("naz_spline_ar_flow_bwd_dims: null output");
  const int rc = spline_ar_bwd_dispatch(d, [&](auto ops) { return decltype(ops)::dims(dims); });
  return rc == -2 ? spline_ar_bwd_unsupported(d) : rc;
}

int spline_ar_flow_pack_bwd(const naz_ar_desc* d, const float* flat, const float* mask, void* packed, hipStream_t s) {
  if (flat == nullptr || packed == nullptr) return set_error("naz_spline_ar_flow_pack_bwd: null pointer");
  const int rc = spline_ar_bwd_dispatch(d, [&](auto ops) {
    return decltype(ops)::pack(flat, mask, static_cast<float*>(packed), d->L, s);
  });
  return rc == -2 ? spline_ar_bwd_unsupported(d) : rc;
}

int spline_ar_flow_bwd_layer(const naz_ar_desc* d, const void* packed_fwd, const void* packed_bwd, const int* perm,
                             int layer, const float* state_out, const float* state_in, const float* ctx, int64_t ldc,
                             const float* g_in, const float* g_lp, float* const* bufs, float* g_out, int64_t B,
                             hipStream_t s) {
  if (d == nullptr || layer < 0 || layer >= d->L) return set_error("naz_spline_ar_flow_bwd_layer: layer out of range");
  const int rc = spline_ar_bwd_dispatch(d, [&](auto ops) {
    using O = decltype(ops);
    ArBwdOut o{};
    if (const int e = O::bind(bufs, g_out, o)) return e;
    return O::layer(O::fimg(packed_fwd, layer), O::bimg(packed_bwd, layer), perm + (int64_t)layer * O::CB::D, state_out,
                    state_in, ctx, ldc, g_in, g_lp, o, B, d->bound, s);
  });
  return rc == -2 ? spline_ar_bwd_unsupported(d) : rc;
}

}  // namespace naz
