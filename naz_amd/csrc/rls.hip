// Rational-LINEAR spline kernels: pyro's _monotonic_rational_spline with order="linear" (pyro's own
// default order; naz's two spline factories take it, naz/flows/transforms.py:165-171, 201-212).
//
// Knots, knot slopes, bin search and identity tails are the quadratic spline's (naz_device.h).  Per
// bin the conditioner emits one more value, the split position λ = (1 − 2·0.025)·sigmoid(u) + 0.025,
// and the map on the bin is two rational-linear pieces joined at θ = λ (Dolatabadi et al. 2020):
//   wb = sqrt(d0/d1),  δ = H/W,  wc = (λ·d0 + (1−λ)·wb·d1)/δ,  s = (1−λ) + λ·wb,
//   ca = yc − ya = λ·wb·H/s,  cb = yb − yc = (1−λ)·H/s               (wa = 1)
//   forward, θ = (x − xk)/W:   θ ≤ λ:  den = (λ−θ) + wc·θ,        y = ya + wc·ca·θ/den
//                              θ > λ:  den = wc·(1−θ) + wb·(θ−λ),  y = yb − wc·cb·(1−θ)/den
//   inverse, u = y − ya, v = yb − y:
//                              u ≤ ca: den = wc·(ca−u) + u,        θ = u·λ/den
//                              u > ca: den = wc·(cb−v) + wb·v,     θ = 1 − v·wb·(1−λ)/den
//   log-det of the map applied: log(dnum) − 2·log(den), dnum = wc·λ·ca or wb·wc·(1−λ)·cb, over W
//   (forward) or times W (inverse).
// This is pyro's num/den form with the common terms of num and den cancelled (yc never formed);
// every den above is positive on its piece.  Branches are SELECTED, never multiplied by a flag.
//
// The bin pick and the map on the bin (rls_pick_select, rls_bin) live in rls_bin.h, which the fused
// autoregressive kernels include too.
//
// Two evaluators: NAZ_RQS_FAST (inference) in float on the hardware transcendentals; the default
// (the autograd walk's forward) in double, see rls_pick_double.  The VJP runs in float.
//
// Kernel structure is rqs.hip's: one workgroup owns 256/Dt rows, stages their raw block
// (Dt·(4K−1) floats per row) in LDS, one thread per (row, dim), fixed-order LDS row sum of the
// log-det.  Raw layout: DENSE [w(Dt·K) | h(Dt·K) | d(Dt·(K−1)) | l(Dt·K)], ARN column p·Dt + i with
// p = k (w), K+k (h), 2K+k (d), 3K−1+k (λ) — pyro's param_dims order [K, K, K−1, K].
#include "naz_device.h"
#include "naz_internal.h"
#include "rls_bin.h"

// backward on the hardware transcendentals, as the quadratic spline's (rqs.hip)
#ifndef NAZ_RLS_BWD_FAST
#define NAZ_RLS_BWD_FAST true
#endif

namespace naz {

// double-precision math for the accurate evaluator (rls_pick_double)
struct MathD {
  static NAZ_DEV double exp(double x) { return ::exp(x); }
  static NAZ_DEV double log(double x) { return ::log(x); }
  static NAZ_DEV double div(double a, double b) { return a / b; }
  static NAZ_DEV double sqrt(double x) { return ::sqrt(x); }
};

// pyro's clamp(searchsorted(knots + eps) − 1, 0, K−1) on full tables, then register selects.
template <int K, bool INV>
NAZ_DEV RlsBin rls_pick(const SplineTables<K>& t, float v) {
  int cnt = 0;
#pragma unroll
  for (int k = 0; k <= K; ++k) cnt += (v >= (INV ? t.ch[k] : t.cw[k]) + kSearchEps) ? 1 : 0;
  int idx = cnt - 1;
  idx = idx < 0 ? 0 : (idx > K - 1 ? K - 1 : idx);
  RlsBin b{t.cw[0], t.cw[1], t.ch[0], t.ch[1], t.dv[0], t.dv[1], 0.f, idx};
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const bool s = idx == k;
    b.cw0 = s ? t.cw[k] : b.cw0;
    b.cw1 = s ? t.cw[k + 1] : b.cw1;
    b.ch0 = s ? t.ch[k] : b.ch0;
    b.ch1 = s ? t.ch[k + 1] : b.ch1;
    b.d0 = s ? t.dv[k] : b.d0;
    b.d1 = s ? t.dv[k + 1] : b.d1;
  }
  return b;
}

// The accurate evaluator's bin (the autograd walk's forward): softmax, knots, slopes and λ in
// double.  In float the knots carry ~1e-7 absolute error, which an inverse through a flat bin
// (dx/dy up to 1e3) multiplies: the float32 reference itself is off by 9e-6 on such elements of the
// nsc test flow, and a training walk feeds that x to the next layer and to every gradient behind it
// (measured: a lower spline's height gradient 1.2e-5 off from that input error alone, 3e-7 from
// everything else upstream).  Select-first like rls_pick_select: the searched table's prefix sums
// are held, the other table's two are accumulated on the fly.
template <int K, bool INV>
NAZ_DEV RlsBinT<double> rls_pick_double(const float* uw, const float* uh, const float* ud, double x, double bound) {
  constexpr double kMin = 1e-3, kEps = 1e-6;  // pyro's min_bin_width = min_bin_height = min_derivative, search eps
  const float* us = INV ? uh : uw;  // searched table
  const float* uo = INV ? uw : uh;
  float ms = us[0], mo = uo[0];
#pragma unroll
  for (int k = 1; k < K; ++k) {
    ms = fmaxf(ms, us[k]);
    mo = fmaxf(mo, uo[k]);
  }
  double Es[K + 1];
  Es[0] = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) Es[k + 1] = Es[k] + ::exp((double)us[k] - (double)ms);
  const double A = 2.0 * bound * (1.0 - kMin * K), m2 = 2.0 * bound * kMin;
  const double As = A / Es[K];
  double s0 = 0.0, s1 = Es[1];
  float udl = ud[0], udh = ud[0];
  int idx = 0;
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const bool s = x >= As * Es[k] + m2 * k - bound + kEps;
    s0 = s ? Es[k] : s0;
    s1 = s ? Es[k + 1] : s1;
    udl = s ? ud[k - 1] : udl;
    if (k < K - 1) udh = s ? ud[k] : udh;
    idx += s ? 1 : 0;
  }
  double o0 = 0.0, o1 = 0.0, ot = 0.0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double e = ::exp((double)uo[k] - (double)mo);
    o0 += k < idx ? e : 0.0;
    o1 += k <= idx ? e : 0.0;
    ot += e;
  }
  const double Ao = A / ot;
  const bool first = idx == 0, last = idx == K - 1;
  const double cs0 = first ? -bound : As * s0 + m2 * idx - bound;
  const double cs1 = last ? bound : As * s1 + m2 * (idx + 1) - bound;
  const double co0 = first ? -bound : Ao * o0 + m2 * idx - bound;
  const double co1 = last ? bound : Ao * o1 + m2 * (idx + 1) - bound;
  auto softplus_d = [](float u) { return u > 20.f ? (double)u : ::log1p(::exp((double)u)); };
  const double d0 = first ? 1.0 - kMin : kMin + softplus_d(udl);
  const double d1 = last ? 1.0 - kMin : kMin + softplus_d(udh);
  return INV ? RlsBinT<double>{co0, co1, cs0, cs1, d0, d1, 0.0, idx} : RlsBinT<double>{cs0, cs1, co0, co1, d0, d1, 0.0, idx};
}

// One (row, dim); ul[k·uls] is bin k's unnormalised λ (in LDS).  Identity tails (|x| > B, NaN) by
// selection; the bin arithmetic runs on the clamped input, so every intermediate is finite for
// any input.  FAST: hardware transcendentals in float (inference); else the accurate evaluator.
template <int K, bool INV, bool FAST>
NAZ_DEV float rls_eval(const float* uw, const float* uh, const float* ud, const float* ul, int uls, float x,
                       float bound, const RqsConsts<K, INV>& rc, float& ld) {
  const bool inside = x >= -bound && x <= bound;       // false for NaN
  const float v = fminf(fmaxf(x, -bound), bound);      // fmaxf(NaN, −B) = −B
  float lb, y;
  if constexpr (FAST) {
    RlsBin b = rls_pick_select<K, INV>(uw, uh, ud, v, bound, rc);
    b.ul = ul[b.idx * uls];
    y = rls_bin<INV, Math<true>, float>(b, v, lb);
  } else {
    RlsBinT<double> b = rls_pick_double<K, INV>(uw, uh, ud, (double)v, (double)bound);
    b.ul = (double)ul[b.idx * uls];
    double ldd;
    y = (float)rls_bin<INV, MathD, double>(b, (double)v, ldd);
    lb = (float)ldd;
  }
  ld = inside ? lb : 0.f;
  return inside ? y : x;
}

// Raw column of (block, dim i, bin k): blocks w = 0, h = 1, d = 2, λ = 3.
template <int K>
NAZ_DEV int rls_col(int layout, int Dt, int blk, int i, int k) {
  const int p0 = blk == 0 ? 0 : (blk == 1 ? K : (blk == 2 ? 2 * K : 3 * K - 1));  // pyro's param offset
  if (layout == NAZ_LAYOUT_DENSE) return Dt * p0 + i * (blk == 2 ? K - 1 : K) + k;
  return (p0 + k) * Dt + i;
}

template <int K, bool INV, bool FAST>
__global__ void __launch_bounds__(256) rls_cond_kernel(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ raw, int64_t ldr,
    float* __restrict__ y, int64_t ldy, float* __restrict__ ld_out, int ld_mode, int64_t B, int Dt,
    int layout, float bound) {
  extern __shared__ float lds[];
  constexpr int PD = 4 * K - 1;
  const int P = Dt * PD;
  const int R = (Dt >= 256) ? 1 : 256 / Dt;
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int rows = (int)((B - r0) < R ? (B - r0) : R);
  float* raw_s = lds;                 // [R][P]
  float* ld_s = lds + (size_t)R * P;  // [R][Dt]

  if (ldr == P) {
    block_copy_to_lds(raw_s, raw + r0 * ldr, rows * P, tid, blockDim.x);
  } else {
    for (int i = tid; i < rows * P; i += blockDim.x) {
      int r = i / P, c = i - r * P;
      raw_s[i] = raw[(r0 + r) * ldr + c];
    }
  }
  __syncthreads();

  const RqsConsts<K, INV> rc(bound);
  const int uls = layout == NAZ_LAYOUT_DENSE ? 1 : Dt;  // stride between a dim's λ columns
  for (int e = tid; e < rows * Dt; e += blockDim.x) {
    const int r = e / Dt, i = e - r * Dt;
    const float* pr = raw_s + (size_t)r * P;
    float uw[K], uh[K], ud[K - 1];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uw[k] = pr[rls_col<K>(layout, Dt, 0, i, k)];
      uh[k] = pr[rls_col<K>(layout, Dt, 1, i, k)];
    }
#pragma unroll
    for (int k = 0; k < K - 1; ++k) ud[k] = pr[rls_col<K>(layout, Dt, 2, i, k)];
    float ld;
    y[(r0 + r) * ldy + i] = rls_eval<K, INV, FAST>(uw, uh, ud, pr + rls_col<K>(layout, Dt, 3, i, 0), uls,
                                                  x[(r0 + r) * ldx + i], bound, rc, ld);
    if (ld_mode == NAZ_LD_PERDIM) ld_out[(r0 + r) * Dt + i] = ld;
    else ld_s[r * Dt + i] = ld;
  }
  if (ld_mode == NAZ_LD_PERDIM) return;
  __syncthreads();
  for (int r = tid; r < rows; r += blockDim.x) {
    float s = 0.f;
    for (int i = 0; i < Dt; ++i) s += ld_s[r * Dt + i];
    if (ld_mode == NAZ_LD_ROWSUM) ld_out[r0 + r] = s;
    else if (ld_mode == NAZ_LD_ROWSUM_ADD) ld_out[r0 + r] += s;
    else ld_out[r0 + r] -= s;
  }
}

// ---------------------------------------------------------------------------
// VJP.  Reverse mode through rls_bin's formulas (forward: outputs (y, ld); inverse: outputs
// (x, ld of the inverse map)), then the quadratic VJP's chain (spline_bwd.h): bin quantities ->
// knots (pinned ends carry no gradient) -> cumsum -> min-width blend -> softmax, slopes ->
// softplus, and λ -> sigmoid of the selected bin only: the λ block's gradient is g_ul at bin idx
// and 0 elsewhere.  Tails: g_in = g_out, no parameter gradient, decided before any bin arithmetic.
// ---------------------------------------------------------------------------
template <int K, bool INV, bool FAST>
NAZ_DEV float rls_vjp(const float* uw, const float* uh, const float* ud, const float* ul, int uls, float bound,
                      float v, float go, float gld, float* gw, float* gh, float* gd, int& idx, float& g_ul) {
  using M = Math<FAST>;
  auto rcp = [](float b) { return FAST ? Math<true>::rcp(b) : 1.f / b; };
#pragma unroll
  for (int k = 0; k < K; ++k) { gw[k] = 0.f; gh[k] = 0.f; }
#pragma unroll
  for (int k = 0; k < K - 1; ++k) gd[k] = 0.f;
  idx = 0;
  g_ul = 0.f;
  if (!(v >= -bound && v <= bound)) return go;  // identity tails

  float fw[K], fh[K];
  softmax_k<K, FAST>(uw, fw);
  softmax_k<K, FAST>(uh, fh);
  SplineTables<K> t;
  if constexpr (FAST) {
    auto knots32 = [&](const float* frac, float minw, float* knots) {
      const float scale = 1.f - minw * (float)K, two_b = 2.f * bound;
      float acc = 0.f;
      knots[0] = -bound;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        acc += minw + scale * frac[k];
        knots[k + 1] = two_b * acc - bound;
      }
      knots[K] = bound;
    };
    knots32(fw, kMinBinWidth, t.cw);
    knots32(fh, kMinBinHeight, t.ch);
  } else {
    knots_from_fractions<K>(fw, kMinBinWidth, bound, t.cw);
    knots_from_fractions<K>(fh, kMinBinHeight, bound, t.ch);
  }
  t.dv[0] = 1.f - kMinDerivative;
  t.dv[K] = 1.f - kMinDerivative;
#pragma unroll
  for (int k = 0; k < K - 1; ++k) t.dv[k + 1] = kMinDerivative + softplus<FAST>(ud[k]);
  RlsBin b = rls_pick<K, INV>(t, v);
  idx = b.idx;
  b.ul = ul[idx * uls];
  const float d0 = b.d0, d1 = b.d1;

  const float W = b.cw1 - b.cw0, H = b.ch1 - b.ch0, iW = rcp(W);
  const float sg = rcp(1.f + M::exp(-b.ul));
  const float lam = (1.f - 2.f * kMinLambda) * sg + kMinLambda, oml = 1.f - lam;
  const float wb = M::sqrt(d0 * rcp(d1));
  const float delta = H * iW, idl = rcp(delta);
  const float wc = (lam * d0 + oml * wb * d1) * idl;
  const float is = rcp(oml + lam * wb), Hs = H * is;
  const float ca = lam * wb * Hs, cb = oml * Hs;
  const float gl_wc = gld * rcp(wc);  // every ld carries log(wc)

  // gradients on: input, θ-independent knots (cw0, ch0), W, H, and the bin's wc, wb, λ, ca, cb
  float g_in, g_cw0, g_ch0, g_W, g_H, g_wc, g_wb, g_lam, g_ca, g_cb;
  if constexpr (!INV) {
    const float th = (v - b.cw0) * iW, om = 1.f - th;
    const bool left = th <= lam;
    const float den = left ? (lam - th) + wc * th : wc * om + wb * (th - lam);
    const float iden = rcp(den);
    const float A = wc * (left ? ca : cb);
    float g_th = go * A * iden;
    g_ch0 = go;
    if (left) {
      const float g_A = go * th * iden;
      const float g_den = -go * A * th * iden * iden - 2.f * gld * iden;
      g_H = 0.f;
      g_wc = g_A * ca + gl_wc + g_den * th;
      g_ca = g_A * wc + gld * rcp(ca);
      g_cb = 0.f;
      g_wb = 0.f;
      g_lam = gld * rcp(lam) + g_den;
      g_th += g_den * (wc - 1.f);
    } else {
      const float g_A = -go * om * iden;
      const float g_den = go * A * om * iden * iden - 2.f * gld * iden;
      g_H = go;
      g_wc = g_A * cb + gl_wc + g_den * om;
      g_cb = g_A * wc + gld * rcp(cb);
      g_ca = 0.f;
      g_wb = gld * rcp(wb) + g_den * (th - lam);
      g_lam = -gld * rcp(oml) - g_den * wb;
      g_th += g_den * (wb - wc);
    }
    g_in = g_th * iW;
    g_cw0 = -g_in;
    g_W = -gld * iW - g_in * th;
  } else {
    const float u = v - b.ch0, vv = b.ch1 - v;
    const bool left = u <= ca;
    const float den = left ? wc * (ca - u) + u : wc * (cb - vv) + wb * vv;
    const float iden = rcp(den);
    const float gq = go * W;  // on θ
    float th;
    if (left) {
      th = u * lam * iden;
      const float g_den = -(gq * th + 2.f * gld) * iden;
      const float g_u = gq * lam * iden - g_den * (wc - 1.f);
      g_lam = gq * u * iden + gld * rcp(lam);
      g_wc = gl_wc + g_den * (ca - u);
      g_ca = gld * rcp(ca) + g_den * wc;
      g_cb = 0.f;
      g_wb = 0.f;
      g_in = g_u;
      g_ch0 = -g_u;
      g_H = 0.f;
    } else {
      const float tq = vv * wb * oml * iden;  // 1 − θ
      th = 1.f - tq;
      const float g_den = (gq * tq - 2.f * gld) * iden;
      const float g_v = -gq * wb * oml * iden - g_den * (wc - wb);
      g_wb = -gq * vv * oml * iden + gld * rcp(wb) + g_den * vv;
      g_lam = gq * vv * wb * iden - gld * rcp(oml);
      g_wc = gl_wc + g_den * (cb - vv);
      g_cb = gld * rcp(cb) + g_den * wc;
      g_ca = 0.f;
      g_in = -g_v;
      g_ch0 = g_v;
      g_H = g_v;
    }
    g_cw0 = go;
    g_W = go * th + gld * iW;
  }
  // ca = λ·wb·Hs, cb = (1−λ)·Hs, Hs = H/s, s = (1−λ) + λ·wb
  g_lam += (g_ca * wb - g_cb) * Hs;
  g_wb += g_ca * lam * Hs;
  const float g_Hs = g_ca * lam * wb + g_cb * oml;
  g_H += g_Hs * is;
  const float g_s = -g_Hs * Hs * is;
  g_lam += g_s * (wb - 1.f);
  g_wb += g_s * lam;
  // wc = (λ·d0 + (1−λ)·wb·d1)/δ
  const float g_n = g_wc * idl, g_dl = -g_wc * wc * idl;
  g_lam += g_n * (d0 - wb * d1);
  g_wb += g_n * oml * d1;
  // wb = sqrt(d0/d1)
  const float g_d0 = g_n * lam + 0.5f * g_wb * wb * rcp(d0);
  const float g_d1 = g_n * oml * wb - 0.5f * g_wb * wb * rcp(d1);
  // δ = H/W
  g_H += g_dl * iW;
  g_W += -g_dl * delta * iW;

  // bin quantities -> knot / slope arrays
  float gcw[K + 1], gch[K + 1], gdv[K + 1];
#pragma unroll
  for (int k = 0; k <= K; ++k) {
    const float a0 = (k == idx) ? 1.f : 0.f, a1 = (k == idx + 1) ? 1.f : 0.f;
    gcw[k] = a0 * (g_cw0 - g_W) + a1 * g_W;
    gch[k] = a0 * (g_ch0 - g_H) + a1 * g_H;
    gdv[k] = a0 * g_d0 + a1 * g_d1;
  }
  // knots j = 1..K-1 (ends pinned): cw_j = 2B·Σ_{i<j} w_i − B  ->  g_w_i = 2B Σ_{j=i+1}^{K-1} g_cw_j
  const float s_w = 1.f - kMinBinWidth * (float)K, s_h = 1.f - kMinBinHeight * (float)K;
  float gfw[K], gfh[K];
  float accw = 0.f, acch = 0.f;
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    gfw[i] = 2.f * bound * accw * s_w;
    gfh[i] = 2.f * bound * acch * s_h;
    if (i >= 1) {
      accw += gcw[i];
      acch += gch[i];
    }
  }
  float dotw = 0.f, doth = 0.f;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    dotw += fw[i] * gfw[i];
    doth += fh[i] * gfh[i];
  }
  g_ul = g_lam * (1.f - 2.f * kMinLambda) * sg * (1.f - sg);
#pragma unroll
  for (int i = 0; i < K; ++i) {
    gw[i] = fw[i] * (gfw[i] - dotw);
    gh[i] = fh[i] * (gfh[i] - doth);
  }
#pragma unroll
  for (int k = 0; k < K - 1; ++k) gd[k] = gdv[k + 1] * rcp(1.f + M::exp(-ud[k]));  // softplus' = sigmoid
  return g_in;
}

//   g_ld_mode: 0 none, 1 one value per row (the row-sum ld), 2 per (row, dim)
//   BCAST:     raw is ONE row shared by all rows (ldr = 0, the coupling's lower spline): the block
//              reduces d(raw) over its rows in LDS and adds it atomically to g_raw[P].
template <int K, bool INV, bool BCAST>
__global__ void __launch_bounds__(256) rls_bwd_kernel(
    const float* __restrict__ x, int64_t ldx, const float* __restrict__ raw, int64_t ldr,
    const float* __restrict__ g_out, int64_t ldgo, const float* __restrict__ g_ld, int g_ld_mode,
    float* __restrict__ g_in, int64_t ldgi, float* __restrict__ g_raw, int64_t ldgr, int64_t B, int Dt, int layout,
    float bound) {
  extern __shared__ float lds[];
  constexpr int PD = 4 * K - 1;
  const int P = Dt * PD;
  const int R = (Dt >= 256) ? 1 : 256 / Dt;
  const int tid = threadIdx.x;
  const int64_t r0 = (int64_t)blockIdx.x * R;
  const int rows = (int)((B - r0) < R ? (B - r0) : R);
  float* raw_s = lds;  // [R][P] (BCAST: [1][P]) then, for BCAST, grads [R][P]
  float* gr_s = lds + (BCAST ? P : (size_t)R * P);
  if (BCAST) {
    for (int i = tid; i < P; i += blockDim.x) raw_s[i] = raw[i];
    for (int i = tid; i < R * P; i += blockDim.x) gr_s[i] = 0.f;
  } else if (ldr == P) {
    block_copy_to_lds(raw_s, raw + r0 * ldr, rows * P, tid, blockDim.x);
  } else {
    for (int i = tid; i < rows * P; i += blockDim.x) {
      const int r = i / P, c = i - r * P;
      raw_s[i] = raw[(r0 + r) * ldr + c];
    }
  }
  __syncthreads();
  const int uls = layout == NAZ_LAYOUT_DENSE ? 1 : Dt;
  for (int e = tid; e < rows * Dt; e += blockDim.x) {
    const int r = e / Dt, i = e - r * Dt;
    const float* pr = raw_s + (BCAST ? 0 : (size_t)r * P);
    float uw[K], uh[K], ud[K - 1];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uw[k] = pr[rls_col<K>(layout, Dt, 0, i, k)];
      uh[k] = pr[rls_col<K>(layout, Dt, 1, i, k)];
    }
#pragma unroll
    for (int k = 0; k < K - 1; ++k) ud[k] = pr[rls_col<K>(layout, Dt, 2, i, k)];
    const int64_t row = r0 + r;
    const float go = g_out != nullptr ? g_out[row * ldgo + i] : 0.f;
    const float gl = g_ld_mode == 1 ? g_ld[row] : (g_ld_mode == 2 ? g_ld[row * Dt + i] : 0.f);
    float gw[K], gh[K], gd[K - 1], g_ul;
    int idx;
    const float gi = rls_vjp<K, INV, NAZ_RLS_BWD_FAST>(uw, uh, ud, pr + rls_col<K>(layout, Dt, 3, i, 0), uls, bound,
                                                      x[row * ldx + i], go, gl, gw, gh, gd, idx, g_ul);
    if (g_in != nullptr) g_in[row * ldgi + i] = gi;
    float* dst = BCAST ? gr_s + (size_t)r * P : g_raw + row * ldgr;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      dst[rls_col<K>(layout, Dt, 0, i, k)] = gw[k];
      dst[rls_col<K>(layout, Dt, 1, i, k)] = gh[k];
      dst[rls_col<K>(layout, Dt, 3, i, k)] = k == idx ? g_ul : 0.f;
    }
#pragma unroll
    for (int k = 0; k < K - 1; ++k) dst[rls_col<K>(layout, Dt, 2, i, k)] = gd[k];
  }
  if (BCAST) {
    __syncthreads();
    for (int c = tid; c < P; c += blockDim.x) {
      float s = 0.f;
      for (int r = 0; r < rows; ++r) s += gr_s[(size_t)r * P + c];
      atomicAdd(g_raw + c, s);
    }
  }
}

template <int K, bool INV>
static int launch_rls_cond(const float* x, int64_t ldx, const float* raw, int64_t ldr, float* y, int64_t ldy,
                           float* ld, int ld_mode, int64_t B, int Dt, int layout, float bound, hipStream_t s) {
  const bool fast = (layout & NAZ_RQS_FAST) != 0;
  layout &= ~NAZ_RQS_FAST;
  const int R = (Dt >= 256) ? 1 : 256 / Dt;
  const size_t lds = ((size_t)R * Dt * (4 * K - 1) + (size_t)R * Dt) * sizeof(float);
  if (lds > 160 * 1024) return set_error("naz_rls: Dt*K too large for one LDS block (%zu bytes)", lds);
  const int64_t grid = (B + R - 1) / R;
  if (fast)
    hipLaunchKernelGGL((rls_cond_kernel<K, INV, true>), dim3((unsigned)grid), dim3(256), lds, s, x, ldx, raw, ldr, y,
                       ldy, ld, ld_mode, B, Dt, layout, bound);
  else
    hipLaunchKernelGGL((rls_cond_kernel<K, INV, false>), dim3((unsigned)grid), dim3(256), lds, s, x, ldx, raw, ldr,
                       y, ldy, ld, ld_mode, B, Dt, layout, bound);
  return check_launch("rls_cond_kernel");
}

template <int K, bool INV>
static int launch_rls_bwd(const float* x, int64_t ldx, const float* raw, int64_t ldr, const float* g_out,
                          int64_t ldgo, const float* g_ld, int g_ld_mode, float* g_in, int64_t ldgi, float* g_raw,
                          int64_t ldgr, int64_t B, int Dt, int layout, float bound, bool bcast, hipStream_t s) {
  const int R = (Dt >= 256) ? 1 : 256 / Dt;
  const size_t P = (size_t)Dt * (4 * K - 1);
  const size_t lds = (bcast ? (P + (size_t)R * P) : (size_t)R * P) * sizeof(float);
  if (lds > 160 * 1024) return set_error("naz_rls_bwd: Dt*K too large for one LDS block (%zu bytes)", lds);
  const int64_t grid = (B + R - 1) / R;
  if (bcast)
    hipLaunchKernelGGL((rls_bwd_kernel<K, INV, true>), dim3((unsigned)grid), dim3(256), lds, s, x, ldx, raw, ldr, g_out,
                       ldgo, g_ld, g_ld_mode, g_in, ldgi, g_raw, ldgr, B, Dt, layout, bound);
  else
    hipLaunchKernelGGL((rls_bwd_kernel<K, INV, false>), dim3((unsigned)grid), dim3(256), lds, s, x, ldx, raw, ldr,
                       g_out, ldgo, g_ld, g_ld_mode, g_in, ldgi, g_raw, ldgr, B, Dt, layout, bound);
  return check_launch("rls_bwd_kernel");
}

int rls_cond(int inverse, const float* x, int64_t ldx, const float* raw, int64_t ldr, float* y, int64_t ldy,
             float* ld, int ld_mode, int64_t B, int Dt, int K, int layout, float bound, hipStream_t s) {
  if (B == 0) return 0;
  int rc = 0;
#define CALLC(KK)                                                                                              \
  rc = inverse ? launch_rls_cond<KK, true>(x, ldx, raw, ldr, y, ldy, ld, ld_mode, B, Dt, layout, bound, s) \
               : launch_rls_cond<KK, false>(x, ldx, raw, ldr, y, ldy, ld, ld_mode, B, Dt, layout, bound, s)
  NAZ_K_DISPATCH(K, CALLC)
#undef CALLC
  return rc;
}

int rls_bwd(int inverse, const float* x, int64_t ldx, const float* raw, int64_t ldr, const float* g_out, int64_t ldgo,
            const float* g_ld, int g_ld_mode, float* g_in, int64_t ldgi, float* g_raw, int64_t ldgr, int64_t B, int Dt,
            int K, int layout, float bound, hipStream_t s) {
  if (B == 0) return 0;
  const bool bcast = ldr == 0;
  int rc = 0;
#define CALLB(KK)                                                                                                 \
  rc = inverse ? launch_rls_bwd<KK, true>(x, ldx, raw, ldr, g_out, ldgo, g_ld, g_ld_mode, g_in, ldgi, g_raw, ldgr, \
                                          B, Dt, layout, bound, bcast, s)                                       \
               : launch_rls_bwd<KK, false>(x, ldx, raw, ldr, g_out, ldgo, g_ld, g_ld_mode, g_in, ldgi, g_raw,    \
                                           ldgr, B, Dt, layout, bound, bcast, s)
  NAZ_K_DISPATCH(K, CALLB)
#undef CALLB
  return rc;
}

}  // namespace naz
