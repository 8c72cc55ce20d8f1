// The rational-linear spline's bin arithmetic (pyro _monotonic_rational_spline, order="linear"),
// shared by the standalone kernels (rls.hip, where the formulas are derived) and the fused
// autoregressive flow kernels (made_ar_r16.h): the selected bin, the select-first pick of it from
// the raw parameters, and the two-piece rational-linear map on it with λ = (1 − 2·kMinLambda)·
// sigmoid(u) + kMinLambda.
#pragma once
#include "naz_device.h"

namespace naz {

// The selected bin: x knots, y knots, knot slopes, and the bin's unnormalised λ, which the caller
// fetches by the bin index (one per-lane LDS read; the other K−1 values are never loaded).
template <typename T>
struct RlsBinT {
  T cw0, cw1, ch0, ch1, d0, d1, ul;
  int idx;
};
using RlsBin = RlsBinT<float>;

// Select-first bin (rqs_select's knot form, naz_device.h): prefix sums of the softmax numerators,
// K−1 compares on the searched table, then only the bin's knots, slopes and λ are formed.
template <int K, bool INV>
NAZ_DEV RlsBin rls_pick_select(const float* uw, const float* uh, const float* ud, float x, float bound,
                               const RqsConsts<K, INV>& rc) {
  constexpr float kL2E = 1.44269504088896341f;
  float Ew[K + 1], Eh[K + 1];
  {
    float mw = uw[0], mh = uh[0];
#pragma unroll
    for (int k = 1; k < K; ++k) {
      mw = fmaxf(mw, uw[k]);
      mh = fmaxf(mh, uh[k]);
    }
    const float mwl = mw * kL2E, mhl = mh * kL2E;
    Ew[0] = 0.f;
    Eh[0] = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      Ew[k + 1] = Ew[k] + __builtin_amdgcn_exp2f(__builtin_fmaf(uw[k], kL2E, -mwl));
      Eh[k + 1] = Eh[k] + __builtin_amdgcn_exp2f(__builtin_fmaf(uh[k], kL2E, -mhl));
    }
  }
  const float Aw = rc.cA * Math<true>::rcp(Ew[K]);
  const float Ah = rc.cA * Math<true>::rcp(Eh[K]);
  const float* Es = INV ? Eh : Ew;  // searched table
  const float* Eo = INV ? Ew : Eh;
  const float As = INV ? Ah : Aw, Ao = INV ? Aw : Ah;
  float s0 = 0.f, s1 = Es[1], o0 = 0.f, o1 = Eo[1], udl = ud[0], udh = ud[0];
  int idx = 0;
#pragma unroll
  for (int k = 1; k < K; ++k) {
    const bool s = x >= __builtin_fmaf(As, Es[k], rc.key[k]);
    s0 = s ? Es[k] : s0;
    s1 = s ? Es[k + 1] : s1;
    o0 = s ? Eo[k] : o0;
    o1 = s ? Eo[k + 1] : o1;
    udl = s ? ud[k - 1] : udl;
    if (k < K - 1) udh = s ? ud[k] : udh;
    idx += s ? 1 : 0;
  }
  const bool first = idx == 0, last = idx == K - 1;
  const float fi = (float)idx;
  const float cs0 = __builtin_fmaf(As, s0, __builtin_fmaf(rc.ms, fi, rc.nb));
  const float cs1 = last ? bound : __builtin_fmaf(As, s1, __builtin_fmaf(rc.ms, fi + 1.f, rc.nb));
  const float co0 = __builtin_fmaf(Ao, o0, __builtin_fmaf(rc.mo, fi, rc.nb));
  const float co1 = last ? bound : __builtin_fmaf(Ao, o1, __builtin_fmaf(rc.mo, fi + 1.f, rc.nb));
  const float d0 = first ? 1.f - kMinDerivative : kMinDerivative + softplus<true>(udl);
  const float d1 = last ? 1.f - kMinDerivative : kMinDerivative + softplus<true>(udh);
  return INV ? RlsBin{co0, co1, cs0, cs1, d0, d1, 0.f, idx} : RlsBin{cs0, cs1, co0, co1, d0, d1, 0.f, idx};
}

// The rational-linear map on one bin, v already inside [−B, B]; ld of the map applied.
template <bool INV, typename M, typename T>
NAZ_DEV T rls_bin(const RlsBinT<T>& b, T v, T& ld) {
  const T one = 1, minl = (T)0.025;
  const T W = b.cw1 - b.cw0, H = b.ch1 - b.ch0;
  const T lam = (one - 2 * minl) * M::div(one, one + M::exp(-b.ul)) + minl;
  const T oml = one - lam;
  const T wb = M::sqrt(M::div(b.d0, b.d1));
  const T wc = M::div((lam * b.d0 + oml * wb * b.d1) * W, H);
  const T Hs = M::div(H, oml + lam * wb);
  const T ca = lam * wb * Hs, cb = oml * Hs;
  T out, den, dnum;
  if constexpr (INV) {
    const T u = v - b.ch0, vv = b.ch1 - v;
    const bool left = u <= ca;
    den = left ? wc * (ca - u) + u : wc * (cb - vv) + wb * vv;  // sums of non-negative terms
    const T q = M::div(left ? u * lam : vv * wb * oml, den);
    out = (left ? q : one - q) * W + b.cw0;
    dnum = (left ? lam * ca : wb * oml * cb) * wc * W;
  } else {
    const T th = M::div(v - b.cw0, W), om = one - th;
    const bool left = th <= lam;
    den = left ? (lam - th) + wc * th : wc * om + wb * (th - lam);
    const T q = M::div(left ? wc * ca * th : wc * cb * om, den);
    out = left ? b.ch0 + q : b.ch1 - q;
    dnum = M::div((left ? lam * ca : wb * oml * cb) * wc, W);
  }
  ld = M::log(dnum) - 2 * M::log(den);
  return out;
}
static_assert(kMinLambda == 0.025f, "rls_bin's min_lambda");

}  // namespace naz
