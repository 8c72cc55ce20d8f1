// MC-dropout form of the fused forward (sampling) kernel of made_ar_r16.h: all L layers of an nsa /
// maf flow in ONE launch with nn.Dropout(p) after every hidden activation (naz
// ConditionalAutoRegressiveNNDropout in train mode; MCDPNormalizingFlow.sample_uncertain, reference
// mcdpflow.py:39-56).  made_ar_fwd_kernel's image, ring schedule and maps; the one difference is that
// each hidden activation becomes keep(seed[l][i], m, n) ? h / (1 - p) : 0 before it is split into the
// next layer's B fragments.
//   * keep is drop_hash (drop_hash.h) against naz_dropout's threshold: m = the row's index in the
//     call + row_offset, n = the hidden unit's natural column 16 b + 4 q + r (block b, quarter q,
//     accumulator register r), so the masks are the ones naz_dropout applies to the [B, H]
//     activation of the per-layer path under the same seed.  Units at or beyond H are exact zeros
//     before and after.
//   * the hash's row term kDropRowMul (m + 1) is formed once per row and xor-ed with the (layer,
//     hidden layer) seed once per layer; the column term is kDropColMul (4 q) (once per lane) plus
//     the compile-time constant kDropColMul (16 b + r + 1) — the same 64-bit value modulo 2^64, so
//     the hash is bit-identical to drop_hash(seed, m, n).
//   * the 1 / (1 - p) scale goes into the ACTIVATION, before the f16 split (the stored activation is
//     δ = σ − ½ with |δ| <= ½, and tanh = −2 δ is folded into the next layer's weights, so dropout of
//     tanh is dropout of δ).  The scaled value must stay inside the f16 hi piece: the entry refuses
//     1 / (1 - p) > kDropMaxScale (|δ'| <= 2^15), it never overflows silently.  With p = 0 the scale
//     is 1 and every unit is kept: bitwise made_ar_fwd_kernel's results.
//   * seeds: one 64-bit seed per (draw, layer, hidden layer) in a device array [P][L][NHID], read by
//     the kernel (nothing baked into the arguments: a captured launch replays with new seeds).
//   * blockIdx.y = draw: all draws share one image; each has its own z, y, out_ld and seeds.
#pragma once
#include "drop_hash.h"
#include "made_ar_r16.h"

namespace naz {

constexpr float kDropMaxScale = 65536.f;

// ar_split4 with the dropout mask: value r of block register r is kept iff keep bit r
template <int HALF>
NAZ_DEV void ar_split4_drop(Frag2& f, const floatx4& a, uint64_t rowseed, uint64_t colbase, uint32_t thresh,
                            float scale) {
  u32x4 H = __builtin_bit_cast(u32x4, f.h), Lo = __builtin_bit_cast(u32x4, f.l);
  float v[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const bool keep = drop_mix(rowseed ^ (colbase + kDropColMul * (uint64_t)r)) >= thresh;
    v[r] = keep ? sig_fold(a[r]) * scale : 0.f;
  }
#pragma unroll
  for (int w = 0; w < 2; ++w) {
    const unsigned hp = pack_f16x2(v[2 * w], v[2 * w + 1]);
    H[2 * HALF + w] = hp;
    Lo[2 * HALF + w] = pack_f16x2(sub_f16_piece<false>(v[2 * w], hp), sub_f16_piece<true>(v[2 * w + 1], hp));
  }
  f.h = __builtin_bit_cast(half8, H);
  f.l = __builtin_bit_cast(half8, Lo);
}

template <class CF>
__global__ void __launch_bounds__(64 * CF::NW, CF::NW / 4) made_ar_fwd_drop_kernel(
    const float* __restrict__ packed, int L, const float* __restrict__ z, int64_t ldz, int64_t sz,
    const float* __restrict__ ctx, int64_t ldc, const float* __restrict__ low, const float* __restrict__ high,
    float* __restrict__ y, int64_t ldy, int64_t sy, float* __restrict__ out_ld, int64_t sld, int64_t B, float bound,
    const uint64_t* __restrict__ seeds, int64_t row_offset, uint32_t thresh, float scale) {
  constexpr int D = CF::D, K = CF::K, NW = CF::NW, NHID = CF::NHID, HB = CF::HB, KSH = CF::KSH;
  static_assert(NW != 4 && !CF::LINEAR, "the quadratic-spline and narrow affine instances only");
  {
    const int64_t dz = blockIdx.y;
    z += dz * sz;
    y += dz * sy;
    if (out_ld != nullptr) out_ld += dz * sld;
    seeds += dz * L * NHID;
  }
  extern __shared__ float4 lds4[];
  float* const slot0 = reinterpret_cast<float*>(lds4);
  float* const slot1 = slot0 + CF::STG;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int q = lane >> 4;
  const int64_t row = (int64_t)blockIdx.x * (16 * NW) + wave * 16 + (lane & 15);
  const bool valid = row < B;
  const int64_t crow = valid ? row : 0;
  // the hash's per-row and per-lane terms (drop_hash: seed ^ rowterm ^ (colq + constant))
  const uint64_t rowterm = kDropRowMul * (uint64_t)(row + row_offset + 1);
  const uint64_t colq = kDropColMul * (uint64_t)(4 * q);

  float v[D];
#pragma unroll
  for (int d = 0; d < D; ++d) v[d] = valid ? z[crow * ldz + d] : 0.f;
  Frag2 cf[CF::KC > 0 ? CF::KC : 1];
#pragma unroll
  for (int t = 0; t < CF::KC; ++t) {
    float c8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int col = 32 * t + 8 * q + j;
      c8[j] = col < CF::C ? ctx[crow * ldc + col] : 0.f;
    }
    cf[t] = split8_f16(c8);
  }
  const RqsConsts<K, false> rc(bound);
  float ldsum = 0.f;
  stage_issue<CF::stage_floats(0), NW>(slot0, packed);
  int g = 0;
  for (int l = 0; l < L; ++l) {
    const float* lp = packed + (int64_t)l * CF::LAYER;
    const float* lnext = packed + (int64_t)(l + 1) * CF::LAYER;
    uint64_t rowseed[NHID];  // seed[l][i] ^ rowterm
#pragma unroll
    for (int i = 0; i < NHID; ++i) rowseed[i] = seeds[(int64_t)l * NHID + i] ^ rowterm;
    Frag2 hf[2][KSH];  // hidden layer i's B fragments in hf[i & 1]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int t = 0; t < KSH; ++t) hf[i][t] = Frag2{half8{}, half8{}};
    // the layer input's f16 split at a per-row power-of-two scale (|x| sc < 2^14)
    float xmax = 0.f;
    if constexpr (CF::AFFINE) {
#pragma unroll
      for (int d = 0; d < D; ++d) xmax = fmaxf(xmax, fabsf(v[d]));
    }
    const int e = xmax >= 16384.f ? __builtin_amdgcn_frexp_expf(xmax) - 14 : 0;
    const float sc = __builtin_amdgcn_ldexpf(1.f, -e), us = __builtin_amdgcn_ldexpf(1.f, e);
    float x8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float s = 0.f;
#pragma unroll
      for (int qq = 0; qq < 4; ++qq)
        if (8 * qq + j < D) s = q == qq ? v[8 * qq + j] : s;
      x8[j] = s * sc;
    }
    const Frag2 xf = split8_f16(x8);
    const float* cur = slot0;
    static_for<0, CF::NU>([&](auto uc) {
      constexpr int u = decltype(uc)::value;
      constexpr int SID = CF::stage_id(u), OFF = CF::unit_off(u);
      constexpr bool NEW_STAGE = u == 0 || SID != CF::stage_id(u > 0 ? u - 1 : 0);
      if constexpr (NEW_STAGE) {  // stage SID has landed in slot (g & 1)
        ring_barrier();  // ... and every wave is done with the other slot
        cur = (g & 1) ? slot1 : slot0;
        float* nxt = (g & 1) ? slot0 : slot1;
        if constexpr (SID + 1 < CF::NSTG) {
          stage_issue<CF::stage_floats(SID + 1), NW>(nxt, lp + (SID + 1) * CF::STG);
        } else {
          if (l + 1 < L) stage_issue<CF::stage_floats(0), NW>(nxt, lnext);
        }
        ++g;
      }
      // the unconditional maf (one degree class: every hidden block of layers 2.. reads all KSH
      // k-steps): scheduled freely across units the D=2 | C=0 instance needs one register more than
      // the 256 of its launch bounds (8 B/lane of scratch); one unit at a time it fits with none
      if constexpr (CF::AFFINE && CF::C == 0) __builtin_amdgcn_sched_barrier(0);
      const u32x4* c4 = reinterpret_cast<const u32x4*>(cur);
      auto afrag = [&](int idx) {
        const int base = (OFF >> 2) + idx * 128 + lane;
        return Frag2{__builtin_bit_cast(half8, c4[base]), __builtin_bit_cast(half8, c4[base + 64])};
      };
      if constexpr (u < NHID * HB) {
        constexpr int i = u / HB, b = u % HB, KT = CF::unit_kts(u);
        const float4 bv = reinterpret_cast<const float4*>(cur + OFF + KT * CF::OT)[q];
        floatx4 acc = floatx4{bv.x, bv.y, bv.z, bv.w};
        if constexpr (i == 0) {
#pragma unroll
          for (int t = 0; t < CF::KC; ++t) acc = mfma3_16(afrag(t), cf[t], acc);
          const floatx4 ax = mfma3_16(afrag(CF::KC), xf, floatx4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[r] = __builtin_fmaf(ax[r], us, acc[r]);
        } else {
#pragma unroll
          for (int t = 0; t < KT; ++t) acc = mfma3_16(afrag(t), hf[(i - 1) & 1][t], acc);
        }
        // unit n = 16 b + 4 q + r: column term kDropColMul (n + 1) = colq + kDropColMul (16 b + 1 + r)
        ar_split4_drop<b & 1>(hf[i & 1][b >> 1], acc, rowseed[i], colq + kDropColMul * (uint64_t)(16 * b + 1), thresh,
                              scale);
      } else {
        // dims 4 g .. 4 g + 3: one dim per row quarter (made_ar_fwd_kernel's output unit)
        constexpr int g = u - NHID * HB, NOG = CF::NOG;
        floatx4 o3[NOG];
        const float4* bias4 = reinterpret_cast<const float4*>(cur + OFF + NOG * KSH * CF::OT);
#pragma unroll
        for (int o = 0; o < NOG; ++o) {
          const float4 bv = bias4[4 * o + q];
          o3[o] = floatx4{bv.x, bv.y, bv.z, bv.w};
        }
#pragma unroll
        for (int t = 0; t < KSH; ++t)
#pragma unroll
          for (int o = 0; o < NOG; ++o) o3[o] = mfma3_16(afrag(o * KSH + t), hf[(NHID - 1) & 1][t], o3[o]);
        float xv = 0.f;  // this quarter's dim
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          if (4 * g + qq < D) xv = q == qq ? v[4 * g + qq < D ? 4 * g + qq : 0] : xv;
        const bool own = 4 * g + q < D;
        float yv, ld;
        if constexpr (CF::AFFINE) {
          const float ls = fminf(fmaxf(o3[0][1], -5.f), 3.f);
          yv = __builtin_fmaf(xv, __expf(ls), o3[0][0]);
          ld = ls;
        } else {
          float uw[K], uh[K], ud[K - 1];
#pragma unroll
          for (int pi = 0; pi < 3 * K - 1; ++pi) {
            const float val = o3[pi >> 2][pi & 3];
            if (pi < K) uw[pi] = val;
            else if (pi < 2 * K) uh[pi - K] = val;
            else ud[pi - 2 * K] = val;
          }
          yv = rqs_select<K, false>(uw, uh, ud, xv, bound, rc, ld);
        }
        ldsum += own ? ld : 0.f;  // summed over the quarters at the end
#pragma unroll
        for (int qq = 0; qq < 4; ++qq)
          if (4 * g + qq < D) v[4 * g + qq < D ? 4 * g + qq : 0] = __shfl(yv, (lane & 15) + 16 * qq);
        __builtin_amdgcn_sched_barrier(0);  // as made_ar_fwd_kernel: keep the groups' output MFMAs apart
      }
    });
  }
  if (low != nullptr) {  // naz inverse_bounding_transform (transforms.py:24-27, flow.py:129)
#pragma unroll
    for (int d = 0; d < D; ++d) v[d] = (1.f / (1.f + expf(-v[d]))) * (high[d] - low[d]) + low[d];
  }
  ldsum += __shfl_xor(ldsum, 16);
  ldsum += __shfl_xor(ldsum, 32);
  if (q == 0 && valid) {
#pragma unroll
    for (int d = 0; d < D; ++d) y[row * ldy + d] = v[d];
    if (out_ld != nullptr) out_ld[row] = ldsum;
  }
}

// the instances: compiled in made_ar_dropout.hip, launched from there
using ArDropMaf2x2 = CfgARF<CfgAR<2, 2, 150, 8, 3, true>>;  // the paper maf
using ArDropMaf4x2 = CfgARF<CfgAR<4, 2, 150, 8, 3, true>>;  // the 4-parameter maf
using ArDropMaf2x0 = CfgARF<CfgAR<2, 0, 150, 8, 3, true>>;  // the unconditional paper maf
using ArDropNsa4x2 = CfgARF<CfgAR<4, 2, 128, 8>>;           // naz's own nsa shape (quadratic)

}  // namespace naz
