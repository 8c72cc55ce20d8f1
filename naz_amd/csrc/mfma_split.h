// MFMA operand types and the exact operand splits shared by the fused flow kernels: the fp32
// 32x32x2 form, the bf16x6 split (three bf16 pieces, six products) and the f16x3 split (fp16
// hi + lo pieces, three products), the accumulator <-> feature maps of the 32-row layout, and the
// sigmoid-fold activation.
#pragma once
#include "naz_device.h"

#include <type_traits>

namespace naz {

typedef float floatx16 __attribute__((ext_vector_type(16)));

NAZ_DEV floatx16 mfma32(float a, float b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}

// accumulator register r on lane-half h holds feature row (within a 32-block)
__host__ __device__ constexpr int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
// Feature (input column of the next GEMM) carried by k-step t on lane-half h.
__host__ __device__ constexpr int hid_feature(int t, int h) { return 32 * (t >> 4) + acc_row(t & 15, h); }

// Accumulators init from the packed bias block [o][h][16]
template <int NB>
NAZ_DEV void init_bias(floatx16 (&acc)[NB], const float* __restrict__ bias, int h) {
#pragma unroll
  for (int o = 0; o < NB; ++o) {
    const float4* b4 = reinterpret_cast<const float4*>(bias + (o * 2 + h) * 16);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = b4[q];
      acc[o][4 * q + 0] = v.x;
      acc[o][4 * q + 1] = v.y;
      acc[o][4 * q + 2] = v.z;
      acc[o][4 * q + 3] = v.w;
    }
  }
}

template <int I, int N, class F>
NAZ_DEV void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// ===========================================================================
// bf16x6 variant: FP32 GEMMs emulated on the bf16 matrix pipe.
//
// Every fp32 operand v is split EXACTLY into three bf16 pieces by truncation
// (hi = v & 0xffff0000, mid = (v - hi) & 0xffff0000, lo = v - hi - mid, which has at most
// 8 significant bits), and each product W·X is formed from the six largest cross terms
//   Wh·Xh + Wh·Xm + Wm·Xh + Wm·Xm + Wh·Xl + Wl·Xh        (dropped terms ~2^-24 relative)
// with v_mfma_f32_32x32x16_bf16 (exact bf16 products, fp32 accumulate).  Six 32-cycle MFMAs
// per K=16 step replace eight 64-cycle v_mfma_f32_32x32x2_f32: 2.67x the FP32 matrix rate.
// On the oracle (config 3, 4096 rows) the log_prob error statistics vs fp64 are those of
// exact FP32 (median 2.70e-7 vs 2.79e-7, q99 4.08e-6 vs 4.03e-6, max 4.46e-5 vs 4.48e-5);
// dropping any of the six products is 3-5x worse.
//
// Operand mapping (v_mfma_f32_32x32x16_bf16): A[i = l&31][k = 8(l>>5) + j], B[k = 8(l>>5) + j]
// [col = l&31], j = 0..7.  The previous GEMM's accumulator registers 8s..8s+7 of block b ARE
// the B fragment of k-step 2b+s, element j carrying feature hid16_feature(2b+s, j, h); the
// packer permutes W's columns to match.  GEMM1's B fragments are built from the context
// half-row and the lane-half's x1 dims.
// ===========================================================================
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

NAZ_DEV floatx16 mfma_bf16(bf16x8 a, bf16x8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

__host__ __device__ constexpr int hid16_feature(int t, int j, int h) {
  return 32 * (t >> 1) + 16 * (t & 1) + 8 * (j >> 2) + 4 * h + (j & 3);
}

// exact 3-way truncation split of one fp32 value: bit patterns whose upper halves are the bf16s
NAZ_DEV void split3_bits(float v, unsigned& hb, unsigned& mb, unsigned& lb) {
  hb = __float_as_uint(v);
  const float r1 = v - __uint_as_float(hb & 0xffff0000u);
  mb = __float_as_uint(r1);
  const float r2 = r1 - __uint_as_float(mb & 0xffff0000u);
  lb = __float_as_uint(r2);
}

__host__ __device__ inline unsigned bf16_hi_bits(float v, int piece) {
  // host+device reference of the same split (used by the packer)
  unsigned b;
  float r = v;
  for (int p = 0;; ++p) {
    __builtin_memcpy(&b, &r, 4);
    const unsigned t = b & 0xffff0000u;
    if (p == piece) return t >> 16;
    float tf;
    __builtin_memcpy(&tf, &t, 4);
    r = r - tf;
  }
}

struct Frag3 {
  bf16x8 h, m, l;
};

// 8 fp32 values -> three bf16x8 fragments (element j = v[j])
NAZ_DEV Frag3 split8(const float (&v)[8]) {
  u32x4 H, M, L;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    unsigned h0, m0, l0, h1, m1, l1;
    split3_bits(v[2 * q], h0, m0, l0);
    split3_bits(v[2 * q + 1], h1, m1, l1);
    H[q] = __builtin_amdgcn_perm(h1, h0, 0x07060302u);
    M[q] = __builtin_amdgcn_perm(m1, m0, 0x07060302u);
    L[q] = __builtin_amdgcn_perm(l1, l0, 0x07060302u);
  }
  return Frag3{__builtin_bit_cast(bf16x8, H), __builtin_bit_cast(bf16x8, M), __builtin_bit_cast(bf16x8, L)};
}

NAZ_DEV floatx16 mfma6(const Frag3& a, const Frag3& b, floatx16 acc) {
  acc = mfma_bf16(a.l, b.h, acc);  // small terms first
  acc = mfma_bf16(a.h, b.l, acc);
  acc = mfma_bf16(a.m, b.m, acc);
  acc = mfma_bf16(a.m, b.h, acc);
  acc = mfma_bf16(a.h, b.m, acc);
  acc = mfma_bf16(a.h, b.h, acc);
  return acc;
}

// fp16x3 (GEMM2/GEMM3 only, whose B operands are tanh outputs in [-1, 1]): v = hi + lo with
// hi = fp16(v), lo = fp16(v - hi) (v - hi is exact), products Wh·Xh + Wh·Xl + Wl·Xh, at half the
// MFMAs of bf16x6.  Weight range is checked at pack time (|W| < 2^15).
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

NAZ_DEV floatx16 mfma_f16(half8 a, half8 b, floatx16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

struct Frag2 {
  half8 h, l;
};

// v - f32(f16 half of hp) in ONE v_fma_mix_f32 (the compiler emits cvt + sub); exact, since
// v - hi is representable.  HI selects the upper f16 of the packed pair.
template <bool HI>
NAZ_DEV float sub_f16_piece(float v, unsigned hp) {
  float r;
  if constexpr (HI)
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hp), "v"(v));
  else
    asm("v_fma_mix_f32 %0, -%1, 1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(hp), "v"(v));
  return r;
}

typedef _Float16 half2v __attribute__((ext_vector_type(2)));
// round-to-nearest-even pair (one v_cvt_pk_f16_f32 on gfx950, same cost as the RTZ form)
NAZ_DEV unsigned pack_f16x2(float a, float b) {
  const half2v h = {(_Float16)a, (_Float16)b};
  return __builtin_bit_cast(unsigned, h);
}

// The lo pieces are two v_fma_mix_f32 + one v_cvt_pk_f16_f32.  The two-instruction form
// (v_fma_mixlo_f16 / v_fma_mixhi_f16 in inline asm) is NOT used: the compiler's hazard recognizer
// does not see an inline-asm write of the B fragment, so an MFMA issued 1-2 instructions later
// can read the register before the VALU write lands (measured: nsc D=8 flows off by 1e-2
// relative).  The last writer stays a compiler-visible v_cvt_pk_f16_f32.
NAZ_DEV Frag2 split8_f16(const float (&v)[8]) {
  u32x4 H, Lo;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const unsigned hp = pack_f16x2(v[2 * q], v[2 * q + 1]);
    H[q] = hp;
    const float r0 = sub_f16_piece<false>(v[2 * q], hp), r1 = sub_f16_piece<true>(v[2 * q + 1], hp);
    Lo[q] = pack_f16x2(r0, r1);
  }
  return Frag2{__builtin_bit_cast(half8, H), __builtin_bit_cast(half8, Lo)};
}

NAZ_DEV floatx16 mfma3(const Frag2& a, const Frag2& b, floatx16 acc) {
  acc = mfma_f16(a.l, b.h, acc);
  acc = mfma_f16(a.h, b.l, acc);
  acc = mfma_f16(a.h, b.h, acc);
  return acc;
}

// fp16 piece (0 = hi, 1 = lo) of a WEIGHT as 16 bits.  Weights are split with round-to-nearest
// (done once per pack): |lo| <= 2^-12 |W|, so the dropped Wl·Xl term and W's residual error are
// ~2^-24 relative.  Activations use the cheaper truncating split (v_cvt_pkrtz) on the fly.
// On the oracle this RNE(W)/RTZ(X) pairing matches exact FP32 (median 3.1e-7 vs 2.8e-7, q99
// 4.1e-6 vs 4.0e-6); RTZ on both sides is measurably worse (median 3.6e-7, q99 5.1e-6).
NAZ_DEV unsigned f16_piece_bits(float v, int piece) {
  const _Float16 hi = (_Float16)v;
  if (piece == 0) return (unsigned)__builtin_bit_cast(unsigned short, hi);
  const _Float16 lo = (_Float16)(v - (float)hi);
  return (unsigned)__builtin_bit_cast(unsigned short, lo);
}

// activation of the x6 kernels: δ = σ − ½ of the pre-scaled accumulator (see kSigScale)
NAZ_DEV float sig_fold(float a) { return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(a)) - 0.5f; }

}  // namespace naz
