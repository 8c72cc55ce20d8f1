// The x6 family of the fused coupling flow: FP32 GEMMs emulated on the bf16 / fp16 matrix pipe
// (mfma_split.h) with the weights streamed through a two-slot LDS-DMA ring.  CfgX6 is the packed
// image of NAZ_MFMA_BF16X6 (P23 = 3) and NAZ_MFMA_F16X3 (P23 = 2); coupling_w32.h runs the latter
// image and coupling_r16.h reuses the ring geometry and the activation fold.
#pragma once
#include "lds_ring.h"
#include "mfma_split.h"

namespace naz {

// LDS ring: two slots of 40 KB per 128-row workgroup (two workgroups per CU use all 160 KB).
// Stage s+1's LDS-DMA copy lands in one slot while stage s computes from the other.
constexpr int kX6Slot = 10240;         // 40 KB: two workgroups per CU (2 x 2 slots = 160 KB)
constexpr int kX6Waves = 4;            // 128 rows per workgroup
constexpr int kX6Rows = 32 * kX6Waves;
constexpr int kChunk = 256;            // one (block, k-step, piece) A fragment set: 64 lanes x 16 B

template <int D_, int C_, int S_, int K_, int H_, bool LOWER_, int P23_ = 3>
struct CfgX6 {
  static constexpr int D = D_, C = C_, S = S_, K = K_, H = H_;
  static constexpr bool LOWER = LOWER_;
  static constexpr int P23 = P23_;                  // operand pieces of GEMM2/3: 3 = bf16x6, 2 = fp16x3
  static constexpr bool F16 = P23 == 2;
  static constexpr int Dt = D - S, P = 3 * K - 1, DH = Dt / 2, SH = S / 2;
  static constexpr int HB = H / 32;
  static constexpr int CT = (C + 15) / 16;          // GEMM1 k-steps over the context
  static constexpr int XT = (SH + 7) / 8;           // GEMM1 k-steps over the lane-half's x1
  static constexpr int KS0 = CT + XT;
  static constexpr int KS1 = 2 * HB;                // GEMM2/3 k-steps (16 features each)
  static constexpr int NO = (DH * P + 15) / 16;     // GEMM3 output blocks
  static constexpr int TBL = 3 * (K + 1);
  static constexpr int OT = 3 * kChunk;             // floats per (block, k-step), GEMM1
  static constexpr int OT23 = P23 * kChunk;         // floats per (block, k-step), GEMM2/3
  static constexpr int pad(int n) { return (n + 255) / 256 * 256; }
  static constexpr int pick_kb(int nb) {            // largest k-steps-per-stage dividing KS1
    int best = 1;
    for (int kb = 1; kb <= KS1; ++kb)
      if (KS1 % kb == 0 && pad(nb * kb * OT23 + nb * 32) <= kX6Slot) best = kb;
    return best;
  }
  static constexpr int KB2 = pick_kb(HB), NB2 = KS1 / KB2;
  static constexpr int KB3 = pick_kb(NO), NB3 = KS1 / KB3;
  // stage A: [HB][KS0][3][256] | bias [HB][2][16] | tables [S][TBL]
  static constexpr int A_BIAS = HB * KS0 * OT;
  static constexpr int A_TBL = A_BIAS + HB * 32;
  static constexpr int A_SIZE = pad(A_TBL + S * TBL);
  // stages B_q: [HB][KB2][3][256] | bias [HB][2][16]
  static constexpr int B_OFF = A_SIZE;
  static constexpr int B_BIAS = HB * KB2 * OT23;
  static constexpr int B_SIZE = pad(B_BIAS + HB * 32);
  // stages C_q: [NO][KB3][3][256] | bias [NO][2][16]
  static constexpr int C_OFF = B_OFF + NB2 * B_SIZE;
  static constexpr int C_BIAS = NO * KB3 * OT23;
  static constexpr int C_SIZE = pad(C_BIAS + NO * 32);
  // f16x3 configs also carry stage A with GEMM1 in fp16 pieces (same bias/table offsets), used
  // by workgroups whose context and data values all fit fp16's range (kG1F16Limit)
  static constexpr int A16_OFF = C_OFF + NB3 * C_SIZE;
  static constexpr int LAYER = F16 ? A16_OFF + A_SIZE : A16_OFF;
  static constexpr int NSTG = 1 + NB2 + NB3;       // stages per layer
  static constexpr int MAXSTAGE = 2 * kX6Slot;      // LDS floats per workgroup (the ring)
  static constexpr __host__ __device__ int stage_off(int j) {
    return j == 0 ? 0 : (j <= NB2 ? B_OFF + (j - 1) * B_SIZE : C_OFF + (j - 1 - NB2) * C_SIZE);
  }
  static constexpr __host__ __device__ int stage_size(int j) { return j == 0 ? A_SIZE : (j <= NB2 ? B_SIZE : C_SIZE); }
  // natural flat layout (same as the FP32 variant)
  static constexpr int N_W0 = H * (C + S), N_B0 = H, N_W1 = H * H, N_B1 = H, N_W2 = Dt * P * H, N_B2 = Dt * P;
  static constexpr int N_LOW = LOWER ? S * (3 * K - 1) : 0;
  static constexpr int FLAT = N_W0 + N_B0 + N_W1 + N_B1 + N_W2 + N_B2 + N_LOW;
  static_assert(Dt % 2 == 0 && S % 2 == 0 && H % 32 == 0 && S > 0 && Dt > 0, "unsupported coupling shape");
  static_assert(A_SIZE <= kX6Slot && B_SIZE <= kX6Slot && C_SIZE <= kX6Slot, "stage exceeds one LDS ring slot");
  static_assert(HB * KS0 * 2 * kChunk <= A_BIAS, "fp16 GEMM1 panels must fit stage A's panel region");
};

// |value| bound under which GEMM1's B operand (context, x1) is split into fp16 hi + lo: hi
// (round-toward-zero) stays finite and lo = v - hi is exact with 11 significant bits.
constexpr float kG1F16Limit = 32768.f;

// GEMM1 input column (in cat([ctx, x1]) order) for k-step t, element j, lane-half h; -1 = zero pad
template <class CF>
__host__ __device__ constexpr int x6_in_col(int t, int j, int h) {
  if (t < CF::CT) {
    const int c = 16 * t + 8 * h + j;
    return c < CF::C ? c : -1;
  }
  const int q = 8 * (t - CF::CT) + j;
  return q < CF::SH ? CF::C + h * CF::SH + q : -1;
}

// DenseNN output column carried by GEMM3 accumulator (block o, register r) on lane-half h; -1 = pad
template <class CF>
__host__ __device__ constexpr int x6_out_row(int o, int r, int h) {
  const int slot = 16 * o + r, qd = slot / CF::P, p = slot - qd * CF::P;
  if (qd >= CF::DH) return -1;
  const int dim = h * CF::DH + qd;
  if (p < CF::K) return dim * CF::K + p;
  if (p < 2 * CF::K) return CF::Dt * CF::K + dim * CF::K + (p - CF::K);
  return 2 * CF::Dt * CF::K + dim * (CF::K - 1) + (p - 2 * CF::K);
}

// Sigmoid fold.  tanh(a) = −2δ with δ = σ(−2a) − ½ = 1 / (1 + 2^(a·2·log2 e)) − ½, so the fused
// kernel's activation is rcp(1 + exp2(acc)) − ½ (4 VALU instead of 5) when the packer
//   * scales GEMM1 and GEMM2 rows (weights and bias) by kSigScale = 2·log2 e, so their
//     accumulators hold a·2·log2 e, and
//   * scales the weights of each activation's consumer (GEMM2, GEMM3) by −2 (exact).
// δ keeps tanh's relative precision near 0 (σ itself would not: its f16 hi/lo split loses
// ~2^-23 absolute at σ ≈ ½).  The pre-activations equal the tanh form's up to one rounding of
// the kSigScale-scaled weights (2^-24 relative), below the fp32 GEMM's own rounding.
constexpr float kSigScale = 2.88539008177792681f;

template <class CF>
__global__ void coupling_pack_x6_kernel(const float* __restrict__ flat, float* __restrict__ packed, int L,
                                        float bound) {
  const int64_t n = (int64_t)L * CF::LAYER;
  unsigned* pu = reinterpret_cast<unsigned*>(packed);
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    const int l = (int)(e / CF::LAYER);
    const int off = (int)(e - (int64_t)l * CF::LAYER);
    const float* W0 = flat + (int64_t)l * CF::FLAT;
    const float* b0 = W0 + CF::N_W0;
    const float* W1 = b0 + CF::N_B0;
    const float* b1 = W1 + CF::N_W1;
    const float* W2 = b1 + CF::N_B1;
    const float* b2 = W2 + CF::N_W2;
    const float* low = b2 + CF::N_B2;
    // operand chunk entry: (o, t, piece, lane, pair) -> two bf16 of W[row][col(j)], W[row][col(j+1)]
    auto chunk_word = [&](int q, int nt, int t0, const float* W, int ldw, bool gemm1, bool f16g1 = false) -> unsigned {
      const int ot = f16g1 ? 2 * kChunk : (gemm1 ? CF::OT : CF::OT23);
      const bool f16 = f16g1 || (!gemm1 && CF::F16);
      const int o = q / (nt * ot), r1 = q - o * nt * ot;
      const int tl = r1 / ot, r2 = r1 - tl * ot;
      const int piece = r2 / kChunk, u = r2 - piece * kChunk;
      const int lane = u >> 2, pair = u & 3, i = lane & 31, kh = lane >> 5;
      const int t = t0 + tl;
      unsigned out = 0;
      for (int e2 = 0; e2 < 2; ++e2) {
        const int j = 2 * pair + e2;
        int col, row;
        if (gemm1) {
          col = x6_in_col<CF>(t, j, kh);
          row = 32 * o + i;
        } else {
          col = hid16_feature(t, j, kh);
          row = 32 * o + i;
        }
        float v = 0.f;
        if (W == W2) {  // output rows permuted into lane-half spline slots
          const int hh = (i >> 2) & 1, rr = (i & 3) + 4 * (i >> 3);
          const int orow = x6_out_row<CF>(o, rr, hh);
          v = orow >= 0 ? W[orow * ldw + col] : 0.f;
        } else if (col >= 0) {
          v = W[row * ldw + col];
        }
        v *= W == W0 ? kSigScale : (W == W1 ? -2.f * kSigScale : -2.f);  // sigmoid fold (see kSigScale)
        out |= (f16 ? f16_piece_bits(v, piece) : bf16_hi_bits(v, piece)) << (16 * e2);
      }
      return out;
    };
    unsigned word = 0;
    float fv = 0.f;
    bool is_word = false;
    const bool a16 = CF::F16 && off >= CF::A16_OFF;
    const int offa = a16 ? off - CF::A16_OFF : off;
    if (offa < CF::A_SIZE && (a16 || off < CF::A16_OFF)) {
      const int off = offa;
      if (off < CF::A_BIAS) {
        if (!a16 || off < CF::HB * CF::KS0 * 2 * kChunk) {
          word = chunk_word(off, CF::KS0, 0, W0, CF::C + CF::S, true, a16);
          is_word = true;
        }
      } else if (off < CF::A_TBL) {
        const int q = off - CF::A_BIAS, o = q / 32, h = (q >> 4) & 1, r = q & 15;
        fv = kSigScale * b0[32 * o + acc_row(r, h)];
      } else if (CF::LOWER && off < CF::A_TBL + CF::S * CF::TBL) {
        const int q = off - CF::A_TBL, g = q / CF::TBL, w = q - g * CF::TBL;
        float uw[CF::K], uh[CF::K], ud[CF::K - 1];
        for (int k = 0; k < CF::K; ++k) {
          uw[k] = low[g * CF::K + k];
          uh[k] = low[CF::S * CF::K + g * CF::K + k];
        }
        for (int k = 0; k < CF::K - 1; ++k) ud[k] = low[2 * CF::S * CF::K + g * (CF::K - 1) + k];
        SplineTables<CF::K> tb;
        build_tables<CF::K>(uw, uh, ud, bound, tb);
        const int which = w / (CF::K + 1), k = w - which * (CF::K + 1);
        fv = which == 0 ? tb.cw[k] : (which == 1 ? tb.ch[k] : tb.dv[k]);
      }
    } else if (off < CF::C_OFF) {
      const int sq = (off - CF::B_OFF) / CF::B_SIZE, q = off - CF::B_OFF - sq * CF::B_SIZE;
      if (q < CF::B_BIAS) {
        word = chunk_word(q, CF::KB2, sq * CF::KB2, W1, CF::H, false);
        is_word = true;
      } else if (q < CF::B_BIAS + CF::HB * 32) {
        const int qq = q - CF::B_BIAS, o = qq / 32, h = (qq >> 4) & 1, r = qq & 15;
        const int orow = 32 * o + acc_row(r, h);
        fv = kSigScale * b1[orow];
      }
    } else {
      const int sq = (off - CF::C_OFF) / CF::C_SIZE, q = off - CF::C_OFF - sq * CF::C_SIZE;
      if (q < CF::C_BIAS) {
        word = chunk_word(q, CF::KB3, sq * CF::KB3, W2, CF::H, false);
        is_word = true;
      } else if (q < CF::C_BIAS + CF::NO * 32) {
        const int qq = q - CF::C_BIAS, o = qq / 32, h = (qq >> 4) & 1, r = qq & 15;
        const int orow = x6_out_row<CF>(o, r, h);
        fv = orow >= 0 ? b2[orow] : 0.f;
      }
    }
    if (is_word) pu[e] = word;
    else packed[e] = fv;
  }
}

template <int NB, int KB>
NAZ_DEV void gemm_x6_stage(floatx16 (&acc)[NB], const float* __restrict__ stage, int lane, const Frag3 (&bf)[KB]) {
  const u32x4* c4 = reinterpret_cast<const u32x4*>(stage);
#pragma unroll
  for (int t = 0; t < KB; ++t) {
#pragma unroll
    for (int o = 0; o < NB; ++o) {
      const int base = ((o * KB + t) * 3) * 64 + lane;
      Frag3 a{__builtin_bit_cast(bf16x8, c4[base]), __builtin_bit_cast(bf16x8, c4[base + 64]),
              __builtin_bit_cast(bf16x8, c4[base + 128])};
      acc[o] = mfma6(a, bf[t], acc[o]);
    }
  }
}

template <int NB, int KB>
NAZ_DEV void gemm_f16_stage(floatx16 (&acc)[NB], const float* __restrict__ stage, int lane, const Frag2 (&bf)[KB]) {
  const u32x4* c4 = reinterpret_cast<const u32x4*>(stage);
#pragma unroll
  for (int t = 0; t < KB; ++t) {
#pragma unroll
    for (int o = 0; o < NB; ++o) {
      const int base = ((o * KB + t) * 2) * 64 + lane;
      Frag2 a{__builtin_bit_cast(half8, c4[base]), __builtin_bit_cast(half8, c4[base + 64])};
      acc[o] = mfma3(a, bf[t], acc[o]);
    }
  }
}

// GEMM over k-steps [T0, T0+KB) with each B fragment split from the activated accumulator
// just before its MFMAs (keeps one fragment live instead of KB).
template <int NB, int KB, int T0, int NX>
NAZ_DEV void gemm_f16_lazy(floatx16 (&acc)[NB], const float* __restrict__ stage, int lane, const floatx16 (&x)[NX]) {
  const u32x4* c4 = reinterpret_cast<const u32x4*>(stage);
#pragma unroll
  for (int t = 0; t < KB; ++t) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = x[(T0 + t) >> 1][8 * ((T0 + t) & 1) + j];
    const Frag2 b = split8_f16(v);
#pragma unroll
    for (int o = 0; o < NB; ++o) {
      const int base = ((o * KB + t) * 2) * 64 + lane;
      Frag2 a{__builtin_bit_cast(half8, c4[base]), __builtin_bit_cast(half8, c4[base + 64])};
      acc[o] = mfma3(a, b, acc[o]);
    }
  }
}

template <int NB, int KB, int T0, int NX>
NAZ_DEV void gemm_x6_lazy(floatx16 (&acc)[NB], const float* __restrict__ stage, int lane, const floatx16 (&x)[NX]) {
  const u32x4* c4 = reinterpret_cast<const u32x4*>(stage);
#pragma unroll
  for (int t = 0; t < KB; ++t) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = x[(T0 + t) >> 1][8 * ((T0 + t) & 1) + j];
    const Frag3 b = split8(v);
#pragma unroll
    for (int o = 0; o < NB; ++o) {
      const int base = ((o * KB + t) * 3) * 64 + lane;
      Frag3 a{__builtin_bit_cast(bf16x8, c4[base]), __builtin_bit_cast(bf16x8, c4[base + 64]),
              __builtin_bit_cast(bf16x8, c4[base + 128])};
      acc[o] = mfma6(a, b, acc[o]);
    }
  }
}

template <int T0, int KB, int NB>
NAZ_DEV void frags_from_acc(const floatx16 (&x)[NB], Frag2 (&bf)[KB]) {
#pragma unroll
  for (int tl = 0; tl < KB; ++tl) {
    const int t = T0 + tl;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = x[t >> 1][8 * (t & 1) + j];
    bf[tl] = split8_f16(v);
  }
}

// B fragments of k-steps [T0, T0+KB) from an accumulator array (already activated)
template <int T0, int KB, int NB>
NAZ_DEV void frags_from_acc(const floatx16 (&x)[NB], Frag3 (&bf)[KB]) {
#pragma unroll
  for (int tl = 0; tl < KB; ++tl) {
    const int t = T0 + tl;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = x[t >> 1][8 * (t & 1) + j];
    bf[tl] = split8(v);
  }
}

template <class CF, bool DIR_INV>
__global__ void __launch_bounds__(kX6Rows * 2, kX6Waves / 2) coupling_x6_kernel(
    const float* __restrict__ packed, int L, const float* __restrict__ x, int64_t ldx,
    const float* __restrict__ ctx, int64_t ldc, const float* __restrict__ low, const float* __restrict__ high,
    float* __restrict__ out_lp, float* __restrict__ yout, int64_t ldy, int64_t B, float bound) {
  extern __shared__ float4 lds4[];
  float* const slot0 = reinterpret_cast<float*>(lds4);
  float* const slot1 = slot0 + kX6Slot;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int h = lane >> 5;
  const int64_t row = (int64_t)blockIdx.x * kX6Rows + wave * 32 + (lane & 31);
  const bool valid = row < B;
  const int64_t crow = valid ? row : 0;

  float zl[CF::SH], zu[CF::DH];
  float ldsum = 0.f, logjac = 0.f;
#pragma unroll
  for (int q = 0; q < CF::SH; ++q) zl[q] = valid ? x[crow * ldx + h * CF::SH + q] : 0.f;
#pragma unroll
  for (int q = 0; q < CF::DH; ++q) zu[q] = valid ? x[crow * ldx + CF::S + h * CF::DH + q] : 0.f;
  if (DIR_INV && low != nullptr) {  // naz bounding_transform (transforms.py:20-23)
    auto bnd = [&](float& v, int dim) {
      const float lo = low[dim], hi = high[dim];
      const float u = (v - lo) / (hi - lo);
      logjac -= logf(u) + log1pf(-u);
      v = logf(u / (1.f - u));
    };
#pragma unroll
    for (int q = 0; q < CF::SH; ++q) bnd(zl[q], h * CF::SH + q);
#pragma unroll
    for (int q = 0; q < CF::DH; ++q) bnd(zu[q], CF::S + h * CF::DH + q);
    if (h == 0) {
      float sl = 0.f;
      for (int d = 0; d < CF::D; ++d) sl += logf(high[d] - low[d]);
      logjac -= sl;
    }
  }

  // GEMM1 precision path for this workgroup: fp16 pieces when every context and data value of
  // its rows is inside kG1F16Limit (x1 stays inside max(|x|, bound) through the lower
  // splines), else the exact-split bf16x6 path.  Uniform per workgroup: it picks stage A.
  int a_off = 0;
  if constexpr (CF::F16) {
    bool ok = bound < kG1F16Limit;
#pragma unroll
    for (int q = 0; q < CF::SH; ++q) ok = ok && fabsf(zl[q]) < kG1F16Limit;
#pragma unroll
    for (int q = 0; q < CF::DH; ++q) ok = ok && fabsf(zu[q]) < kG1F16Limit;
#pragma unroll
    for (int t = 0; t < CF::CT; ++t)
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) {
        const int c = 16 * t + 8 * h + jj;
        if (c < CF::C) ok = ok && fabsf(ctx[crow * ldc + c]) < kG1F16Limit;
      }
    // workgroup AND through ring slot 1 (unused until the first in-loop barrier; static LDS
    // for __syncthreads_and would push the workgroup past 80 KB = one workgroup per CU)
    int* flags = reinterpret_cast<int*>(slot1);
    const bool wave_ok = __all(ok);  // every lane votes (inside the lane-0 branch only lane 0 would)
    if (lane == 0) flags[wave] = wave_ok ? 1 : 0;
    __syncthreads();
    bool all_ok = true;
#pragma unroll
    for (int w = 0; w < kX6Waves; ++w) all_ok = all_ok && flags[w] != 0;
    a_off = all_ok ? CF::A16_OFF : 0;
  }
  const bool g1f16 = a_off != 0;

  stage_issue<CF::A_SIZE, kX6Waves>(slot0, packed + (int64_t)(DIR_INV ? (L - 1) : 0) * CF::LAYER + a_off);

  const RqsConsts<CF::K, DIR_INV> rc(bound);
  int g = 0;  // global stage counter: stage g lives in slot (g & 1)
  for (int li = 0; li < L; ++li) {
    const int l = DIR_INV ? (L - 1 - li) : li;
    const float* lp = packed + (int64_t)l * CF::LAYER;
    const float* lnext = packed + (int64_t)(DIR_INV ? (l - 1) : (l + 1)) * CF::LAYER;
    floatx16 acc1[CF::HB], acc2[CF::HB], acc3[CF::NO];

    static_for<0, CF::NSTG>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      ring_barrier();  // stage j has landed in slot (g&1); every wave is done with the other slot
      const float* cur = (g & 1) ? slot1 : slot0;
      float* nxt = (g & 1) ? slot0 : slot1;
      if constexpr (j + 1 < CF::NSTG) {
        stage_issue<CF::stage_size(j + 1), kX6Waves>(nxt, lp + CF::stage_off(j + 1));
      } else {
        if (li + 1 < L) stage_issue<CF::A_SIZE, kX6Waves>(nxt, lnext + a_off);
      }
      ++g;

      if constexpr (j == 0) {
        // ---------------- stage A: lower spline (inverse), GEMM1 over [ctx | x1]
        float x1[CF::SH];
#pragma unroll
        for (int q = 0; q < CF::SH; ++q) {
          if constexpr (DIR_INV && CF::LOWER) {
            float ld;
            zl[q] = rqs_table<CF::K, true>(cur + CF::A_TBL + (h * CF::SH + q) * CF::TBL, zl[q], bound, ld);
            ldsum -= ld;
          }
          x1[q] = zl[q];
        }
        auto g1_in = [&](int t, float (&v)[8]) {
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            if (t < CF::CT) {
              const int c = 16 * t + 8 * h + jj;
              v[jj] = (c < CF::C) ? ctx[crow * ldc + c] : 0.f;
            } else {
              const int q = 8 * (t - CF::CT) + jj;
              v[jj] = q < CF::SH ? x1[q < CF::SH ? q : 0] : 0.f;
            }
          }
        };
        init_bias<CF::HB>(acc1, cur + CF::A_BIAS, h);
        if (CF::F16 && g1f16) {
          Frag2 bf[CF::KS0];
#pragma unroll
          for (int t = 0; t < CF::KS0; ++t) {
            float v[8];
            g1_in(t, v);
            bf[t] = split8_f16(v);
          }
          gemm_f16_stage<CF::HB, CF::KS0>(acc1, cur, lane, bf);
        } else {
          Frag3 bf[CF::KS0];
#pragma unroll
          for (int t = 0; t < CF::KS0; ++t) {
            float v[8];
            g1_in(t, v);
            bf[t] = split8(v);
          }
          gemm_x6_stage<CF::HB, CF::KS0>(acc1, cur, lane, bf);
        }
        if constexpr (!DIR_INV && CF::LOWER) {
#pragma unroll
          for (int q = 0; q < CF::SH; ++q) {
            float ld;
            zl[q] = rqs_table<CF::K, false>(cur + CF::A_TBL + (h * CF::SH + q) * CF::TBL, zl[q], bound, ld);
            ldsum += ld;
          }
        }
      } else if constexpr (j <= CF::NB2) {
        // ---------------- stage B_q: GEMM2 k-steps [T0, T0 + KB2)
        constexpr int q = j - 1, T0 = q * CF::KB2;
#pragma unroll
        for (int b = (T0 + 1) / 2; b < (T0 + CF::KB2 + 1) / 2; ++b)  // activate blocks first used here
#pragma unroll
          for (int r = 0; r < 16; ++r) acc1[b][r] = sig_fold(acc1[b][r]);
        if constexpr (q == 0) init_bias<CF::HB>(acc2, cur + CF::B_BIAS, h);
        if constexpr (CF::F16) gemm_f16_lazy<CF::HB, CF::KB2, T0>(acc2, cur, lane, acc1);
        else gemm_x6_lazy<CF::HB, CF::KB2, T0>(acc2, cur, lane, acc1);
      } else {
        // ---------------- stage C_q: GEMM3 k-steps [T0, T0 + KB3) -> raw spline params
        constexpr int q = j - 1 - CF::NB2, T0 = q * CF::KB3;
#pragma unroll
        for (int b = (T0 + 1) / 2; b < (T0 + CF::KB3 + 1) / 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc2[b][r] = sig_fold(acc2[b][r]);
        if constexpr (q == 0) init_bias<CF::NO>(acc3, cur + CF::C_BIAS, h);
        if constexpr (CF::F16) gemm_f16_lazy<CF::NO, CF::KB3, T0>(acc3, cur, lane, acc2);
        else gemm_x6_lazy<CF::NO, CF::KB3, T0>(acc3, cur, lane, acc2);
      }
    });

    // ---------------- upper spline on this lane's DH dims (the next layer's stage A is in flight)
#pragma unroll
    for (int q = 0; q < CF::DH; ++q) {
      float uw[CF::K], uh[CF::K], ud[CF::K - 1];
#pragma unroll
      for (int k = 0; k < CF::K; ++k) {
        const int sw = q * CF::P + k, sh = q * CF::P + CF::K + k;
        uw[k] = acc3[sw >> 4][sw & 15];
        uh[k] = acc3[sh >> 4][sh & 15];
      }
#pragma unroll
      for (int k = 0; k < CF::K - 1; ++k) {
        const int sd = q * CF::P + 2 * CF::K + k;
        ud[k] = acc3[sd >> 4][sd & 15];
      }
      float ld;
      zu[q] = rqs_select<CF::K, DIR_INV>(uw, uh, ud, zu[q], bound, rc, ld);
      ldsum += DIR_INV ? -ld : ld;
    }
  }

  if constexpr (DIR_INV) {
    constexpr float kLogSqrt2Pi = 0.91893853320467274178f;
    float base = 0.f;
#pragma unroll
    for (int q = 0; q < CF::SH; ++q) base += -(zl[q] * zl[q]) / 2.f - kLogSqrt2Pi;
#pragma unroll
    for (int q = 0; q < CF::DH; ++q) base += -(zu[q] * zu[q]) / 2.f - kLogSqrt2Pi;
    float v = base - ldsum + logjac;
    v += __shfl_xor(v, 32);
    if (h == 0 && valid) out_lp[row] = v;
  } else {
    if (low != nullptr) {
#pragma unroll
      for (int q = 0; q < CF::SH; ++q) {
        const int d = h * CF::SH + q;
        zl[q] = (1.f / (1.f + expf(-zl[q]))) * (high[d] - low[d]) + low[d];
      }
#pragma unroll
      for (int q = 0; q < CF::DH; ++q) {
        const int d = CF::S + h * CF::DH + q;
        zu[q] = (1.f / (1.f + expf(-zu[q]))) * (high[d] - low[d]) + low[d];
      }
    }
    if (valid) {
#pragma unroll
      for (int q = 0; q < CF::SH; ++q) yout[row * ldy + h * CF::SH + q] = zl[q];
#pragma unroll
      for (int q = 0; q < CF::DH; ++q) yout[row * ldy + CF::S + h * CF::DH + q] = zu[q];
    }
    if (out_lp != nullptr) {
      float v = ldsum + __shfl_xor(ldsum, 32);
      if (h == 0 && valid) out_lp[row] = v;
    }
  }
}

}  // namespace naz
