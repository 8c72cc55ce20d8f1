// LDS staging primitives of the fused flow kernels: HBM/L2 -> LDS stage copies by LDS-DMA (the
// two-slot weight ring published by naz_device.h's ring_barrier) and untracked LDS reads with
// counted waits.
#pragma once
#include "naz_device.h"

namespace naz {

// ---------------------------------------------------------------------------
// Stage copy HBM/L2 -> LDS (16-byte loads, all 256 threads)
// ---------------------------------------------------------------------------
// LDS (address space 3) pointer of a generic pointer into __shared__ memory: the low 32 bits
// of a flat LDS address are the LDS offset.  An addrspacecast would instead emit a null check
// against src_shared_base, which hipcc (ROCm 7.2) mis-encodes (v_cmp_ne_u32_e32 with
// src_shared_base as src1: "Operand has incorrect register class") once the address space
// cannot be inferred (the wide H = 512 forward kernel).
NAZ_DEV __attribute__((address_space(3))) void* to_lds(const void* p) {
  return (__attribute__((address_space(3))) void*)(uint32_t)(uintptr_t)p;
}

typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
// One 16-byte LDS read whose destination hipcc does not track (inline asm): the compiler's waitcnt
// model treats LDS returns as out of order while an LDS-DMA (global_load_lds) is in flight — i.e.
// always inside the ring kernels — and so waits lgkmcnt(0) before every use, including on the
// reads just issued for the NEXT use.  Here the wait is explicit and counted (lds_wait<N>): LDS
// reads return in order (LGKM also counts SMEM, which returns out of order: the kernels using this
// issue none across a counted wait — tests/test_isa_ring.py's counted-wait rule — and the DMA
// counts on vmcnt).  Users: coupling_w32.h (A fragments), made_ar_wide.h.
template <int OFF>
NAZ_DEV u32x4_t lds_read_b128_untracked(unsigned addr) {
  u32x4_t v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF));
  return v;
}
template <int N>
NAZ_DEV void lds_wait() {
  // s_waitcnt lgkmcnt(N), vmcnt / expcnt left at their maxima (gfx9 encoding)
  __builtin_amdgcn_s_waitcnt(0xC07F | (N << 8));
}

// Asynchronous stage copy HBM/L2 -> LDS with LDS-DMA (global_load_lds_dwordx4): wave w
// moves 1 KB chunks w, w+4, ...; no VGPRs hold the data.  Completion is published by the
// next ring_barrier() (naz_device.h: explicit vmcnt(0), then the barrier) — never by a bare
// __syncthreads(), which hipcc does not always precede with vmcnt(0).
template <int NFLOATS, int NW = 4>
NAZ_DEV void stage_issue(float* lds, const float* __restrict__ src) {
  static_assert(NFLOATS % 256 == 0, "stage must be whole 1 KB chunks");
  constexpr int CHUNKS = NFLOATS / 256;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int c0 = 0; c0 < CHUNKS; c0 += NW) {
    const int c = c0 + wave;
    if (c0 + NW - 1 < CHUNKS || c < CHUNKS) {
      __builtin_amdgcn_global_load_lds(
          (const void __attribute__((address_space(1)))*)(src + c * 256 + lane * 4),
          to_lds(lds + c * 256), 16, 0, 0);
    }
  }
}

// A stage source addressed as base + a wave-uniform float offset.  The same copy through a buffer
// resource (buffer_load_dwordx4 ... lds: one per-lane offset VGPR, scalar chunk offsets, so no
// 64-bit VALU address add per chunk and lane as global_load_lds needs) is not used: same-box A/B
// on the headline kernel, 2^20 rows, two repetitions: global_load_lds 2.242 / 2.243 ms,
// buffer_load ... lds 2.284 / 2.290 ms (profiles/r03_s3_ab_ring.txt) — the saved address adds do
// not pay for the slower form.
struct RingSrc {
  const float* base;
};

template <int NFLOATS, int NW>
NAZ_DEV void stage_issue(float* lds, const RingSrc& src, int off) {
  stage_issue<NFLOATS, NW>(lds, src.base + off);
}

// stage_issue of the first nch (wave-uniform, <= NFLOATS / 256) 1 KB chunks only
template <int NFLOATS, int NW>
NAZ_DEV void stage_issue_lim(float* lds, const float* __restrict__ src, int nch) {
  static_assert(NFLOATS % 256 == 0, "stage must be whole 1 KB chunks");
  constexpr int CHUNKS = NFLOATS / 256;
  // (the lane offset is formed here, per issue: hoisted out of the layer loop as a 64-bit per-lane
  // source base it was one of the three pointers the nsa16 inverse spilled, and its scratch reload
  // sat right before a stage's DMA issue)
  int lane = threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  nch = nch < CHUNKS ? nch : CHUNKS;
#pragma unroll
  for (int c0 = 0; c0 < CHUNKS; c0 += NW) {
    const int c = c0 + wave;
    if (c < nch) {
      __builtin_amdgcn_global_load_lds(
          (const void __attribute__((address_space(1)))*)(src + c * 256 + lane * 4),
          to_lds(lds + c * 256), 16, 0, 0);
    }
  }
}

}  // namespace naz
