// The MC-dropout mask: a counter-based hash of (seed, row, column), shared by naz_dropout
// (elementwise.hip) and the fused dropout sampler (made_ar_dropout.h), which must draw the same
// masks.  keep(seed, m, n) = drop_hash(seed, m, n) >= drop_threshold(p); kept values are scaled
// by drop_scale(p) = 1 / (1 - p).
#pragma once
#include <stdint.h>

#include "naz_device.h"

namespace naz {

constexpr uint64_t kDropRowMul = 0x9E3779B97F4A7C15ull, kDropColMul = 0xC2B2AE3D27D4EB4Full;

// murmur3 fmix64 of the combined counter, low 32 bits
NAZ_DEV uint32_t drop_mix(uint64_t h) {
  h ^= h >> 33;
  h *= 0xFF51AFD7ED558CCDull;
  h ^= h >> 33;
  h *= 0xC4CEB9FE1A85EC53ull;
  h ^= h >> 33;
  return (uint32_t)h;
}

NAZ_DEV uint32_t drop_hash(uint64_t seed, int64_t m, int n) {
  return drop_mix(seed ^ (kDropRowMul * (uint64_t)(m + 1)) ^ (kDropColMul * (uint64_t)(n + 1)));
}

// host: the hash threshold and the kept values' scale of a dropout probability p in [0, 1]
inline uint32_t drop_threshold(float p) {
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (uint32_t)t;
}
inline float drop_scale(float p) { return p >= 1.f ? 0.f : 1.f / (1.f - p); }

}  // namespace naz
