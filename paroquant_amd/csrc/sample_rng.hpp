// The sampler's random numbers (csrc/sample.hip): ONE counter-based function for the kernel and for the host export
// paro_sample_uniform, so a test or a user can restate any draw on the CPU.  No state: the value depends on (seed, ctr) alone --
// ctr is the position the drawn token will occupy --, which makes graph replay, rewinds and re-seeding well defined.
// The function is the splitmix64 stream whose start is mix(seed), read at step ctr: top 24 bits, u = bits / 2^24 in [0, 1).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PARO_HD __host__ __device__
#else
#define PARO_HD
#endif

namespace paro {

PARO_HD inline uint64_t sample_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// 24 random bits of (seed, ctr)
PARO_HD inline uint32_t sample_bits24(uint64_t seed, int64_t ctr) {
  const uint64_t gamma = 0x9E3779B97F4A7C15ull;
  return (uint32_t)(sample_mix64(sample_mix64(seed) + ((uint64_t)ctr + 1ull) * gamma) >> 40);
}

PARO_HD inline float sample_uniform(uint64_t seed, int64_t ctr) { return (float)sample_bits24(seed, ctr) * (1.0f / 16777216.0f); }

}  // namespace paro
