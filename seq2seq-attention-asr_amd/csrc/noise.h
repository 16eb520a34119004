// Counter-based standard normals shared by the optimizer's gradient noise (optim.hip) and the weight-noise
// sampler (wnoise.hip): a pure function of (seed, step, element), so any launch geometry -- and every
// data-parallel rank -- draws the same values.  oracle/s2s_oracle.py: gradient_noise restates it, and
// tests/test_gpu_parity.py::test_optimizer_step_matches_oracle pins the bits.
#pragma once

#include <hip/hip_runtime.h>

namespace s2s {

constexpr unsigned long long kGolden = 0x9e3779b97f4a7c15ull;

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the key of step t of a seed's stream
__device__ __forceinline__ unsigned long long noise_key(unsigned long long seed, unsigned t) {
  return mix64(seed * kGolden + t);
}

// N(0, 1) for element i of the step keyed by mix64(seed * kGolden + t): u1 in (0, 1], u2 in [0, 1)
// from 24-bit fields of mix64(key + i * kGolden), z = sqrt(-2 ln u1) cos(2 pi u2)
// (oracle/s2s_oracle.py: gradient_noise restates it)
__device__ __forceinline__ float noise_normal(unsigned long long key, size_t i) {
  const unsigned long long h = mix64(key + (unsigned long long)i * kGolden);
  const float u1 = (float)((h >> 40) + 1) * (1.0f / 16777216.0f);
  const float u2 = (float)((h >> 16) & 0xffffffull) * (1.0f / 16777216.0f);
  return sqrtf(-2.f * logf(u1)) * cosf(6.28318530717958647692f * u2);
}

}  // namespace s2s
