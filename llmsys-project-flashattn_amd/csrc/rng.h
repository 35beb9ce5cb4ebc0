// The library's counter-based uniform RNG, shared by mt_rand_uniform / mt_dropout
// (combine.hip) and mt_select_token (select_token.hip):
//   u[i] = top 24 bits of splitmix64(seed + golden·(i+1)) / 2^24, in [0, 1).
// Stateless: a draw is a function of (seed, index) alone, independent of the grid.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mt {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// the value mt_rand_uniform(out, n, seed) writes at out[i]
__device__ __forceinline__ float uniform24(uint64_t seed, int64_t i) {
  const uint64_t h = mix64(seed + 0x9e3779b97f4a7c15ull * (uint64_t)(i + 1));
  return (float)(h >> 40) * (1.0f / 16777216.0f);
}

}  // namespace mt
