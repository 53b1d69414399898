// draw_hash.h -- the counter-based hash the RANSAC steps of the cloud family draw their samples with (dendro.h: DESIGN.md
// f-11 rule 5; ground.h: f-12 rule 3), as __host__ __device__ code that hipcc and a plain g++ both compile.  Integers
// only: the same bits everywhere.
#pragma once
#include <cstdint>

#ifdef __HIPCC__
#define SFM_DRAW_INLINE __host__ __device__ __forceinline__
#else
#define SFM_DRAW_INLINE inline __attribute__((always_inline))
#endif

namespace sfmdraw {

SFM_DRAW_INLINE uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}
// a hash of (seed, stream k, iteration j, draw d): k is the slice of f-11, the constant 0x67726E64 of f-12
SFM_DRAW_INLINE uint32_t draw_hash(uint32_t seed, uint32_t k, uint32_t j, uint32_t d) {
  uint32_t x = mix32(seed + 0x9E3779B9u);
  x = mix32(x ^ k);
  x = mix32((x + 0x85EBCA6Bu) ^ j);
  x = mix32((x + 0xC2B2AE35u) ^ d);
  return x;
}
// a position in a list of n: (u64(hash) n) >> 32
SFM_DRAW_INLINE uint32_t draw_index(uint32_t seed, uint32_t k, uint32_t j, uint32_t d, uint32_t n) {
  return (uint32_t)(((uint64_t)draw_hash(seed, k, j, d) * (uint64_t)n) >> 32);
}

}  // namespace sfmdraw
