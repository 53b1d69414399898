// block_sum.h -- the fixed-order sum of 256 slots that DESIGN.md f-9, f-11 and f-12 rule: slot i mod 256 in ascending i,
// then four 64-entry trees (strides 32 .. 1), then (w0 + w1) + (w2 + w3).  The host form (chunk_tree) is what the CPU
// test stubs compile through poisson.h and dendro.h; the device form is the same order over the 256 threads of a
// workgroup: the wave butterfly x = x + shfl_xor(x, off), lane 0 of each wave to LDS, then the pairing above.
#pragma once
#include <cstdint>

namespace sfmsum {

constexpr int CHUNK = 256;  // slots of a fixed-order sum = threads of a workgroup

// the tree of one chunk (v is overwritten)
inline double chunk_tree(double v[CHUNK]) {
  for (int w = 0; w < 4; ++w)
    for (int off = 32; off >= 1; off >>= 1)
      for (int t = 0; t < off; ++t) v[64 * w + t] = v[64 * w + t] + v[64 * w + t + off];
  return (v[0] + v[64]) + (v[128] + v[192]);
}

#ifdef __HIPCC__
// chunk_tree over the 256 threads of a workgroup, Q sums at once (sh: Q rows of 4), or the first nq of them where the
// number is known only at run time (uniform over the workgroup; dnd_refit: 8 or 1); every thread gets the values.  The
// loops carry no unroll pragma: with nq = Q the compiler unrolls them as it did, and dnd_refit keeps its run-time loop and
// with it its registers
template <int Q>
__device__ __forceinline__ void block_tree(double v[Q], double (*sh)[4], int nq = Q) {
  for (int q = 0; q < nq; ++q) {
    double x = v[q];
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) sh[q][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  for (int q = 0; q < nq; ++q) v[q] = (sh[q][0] + sh[q][1]) + (sh[q][2] + sh[q][3]);
  __syncthreads();
}
// the same for a count (integers: any order gives the same sum)
__device__ __forceinline__ uint32_t block_count(uint32_t v, uint32_t* sh) {
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  v = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return v;
}
#endif

}  // namespace sfmsum
