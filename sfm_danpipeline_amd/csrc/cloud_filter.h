// cloud_filter.h -- the rules of the two filters that stand between a dense cloud and everything after it, PCL 1.8.1's
// VoxelGrid (pcl/filters/impl/voxel_grid.hpp) and StatisticalOutlierRemoval (statistical_outlier_removal.hpp), as
// __host__ __device__ code that hipcc and a plain g++ both compile.  The device code (cloud_filter.hip) and the CPU test
// stub (tests/stub/cloud_filter_capi.cpp) share these bodies, so the device result is checked bit for bit against a CPU
// build.  Compile with -ffp-contract=off.  No libm beyond sqrt and floor.  C++14.
// PARITY UNPINNED: PCL is not in the image; the operation order is recalled from its sources (where a
// dagger marks what nobody here can check).
//
// VoxelGrid
//   V1  leaf[3]: floats, each > 0 and finite; inv[a] = 1.0f / leaf[a] in float.
//   V2  min_p / max_p: the box of the finite points, as floats.  d[a] = (int64)((max_p[a] - min_p[a]) * inv[a]) + 1, float
//       arithmetic, truncating cast; d[0] d[1] d[2] > INT32_MAX is refused (PCL warns and copies the input).  Ours, not
//       PCL's (its int would wrap): refused too when floor(min_p[a] * inv[a]) or floor(max_p[a] * inv[a]) does not fit an
//       int32, when the product of the actual extents div[a] = max_b[a] - min_b[a] + 1 exceeds INT32_MAX, and when one
//       div[a] exceeds 2^24 (beyond it the float difference of V3 is no longer exact and could leave the box).
//   V3  min_b[a] = (int)floor(min_p[a] * inv[a]); a finite point's ijk[a] = (int)(floor(p[a] * inv[a]) - (float)min_b[a]),
//       all in float; idx = ijk[0] + ijk[1] div[0] + ijk[2] div[0] div[1].  A non-finite point is in no voxel.
//   V4  a voxel is emitted iff it holds at least min_points points; the output is in ascending idx.
//   V5  centroid: float sums of x, y and z over the voxel's points, then sum / (float)count per component.  The order is
//       ours (PCL's is whatever its unstable std::sort leaves): the points of a voxel in ascending input index, cut into
//       consecutive blocks of BLOCK = 64; each block is summed sequentially from 0.0f (block_sum), and the block sums
//       are added sequentially, in ascending order, to a total that starts at 0.0f (fold_block).  A run of at most 64
//       points is one block: its total is 0.0f + the block's sum, which has the block sum's bits (a sum that starts at
//       +0.0f is never -0.0f).
//   V6  rgb (0x00RRGGBB): u64 channel sums, truncating integer division by the count, top byte 0 -- PCL's float
//       accumulate and uint8 cast while a channel sum stays below 2^24 (count <= 65793).  normals: summed by V5's order,
//       then each component divided by sqrt((x*x + y*y) + z*z) in float; a length of zero or NaN gives 0x7FC00000 in all
//       three (so a NaN input normal propagates to its voxel).
//   V7  voxel_of[i]: the output row of point i's voxel; -1 for a non-finite point or a voxel V4 dropped.
//
// StatisticalOutlierRemoval
//   S1  mean_k in 1..63; every finite point's mean_k + 1 nearest finite points by sfmcloud::dist2, itself and its
//       duplicates included, in ascending d2.  Ties do not matter: equal d2 give equal terms.
//   S2  dist_sum = sum over k = 1..mean_k of sqrt((double)d2[k]) (slot 0 skipped), sequential in ascending k, in f64;
//       mean_dist = (float)(dist_sum / mean_k).  A non-finite point: mean_dist 0, never kept.
//   S3  sum += (double)md and sq += (double)(md * md) (the product in float) over the points.  The order is a rule: the
//       points are cut into consecutive blocks of SUM_BLOCK = 256 input indices; each block is summed sequentially in
//       ascending index from 0.0 (a non-finite point adds its +0.0: nothing), and the block partials are added
//       sequentially in ascending order from 0.0.  mean = sum / N, var = (sq - sum * sum / N) / (N - 1) with N the
//       finite count, var clamped to 0 from below (rounding can leave it negative and sqrt would give NaN), thr =
//       mean + std_mul * sqrt(var).
//   S4  kept iff (double)md <= thr; with `negative` iff (double)md > thr.
//   S5  no finite point: nothing kept, no error.  0 < N <= mean_k: refused (PCL reads stale list slots there).
#pragma once
#include "cloud.h"

namespace sfmfilter {

constexpr int BLOCK = 64;        // V5: points per sequentially summed block
constexpr int SUM_BLOCK = 256;   // S3: points per partial
constexpr int MEAN_K_MAX = 63;   // S1
constexpr int DIV_MAX = 1 << 24; // V2: largest extent of one axis, in voxels

enum { PLAN_OK = 0, PLAN_ARG = 1, PLAN_UNSUPPORTED = 2 };

struct VoxelPlan {
  float inv[3];
  int min_b[3], div[3];
  long long ncell;  // div[0] div[1] div[2] <= INT32_MAX
};

SFM_CLOUD_INLINE bool fits_int32(float f) { return f >= -2147483648.0f && f < 2147483648.0f; }

// V1, V2 for a cloud with at least one finite point
SFM_CLOUD_INLINE int voxel_plan(const float leaf[3], const float min_p[3], const float max_p[3], VoxelPlan& p) {
  for (int a = 0; a < 3; ++a) {
    if (!(leaf[a] > 0.0f) || leaf[a] - leaf[a] != 0.0f) return PLAN_ARG;
    p.inv[a] = 1.0f / leaf[a];
  }
  long long prod = 1, cells = 1;
  for (int a = 0; a < 3; ++a) {
    const float ext = (max_p[a] - min_p[a]) * p.inv[a];
    if (!(ext < 2147483648.0f)) return PLAN_UNSUPPORTED;  // (also inf and NaN: one d[a] alone is past INT32_MAX)
    prod *= (long long)ext + 1;
    if (prod > (long long)INT_MAX) return PLAN_UNSUPPORTED;
  }
  for (int a = 0; a < 3; ++a) {
    const float fl = floorf(min_p[a] * p.inv[a]), fh = floorf(max_p[a] * p.inv[a]);
    if (!fits_int32(fl) || !fits_int32(fh)) return PLAN_UNSUPPORTED;
    p.min_b[a] = (int)fl;
    const long long dv = (long long)(int)fh - (long long)p.min_b[a] + 1;
    if (dv > (long long)DIV_MAX) return PLAN_UNSUPPORTED;
    p.div[a] = (int)dv;
    cells *= dv;
    if (cells > (long long)INT_MAX) return PLAN_UNSUPPORTED;
  }
  p.ncell = cells;
  return PLAN_OK;
}

// V3 for a finite point
SFM_CLOUD_INLINE int voxel_key(const VoxelPlan& p, float x, float y, float z) {
  const int i = (int)(floorf(x * p.inv[0]) - (float)p.min_b[0]);
  const int j = (int)(floorf(y * p.inv[1]) - (float)p.min_b[1]);
  const int k = (int)(floorf(z * p.inv[2]) - (float)p.min_b[2]);
  return i + j * p.div[0] + k * p.div[0] * p.div[1];
}

// V5: the sums of the C components of points [j0, j1) of a run, j1 - j0 <= BLOCK; get(j, v) reads point j's components
template <int C, class Get>
SFM_CLOUD_INLINE void block_sum(int j0, int j1, Get get, float (&s)[C]) {
  for (int c = 0; c < C; ++c) s[c] = 0.0f;
  for (int j = j0; j < j1; ++j) {
    float v[C];
    get(j, v);
    for (int c = 0; c < C; ++c) s[c] += v[c];
  }
}
template <int C>
SFM_CLOUD_INLINE void fold_block(float (&total)[C], const float (&s)[C]) {
  for (int c = 0; c < C; ++c) total[c] += s[c];
}
// ... and of a whole run of `count` points, by one thread
template <int C, class Get>
SFM_CLOUD_INLINE void run_sum(int count, Get get, float (&total)[C]) {
  for (int c = 0; c < C; ++c) total[c] = 0.0f;
  for (int b = 0; b < count; b += BLOCK) {
    float s[C];
    block_sum<C>(b, b + BLOCK < count ? b + BLOCK : count, get, s);
    fold_block<C>(total, s);
  }
}

SFM_CLOUD_INLINE float centroid(float sum, int count) { return sum / (float)count; }

// V6
SFM_CLOUD_INLINE void rgb_add(uint64_t (&s)[3], uint32_t c) {
  s[0] += (c >> 16) & 255u;
  s[1] += (c >> 8) & 255u;
  s[2] += c & 255u;
}
SFM_CLOUD_INLINE uint32_t rgb_mean(const uint64_t (&s)[3], int count) {
  const uint64_t n = (uint64_t)count;
  return ((uint32_t)(s[0] / n) << 16) | ((uint32_t)(s[1] / n) << 8) | (uint32_t)(s[2] / n);
}
SFM_CLOUD_INLINE void normal_mean(const float s[3], float out[3]) {
  const float l = sqrtf((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]);
  if (l == 0.0f || l != l) {
    out[0] = out[1] = out[2] = sfmcloud::qnan();
    return;
  }
  for (int c = 0; c < 3; ++c) out[c] = sfmcloud::canon(s[c] / l);
}

// S2
SFM_CLOUD_INLINE double dist_term(float d2) { return sqrt((double)d2); }
SFM_CLOUD_INLINE float mean_dist(double dist_sum, int mean_k) { return (float)(dist_sum / (double)mean_k); }

// S3: one block's partials over md[i0, i1), i1 - i0 <= SUM_BLOCK
SFM_CLOUD_INLINE void stat_partial(const float* md, long long i0, long long i1, double& sum, double& sq) {
  sum = 0.0;
  sq = 0.0;
  for (long long i = i0; i < i1; ++i) {
    const float m = md[i];
    sum += (double)m;
    sq += (double)(m * m);
  }
}
// ... and the threshold from the partials, in ascending order (part: sum, sq per block)
SFM_CLOUD_INLINE double threshold(const double* part, long long n_part, int n_valid, double std_mul) {
  double sum = 0.0, sq = 0.0;
  for (long long b = 0; b < n_part; ++b) {
    sum += part[2 * b];
    sq += part[2 * b + 1];
  }
  const double N = (double)n_valid;
  const double mean = sum / N;
  double var = (sq - sum * sum / N) / (N - 1.0);
  if (var < 0.0) var = 0.0;
  return mean + std_mul * sqrt(var);
}

// S4 for a finite point
SFM_CLOUD_INLINE bool stat_keep(float md, double thr, bool negative) { return negative ? (double)md > thr : (double)md <= thr; }

}  // namespace sfmfilter
