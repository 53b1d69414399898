// cloud.h -- the numerics of map3D's step 10 (reference src/Sfm.cpp:94-102, bodies :1323-1383) as __host__ __device__
// code that hipcc and a plain g++ both compile: PCL 1.8.1's PassThrough limit test, RadiusOutlierRemoval's neighbour
// test (FLANN L2_Simple), the k-nearest list of NormalEstimation, computeMeanAndCovarianceMatrix, pcl::eigen33 and
// flipNormalTowardsViewpoint.  The device code (cloud.hip) and the CPU test stub (tests/stub/cloud_capi.cpp) share
// these bodies, so the device result is checked bit for bit against a CPU build.  Compile with -ffp-contract=off.
// The eigen step's atan2 / cos / sin are restated here with + - * / sqrt only (double, then rounded to float), so no
// libm or device-library routine enters the result.  C++14: the host mirror's sanitizer builds include it.
// PARITY UNPINNED: PCL / FLANN are not in the image; the operation order is recalled from their sources.
#pragma once
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>

#ifdef __HIPCC__
#define SFM_CLOUD_INLINE __host__ __device__ __forceinline__
#else
#define SFM_CLOUD_INLINE inline __attribute__((always_inline))
#endif

namespace sfmcloud {

constexpr int KMAX = 32;  // largest k of the fused k-NN + normal kernel

SFM_CLOUD_INLINE float bits_f(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
// the NaN every NaN output is written as (std::numeric_limits<float>::quiet_NaN(), what PCL stores): 0/0 gives
// 0xFFC00000 on x86 and 0x7FC00000 on the device, so computed NaNs are canonicalised to this one
SFM_CLOUD_INLINE float qnan() { return bits_f(0x7FC00000u); }
SFM_CLOUD_INLINE float canon(float x) { return x != x ? qnan() : x; }
SFM_CLOUD_INLINE bool finite3(float x, float y, float z) {
  return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f;  // (inf - inf and NaN - NaN are NaN)
}
// an order-preserving map of floats to unsigned (-0 below +0, the infinities at the ends of the numbers), so that a
// bounding box is a min / max reduction over integers whose result does not depend on the order of the operands
SFM_CLOUD_INLINE uint32_t ord_key(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SFM_CLOUD_INLINE float ord_val(uint32_t k) { return bits_f((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k); }

// FLANN L2_Simple: ((dx*dx) + dy*dy) + dz*dz in float, no contraction
SFM_CLOUD_INLINE float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return ((dx * dx) + dy * dy) + dz * dz;
}
// setRadiusSearch(double r): FLANN searches with (float)(r * r), squared in double
SFM_CLOUD_INLINE float radius2(double r) { return (float)(r * r); }
// a neighbour of the radius search: d2 < r2 (strict)
SFM_CLOUD_INLINE bool in_radius(float d2, float r2) { return d2 < r2; }

// ---- the geometry of a uniform grid (cloud_grid.h's grid_build, the kernels that walk a grid, and the CPU stubs that
// restate a walk's order): dimensions floor(extent / cell) + 1 per axis capped at AXIS_CAP, the cell doubled while the grid
// holds more than CELL_CAP cells; a coordinate's cell by floor((v - o) / cell) in double, clamped to the grid; keys x-fastest
constexpr long long AXIS_CAP = 1 << 12;  // cells per axis
constexpr long long CELL_CAP = 1 << 22;  // cells in all
struct GridGeom {
  double o[3], cell;
  int D[3];
  long long ncell;
};
// the grid over the box [lo, hi] of `n_valid` finite points (no point: one cell) that starts from cells of `cell`
SFM_CLOUD_INLINE void grid_geometry(const double lo[3], const double hi[3], int n_valid, double cell, GridGeom& g) {
  for (;;) {
    long long tot = 1;
    for (int a = 0; a < 3; ++a) {
      const double ext = n_valid ? hi[a] - lo[a] : 0.0;
      const double d = floor(ext / cell) + 1.0;
      g.D[a] = (int)((double)AXIS_CAP < d ? (double)AXIS_CAP : d);
      tot *= g.D[a];
    }
    if (tot <= CELL_CAP) {
      g.ncell = tot;
      break;
    }
    cell *= 2;
  }
  for (int a = 0; a < 3; ++a) g.o[a] = lo[a];
  g.cell = cell;
}
SFM_CLOUD_INLINE int cell_of(double v, double o, double cell, int D) {
  double f = floor((v - o) / cell);
  f = f < 0.0 ? 0.0 : f;
  f = f > (double)(D - 1) ? (double)(D - 1) : f;
  return (int)f;
}
// the radius grid's starting cell for radius r (the margin covers the float rounding of d2 and the double rounding of cell_of)
SFM_CLOUD_INLINE double radius_cell(double r) { return r * (1.0 + 1.0 / 1024.0); }
SFM_CLOUD_INLINE int cell_key(const GridGeom& g, float x, float y, float z) {
  const int cx = cell_of(x, g.o[0], g.cell, g.D[0]), cy = cell_of(y, g.o[1], g.cell, g.D[1]), cz = cell_of(z, g.o[2], g.cell, g.D[2]);
  return (cz * g.D[1] + cy) * g.D[0] + cx;
}

// PassThrough on one field (limits as float, inclusive): a non-finite point is always dropped; otherwise kept iff
// the value lies inside [lo, hi] (negative: iff it lies outside)
SFM_CLOUD_INLINE bool passthrough_keep(float x, float y, float z, int axis, float lo, float hi, bool negative) {
  if (!finite3(x, y, z)) return false;
  const float v = axis == 0 ? x : axis == 1 ? y : z;
  const bool inside = !(v < lo || v > hi);
  return negative ? !inside : inside;
}
// RadiusOutlierRemoval: k counts the point itself and its duplicates; an outlier iff k <= min_pts
SFM_CLOUD_INLINE bool radius_keep(int k, int min_pts) { return k > min_pts; }

// the (d2, index) order of the k-nearest list
SFM_CLOUD_INLINE bool knn_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

// inserts (d, i) into the list sorted by knn_less.  All N slots are compare-and-swapped with compile-time indices
// (the list stays in registers on the device); the caller passes a candidate only when it beats the k-th entry, so
// the first k slots hold the k nearest seen so far and the slots after them are whatever was pushed down.
template <int N>
SFM_CLOUD_INLINE void knn_insert(float (&d)[N], int (&id)[N], float cd, int ci) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    const bool lt = knn_less(cd, ci, d[s], id[s]);
    const float td = d[s];
    const int ti = id[s];
    d[s] = lt ? cd : td;
    id[s] = lt ? ci : ti;
    cd = lt ? td : cd;
    ci = lt ? ti : ci;
  }
}
template <int N>
SFM_CLOUD_INLINE void knn_init(float (&d)[N], int (&id)[N]) {
#pragma unroll
  for (int s = 0; s < N; ++s) {
    d[s] = bits_f(0x7F800000u);  // +inf
    id[s] = INT_MAX;
  }
}
// slot k - 1 of the list without a dynamic register index
template <int N>
SFM_CLOUD_INLINE void knn_kth(const float (&d)[N], const int (&id)[N], int k, float& kd, int& ki) {
  kd = d[0];
  ki = id[0];
#pragma unroll
  for (int s = 1; s < N; ++s) {
    kd = s == k - 1 ? d[s] : kd;
    ki = s == k - 1 ? id[s] : ki;
  }
}

// computeMeanAndCovarianceMatrix (float): 9 sums in list order, each divided by the count, then
// cov = E[ab] - E[a]E[b]; the symmetric half copied.  cov: row-major 3 x 3.
struct Accu {
  float a[9];
};
SFM_CLOUD_INLINE void accu_zero(Accu& s) {
  for (int i = 0; i < 9; ++i) s.a[i] = 0.0f;
}
SFM_CLOUD_INLINE void accu_add(Accu& s, float x, float y, float z) {
  s.a[0] += x * x;
  s.a[1] += x * y;
  s.a[2] += x * z;
  s.a[3] += y * y;
  s.a[4] += y * z;
  s.a[5] += z * z;
  s.a[6] += x;
  s.a[7] += y;
  s.a[8] += z;
}
SFM_CLOUD_INLINE void accu_covariance(Accu& s, int count, float cov[9]) {
  const float c = (float)count;
  for (int i = 0; i < 9; ++i) s.a[i] /= c;
  cov[0] = s.a[0] - s.a[6] * s.a[6];
  cov[1] = s.a[1] - s.a[6] * s.a[7];
  cov[2] = s.a[2] - s.a[6] * s.a[8];
  cov[4] = s.a[3] - s.a[7] * s.a[7];
  cov[5] = s.a[4] - s.a[7] * s.a[8];
  cov[8] = s.a[5] - s.a[8] * s.a[8];
  cov[3] = cov[1];
  cov[6] = cov[2];
  cov[7] = cov[5];
}

// ---- the eigen step's trigonometry: + - * / sqrt in double, no libm
constexpr double PI = 3.141592653589793116;  // (the double nearest pi)

// atan(t) for t in [0, 1]: two half-angle steps take t below tan(pi/16) < 0.2, then the Taylor series (t^2 < 0.04:
// 16 terms leave < 1e-22 relative)
SFM_CLOUD_INLINE double atan01(double t) {
  t = t / (1.0 + sqrt(1.0 + t * t));
  t = t / (1.0 + sqrt(1.0 + t * t));
  const double tt = t * t;
  double p = 0.0;
  for (int k = 15; k >= 0; --k) p = p * tt + ((k & 1) ? -1.0 : 1.0) / (double)(2 * k + 1);
  return 4.0 * (t * p);
}
SFM_CLOUD_INLINE bool negative_sign(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u >> 63) != 0;
}
// atan2(y, x) for finite or NaN arguments (the signs of zeros as libm: atan2(+-0, -0) = +-pi)
SFM_CLOUD_INLINE double atan2_own(double y, double x) {
  if (x != x || y != y) return x + y;
  const double ax = fabs(x), ay = fabs(y);
  double a;
  if (ax == 0.0 && ay == 0.0) a = 0.0;
  else if (ay <= ax) a = atan01(ay / ax);
  else a = PI * 0.5 - atan01(ax / ay);
  if (negative_sign(x)) a = PI - a;
  return negative_sign(y) ? -a : a;
}
// cos / sin by their Taylor series, for |x| <= pi (the eigen step passes [0, pi/3]); 20 terms
SFM_CLOUD_INLINE double cos_own(double x) {
  const double xx = x * x;
  double p = 0.0;
  for (int k = 20; k >= 1; --k) p = 1.0 - p * xx / (double)((2 * k - 1) * (2 * k));
  return p;
}
SFM_CLOUD_INLINE double sin_own(double x) {
  const double xx = x * x;
  double p = 0.0;
  for (int k = 20; k >= 1; --k) p = 1.0 - p * xx / (double)((2 * k) * (2 * k + 1));
  return x * p;
}
SFM_CLOUD_INLINE float atan2f_own(float y, float x) { return (float)atan2_own((double)y, (double)x); }
SFM_CLOUD_INLINE float cosf_own(float x) { return (float)cos_own((double)x); }
SFM_CLOUD_INLINE float sinf_own(float x) { return (float)sin_own((double)x); }

// pcl::computeRoots2: roots (0, (b - sd) / 2, (b + sd) / 2) of x^2 - b x + c, d = b*b - 4.0*c in double
SFM_CLOUD_INLINE void roots2(float b, float c, float r[3]) {
  r[0] = 0.0f;
  float d = (float)((double)(b * b) - 4.0 * (double)c);
  if (d < 0.0f) d = 0.0f;
  const float sd = sqrtf(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}
// pcl::computeRoots: the characteristic cubic of a symmetric 3 x 3, trigonometric method, roots ascending
SFM_CLOUD_INLINE void roots3(const float m[9], float r[3]) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (fabsf(c0) < FLT_EPSILON) {  // one root is 0: the quadratic
    roots2(c2, c1, r);
    return;
  }
  const float s_inv3 = (float)(1.0 / 3.0);
  const float s_sqrt3 = sqrtf(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f) a_over_3 = 0.0f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f) q = 0.0f;
  const float rho = sqrtf(-a_over_3);
  const float theta = atan2f_own(sqrtf(-q), half_b) * s_inv3;
  const float cos_theta = cosf_own(theta), sin_theta = sinf_own(theta);
  r[0] = c2_over_3 + 2.0f * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  float t;
  if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  if (r[0] <= 0.0f) roots2(c2, c1, r);  // (a PSD matrix has no negative eigenvalue)
}
SFM_CLOUD_INLINE void cross(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
SFM_CLOUD_INLINE float sqnorm(const float v[3]) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

// pcl::eigen33(mat, eigenvalue, eigenvector): scale by the largest |coefficient| (1 when that is <= FLT_MIN), roots,
// smallest root * scale, eigenvector = the largest of the three row cross products of (M / scale - root0 I),
// normalised (NaN when all three vanish: an isotropic, collinear or all-identical neighbourhood)
SFM_CLOUD_INLINE void eigen33(const float cov[9], float& value, float vec[3]) {
  float scale = 0.0f;
  for (int i = 0; i < 9; ++i) scale = fabsf(cov[i]) > scale ? fabsf(cov[i]) : scale;
  if (scale <= FLT_MIN) scale = 1.0f;
  float m[9];
  for (int i = 0; i < 9; ++i) m[i] = cov[i] / scale;
  float r[3];
  roots3(m, r);
  value = r[0] * scale;
  m[0] -= r[0];
  m[4] -= r[0];
  m[8] -= r[0];
  float v1[3], v2[3], v3[3];
  cross(m, m + 3, v1);
  cross(m, m + 6, v2);
  cross(m + 3, m + 6, v3);
  const float l1 = sqnorm(v1), l2 = sqnorm(v2), l3 = sqnorm(v3);
  const float* v;
  float l;
  if (l1 >= l2 && l1 >= l3) { v = v1; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { v = v2; l = l2; }
  else { v = v3; l = l3; }
  const float s = sqrtf(l);
  vec[0] = v[0] / s;
  vec[1] = v[1] / s;
  vec[2] = v[2] / s;
}

// flipNormalTowardsViewpoint: flip iff (vp - p) . n < 0, the dot summed x, y, z
SFM_CLOUD_INLINE void flip_towards(float px, float py, float pz, const float vp[3], float n[3]) {
  const float dx = vp[0] - px, dy = vp[1] - py, dz = vp[2] - pz;
  const float c = (dx * n[0] + dy * n[1]) + dz * n[2];
  if (c < 0.0f) {
    n[0] = -n[0];
    n[1] = -n[1];
    n[2] = -n[2];
  }
}

// NormalEstimation's per-point tail once the covariance of `count` neighbours is known: fewer than 3 neighbours ->
// NaN normal and curvature; else eigen33, curvature = |lambda0 / trace| (0 when the trace is 0), flip towards vp.
// out: nx, ny, nz, curvature, NaNs canonical.
SFM_CLOUD_INLINE void normal_from_cov(const float cov[9], int count, float px, float py, float pz, const float vp[3],
                                      float out[4]) {
  if (count < 3) {
    out[0] = out[1] = out[2] = out[3] = qnan();
    return;
  }
  float value, n[3];
  eigen33(cov, value, n);
  const float tr = cov[0] + cov[4] + cov[8];
  const float curv = tr != 0.0f ? fabsf(value / tr) : 0.0f;
  flip_towards(px, py, pz, vp, n);
  out[0] = canon(n[0]);
  out[1] = canon(n[1]);
  out[2] = canon(n[2]);
  out[3] = canon(curv);
}

}  // namespace sfmcloud
