// mls.h -- the rules and the arithmetic of the moving-least-squares smoothing of a cloud (include/sfmhip.h,
// sfmhip_cloud_mls) as __host__ __device__ code that hipcc and a plain g++ both compile: PCL 1.8.1's
// MovingLeastSquares::computeMLSPointNormal with no upsampling (NONE) and SIMPLE projection.  The device code (mls.hip) and
// the CPU test stub (tests/stub/mls_capi.cpp) share these bodies and feed them the neighbours in one written order (M2), so
// the device result is checked bit for bit against a CPU build.  Compile with -ffp-contract=off.  Everything is + - * / sqrt
// in double: the trigonometry of the eigen step is cloud.h's, exp is restated below (M6); no libm or device-library routine
// enters the result.
// PARITY UNPINNED: PCL is not in the image; the rules are recalled from its sources.  What nothing here can check is marked
// + (ours) or left to the rule list of include/sfmhip.h.
#pragma once
#include "cloud.h"
#include <cfloat>

namespace sfmmls {

using sfmcloud::atan2_own;
using sfmcloud::cos_own;
using sfmcloud::sin_own;

SFM_CLOUD_INLINE double bits_d(uint64_t u) {
  double d;
  memcpy(&d, &u, 8);
  return d;
}
SFM_CLOUD_INLINE bool finite_d(double x) { return x - x == 0.0; }
// Eigen's dot of two 3-vectors: ((a0 b0 + a1 b1) + a2 b2)
SFM_CLOUD_INLINE double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// ---- M6: exp(x) for x <= 0.  k = floor(x / ln 2 + 1/2), r = (x - k ln2_hi) - k ln2_lo (|r| <= 0.347, the first product
// exact: ln2_hi ends in 21 zero bits), the Taylor polynomial of degree 13 by Horner (the first term left out is below
// 6e-18 of the sum), times 2^k set through the exponent bits (k >= -1022: a normal number).  0 below -708.
SFM_CLOUD_INLINE double exp_neg(double x) {
  if (x != x) return x;
  if (x < -708.0) return 0.0;
  const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10, INV_LN2 = 1.44269504088896338700e+00;
  const double kf = floor(x * INV_LN2 + 0.5);
  const double r = (x - kf * LN2_HI) - kf * LN2_LO;
  double p = 1.0 / 6227020800.0;  // 1 / 13!
  p = p * r + 1.0 / 479001600.0;
  p = p * r + 1.0 / 39916800.0;
  p = p * r + 1.0 / 3628800.0;
  p = p * r + 1.0 / 362880.0;
  p = p * r + 1.0 / 40320.0;
  p = p * r + 1.0 / 5040.0;
  p = p * r + 1.0 / 720.0;
  p = p * r + 1.0 / 120.0;
  p = p * r + 1.0 / 24.0;
  p = p * r + 1.0 / 6.0;
  p = p * r + 0.5;
  p = p * r + 1.0;
  p = p * r + 1.0;
  const int k = (int)kf;
  return p * bits_d((uint64_t)(k + 1023) << 52);
}

// ---- M3: computeMeanAndCovarianceMatrix in double: 9 sums in M2's order, each divided by the count, E[ab] - E[a]E[b]
struct Accu {
  double a[9];
};
SFM_CLOUD_INLINE void accu_zero(Accu& s) {
  for (int i = 0; i < 9; ++i) s.a[i] = 0.0;
}
SFM_CLOUD_INLINE void accu_add(Accu& s, double x, double y, double z) {
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
SFM_CLOUD_INLINE void accu_covariance(Accu& s, int count, double cov[9], double mean[3]) {
  const double c = (double)count;
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
  mean[0] = s.a[6], mean[1] = s.a[7], mean[2] = s.a[8];
}

// pcl::computeRoots2 / computeRoots / eigen33 with Scalar = double (cloud.h's float bodies, restated: theirs keep their bits)
SFM_CLOUD_INLINE void roots2(double b, double c, double r[3]) {
  r[0] = 0.0;
  double d = b * b - 4.0 * c;
  if (d < 0.0) d = 0.0;
  const double sd = sqrt(d);
  r[2] = 0.5 * (b + sd);
  r[1] = 0.5 * (b - sd);
}
SFM_CLOUD_INLINE void roots3(const double m[9], double r[3]) {
  const double m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const double c0 = m00 * m11 * m22 + 2.0 * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const double c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const double c2 = m00 + m11 + m22;
  if (fabs(c0) < DBL_EPSILON) {  // one root is 0: the quadratic
    roots2(c2, c1, r);
    return;
  }
  const double s_inv3 = 1.0 / 3.0;
  const double s_sqrt3 = sqrt(3.0);
  const double c2_over_3 = c2 * s_inv3;
  double a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0) a_over_3 = 0.0;
  const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
  double q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0) q = 0.0;
  const double rho = sqrt(-a_over_3);
  const double theta = atan2_own(sqrt(-q), half_b) * s_inv3;
  const double cos_theta = cos_own(theta), sin_theta = sin_own(theta);
  r[0] = c2_over_3 + 2.0 * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  double t;
  if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  if (r[1] >= r[2]) {
    t = r[1]; r[1] = r[2]; r[2] = t;
    if (r[0] >= r[1]) { t = r[0]; r[0] = r[1]; r[1] = t; }
  }
  if (r[0] <= 0.0) roots2(c2, c1, r);  // (a PSD matrix has no negative eigenvalue)
}
SFM_CLOUD_INLINE void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// smallest eigenvalue and its vector: NaN components when all three row cross products vanish (M4)
SFM_CLOUD_INLINE void eigen33(const double cov[9], double& value, double vec[3]) {
  double scale = 0.0;
  for (int i = 0; i < 9; ++i) scale = fabs(cov[i]) > scale ? fabs(cov[i]) : scale;
  if (scale <= DBL_MIN) scale = 1.0;
  double m[9];
  for (int i = 0; i < 9; ++i) m[i] = cov[i] / scale;
  double r[3];
  roots3(m, r);
  value = r[0] * scale;
  m[0] -= r[0];
  m[4] -= r[0];
  m[8] -= r[0];
  double v1[3], v2[3], v3[3];
  cross3(m, m + 3, v1);
  cross3(m, m + 6, v2);
  cross3(m + 3, m + 6, v3);
  const double l1 = dot3(v1, v1), l2 = dot3(v2, v2), l3 = dot3(v3, v3);
  const bool p1 = l1 >= l2 && l1 >= l3, p2 = l2 >= l1 && l2 >= l3;
  const double l = p1 ? l1 : p2 ? l2 : l3;
  const double s = sqrt(l);
  for (int a = 0; a < 3; ++a) vec[a] = (p1 ? v1[a] : p2 ? v2[a] : v3[a]) / s;
}

// what M3 leaves for a point with >= 3 neighbours: the plane, the projected point, the curvature, the local frame
struct Plane {
  double n[3], q[3], curv;
  double ua[3], va[3];  // M5's frame (set by frame())
  bool degenerate;      // M4: n is not finite
};
SFM_CLOUD_INLINE void plane_fit(Accu& acc, int count, const double p[3], Plane& pl) {
  double cov[9], mean[3], value;
  accu_covariance(acc, count, cov, mean);
  eigen33(cov, value, pl.n);
  pl.degenerate = !(finite_d(pl.n[0]) && finite_d(pl.n[1]) && finite_d(pl.n[2]));
  const double d = -1.0 * dot3(pl.n, mean);
  const double dist = dot3(p, pl.n) + d;
  for (int a = 0; a < 3; ++a) pl.q[a] = p[a] - dist * pl.n[a];
  const double tr = cov[0] + cov[4] + cov[8];
  pl.curv = tr != 0.0 ? fabs(value / tr) : 0.0;
}
// Eigen's unitOrthogonal of n, then u = n x v
SFM_CLOUD_INLINE void frame(Plane& pl) {
  const double* n = pl.n;
  if (!(fabs(n[0]) <= 1e-12 * fabs(n[2])) || !(fabs(n[1]) <= 1e-12 * fabs(n[2]))) {
    const double s = sqrt(n[0] * n[0] + n[1] * n[1]);
    pl.va[0] = -n[1] / s, pl.va[1] = n[0] / s, pl.va[2] = 0.0;
  } else {
    const double s = sqrt(n[1] * n[1] + n[2] * n[2]);
    pl.va[0] = 0.0, pl.va[1] = -n[2] / s, pl.va[2] = n[1] / s;
  }
  cross3(pl.n, pl.va, pl.ua);
}

// ---- M5: the weighted normal equations of the polynomial of order O in (u, v).  Terms u^a v^b in PCL's order (a = 0..O,
// b = 0..O - a); A[j][k] = sum w t_j t_k depends on (a_j + a_k, b_j + b_k) only, so the distinct moments sum w u^a v^b
// (a + b <= 2 O) are what is accumulated: 15 for order 2, 6 for order 1.
template <int O>
struct Fit {
  static constexpr int NC = (O + 1) * (O + 2) / 2;
  static constexpr int D = 2 * O;
  static constexpr int NM = (D + 1) * (D + 2) / 2;
  double M[NM > 0 ? NM : 1];
  double B[NC];
};
constexpr int midx(int D, int a, int b) { return a * (D + 1) - a * (a - 1) / 2 + b; }
constexpr int term_a(int O, int j) { return j < O + 1 ? 0 : j < 2 * O + 1 ? 1 : 2; }          // (O <= 2)
constexpr int term_b(int O, int j) { return j < O + 1 ? j : j < 2 * O + 1 ? j - (O + 1) : 0; }

template <int O>
SFM_CLOUD_INLINE void fit_zero(Fit<O>& f) {
#pragma unroll
  for (int i = 0; i < Fit<O>::NM; ++i) f.M[i] = 0.0;
#pragma unroll
  for (int i = 0; i < Fit<O>::NC; ++i) f.B[i] = 0.0;
}
// one neighbour x (as doubles): e = x - q, w = exp(-(e.e) / g), u = e.u_axis, v = e.v_axis, f = e.n; powers by repeated
// multiplication, M[a][b] += w (u^a v^b), B[j] += (w t_j) f
template <int O>
SFM_CLOUD_INLINE void fit_add(Fit<O>& f, const Plane& pl, double g, double x, double y, double z) {
  constexpr int D = Fit<O>::D;
  const double e[3] = {x - pl.q[0], y - pl.q[1], z - pl.q[2]};
  const double w = exp_neg(-dot3(e, e) / g);
  const double u = dot3(e, pl.ua), v = dot3(e, pl.va), h = dot3(e, pl.n);
  double up[D + 1], vp[D + 1];
  up[0] = vp[0] = 1.0;
#pragma unroll
  for (int k = 1; k <= D; ++k) up[k] = up[k - 1] * u, vp[k] = vp[k - 1] * v;
#pragma unroll
  for (int a = 0; a <= D; ++a)
#pragma unroll
    for (int b = 0; b <= D - a; ++b) f.M[midx(D, a, b)] += w * (up[a] * vp[b]);
#pragma unroll
  for (int j = 0; j < Fit<O>::NC; ++j) f.B[j] += (w * (up[term_a(O, j)] * vp[term_b(O, j)])) * h;
}
// Cholesky (LLT) of A, forward then back substitution, every loop of constant extent (registers on the device).  false when
// a pivot is <= 0 or not finite, or a coefficient is not finite (+).
template <int O>
SFM_CLOUD_INLINE bool fit_solve(const Fit<O>& f, double c[Fit<O>::NC]) {
  constexpr int N = Fit<O>::NC, D = Fit<O>::D;
  double L[N][N];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = f.M[midx(D, term_a(O, j) + term_a(O, j), term_b(O, j) + term_b(O, j))];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && d > 0.0 && finite_d(d);
    const double s = sqrt(d);
    L[j][j] = s;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double t = f.M[midx(D, term_a(O, i) + term_a(O, j), term_b(O, i) + term_b(O, j))];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / s;
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double t = f.B[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) t -= L[k][i] * c[k];
    c[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) ok = ok && finite_d(c[i]);
  return ok;
}

// a point's status (M3 - M5) and its output row (M7): floats rounded once from the doubles, NaNs canonical
enum Status { ST_DROPPED = 0, ST_PLANE = 1, ST_PLANE_ONLY = 2, ST_DEGENERATE = 3, ST_FIT_FAILED = 4, ST_FIT = 5 };
constexpr int MIN_NEIGHBOURS = 3;
SFM_CLOUD_INLINE int n_coeff(int order) { return (order + 1) * (order + 2) / 2; }
// the Gaussian's g: the option, or r * r in double when it is <= 0
SFM_CLOUD_INLINE double gauss_param(double sqr_gauss_param, double radius) { return sqr_gauss_param > 0.0 ? sqr_gauss_param : radius * radius; }

SFM_CLOUD_INLINE void write_row(const double q[3], const double n[3], double curv, bool nan_normal, float xyz[3], float n4[4]) {
  for (int a = 0; a < 3; ++a) xyz[a] = (float)q[a];
  for (int a = 0; a < 3; ++a) n4[a] = nan_normal ? sfmcloud::qnan() : sfmcloud::canon((float)n[a]);
  n4[3] = nan_normal ? sfmcloud::qnan() : sfmcloud::canon((float)curv);
}
// M4: the point unmoved, NaN normal and curvature
SFM_CLOUD_INLINE void write_degenerate(const double p[3], float xyz[3], float n4[4]) {
  const double z[3] = {0.0, 0.0, 0.0};
  write_row(p, z, 0.0, true, xyz, n4);
}
// M5's tail: q += c[0] n, normal = n - c[O + 1] u_axis - c[1] v_axis, normalised
template <int O>
SFM_CLOUD_INLINE void fit_apply(const Plane& pl, const double c[Fit<O>::NC], double q[3], double nrm[3]) {
  for (int a = 0; a < 3; ++a) {
    q[a] = pl.q[a] + c[0] * pl.n[a];
    nrm[a] = (pl.n[a] - c[O + 1] * pl.ua[a]) - c[1] * pl.va[a];
  }
  const double s = sqrt(dot3(nrm, nrm));
  for (int a = 0; a < 3; ++a) nrm[a] = nrm[a] / s;
}

}  // namespace sfmmls
