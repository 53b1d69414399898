// pnp.h -- the numerics of findCameraPosePNP's cv::solvePnPRansac(..., CV_EPNP) (reference src/Sfm.cpp:1153) as
// __host__ __device__ code that hipcc and a plain g++ both compile: EPnP for n >= 5 points (OpenCV 3.4.1 calib3d/epnp.cpp),
// Rodrigues in both directions and PnPRansacCallback::computeError's per-point error.  (The replay of ptsetreg.cpp's RANSAC
// loop over per-iteration inlier counts is ransac_host.h's ransac_replay; the end of this file states how PnP calls it.)  The device code (pnp.hip) and the CPU test stub
// (tests/stub/pnp_capi.cpp) share these bodies, so the device result is checked bit for bit against a CPU build of the
// same operations.  The rule list is in include/sfmhip.h (sfmhip_pnp_ransac).  Compile with -ffp-contract=off.
// PARITY UNPINNED: OpenCV is not in the image; the operation order is recalled from its 3.4.1 sources.
//
// Two things here are this project's own and not the library's:
//   - a sum over the points of a problem (centroid, covariance, M^T M, the Procrustes sums, the reprojection error) is
//     taken in ONE fixed order, whoever computes it: point i goes to slot i mod 256 (slots start at +0.0 and add their
//     points in ascending i); each group of 64 slots is folded by strides 32, 16, 8, 4, 2, 1 (slot l += slot l + stride);
//     the four group sums are added as (g0 + g1) + (g2 + g3).  A workgroup of 256 lanes does this with wave shuffles, a
//     single thread does it in a loop, and for five points it is ((t0 + t4) + t2) + (t1 + t3);
//   - sin, cos and acos are restated below in plain f64 arithmetic (measured: at most 1 ulp from libm on 20 000 random arguments each; the test allows 2): libm's
//     and the device library's differ in the last bit, and a pose must not.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include "camera.h"
#include "jacobi.h"
#include "pose.h"

#ifdef __HIPCC__
#define SFM_PNP_HD __host__ __device__
#else
#define SFM_PNP_HD
#endif

namespace sfmpnp {

using sfmjacobi::jacobi_svd;

enum {
  FLAG_RANK_DEFICIENT = 1,  // the control-point covariance of a point set has rank < 3 (planar / collinear points): not solved
  FLAG_SVD_RANDOM = 2,      // a 3 x 3 singular value <= DBL_MIN: the library's random-vector branch (not restated, pose.h)
  FLAG_QR_SINGULAR = 4      // qr_solve met a zero column: the library returns with its x uninitialised; here x = 0
};
enum { MODEL_POINTS = 5, SLOTS = 256 };

// element i of a work area whose consecutive doubles are S apart (S = 64: interleaved over a wave)
template <int S>
struct Mem {
  double* p;
  SFM_PNP_HD double& operator[](int i) const { return p[(size_t)i * S]; }
};

// the work area of one solve, in doubles
enum {
  W_AT = 0,      // 12 x 12: M^T M, then the rows of U^T
  W_VT = 144,    // 12 x 12
  W_W = 288,     // 12
  W_L = 300,     // 6 x 10
  W_SA = 360,    // k x 6, k <= 5: the transposed 6 x k system of a beta approximation
  W_SV = 390,    // k x k
  W_SW = 415,    // k
  W_QA = 420,    // 6 x 4 (Gauss-Newton)
  W_QB = 444,    // 6
  W_QA1 = 450,   // 4
  W_QA2 = 454,   // 4
  W_QX = 458,    // 4
  W_CWS = 462,   // 4 x 3 control points
  W_CI = 474,    // 3 x 3
  W_BET = 483,   // 3 x 4
  W_CCS = 495,   // 4 x 3
  W_PCW = 507,   // pc0, pw0
  W_RT = 513,    // 3 x (R 9, t 3)
  W_ERR = 549,   // 3
  W_RHO = 552,   // 6
  W_ACC = 558,   // 2 x 78: the output of a sum over the points (and the second accumulator of the five-point form)
  WORK_DOUBLES = 714
};

// ------------------------------------------------------------------ sin, cos, acos
// x >= 0 of moderate size (a rotation angle): k = round(x * 2 / pi), y = x - k * pi / 2 with pi / 2 in two pieces, Taylor
// polynomials of sin and cos on |y| <= pi / 4 (Horner), the quadrant from k
SFM_PNP_HD inline void sincos_restated(double x, double& s, double& c) {
  const double k = floor(x * 0.63661977236758134308 + 0.5);
  const double y = (x - k * 1.57079632679489655800e+00) - k * 6.12323399573676603587e-17;
  const double z = y * y;
  double ps = -1.0 / 121645100408832000.0;                 // 19!
  ps = 1.0 / 355687428096000.0 + z * ps;                   // 17!
  ps = -1.0 / 1307674368000.0 + z * ps;                    // 15!
  ps = 1.0 / 6227020800.0 + z * ps;                        // 13!
  ps = -1.0 / 39916800.0 + z * ps;                         // 11!
  ps = 1.0 / 362880.0 + z * ps;                            // 9!
  ps = -1.0 / 5040.0 + z * ps;                             // 7!
  ps = 1.0 / 120.0 + z * ps;                               // 5!
  ps = -1.0 / 6.0 + z * ps;                                // 3!
  const double sy = y + y * (z * ps);
  double pc = 1.0 / 2432902008176640000.0;                 // 20!
  pc = -1.0 / 6402373705728000.0 + z * pc;                 // 18!
  pc = 1.0 / 20922789888000.0 + z * pc;                    // 16!
  pc = -1.0 / 87178291200.0 + z * pc;                      // 14!
  pc = 1.0 / 479001600.0 + z * pc;                         // 12!
  pc = -1.0 / 3628800.0 + z * pc;                          // 10!
  pc = 1.0 / 40320.0 + z * pc;                             // 8!
  pc = -1.0 / 720.0 + z * pc;                              // 6!
  pc = 1.0 / 24.0 + z * pc;                                // 4!
  const double cy = (1.0 - 0.5 * z) + z * (z * pc);
  const int q = (int)((long long)k & 3);
  s = q == 0 ? sy : q == 1 ? cy : q == 2 ? -sy : -cy;
  c = q == 0 ? cy : q == 1 ? -sy : q == 2 ? -cy : sy;
}

// acos on [-1, 1]: the rational approximation of asin's remainder (the coefficients FreeBSD's msun e_acos.c publishes),
// with the head of sqrt(z) taken as its float value instead of by clearing the low word
SFM_PNP_HD inline double acos_poly(double z) {
  const double p = z * (1.66666666666666657415e-01 +
                        z * (-3.25565818622400915405e-01 +
                             z * (2.01212532134862925881e-01 +
                                  z * (-4.00555345006794114027e-02 + z * (7.91534994289814532176e-04 + z * 3.47933107596021167570e-05)))));
  const double q =
      1.0 + z * (-2.40339491173441421878e+00 + z * (2.02094576023350569471e+00 + z * (-6.88283971605453293030e-01 + z * 7.70381505559019352791e-02)));
  return p / q;
}
SFM_PNP_HD inline double acos_restated(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
  if (!(x > -1.0)) return x == -1.0 ? pi + 2.0 * pio2_lo : NAN;
  if (!(x < 1.0)) return x == 1.0 ? 0.0 : NAN;
  if (fabs(x) < 0.5) {
    const double r = acos_poly(x * x);
    return pio2_hi - (x - (pio2_lo - r * x));
  }
  if (x < 0) {
    const double z = (1.0 + x) * 0.5, s = sqrt(z), r = acos_poly(z), w = r * s - pio2_lo;
    return pi - 2.0 * (s + w);
  }
  const double z = (1.0 - x) * 0.5, s = sqrt(z), df = (double)(float)s, c = (z - df * df) / (s + df), r = acos_poly(z), w = r * s + c;
  return 2.0 * (df + w);
}

// ------------------------------------------------------------------ Rodrigues (calib3d/calibration.cpp cvRodrigues2)
// vector -> matrix: theta = norm(r); theta < DBL_EPSILON: I; else R = c I + (1 - c) r r^T + s [r]x with r /= theta
SFM_PNP_HD inline void rodrigues_to_matrix(const double rv[3], double R[9]) {
  const double theta = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
  if (theta < DBL_EPSILON) {
    for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  double s, c;
  sincos_restated(theta, s, c);
  const double c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
  const double x = rv[0] * itheta, y = rv[1] * itheta, z = rv[2] * itheta;
  const double rrt[9] = {x * x, x * y, x * z, x * y, y * y, y * z, x * z, y * z, z * z};
  const double rx[9] = {0, -z, y, z, 0, -x, -y, x, 0};
  for (int k = 0; k < 9; ++k) R[k] = (c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k]) + s * rx[k];
}

// matrix -> vector: an entry outside [-100, 100) (or not a number) gives the zero vector; R <- U Vt of its SVD; then the
// library's branches on s = |axis| / 2 and c = (trace - 1) / 2.  Returns svd3's flag as FLAG_SVD_RANDOM.
SFM_PNP_HD inline int rodrigues_to_vector(const double Rin[9], double rv[3]) {
  for (int k = 0; k < 9; ++k)
    if (!(Rin[k] >= -100. && Rin[k] < 100.)) {
      rv[0] = rv[1] = rv[2] = 0;
      return 0;
    }
  double U[9], W[3], Vt[9], R[9];
  const int fl = sfmpose::svd3(Rin, U, W, Vt) ? FLAG_SVD_RANDOM : 0;
  sfmpose::mul3(U, Vt, R);
  double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
  const double s = sqrt((rx * rx + ry * ry + rz * rz) * 0.25);
  double c = (R[0] + R[4] + R[8] - 1) * 0.5;
  c = c > 1. ? 1. : c < -1. ? -1. : c;
  double theta = acos_restated(c);
  if (s < 1e-5) {
    if (c > 0) {
      rx = ry = rz = 0;
    } else {
      double t = (R[0] + 1) * 0.5;
      rx = sqrt(t > 0. ? t : 0.);
      t = (R[4] + 1) * 0.5;
      ry = sqrt(t > 0. ? t : 0.) * (R[1] < 0 ? -1. : 1.);
      t = (R[8] + 1) * 0.5;
      rz = sqrt(t > 0. ? t : 0.) * (R[2] < 0 ? -1. : 1.);
      if (fabs(rx) < fabs(ry) && fabs(rx) < fabs(rz) && (R[5] > 0) != (ry * rz > 0)) rz = -rz;
      theta /= sqrt(rx * rx + ry * ry + rz * rz);
      rx *= theta;
      ry *= theta;
      rz *= theta;
    }
  } else {
    double vth = 1 / (2 * s);
    vth *= theta;
    rx *= vth;
    ry *= vth;
    rz *= vth;
  }
  rv[0] = rx;
  rv[1] = ry;
  rv[2] = rz;
  return fl;
}

// P = [R(rvec) | t], row-major 3 x 4
SFM_PNP_HD inline void pose_matrix(const double rv[3], const double tv[3], double P[12]) {
  double R[9];
  rodrigues_to_matrix(rv, R);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P[4 * r + c] = R[3 * r + c];
    P[4 * r + 3] = tv[r];
  }
}

// PnPRansacCallback::computeError for one correspondence: projectPoints in f64 from the float point, the projection stored
// as float, the difference and its squared L2 norm in float
SFM_PNP_HD inline float reproj_err2(const double P[12], const double* K, const double* dist, float X, float Y, float Z, float u,
                                    float v) {
  const double Xd[3] = {(double)X, (double)Y, (double)Z};
  double pu, pv;
  sfmcam::project_point(P, K, dist, Xd, pu, pv);
  const float dx = u - (float)pu, dy = v - (float)pv;
  float s = 0;
  s += dx * dx;
  s += dy * dy;
  return s;
}

// ------------------------------------------------------------------ EPnP: what one point contributes
SFM_PNP_HD inline double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// compute_barycentric_coordinates for one point
SFM_PNP_HD inline void alphas_of(const double cws[12], const double ci[9], const double pw[3], double a[4]) {
#pragma unroll
  for (int j = 0; j < 3; ++j)
    a[1 + j] = ci[3 * j] * (pw[0] - cws[0]) + ci[3 * j + 1] * (pw[1] - cws[1]) + ci[3 * j + 2] * (pw[2] - cws[2]);
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

// fill_M's two rows for one point (fu = fv = 1, uc = vc = 0) and their part of the upper triangle of M^T M, row by row
SFM_PNP_HD inline void mtm_terms(const double a[4], double u, double v, double t[78]) {
  double M1[12], M2[12];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    M1[3 * i] = a[i];
    M1[3 * i + 1] = 0.0;
    M1[3 * i + 2] = a[i] * (0.0 - u);
    M2[3 * i] = 0.0;
    M2[3 * i + 1] = a[i];
    M2[3 * i + 2] = a[i] * (0.0 - v);
  }
  int idx = 0;
#pragma unroll
  for (int r = 0; r < 12; ++r)
#pragma unroll
    for (int c = r; c < 12; ++c) t[idx++] = M1[r] * M1[c] + M2[r] * M2[c];
}

// compute_pcs for one point
SFM_PNP_HD inline void pc_of(const double a[4], const double ccs[12], double pc[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) pc[j] = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
}

// reprojection_error's term for one point
SFM_PNP_HD inline double reproj_term(const double R[9], const double t[3], const double pw[3], double u, double v) {
  const double Xc = dot3(R, pw) + t[0], Yc = dot3(R + 3, pw) + t[1], inv_Zc = 1.0 / (dot3(R + 6, pw) + t[2]);
  const double ue = Xc * inv_Zc, ve = Yc * inv_Zc;
  return sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}

// ------------------------------------------------------------------ EPnP: the serial stages (one thread; w = its work area)
// choose_control_points after the sums (c0 = centroid, cov = upper triangle of PW0^T PW0) and cvInvert(CC, CV_SVD):
// w[W_CWS], w[W_CI].  Returns flags; FLAG_RANK_DEFICIENT when the third singular value is <= 1e-12 of the first.
template <int S>
SFM_PNP_HD inline int stage_control(int n, const double c0[3], const double cov[6], Mem<S> w) {
  const double A[9] = {cov[0], cov[1], cov[2], cov[1], cov[3], cov[4], cov[2], cov[4], cov[5]};
  double U[9], D[3], Vt[9];
  int fl = sfmpose::svd3(A, U, D, Vt) ? FLAG_SVD_RANDOM : 0;
  if (!(D[2] > D[0] * 1e-12)) fl |= FLAG_RANK_DEFICIENT;
  double cws[12];
  for (int j = 0; j < 3; ++j) cws[j] = c0[j];
  for (int i = 1; i < 4; ++i) {
    const double k = sqrt(D[i - 1] / (double)n);
    for (int j = 0; j < 3; ++j) cws[3 * i + j] = c0[j] + k * U[3 * j + (i - 1)];  // uct[3 (i - 1) + j]
  }
  double cc[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 1; j < 4; ++j) cc[3 * i + j - 1] = cws[3 * j + i] - cws[i];
  // SVD::compute + SVD::backSubst against the identity: x += vt[k][i] * (u[j][k] / w[k]) for w[k] above 2 eps sum(w)
  if (sfmpose::svd3(cc, U, D, Vt)) fl |= FLAG_SVD_RANDOM;
  double thr = 0;
  for (int k = 0; k < 3; ++k) thr += D[k];
  thr *= DBL_EPSILON * 2;
  double ci[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < 3; ++k) {
    double wi = D[k];
    if (fabs(wi) <= thr) continue;
    wi = 1 / wi;
    double buf[3];
    for (int j = 0; j < 3; ++j) buf[j] = U[3 * j + k] * wi;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) ci[3 * i + j] = ci[3 * i + j] + Vt[3 * k + i] * buf[j];
  }
  for (int k = 0; k < 12; ++k) w[W_CWS + k] = cws[k];
  for (int k = 0; k < 9; ++k) w[W_CI + k] = ci[k];
  return fl;
}

// cvSolve(L_6xK, Rho, x, CV_SVD): JacobiSVD on the transposed system, SVBkSb with one right-hand side
template <int K, int S>
SFM_PNP_HD inline void svd_solve6(Mem<S> w, const int (&cols)[K], double x[K]) {
  for (int c = 0; c < K; ++c)
    for (int r = 0; r < 6; ++r) w[W_SA + c * 6 + r] = w[W_L + r * 10 + cols[c]];
  jacobi_svd<6, K, K, 6, S>(&w[W_SA], &w[W_SW], &w[W_SV]);
  double thr = 0;
  for (int c = 0; c < K; ++c) thr += w[W_SW + c];
  thr *= DBL_EPSILON * 2;
#pragma unroll
  for (int j = 0; j < K; ++j) x[j] = 0;
  for (int c = 0; c < K; ++c) {
    double wi = w[W_SW + c];
    if (fabs(wi) <= thr) continue;
    wi = 1 / wi;
    double s = 0;
    for (int j = 0; j < 6; ++j) s += w[W_SA + c * 6 + j] * w[W_RHO + j];
    s *= wi;
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = x[j] + s * w[W_SV + c * K + j];
  }
}

// epnp::qr_solve on the 6 x 4 system of w[W_QA], w[W_QB] -> w[W_QX] (the file's own Householder QR; its column maximum
// looks at rows k .. nr - 2, as the file does).  Returns FLAG_QR_SINGULAR (x = 0) when a column is zero.
template <int S>
SFM_PNP_HD inline int qr_solve64(Mem<S> w) {
  const int nr = 6, nc = 4;
  for (int k = 0; k < nc; ++k) {
    double eta = fabs(w[W_QA + k * nc + k]);
    for (int i = k + 1; i < nr; ++i) {
      const double elt = fabs(w[W_QA + (i - 1) * nc + k]);
      if (eta < elt) eta = elt;
    }
    if (eta == 0) {
      for (int i = 0; i < nc; ++i) w[W_QX + i] = 0;
      return FLAG_QR_SINGULAR;
    }
    double sum2 = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; ++i) {
      const double t = w[W_QA + i * nc + k] * inv_eta;
      w[W_QA + i * nc + k] = t;
      sum2 += t * t;
    }
    double sigma = sqrt(sum2);
    if (w[W_QA + k * nc + k] < 0) sigma = -sigma;
    const double akk = w[W_QA + k * nc + k] + sigma;
    w[W_QA + k * nc + k] = akk;
    w[W_QA1 + k] = sigma * akk;
    w[W_QA2 + k] = -eta * sigma;
    for (int j = k + 1; j < nc; ++j) {
      double sum = 0;
      for (int i = k; i < nr; ++i) sum += w[W_QA + i * nc + k] * w[W_QA + i * nc + j];
      const double tau = sum / w[W_QA1 + k];
      for (int i = k; i < nr; ++i) w[W_QA + i * nc + j] -= tau * w[W_QA + i * nc + k];
    }
  }
  for (int j = 0; j < nc; ++j) {  // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; ++i) tau += w[W_QA + i * nc + j] * w[W_QB + i];
    tau /= w[W_QA1 + j];
    for (int i = j; i < nr; ++i) w[W_QB + i] -= tau * w[W_QA + i * nc + j];
  }
  w[W_QX + nc - 1] = w[W_QB + nc - 1] / w[W_QA2 + nc - 1];  // X = R^-1 b
  for (int i = nc - 2; i >= 0; --i) {
    double sum = 0;
    for (int j = i + 1; j < nc; ++j) sum += w[W_QA + i * nc + j] * w[W_QX + j];
    w[W_QX + i] = (w[W_QB + i] - sum) / w[W_QA2 + i];
  }
  return 0;
}

// gauss_newton: five steps on betas (in place)
template <int S>
SFM_PNP_HD inline int gauss_newton(Mem<S> w, double b[4]) {
  int fl = 0;
  for (int it = 0; it < 5; ++it) {
    for (int i = 0; i < 6; ++i) {
      double L[10];
#pragma unroll
      for (int k = 0; k < 10; ++k) L[k] = w[W_L + i * 10 + k];
      w[W_QA + i * 4 + 0] = 2 * L[0] * b[0] + L[1] * b[1] + L[3] * b[2] + L[6] * b[3];
      w[W_QA + i * 4 + 1] = L[1] * b[0] + 2 * L[2] * b[1] + L[4] * b[2] + L[7] * b[3];
      w[W_QA + i * 4 + 2] = L[3] * b[0] + L[4] * b[1] + 2 * L[5] * b[2] + L[8] * b[3];
      w[W_QA + i * 4 + 3] = L[6] * b[0] + L[7] * b[1] + L[8] * b[2] + 2 * L[9] * b[3];
      w[W_QB + i] = w[W_RHO + i] - (L[0] * b[0] * b[0] + L[1] * b[0] * b[1] + L[2] * b[1] * b[1] + L[3] * b[0] * b[2] +
                                    L[4] * b[1] * b[2] + L[5] * b[2] * b[2] + L[6] * b[0] * b[3] + L[7] * b[1] * b[3] +
                                    L[8] * b[2] * b[3] + L[9] * b[3] * b[3]);
    }
    fl |= qr_solve64<S>(w);
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] += w[W_QX + i];
  }
  return fl;
}

// after M^T M is in w[W_AT] (full, symmetric): its SVD (U^T in place), L_6x10, rho, and the three refined beta sets
template <int S>
SFM_PNP_HD inline int stage_betas(Mem<S> w) {
  jacobi_svd<12, 12, 12, 12, S>(&w[W_AT], &w[W_W], &w[W_VT]);
  // compute_L_6x10: v[i] = row 11 - i of U^T; dv[i][pair] = v[i](a) - v[i](b) over the pairs of control points
#pragma unroll
  for (int pr = 0; pr < 6; ++pr) {
    const int a = pr < 3 ? 0 : pr < 5 ? 1 : 2, b = pr < 3 ? pr + 1 : pr < 5 ? pr - 1 : 3;
    double dv[4][3];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int c = 0; c < 3; ++c) dv[i][c] = w[W_AT + 12 * (11 - i) + 3 * a + c] - w[W_AT + 12 * (11 - i) + 3 * b + c];
    const int r = W_L + 10 * pr;
    w[r + 0] = dot3(dv[0], dv[0]);
    w[r + 1] = 2.0 * dot3(dv[0], dv[1]);
    w[r + 2] = dot3(dv[1], dv[1]);
    w[r + 3] = 2.0 * dot3(dv[0], dv[2]);
    w[r + 4] = 2.0 * dot3(dv[1], dv[2]);
    w[r + 5] = dot3(dv[2], dv[2]);
    w[r + 6] = 2.0 * dot3(dv[0], dv[3]);
    w[r + 7] = 2.0 * dot3(dv[1], dv[3]);
    w[r + 8] = 2.0 * dot3(dv[2], dv[3]);
    w[r + 9] = dot3(dv[3], dv[3]);
    // compute_rho: dist2 of the same pair of control points
    const double d0 = w[W_CWS + 3 * a] - w[W_CWS + 3 * b], d1 = w[W_CWS + 3 * a + 1] - w[W_CWS + 3 * b + 1],
                 d2 = w[W_CWS + 3 * a + 2] - w[W_CWS + 3 * b + 2];
    w[W_RHO + pr] = d0 * d0 + d1 * d1 + d2 * d2;
  }
  int fl = 0;
  double be[4];
  {  // find_betas_approx_1: [B11 B12 B13 B14]
    const int cols[4] = {0, 1, 3, 6};
    double b4[4];
    svd_solve6<4, S>(w, cols, b4);
    if (b4[0] < 0) {
      be[0] = sqrt(-b4[0]);
      be[1] = -b4[1] / be[0];
      be[2] = -b4[2] / be[0];
      be[3] = -b4[3] / be[0];
    } else {
      be[0] = sqrt(b4[0]);
      be[1] = b4[1] / be[0];
      be[2] = b4[2] / be[0];
      be[3] = b4[3] / be[0];
    }
    fl |= gauss_newton<S>(w, be);
    for (int i = 0; i < 4; ++i) w[W_BET + i] = be[i];
  }
  {  // find_betas_approx_2: [B11 B12 B22]
    const int cols[3] = {0, 1, 2};
    double b3[3];
    svd_solve6<3, S>(w, cols, b3);
    if (b3[0] < 0) {
      be[0] = sqrt(-b3[0]);
      be[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
      be[0] = sqrt(b3[0]);
      be[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) be[0] = -be[0];
    be[2] = 0.0;
    be[3] = 0.0;
    fl |= gauss_newton<S>(w, be);
    for (int i = 0; i < 4; ++i) w[W_BET + 4 + i] = be[i];
  }
  {  // find_betas_approx_3: [B11 B12 B22 B13 B23]
    const int cols[5] = {0, 1, 2, 3, 4};
    double b5[5];
    svd_solve6<5, S>(w, cols, b5);
    if (b5[0] < 0) {
      be[0] = sqrt(-b5[0]);
      be[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
      be[0] = sqrt(b5[0]);
      be[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) be[0] = -be[0];
    be[2] = b5[3] / be[0];
    be[3] = 0.0;
    fl |= gauss_newton<S>(w, be);
    for (int i = 0; i < 4; ++i) w[W_BET + 8 + i] = be[i];
  }
  return fl;
}

// compute_ccs for beta set N, then solve_for_sign by the first point's camera-frame depth (pw0 = the first point)
template <int S>
SFM_PNP_HD inline void stage_ccs(Mem<S> w, int N, const double pw_first[3]) {
  double ccs[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) ccs[k] = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double bi = w[W_BET + 4 * N + i];
#pragma unroll
    for (int k = 0; k < 12; ++k) ccs[k] += bi * w[W_AT + 12 * (11 - i) + k];
  }
  double cws[12], ci[9], a[4], pc[3];
#pragma unroll
  for (int k = 0; k < 12; ++k) cws[k] = w[W_CWS + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) ci[k] = w[W_CI + k];
  alphas_of(cws, ci, pw_first, a);
  pc_of(a, ccs, pc);
  const bool neg = pc[2] < 0.0;
#pragma unroll
  for (int k = 0; k < 12; ++k) w[W_CCS + k] = neg ? -ccs[k] : ccs[k];
}

// estimate_R_and_t after the sums (abt: 9, row-major; w[W_PCW] = pc0, pw0) -> w[W_RT + 12 N]
template <int S>
SFM_PNP_HD inline int stage_rt(Mem<S> w, int N, const double abt[9]) {
  double U[9], D[3], Vt[9], R[9];
  const int fl = sfmpose::svd3(abt, U, D, Vt) ? FLAG_SVD_RANDOM : 0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[3 * i + j] = U[3 * i] * Vt[j] + U[3 * i + 1] * Vt[3 + j] + U[3 * i + 2] * Vt[6 + j];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                     R[0] * R[5] * R[7];
  if (det < 0) {
    R[6] = -R[6];
    R[7] = -R[7];
    R[8] = -R[8];
  }
  const double pc0[3] = {w[W_PCW], w[W_PCW + 1], w[W_PCW + 2]}, pw0[3] = {w[W_PCW + 3], w[W_PCW + 4], w[W_PCW + 5]};
  for (int k = 0; k < 9; ++k) w[W_RT + 12 * N + k] = R[k];
  for (int i = 0; i < 3; ++i) w[W_RT + 12 * N + 9 + i] = pc0[i] - dot3(R + 3 * i, pw0);
  return fl;
}

// compute_pose's choice: N = 1, then 2 if its error is smaller, then 3 if smaller than the choice so far (0-based here)
template <int S>
SFM_PNP_HD inline int stage_choose(Mem<S> w) {
  int N = 0;
  if (w[W_ERR + 1] < w[W_ERR + 0]) N = 1;
  if (w[W_ERR + 2] < w[W_ERR + N]) N = 2;
  return N;
}

// ------------------------------------------------------------------ EPnP by one thread
// Pts: n, get(i, pw[3], uv[2]).  Red: run<K>(n, f, w): the sum over the points of f(i, t[K]) in the fixed order, into
// w[W_ACC .. W_ACC + K).  Returns the flags; R, t untouched when FLAG_RANK_DEFICIENT is set.
template <int S, class Pts, class Red>
SFM_PNP_HD inline int epnp_solve(const Pts& pts, Red& red, Mem<S> w, double R[9], double t[3]) {
  const int n = pts.n;
  double c0[3], cov[6];
  red.template run<3>(n, [&](int i, double* o) {
    double pw[3], uv[2];
    pts.get(i, pw, uv);
    o[0] = pw[0];
    o[1] = pw[1];
    o[2] = pw[2];
  }, w);
  for (int j = 0; j < 3; ++j) c0[j] = w[W_ACC + j] / (double)n;
  red.template run<6>(n, [&](int i, double* o) {
    double pw[3], uv[2];
    pts.get(i, pw, uv);
    const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
    o[0] = d0 * d0;
    o[1] = d0 * d1;
    o[2] = d0 * d2;
    o[3] = d1 * d1;
    o[4] = d1 * d2;
    o[5] = d2 * d2;
  }, w);
  for (int j = 0; j < 6; ++j) cov[j] = w[W_ACC + j];
  int fl = stage_control<S>(n, c0, cov, w);
  if (fl & FLAG_RANK_DEFICIENT) return fl;
  double cws[12], ci[9];
  for (int k = 0; k < 12; ++k) cws[k] = w[W_CWS + k];
  for (int k = 0; k < 9; ++k) ci[k] = w[W_CI + k];
  red.template run<78>(n, [&](int i, double* o) {
    double pw[3], uv[2], a[4];
    pts.get(i, pw, uv);
    alphas_of(cws, ci, pw, a);
    mtm_terms(a, uv[0], uv[1], o);
  }, w);
  {
    int idx = 0;
    for (int r = 0; r < 12; ++r)
      for (int c = r; c < 12; ++c, ++idx) {
        const double v = w[W_ACC + idx];
        w[W_AT + 12 * r + c] = v;
        w[W_AT + 12 * c + r] = v;
      }
  }
  fl |= stage_betas<S>(w);
  double pw_first[3], uv_first[2];
  pts.get(0, pw_first, uv_first);
  for (int N = 0; N < 3; ++N) {
    stage_ccs<S>(w, N, pw_first);
    double ccs[12];
    for (int k = 0; k < 12; ++k) ccs[k] = w[W_CCS + k];
    red.template run<6>(n, [&](int i, double* o) {
      double pw[3], uv[2], a[4], pc[3];
      pts.get(i, pw, uv);
      alphas_of(cws, ci, pw, a);
      pc_of(a, ccs, pc);
      o[0] = pc[0];
      o[1] = pc[1];
      o[2] = pc[2];
      o[3] = pw[0];
      o[4] = pw[1];
      o[5] = pw[2];
    }, w);
    double pc0[3], pw0[3];
    for (int j = 0; j < 3; ++j) {
      pc0[j] = w[W_ACC + j] / (double)n;
      pw0[j] = w[W_ACC + 3 + j] / (double)n;
      w[W_PCW + j] = pc0[j];
      w[W_PCW + 3 + j] = pw0[j];
    }
    red.template run<9>(n, [&](int i, double* o) {
      double pw[3], uv[2], a[4], pc[3];
      pts.get(i, pw, uv);
      alphas_of(cws, ci, pw, a);
      pc_of(a, ccs, pc);
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) o[3 * j + k] = (pc[j] - pc0[j]) * (pw[k] - pw0[k]);
    }, w);
    double abt[9];
    for (int k = 0; k < 9; ++k) abt[k] = w[W_ACC + k];
    fl |= stage_rt<S>(w, N, abt);
    double Rn[9], tn[3];
    for (int k = 0; k < 9; ++k) Rn[k] = w[W_RT + 12 * N + k];
    for (int k = 0; k < 3; ++k) tn[k] = w[W_RT + 12 * N + 9 + k];
    red.template run<1>(n, [&](int i, double* o) {
      double pw[3], uv[2];
      pts.get(i, pw, uv);
      o[0] = reproj_term(Rn, tn, pw, uv[0], uv[1]);
    }, w);
    w[W_ERR + N] = w[W_ACC] / (double)n;
  }
  const int N = stage_choose<S>(w);
  for (int k = 0; k < 9; ++k) R[k] = w[W_RT + 12 * N + k];
  for (int k = 0; k < 3; ++k) t[k] = w[W_RT + 12 * N + 9 + k];
  return fl;
}

// the fixed-order sum for exactly five points by one thread: ((t0 + t4) + t2) + (t1 + t3), every term entering as 0.0 + t
template <int S>
struct ReduceFive {
  template <int K, class F>
  SFM_PNP_HD void run(int, F f, Mem<S> w) {
    double t[K];
    f(0, t);
#pragma unroll
    for (int k = 0; k < K; ++k) w[W_ACC + k] = 0.0 + t[k];
    f(4, t);
#pragma unroll
    for (int k = 0; k < K; ++k) w[W_ACC + k] = w[W_ACC + k] + (0.0 + t[k]);
    f(2, t);
#pragma unroll
    for (int k = 0; k < K; ++k) w[W_ACC + k] = w[W_ACC + k] + (0.0 + t[k]);
    f(1, t);
#pragma unroll
    for (int k = 0; k < K; ++k) w[W_ACC + 78 + k] = 0.0 + t[k];
    f(3, t);
#pragma unroll
    for (int k = 0; k < K; ++k) w[W_ACC + k] = w[W_ACC + k] + (w[W_ACC + 78 + k] + (0.0 + t[k]));
  }
};

// one RANSAC sample: five float correspondences (object point, pixel) -> the model (rvec, tvec).  undistortPoints writes
// float, EPnP reads the floats.  Returns 1 model (0 when the sample is flagged rank-deficient) | flags << 8.
struct FivePoints {
  int n;
  double pw[5][3], uv[5][2];
  SFM_PNP_HD void get(int i, double* p, double* q) const {
    // (i is a constant at every call site of ReduceFive; the selects keep the arrays in registers otherwise)
#pragma unroll
    for (int k = 0; k < 5; ++k)
      if (k == i) {
        p[0] = pw[k][0];
        p[1] = pw[k][1];
        p[2] = pw[k][2];
        q[0] = uv[k][0];
        q[1] = uv[k][1];
      }
  }
};
template <int S>
SFM_PNP_HD inline int solve_sample(const float xyz[5][3], const float xy[5][2], const double* K, const double* dist, Mem<S> w,
                                   double model[6]) {
  FivePoints pts;
  pts.n = 5;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    double x, y;
    sfmcam::undistort_point(K, dist, (double)xy[k][0], (double)xy[k][1], x, y);
    pts.uv[k][0] = (double)(float)x;
    pts.uv[k][1] = (double)(float)y;
    for (int j = 0; j < 3; ++j) pts.pw[k][j] = (double)xyz[k][j];
  }
  ReduceFive<S> red;
  double R[9], t[3];
  int fl = epnp_solve<S>(pts, red, w, R, t);
  if (fl & FLAG_RANK_DEFICIENT) {
    for (int k = 0; k < 6; ++k) model[k] = 0;
    return 0 | (fl << 8);
  }
  fl |= rodrigues_to_vector(R, model);
  for (int k = 0; k < 3; ++k) model[3 + k] = t[k];
  return 1 | (fl << 8);
}

}  // namespace sfmpnp

// ==================================================================== host only: how PnP calls ptsetreg.cpp's loop
#include <algorithm>
#include <vector>
#include "ransac_host.h"

namespace sfmpnp {

using sfmransac::Job;
using sfmransac::Keep;
using sfmransac::ViewState;

// sfmransac::ransac_replay as solvePnPRansac runs it: five points and one model per sample, the per-count sample streams,
// the limit max_iters (none: a view of more than five correspondences is not looked at).  pnp.hip and the CPU test stub
// both call this, each with its backend.
template <class Backend>
int ransac_replay(Backend& be, int n_views, const int32_t* offsets, double confidence, int max_iters, std::vector<ViewState>& vs,
                  int& flags_any) {
  sfmransac::CountSamples draw;
  return sfmransac::ransac_replay(be, draw, MODEL_POINTS, 1, n_views, offsets, confidence, std::max(max_iters, 0), vs, flags_any);
}

}  // namespace sfmpnp
