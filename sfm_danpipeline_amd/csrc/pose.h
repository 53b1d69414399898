// pose.h -- the numerics of getCameraPose (reference src/Sfm.cpp:713-799) as __host__ __device__ code that hipcc and a
// plain g++ both compile: OpenCV 3.4.1's triangulatePoints DLT (the 4 x 4 one-sided Jacobi of triangulate.hip),
// SVD::compute on a 3 x 3, decomposeEssentialMat, recoverPose's per-point test of its four candidate poses and its
// selection rule, and CheckCoherentRotation (Eigen FullPivLU determinant, narrowed to float by fabsf).  The device code
// (pose.hip, triangulate.hip) and the CPU test stub (tests/stub/pose_capi.cpp) share these bodies, so the device result
// is checked bit for bit against a CPU build of the same operations.  Compile with -ffp-contract=off.
// PARITY UNPINNED: OpenCV and Eigen are not in the image; the operation order is recalled from their 3.4.1 / 3.3 sources.
#pragma once
#include <cfloat>
#include <cmath>
#include "hypot_glibc.h"

#ifdef __HIPCC__
#define SFM_POSE_INLINE __host__ __device__ __forceinline__
#else
#define SFM_POSE_INLINE inline __attribute__((always_inline))
#endif

namespace sfmpose {

enum { FLAG_SVD_RANDOM = 1 };  // a singular value <= DBL_MIN: JacobiSVDImpl_ fills the vector from RNG(0x12345678) (not restated)

// One-sided Jacobi on At (rows = columns of A), as OpenCV's JacobiSVDImpl_<double> runs it for a 4x4: rotations until
// every row pair is orthogonal to 10*eps, singular values = row norms, selection sort descending; returns Vt row 3.  All
// indices are compile-time so the 32 doubles stay in registers.  On the device the loop exit is wave-uniform; a lane that
// has converged sees no further rotation, so its values equal the host's per-lane exit.
SFM_POSE_INLINE void dlt_null_vector(double At[4][4], double out[4]) {
  const double eps = DBL_EPSILON * 10;
  double W[4], Vt[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sd += At[i][k] * At[i][k];
    W[i] = sd;
#pragma unroll
    for (int k = 0; k < 4; ++k) Vt[i][k] = (i == k) ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) {
        double a = W[i], p = 0, b = W[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) p += At[i][k] * At[j][k];
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = sfm_hypot(p, beta);  // (the host libm's hypot, bit for bit: hypot_glibc.h)
        double c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = sqrt(delta / gamma);
          c = p / (gamma * s * 2);
        } else {
          c = sqrt((gamma + beta) / (gamma * 2));
          s = p / (gamma * c * 2);
        }
        a = b = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double t0 = c * At[i][k] + s * At[j][k];
          const double t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0;
          At[j][k] = t1;
          a += t0 * t0;
          b += t1 * t1;
        }
        W[i] = a;
        W[j] = b;
        changed = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const double t0 = c * Vt[i][k] + s * Vt[j][k];
          const double t1 = -s * Vt[i][k] + c * Vt[j][k];
          Vt[i][k] = t0;
          Vt[j][k] = t1;
        }
      }
#ifdef __HIP_DEVICE_COMPILE__
    if (!__any(changed)) break;  // wave-uniform exit; converged lanes see no further rotation
#else
    if (!changed) break;
#endif
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) sd += At[i][k] * At[i][k];
    W[i] = sqrt(sd);
  }
  // row of the smallest singular value under OpenCV's descending selection sort = the LAST
  // position; among equal values the sort keeps the earlier row earlier, so take the last
  // index attaining the minimum... except that selection sort swaps can reorder equal values;
  // replay the sort on (W, row id) to land on exactly the row OpenCV leaves in position 3.
  int id[4] = {0, 1, 2, 3};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    int j = i;
#pragma unroll
    for (int k = i + 1; k < 4; ++k)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      const double tw = W[i];
      W[i] = W[j];
      W[j] = tw;
      const int ti = id[i];
      id[i] = id[j];
      id[j] = ti;
    }
  }
  const int sel = id[3];
#pragma unroll
  for (int k = 0; k < 4; ++k) out[k] = sel == 0 ? Vt[0][k] : sel == 1 ? Vt[1][k] : sel == 2 ? Vt[2][k] : Vt[3][k];
}

// SVD::compute(E, D, U, Vt) for a 3 x 3 (core/lapack.cpp _SVDcompute + JacobiSVDImpl_<double>, m = n = n1 = 3): the
// Jacobi runs on At = E^T, U's columns are the sorted rows of At scaled by 1 / sd.  A singular value <= DBL_MIN (where the
// library draws a random vector) sets FLAG_SVD_RANDOM and leaves that column zero.
SFM_POSE_INLINE int svd3(const double E[9], double U[9], double W[3], double Vt[9]) {
  const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
  double At[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 3; ++k) {
      At[i][k] = E[3 * k + i];
      V[i][k] = i == k ? 1.0 : 0.0;
    }
  for (int i = 0; i < 3; ++i) {
    double sd = 0;
    for (int k = 0; k < 3; ++k) sd += At[i][k] * At[i][k];
    W[i] = sd;
  }
  for (int iter = 0; iter < 30; ++iter) {
    bool changed = false;
    for (int i = 0; i < 2; ++i)
      for (int j = i + 1; j < 3; ++j) {
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < 3; ++k) p += At[i][k] * At[j][k];
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = sfm_hypot(p, beta);
        double c, s;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          s = sqrt(delta / gamma);
          c = p / (gamma * s * 2);
        } else {
          c = sqrt((gamma + beta) / (gamma * 2));
          s = p / (gamma * c * 2);
        }
        a = b = 0;
        for (int k = 0; k < 3; ++k) {
          const double t0 = c * At[i][k] + s * At[j][k];
          const double t1 = -s * At[i][k] + c * At[j][k];
          At[i][k] = t0;
          At[j][k] = t1;
          a += t0 * t0;
          b += t1 * t1;
        }
        W[i] = a;
        W[j] = b;
        changed = true;
        for (int k = 0; k < 3; ++k) {
          const double t0 = c * V[i][k] + s * V[j][k];
          const double t1 = -s * V[i][k] + c * V[j][k];
          V[i][k] = t0;
          V[j][k] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < 3; ++i) {
    double sd = 0;
    for (int k = 0; k < 3; ++k) sd += At[i][k] * At[i][k];
    W[i] = sqrt(sd);
  }
  for (int i = 0; i < 2; ++i) {
    int j = i;
    for (int k = i + 1; k < 3; ++k)
      if (W[j] < W[k]) j = k;
    if (i != j) {
      double t = W[i];
      W[i] = W[j];
      W[j] = t;
      for (int k = 0; k < 3; ++k) {
        t = At[i][k];
        At[i][k] = At[j][k];
        At[j][k] = t;
        t = V[i][k];
        V[i][k] = V[j][k];
        V[j][k] = t;
      }
    }
  }
  int flags = 0;
  for (int i = 0; i < 3; ++i) {
    const double sd = W[i];
    if (!(sd > minval)) flags |= FLAG_SVD_RANDOM;
    const double sc = sd > minval ? 1 / sd : 0.;
    for (int k = 0; k < 3; ++k) U[3 * k + i] = At[i][k] * sc;
    for (int k = 0; k < 3; ++k) Vt[3 * i + k] = V[i][k];
  }
  return flags;
}

// cv::determinant of a 3 x 3 double (core/lapack.cpp)
SFM_POSE_INLINE double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// c = a * b for 3 x 3 row-major, each sum in k order (gemm's small-matrix path, no FMA)
SFM_POSE_INLINE void mul3(const double* a, const double* b, double* c) {
  for (int r = 0; r < 3; ++r)
    for (int col = 0; col < 3; ++col) c[3 * r + col] = a[3 * r] * b[col] + a[3 * r + 1] * b[3 + col] + a[3 * r + 2] * b[6 + col];
}

// cv::decomposeEssentialMat (calib3d/five-point.cpp): R1 = U W Vt, R2 = U W^T Vt, t = U.col(2), with U and Vt negated
// when their determinant is negative.  Returns svd3's flags.
SFM_POSE_INLINE int decompose_essential(const double E[9], double R1[9], double R2[9], double t[3]) {
  double U[9], D[3], Vt[9];
  const int flags = svd3(E, U, D, Vt);
  if (det3(U) < 0)
    for (int k = 0; k < 9; ++k) U[k] *= -1.;
  if (det3(Vt) < 0)
    for (int k = 0; k < 9; ++k) Vt[k] *= -1.;
  const double W[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1}, Wt[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
  double UW[9];
  mul3(U, W, UW);  // (U * W) * Vt: the MatExpr evaluates the first product into a Mat
  mul3(UW, Vt, R1);
  mul3(U, Wt, UW);
  mul3(UW, Vt, R2);
  for (int k = 0; k < 3; ++k) t[k] = U[3 * k + 2] * 1.0;
  return flags;
}

// the candidate pose i (0..3) = [R1|t], [R2|t], [R1|-t], [R2|-t] as a 3 x 4 row-major P
SFM_POSE_INLINE void candidate(const double R1[9], const double R2[9], const double t[3], int i, double P[12]) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) P[4 * r + c] = ((i & 1) ? R2[3 * r + c] : R1[3 * r + c]) * 1.0;
    P[4 * r + 3] = (i & 2) ? -t[r] * 1.0 : t[r] * 1.0;
  }
}

// recoverPose's cheirality test of one normalised correspondence against P0 = [I|0] and P (calib3d/five-point.cpp):
// Q = triangulatePoints(P0, P, x1, x2); ok = Q2 Q3 > 0; Q /= Q3 (row 3 -> Q3 / Q3); ok &= Q2 < thr; z = P.row(2) Q
// (k order); ok &= z > 0 && z < thr.  Comparisons with a NaN are false.
SFM_POSE_INLINE bool cheirality(const double P[12], double x1, double y1, double x2, double y2, double dist_thr) {
  double At[4][4];  // At[c][r] = A[r][c]; A rows: x1 P0(2) - P0(0), y1 P0(2) - P0(1), x2 P(2) - P(0), y2 P(2) - P(1)
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double p0r0 = k == 0 ? 1.0 : 0.0, p0r1 = k == 1 ? 1.0 : 0.0, p0r2 = k == 2 ? 1.0 : 0.0;
    At[k][0] = x1 * p0r2 - p0r0;
    At[k][1] = y1 * p0r2 - p0r1;
    At[k][2] = x2 * P[8 + k] - P[0 + k];
    At[k][3] = y2 * P[8 + k] - P[4 + k];
  }
  double Q[4];
  dlt_null_vector(At, Q);
  bool ok = Q[2] * Q[3] > 0;
  const double X = Q[0] / Q[3], Y = Q[1] / Q[3], Z = Q[2] / Q[3], Wh = Q[3] / Q[3];
  ok = ok && Z < dist_thr;
  const double z = P[8] * X + P[9] * Y + P[10] * Z + P[11] * Wh;
  return ok && z > 0 && z < dist_thr;
}

// recoverPose's normalisation of a pixel: the one focal for both axes, by findEssentialMat's MatExpr route,
// (col - pp) / f = col * (1 / f) + (-pp * (1 / f))
SFM_POSE_INLINE void normalize(double u, double v, double f, double ppx, double ppy, double& x, double& y) {
  const double a = 1. / f;
  x = u * a + -ppx * a;
  y = v * a + -ppy * a;
}

// the four candidates' bits (bit i: candidate i passes) for one correspondence in pixels
SFM_POSE_INLINE unsigned candidate_bits(const double P[4][12], double u1, double v1, double u2, double v2, double f, double ppx,
                                        double ppy, double dist_thr) {
  double x1, y1, x2, y2;
  normalize(u1, v1, f, ppx, ppy, x1, y1);
  normalize(u2, v2, f, ppx, ppy, x2, y2);
  unsigned bits = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) bits |= cheirality(P[i], x1, y1, x2, y2, dist_thr) ? 1u << i : 0u;
  return bits;
}

// recoverPose's choice among the four counts: the first candidate whose count is >= every other
SFM_POSE_INLINE int select_candidate(const int g[4]) {
  if (g[0] >= g[1] && g[0] >= g[2] && g[0] >= g[3]) return 0;
  if (g[1] >= g[0] && g[1] >= g[2] && g[1] >= g[3]) return 1;
  if (g[2] >= g[0] && g[2] >= g[1] && g[2] >= g[3]) return 2;
  return 3;
}

// Eigen::FullPivLU<MatrixXd>(R).determinant() (Eigen 3.3): the largest |coefficient| of the remaining corner as pivot
// (column-major visit, the first of equal values), row and column swaps counted, the column below the pivot divided by
// it, the corner updated by the outer product; det = (+-1) * the diagonal's product in order
SFM_POSE_INLINE double fullpivlu_det3(const double R[9]) {
  double m[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) m[i][j] = R[3 * i + j];
  int swaps = 0;
  for (int k = 0; k < 3; ++k) {
    int br = k, bc = k;
    double best = fabs(m[k][k]);
    for (int j = k; j < 3; ++j)
      for (int i = k; i < 3; ++i)
        if (fabs(m[i][j]) > best) {
          best = fabs(m[i][j]);
          br = i;
          bc = j;
        }
    if (best == 0) break;  // (the remaining pivots stay zero: det = 0)
    if (br != k) {
      for (int j = 0; j < 3; ++j) {
        const double tmp = m[k][j];
        m[k][j] = m[br][j];
        m[br][j] = tmp;
      }
      ++swaps;
    }
    if (bc != k) {
      for (int i = 0; i < 3; ++i) {
        const double tmp = m[i][k];
        m[i][k] = m[i][bc];
        m[i][bc] = tmp;
      }
      ++swaps;
    }
    for (int i = k + 1; i < 3; ++i) m[i][k] /= m[k][k];
    for (int j = k + 1; j < 3; ++j)
      for (int i = k + 1; i < 3; ++i) m[i][j] -= m[i][k] * m[k][j];
  }
  const double prod = m[0][0] * m[1][1] * m[2][2];
  return (double)(swaps % 2 ? -1 : 1) * prod;
}

// CheckCoherentRotation's test (src/Sfm.cpp:793): fabsf(det) - 1.0 > 1e-07 fails.  fabsf narrows det to float: a det
// that rounds to 1.0f passes, 1.0000001f fails, a NaN passes.
SFM_POSE_INLINE bool coherent_det(double det) { return !(fabsf((float)det) - 1.0 > 1e-07); }

}  // namespace sfmpose
