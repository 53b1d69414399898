// jacobi.h -- OpenCV 3.4.1's general one-sided Jacobi SVD (core/lapack.cpp JacobiSVDImpl_<double>) as __host__ __device__
// code: the five-point solver of score.hip runs it on 9 x 5 / 4 x 3 systems, EPnP (pnp.h) on its 12 x 12 and 6 x k ones, and
// the CPU test stubs compile the same body.  (The fixed 3 x 3 and 4 x 4 forms that live in registers are in pose.h.)
// Compile with -ffp-contract=off.
#pragma once
#include <cfloat>
#include <cmath>
#include "hypot_glibc.h"

namespace sfmjacobi {

// ---- cv::RNG (multiply with carry), as JacobiSVDImpl_ seeds it
struct DevRng {
  unsigned long long state;
  SFM_HD unsigned next() {
    state = (unsigned long long)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
  }
};

// ---- core/lapack.cpp JacobiSVDImpl_<double>: one-sided Jacobi on the N rows (length M, stride LDA) of At; rows N..N1-1
// (and rows whose singular value is <= DBL_MIN) filled from RNG(0x12345678) sign vectors, orthogonalised twice against
// the rows before them.  Vt (N x N) accumulates the rotations.  Operation for operation the restatement in
// the CPU restatement used as checker (test infrastructure), which cites the library.
// S: the distance in doubles between consecutive elements of At, W and Vt (1: dense; 64: the work area of one lane
// interleaved with those of the other lanes of its wave, so that a wave's accesses coalesce).
template <int M, int N, int N1, int LDA, int S = 1>
SFM_HD inline void jacobi_svd(double* At, double* W, double* Vt) {
  const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
  const int max_iter = M > 30 ? M : 30;
  for (int i = 0; i < N; ++i) {
    double sd = 0;
    for (int k = 0; k < M; ++k) {
      const double t = At[(i * LDA + k) * S];
      sd += t * t;
    }
    W[i * S] = sd;
    for (int k = 0; k < N; ++k) Vt[(i * N + k) * S] = 0;
    Vt[(i * N + i) * S] = 1;
  }
  for (int iter = 0; iter < max_iter; ++iter) {
    bool changed = false;
    for (int i = 0; i < N - 1; ++i)
      for (int j = i + 1; j < N; ++j) {
        double *Ai = At + i * LDA * S, *Aj = At + j * LDA * S;
        double a = W[i * S], p = 0, b = W[j * S];
        for (int k = 0; k < M; ++k) p += Ai[k * S] * Aj[k * S];
        if (fabs(p) <= eps * sqrt(a * b)) continue;
        p *= 2;
        const double beta = a - b, gamma = sfm_hypot(p, beta);  // (the host libm's hypot, bit for bit: hypot_glibc.h)
        double c, sn;
        if (beta < 0) {
          const double delta = (gamma - beta) * 0.5;
          sn = sqrt(delta / gamma);
          c = p / (gamma * sn * 2);
        } else {
          c = sqrt((gamma + beta) / (gamma * 2));
          sn = p / (gamma * c * 2);
        }
        a = b = 0;
        for (int k = 0; k < M; ++k) {
          const double t0 = c * Ai[k * S] + sn * Aj[k * S];
          const double t1 = -sn * Ai[k * S] + c * Aj[k * S];
          Ai[k * S] = t0;
          Aj[k * S] = t1;
          a += t0 * t0;
          b += t1 * t1;
        }
        W[i * S] = a;
        W[j * S] = b;
        changed = true;
        double *Vi = Vt + i * N * S, *Vj = Vt + j * N * S;
        for (int k = 0; k < N; ++k) {
          const double t0 = c * Vi[k * S] + sn * Vj[k * S];
          const double t1 = -sn * Vi[k * S] + c * Vj[k * S];
          Vi[k * S] = t0;
          Vj[k * S] = t1;
        }
      }
    if (!changed) break;
  }
  for (int i = 0; i < N; ++i) {
    double sd = 0;
    for (int k = 0; k < M; ++k) {
      const double t = At[(i * LDA + k) * S];
      sd += t * t;
    }
    W[i * S] = sqrt(sd);
  }
  for (int i = 0; i < N - 1; ++i) {
    int j = i;
    for (int k = i + 1; k < N; ++k)
      if (W[j * S] < W[k * S]) j = k;
    if (i != j) {
      double t = W[i * S];
      W[i * S] = W[j * S];
      W[j * S] = t;
      for (int k = 0; k < M; ++k) {
        t = At[(i * LDA + k) * S];
        At[(i * LDA + k) * S] = At[(j * LDA + k) * S];
        At[(j * LDA + k) * S] = t;
      }
      for (int k = 0; k < N; ++k) {
        t = Vt[(i * N + k) * S];
        Vt[(i * N + k) * S] = Vt[(j * N + k) * S];
        Vt[(j * N + k) * S] = t;
      }
    }
  }
  DevRng rng{0x12345678ull};
  for (int i = 0; i < N1; ++i) {
    double sd = i < N ? W[i * S] : 0;
    for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
      const double val0 = 1. / M;
      for (int k = 0; k < M; ++k) At[(i * LDA + k) * S] = (rng.next() & 256) != 0 ? val0 : -val0;
      for (int it2 = 0; it2 < 2; ++it2)
        for (int j = 0; j < i; ++j) {
          sd = 0;
          for (int k = 0; k < M; ++k) sd += At[(i * LDA + k) * S] * At[(j * LDA + k) * S];
          double asum = 0;
          for (int k = 0; k < M; ++k) {
            const double t = At[(i * LDA + k) * S] - sd * At[(j * LDA + k) * S];
            At[(i * LDA + k) * S] = t;
            asum += fabs(t);
          }
          asum = asum > eps * 100 ? 1 / asum : 0;
          for (int k = 0; k < M; ++k) At[(i * LDA + k) * S] *= asum;
        }
      sd = 0;
      for (int k = 0; k < M; ++k) {
        const double t = At[(i * LDA + k) * S];
        sd += t * t;
      }
      sd = sqrt(sd);
    }
    const double sc = sd > minval ? 1 / sd : 0.;
    for (int k = 0; k < M; ++k) At[(i * LDA + k) * S] *= sc;
  }
}

}  // namespace sfmjacobi
