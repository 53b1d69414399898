// score_host.h -- the host half of cv::findHomography's RANSAC (OpenCV 3.4.1 calib3d/fundam.cpp) that score.hip's
// sfmhip_score_homography needs beside ransac_host.h: HomographyEstimatorCallback::checkSubset and the per-pair sample
// stream that draws again when it rejects a sample.  Host code only (the CPU test stub compiles it too).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>
#include "ransac_host.h"

namespace sfmransac {

inline bool have_collinear(const float (*p)[2], int count) {
  const int i = count - 1;
  for (int j = 0; j < i; ++j) {
    const double dx1 = p[j][0] - p[i][0], dy1 = p[j][1] - p[i][1];
    for (int k = 0; k < j; ++k) {
      const double dx2 = p[k][0] - p[i][0], dy2 = p[k][1] - p[i][1];
      if (std::fabs(dx2 * dy1 - dy2 * dx1) <= FLT_EPSILON * (std::fabs(dx1) + std::fabs(dy1) + std::fabs(dx2) + std::fabs(dy2))) return true;
    }
  }
  return false;
}
inline double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
inline bool homography_check_subset(const float (*s1)[2], const float (*s2)[2]) {
  if (have_collinear(s1, 4) || have_collinear(s2, 4)) return false;
  static const int tt[4][3] = {{0, 1, 2}, {1, 2, 3}, {0, 2, 3}, {0, 1, 3}};
  int negative = 0;
  for (int i = 0; i < 4; ++i) {
    const int* t = tt[i];
    const double A[9] = {s1[t[0]][0], s1[t[0]][1], 1., s1[t[1]][0], s1[t[1]][1], 1., s1[t[2]][0], s1[t[2]][1], 1.};
    const double B[9] = {s2[t[0]][0], s2[t[0]][1], 1., s2[t[1]][0], s2[t[1]][1], 1., s2[t[2]][0], s2[t[2]][1], 1.};
    negative += det3(A) * det3(B) < 0;
  }
  return negative == 0 || negative == 4;
}
struct HSampleStream {  // per pair: the accepted 4-point samples in order (-1: getSubset gave up after 10000 attempts)
  CvRng rng;
  std::vector<int> idx;
  bool dead = false;
  void extend(const float* m1, const float* m2, int count, int n_iters) {
    while ((int)idx.size() < 4 * n_iters) {
      int s[4] = {-1, -1, -1, -1};
      bool found = false;
      for (int attempt = 0; attempt < 10000 && !dead; ++attempt) {
        for (int i = 0; i < 4;) {
          const int v = rng.uniform(0, count);
          int j = 0;
          for (; j < i; ++j)
            if (s[j] == v) break;
          if (j < i) continue;
          s[i++] = v;
        }
        float a[4][2], b[4][2];
        for (int k = 0; k < 4; ++k) {
          a[k][0] = m1[2 * s[k]]; a[k][1] = m1[2 * s[k] + 1];
          b[k][0] = m2[2 * s[k]]; b[k][1] = m2[2 * s[k] + 1];
        }
        if (homography_check_subset(a, b)) {
          found = true;
          break;
        }
      }
      if (!found) {
        dead = true;
        s[0] = s[1] = s[2] = s[3] = -1;
      }
      idx.insert(idx.end(), s, s + 4);
    }
  }
};
// the sampler of the homography RANSAC: one stream per pair, over the pair's float points (all pairs' points; offsets)
struct PairSamples {
  const float *p1, *p2;
  const int32_t* offsets;
  std::vector<HSampleStream> streams;
  const int* rows(int view, int count, int first, int n) {
    HSampleStream& ss = streams[view];
    ss.extend(p1 + 2 * (size_t)offsets[view], p2 + 2 * (size_t)offsets[view], count, first + n);
    return ss.idx.data() + 4 * (size_t)first;
  }
};

}  // namespace sfmransac
