// ransac_host.h -- the host half of OpenCV 3.4.1's RANSACPointSetRegistrator (calib3d/ptsetreg.cpp) that the essential-matrix,
// homography and PnP RANSACs share: cv::RNG as run() seeds it, getSubset's distinct-index draw of five indices, and
// RANSACUpdateNumIters.  Host code only (the CPU test stubs compile it too).
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <vector>

namespace sfmransac {

struct CvRng {
  unsigned long long state = 0xFFFFFFFFFFFFFFFFull;  // RNG rng((uint64)-1)
  unsigned next() {
    state = (unsigned long long)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
  }
  int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};
struct SampleStream {  // the samples of one match count, generated on demand
  CvRng rng;
  std::vector<int> idx;  // 5 per iteration
  void extend(int count, int n_iters) {
    while ((int)idx.size() < 5 * n_iters) {
      int s[5];
      for (int i = 0; i < 5;) {
        const int v = rng.uniform(0, count);
        int j = 0;
        for (; j < i; ++j)
          if (s[j] == v) break;
        if (j < i) continue;  // drawn before: again
        s[i++] = v;
      }
      idx.insert(idx.end(), s, s + 5);
    }
  }
};
// cv::RANSACUpdateNumIters (calib3d/ptsetreg.cpp), with the host libm as the reference runs it
inline int ransac_update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = std::max(p, 0.0);
  p = std::min(p, 1.0);
  ep = std::max(ep, 0.0);
  ep = std::min(ep, 1.0);
  double num = std::max(1.0 - p, DBL_MIN);
  double denom = 1.0 - std::pow(1.0 - ep, model_points);
  if (denom < DBL_MIN) return 0;
  num = std::log(num);
  denom = std::log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::nearbyint(num / denom);  // cvRound
}

}  // namespace sfmransac
