// verify.h -- the rules of the two-view verification of match lists as code that hipcc and g++ both
// compile: where a pair's list starts and where a feature's pixel lies (V1), findEssentialMat's normalisation (V1), the one
// inlier test of the essential-matrix RANSAC (V3: score.hip counts with it, verify.hip compacts with it), which pairs are
// kept (V4), and, for the host, the refusals (V6) and the stable compaction in plain loops (V5: what
// tests/stub/verify_capi.cpp calls and verify.hip's output is compared with, byte for byte).  Compile with -ffp-contract=off.
// PARITY UNPINNED, as for the score entries: the reference never filters its lists.
#pragma once
#include <cstddef>
#include <cstdint>
#include "tracks.h"  // (SFM_HD; pair_ok, match_ok)
#ifndef __HIPCC__
#include <vector>
#endif

namespace sfmverify {

struct Opts {
  double prob;          // findEssentialMat's confidence
  double threshold;     // ... and its threshold, in pixels
  int32_t min_inliers;  // V4: a pair with fewer RANSAC inliers keeps no match
  int32_t reserved;
};

struct Stats {
  int64_t pairs, pairs_kept, pairs_no_model, matches_in, matches_out;
};

SFM_HD inline Opts default_opts() { return Opts{0.999, 1.0, 15, 0}; }

// ---------------------------------------------------------------- V1
// the first match of pair p: a match plan keeps `stride` slots per pair, host lists are packed (off: their exclusive scan)
SFM_HD inline long long list_start(const int32_t* off, int stride, int p) { return stride > 0 ? (long long)p * stride : (long long)off[p]; }
// image v's feature f: its x at xy[pixel_index], its y one after
SFM_HD inline size_t pixel_index(const int32_t* xy_ptr, int v, int f) { return 2 * ((size_t)xy_ptr[v] + (size_t)f); }

// findEssentialMat's (col - c) / f, evaluated as col * (1 / f) + (-c * (1 / f)): the products and sums of score_normalize
struct Norm {
  double ax, bx, ay, by;
};
SFM_HD inline Norm norm_of(const double* K9) {
  Norm n;
  n.ax = 1. / K9[0];
  n.bx = -K9[2] * n.ax;
  n.ay = 1. / K9[4];
  n.by = -K9[5] * n.ay;
  return n;
}
SFM_HD inline double norm_x(const Norm& n, double x) { return x * n.ax + n.bx; }
SFM_HD inline double norm_y(const Norm& n, double y) { return y * n.ay + n.by; }
// the RANSAC's threshold on the squared Sampson-like error of is_inlier: (threshold / ((fx + fy) / 2))^2 as a float
SFM_HD inline float error_bound(double fx, double fy, double threshold) {
  const double thr = threshold / ((fx + fy) / 2);
  return (float)(thr * thr);
}

// a pair and a match the lists may name: T1 of the tracks that read the result
using sfmtracks::match_ok;
using sfmtracks::pair_ok;

// ---------------------------------------------------------------- V3
// EMEstimatorCallback::computeError + findInliers for one correspondence (normalised points, E row-major)
SFM_HD inline __attribute__((always_inline)) bool is_inlier(const double* E, double x1, double y1, double x2, double y2, float t) {
  const double ex0 = E[0] * x1 + E[1] * y1 + E[2] * 1.0;
  const double ex1 = E[3] * x1 + E[4] * y1 + E[5] * 1.0;
  const double ex2 = E[6] * x1 + E[7] * y1 + E[8] * 1.0;
  const double et0 = E[0] * x2 + E[3] * y2 + E[6] * 1.0;
  const double et1 = E[1] * x2 + E[4] * y2 + E[7] * 1.0;
  const double x2tEx1 = x2 * ex0 + y2 * ex1 + 1.0 * ex2;
  const double a = ex0 * ex0, b = ex1 * ex1, c = et0 * et0, d = et1 * et1;
  const float err = (float)(x2tEx1 * x2tEx1 / (a + b + c + d));
  return err <= t;
}
// the mask byte of one match from its pair's code (0: no model, 1: a RANSAC model, 2: exactly five matches, all inliers)
SFM_HD inline bool mask_of(int has, bool inlier) { return has == 2 ? true : has == 1 ? inlier : false; }

// ---------------------------------------------------------------- V4
SFM_HD inline bool pair_kept(int has, int inliers, int min_inliers) { return has != 0 && inliers >= min_inliers; }
// what the compaction reads per pair: the code of a kept pair, 0 for every other
SFM_HD inline uint8_t pair_code(int has, int inliers, int min_inliers) { return pair_kept(has, inliers, min_inliers) ? (uint8_t)has : (uint8_t)0; }

// ---------------------------------------------------------------- V6, the part that needs no lists
// K and xy_ptr present, prob inside (0, 1), no negative n_feat, xy_ptr starting at >= 0 and never decreasing, every image
// with a pixel for each of its features
SFM_HD inline bool args_ok(int n_images, const int32_t* n_feat, const int32_t* xy_ptr, const double* K9, const Opts& o) {
  if (n_images < 0 || !K9 || !xy_ptr || (n_images && !n_feat)) return false;
  if (!(o.prob > 0 && o.prob < 1)) return false;
  if (xy_ptr[0] < 0) return false;
  for (int v = 0; v < n_images; ++v) {
    if (n_feat[v] < 0 || xy_ptr[v + 1] < xy_ptr[v]) return false;
    if (xy_ptr[v + 1] - xy_ptr[v] < n_feat[v]) return false;
  }
  return true;
}

#ifndef __HIPCC__
// V6 over host lists (packed): false = refused
inline bool lists_ok(int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs, const int32_t* counts, const int32_t* q,
                     const int32_t* t, const double* xy) {
  if (n_pairs < 0 || (n_pairs && (!pairs || !counts))) return false;
  int64_t ne = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (counts[p] < 0 || !pair_ok(pairs[2 * p], pairs[2 * p + 1], n_images)) return false;
    if (counts[p] && (!q || !t || !xy)) return false;
    const int nfa = n_feat[pairs[2 * p]], nfb = n_feat[pairs[2 * p + 1]];
    for (int k = 0; k < counts[p]; ++k)
      if (!match_ok(q[ne + k], t[ne + k], nfa, nfb)) return false;
    ne += counts[p];
    if (ne > INT32_MAX - 1) return false;
  }
  return true;
}

// V4 + V5 in plain loops over packed lists: survives(p, k) is the mask of pair p's match k (asked for kept pairs only).
// out_q / out_t: packed, room for every input match.
template <class Survives>
inline void compact_host(int n_pairs, const int32_t* counts, const int32_t* q, const int32_t* t, const uint8_t* has,
                         const int32_t* inliers, int min_inliers, Survives survives, int32_t* out_counts, int32_t* out_q,
                         int32_t* out_t, uint8_t* kept, Stats& st) {
  st = Stats{n_pairs, 0, 0, 0, 0};
  int64_t in = 0, out = 0;
  for (int p = 0; p < n_pairs; ++p) {
    const bool k = pair_kept(has[p], inliers[p], min_inliers);
    int c = 0;
    if (k)
      for (int i = 0; i < counts[p]; ++i)
        if (survives(p, i)) {
          out_q[out + c] = q[in + i];
          out_t[out + c] = t[in + i];
          ++c;
        }
    out_counts[p] = c;
    kept[p] = k ? 1 : 0;
    st.pairs_kept += k ? 1 : 0;
    st.pairs_no_model += has[p] == 0 ? 1 : 0;
    in += counts[p];
    out += c;
  }
  st.matches_in = in;
  st.matches_out = out;
}

// V1 + V3 + V4 + V5 from each pair's best E: the points gathered and normalised per match, the mask by is_inlier
inline void verify_host(int n_pairs, const int32_t* pairs, const int32_t* counts, const int32_t* q, const int32_t* t,
                        const int32_t* xy_ptr, const double* xy, const double* K9, double threshold, const double* E,
                        const uint8_t* has, const int32_t* inliers, int min_inliers, int32_t* out_counts, int32_t* out_q,
                        int32_t* out_t, uint8_t* kept, Stats& st) {
  const Norm n = norm_of(K9);
  const float bound = error_bound(K9[0], K9[4], threshold);
  std::vector<int64_t> off((size_t)n_pairs + 1, 0);
  for (int p = 0; p < n_pairs; ++p) off[(size_t)p + 1] = off[p] + counts[p];
  auto survives = [&](int p, int i) {
    const size_t l = pixel_index(xy_ptr, pairs[2 * p], q[off[p] + i]), r = pixel_index(xy_ptr, pairs[2 * p + 1], t[off[p] + i]);
    const bool inl = has[p] == 1 && is_inlier(E + 9 * (size_t)p, norm_x(n, xy[l]), norm_y(n, xy[l + 1]), norm_x(n, xy[r]), norm_y(n, xy[r + 1]), bound);
    return mask_of(has[p], inl);
  };
  compact_host(n_pairs, counts, q, t, has, inliers, min_inliers, survives, out_counts, out_q, out_t, kept, st);
}
#endif

}  // namespace sfmverify
