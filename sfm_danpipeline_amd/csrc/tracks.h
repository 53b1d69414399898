// tracks.h -- the rules of the multi-view tracks as code that hipcc and g++ both compile: what makes an
// edge valid (T1), which image a node lies in, which components are kept (T4), the N-view DLT of one track (R1-R4) with the
// run-time-row-count form of jacobi.h's one-sided Jacobi, and, for the host, the whole build in plain loops (build_host:
// what tests/stub/tracks_capi.cpp calls and tracks.hip's output is compared with, byte for byte).  Compile with
// -ffp-contract=off.  PARITY UNPINNED: the reference builds no tracks.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include "hypot_glibc.h"
#include "camera.h"
#ifndef __HIPCC__
#include <vector>
#endif

namespace sfmtracks {

struct Opts {
  int32_t min_len;     // a kept track has >= max(2, min_len) nodes
  int32_t front_only;  // R4: keep also asks for a positive depth in every used view
};

struct Stats {
  int64_t nodes, edges, components, conflicting, short_tracks, n_tracks, n_obs;
};

SFM_HD inline Opts default_opts() { return Opts{2, 0}; }
SFM_HD inline int need_len(int min_len) { return min_len > 2 ? min_len : 2; }

// T1
SFM_HD inline bool pair_ok(int a, int b, int n_images) { return a >= 0 && a < n_images && b >= 0 && b < n_images && a != b; }
SFM_HD inline bool match_ok(int q, int t, int nfa, int nfb) { return q >= 0 && q < nfa && t >= 0 && t < nfb; }

// the image of a node: the last i with base[i] <= node (base: n_images + 1 entries, the exclusive scan of n_feat; an image
// without features shares its base with the next one and is never the answer)
SFM_HD inline int image_of(const int32_t* base, int n_images, int node) {
  int lo = 0, hi = n_images;  // base[lo] <= node < base[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (base[mid] <= node) lo = mid;
    else hi = mid;
  }
  return lo;
}

// R2: the right singular vector of the smallest singular value of the M x 4 system whose columns are the rows of At (row i,
// entry k at At[(i * LDA + k) * S]), by jacobi.h's one-sided Jacobi with N = 4 and a run-time M: the same operation order,
// sums over k ascending, max_iter = max(M, 30), the same descending selection sort replayed on (W, row), the last row.  W and
// Vt stay in registers (every index into them is a compile-time constant); only At lives in memory.  At M = 4 this is
// pose.h's dlt_null_vector operation for operation.
template <int S>
SFM_HD inline void null_vector(double* At, int M, int LDA, double out[4]) {
  const double eps = DBL_EPSILON * 10;
  const int max_iter = M > 30 ? M : 30;
  double W[4], Vt[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
    for (int k = 0; k < M; ++k) {
      const double t = At[(i * LDA + k) * S];
      sd += t * t;
    }
    W[i] = sd;
#pragma unroll
    for (int k = 0; k < 4; ++k) Vt[i][k] = (i == k) ? 1.0 : 0.0;
  }
#pragma unroll 1
  for (int iter = 0; iter < max_iter; ++iter) {
    bool changed = false;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = i + 1; j < 4; ++j) {
        double *Ai = At + (size_t)i * LDA * S, *Aj = At + (size_t)j * LDA * S;
        double a = W[i], p = 0, b = W[j];
        for (int k = 0; k < M; ++k) p += Ai[k * S] * Aj[k * S];
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
        for (int k = 0; k < M; ++k) {
          const double t0 = c * Ai[k * S] + s * Aj[k * S];
          const double t1 = -s * Ai[k * S] + c * Aj[k * S];
          Ai[k * S] = t0;
          Aj[k * S] = t1;
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
    if (!changed) break;  // (per lane: a lane that has converged would see no further rotation anyway)
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double sd = 0;
    for (int k = 0; k < M; ++k) {
      const double t = At[(i * LDA + k) * S];
      sd += t * t;
    }
    W[i] = sqrt(sd);
  }
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

// R1-R4 for the track whose observations are [beg, end) of the CSR.  views: 12 doubles per image; xy: pixel pairs, image
// v's feature f at xy[2 * (xy_ptr[v] + f)]; At: a work area of 4 rows of LDA >= 2 (end - beg) entries at stride S; err is
// indexed like the CSR.
template <int S>
SFM_HD inline void triangulate_track(int beg, int end, const int32_t* trk_view, const int32_t* trk_feat, const double* views,
                                     const uint8_t* has_pose, const double* K, const double* dist, const int32_t* xy_ptr,
                                     const double* xy, float max_err, int min_views, int front_only, double* At, int LDA,
                                     double X[3], float* err, int32_t* n_used, uint8_t* keep) {
  int m = 0;
  for (int j = beg; j < end; ++j) {
    const int v = trk_view[j];
    if (!has_pose[v]) continue;
    const size_t o = 2 * ((size_t)xy_ptr[v] + (size_t)trk_feat[j]);
    double x, y;
    sfmcam::undistort_point(K, dist, xy[o], xy[o + 1], x, y);
    const double* P = views + 12 * (size_t)v;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      At[((size_t)k * LDA + 2 * m) * S] = x * P[8 + k] - P[0 + k];
      At[((size_t)k * LDA + 2 * m + 1) * S] = y * P[8 + k] - P[4 + k];
    }
    ++m;
  }
  *n_used = m;
  if (m < 2) {
    X[0] = X[1] = X[2] = NAN;
    *keep = 0;
    if (err)
      for (int j = beg; j < end; ++j) err[j] = -1.0f;
    return;
  }
  double v4[4];
  null_vector<S>(At, 2 * m, LDA, v4);
  const double scale = v4[3] != 0 ? 1. / v4[3] : 1.;
  X[0] = v4[0] * scale;
  X[1] = v4[1] * scale;
  X[2] = v4[2] * scale;
  bool over = false, front = true;
  for (int j = beg; j < end; ++j) {
    const int v = trk_view[j];
    if (!has_pose[v]) {
      if (err) err[j] = -1.0f;
      continue;
    }
    const size_t o = 2 * ((size_t)xy_ptr[v] + (size_t)trk_feat[j]);
    const double* P = views + 12 * (size_t)v;
    double pu, pv;
    sfmcam::project_point(P, K, dist, X, pu, pv);
    const double dx = pu - xy[o], dy = pv - xy[o + 1];
    const float e = (float)sqrt(dx * dx + dy * dy);
    if (err) err[j] = e;
    if (max_err < e) over = true;
    const double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
    if (!(z > 0)) front = false;
  }
  *keep = (m >= need_len(min_views) && !over && (!front_only || front)) ? 1 : 0;
}

#ifndef __HIPCC__
// T1-T5 in plain loops.  false: refused (T1, a negative count or size, or more than 2^31 - 2 nodes or edges), nothing written.
inline bool build_host(int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs, const int32_t* counts,
                       const int32_t* q, const int32_t* t, Opts o, Stats& st, std::vector<int32_t>& trk_ptr,
                       std::vector<int32_t>& trk_view, std::vector<int32_t>& trk_feat, std::vector<int32_t>& node_track) {
  if (n_images < 0 || n_pairs < 0) return false;
  std::vector<int32_t> base((size_t)n_images + 1, 0);
  int64_t nn = 0, ne = 0;
  for (int i = 0; i < n_images; ++i) {
    if (n_feat[i] < 0) return false;
    nn += n_feat[i];
    if (nn > INT32_MAX - 1) return false;
    base[(size_t)i + 1] = (int32_t)nn;
  }
  for (int p = 0; p < n_pairs; ++p) {
    if (counts[p] < 0 || !pair_ok(pairs[2 * p], pairs[2 * p + 1], n_images)) return false;
    const int nfa = n_feat[pairs[2 * p]], nfb = n_feat[pairs[2 * p + 1]];
    for (int k = 0; k < counts[p]; ++k)
      if (!match_ok(q[ne + k], t[ne + k], nfa, nfb)) return false;
    ne += counts[p];
    if (ne > INT32_MAX - 1) return false;
  }
  const int n = (int)nn;
  std::vector<int32_t> parent((size_t)n);
  for (int i = 0; i < n; ++i) parent[i] = i;
  auto find = [&](int x) {
    while (parent[x] != x) {
      parent[x] = parent[parent[x]];
      x = parent[x];
    }
    return x;
  };
  int64_t e = 0;
  for (int p = 0; p < n_pairs; ++p)
    for (int k = 0; k < counts[p]; ++k, ++e) {
      const int a = find(base[pairs[2 * p]] + q[e]), b = find(base[pairs[2 * p + 1]] + t[e]);
      if (a < b) parent[b] = a;
      else parent[a] = b;
    }
  // nodes ascend by (image, feature): a component's nodes come in that order, and two of one image are neighbours (T3)
  std::vector<int32_t> len((size_t)n, 0), last_img((size_t)n, -1);
  std::vector<uint8_t> conf((size_t)n, 0);
  for (int i = 0; i < n; ++i) {
    const int r = find(i), im = image_of(base.data(), n_images, i);
    parent[i] = r;
    ++len[r];
    if (last_img[r] == im) conf[r] = 1;
    last_img[r] = im;
  }
  st = Stats{n, ne, 0, 0, 0, 0, 0};
  const int need = need_len(o.min_len);
  std::vector<int32_t> tno((size_t)n, -1);
  trk_ptr.assign(1, 0);
  for (int r = 0; r < n; ++r) {
    if (parent[r] != r || len[r] < 2) continue;
    ++st.components;
    if (conf[r]) ++st.conflicting;
    else if (len[r] < need) ++st.short_tracks;
    else {
      tno[r] = (int32_t)st.n_tracks++;
      st.n_obs += len[r];
      trk_ptr.push_back((int32_t)st.n_obs);
    }
  }
  trk_view.assign((size_t)st.n_obs, 0);
  trk_feat.assign((size_t)st.n_obs, 0);
  node_track.assign((size_t)n, -1);
  std::vector<int32_t> fill(trk_ptr.begin(), trk_ptr.end() - 1);
  for (int i = 0; i < n; ++i) {
    const int tr = tno[parent[i]];
    if (tr < 0) continue;
    const int im = image_of(base.data(), n_images, i);
    trk_view[fill[tr]] = im;
    trk_feat[fill[tr]] = i - base[im];
    ++fill[tr];
    node_track[i] = tr;
  }
  return true;
}

// R1-R4 over every track of a CSR, one after the other
inline void triangulate_host(int n_tracks, const int32_t* trk_ptr, const int32_t* trk_view, const int32_t* trk_feat, const double* views,
                             const uint8_t* has_pose, const double* K, const double* dist, const int32_t* xy_ptr, const double* xy,
                             float max_err, int min_views, int front_only, double* X, float* err, int32_t* n_used, uint8_t* keep) {
  std::vector<double> At;
  for (int tr = 0; tr < n_tracks; ++tr) {
    const int beg = trk_ptr[tr], end = trk_ptr[tr + 1], lda = 2 * (end - beg);
    At.assign((size_t)4 * lda + 1, 0.0);
    triangulate_track<1>(beg, end, trk_view, trk_feat, views, has_pose, K, dist, xy_ptr, xy, max_err, min_views, front_only, At.data(),
                         lda, X + 3 * (size_t)tr, err, n_used + tr, keep + tr);
  }
}
#endif

}  // namespace sfmtracks
