// register.h -- the rules of the cloud registration (nearest points of one cloud in another, rigid and
// similarity ICP) as code that hipcc and a plain g++ both compile: moving a point, the pair test, the terms of the two
// fixed-order sums, the Umeyama / Horn estimate over pose.h's svd3 and the loop's stop decision.  The device code
// (register.hip) and the CPU test stub (tests/stub/register_capi.cpp) share these bodies, so the device result is checked
// bit for bit against a CPU build.  Compile with -ffp-contract=off.  Below the shared part: the host's search (a plain
// uniform grid of its own: a pair is the least (d2, index), which no search structure changes) and the fixed-order sum.  The
// host form of the whole call (run_host, run_host_batch) is an adapter of register_icp.h's one loop, included at the end.
// PARITY UNPINNED: PCL is not in the image; what is marked + in DESIGN.md f-17 is a reading of PCL 1.8.1 from memory.
#pragma once
#include <cstdint>
#include <cstring>
#include "block_sum.h"
#include "cloud.h"
#include "pose.h"

#ifdef __HIPCC__
#define SFM_REG_INLINE __host__ __device__ __forceinline__
#else
#define SFM_REG_INLINE inline __attribute__((always_inline))
#endif

namespace sfmreg {

// the C ABI's structs (include/sfmhip.h), field for field
struct Transform {
  double R[9], t[3], scale;  // x -> scale R x + t, R row-major
};
struct Opts {
  int32_t max_iters, with_scale, min_pairs, reserved;
  double max_dist, eps;
};
struct Result {
  Transform T;
  int32_t iterations, pairs, converged, flags;
  double mse;
};
enum { F_FEW = 1, F_DEGENERATE = 2 };
enum { CONV_LIMIT = 0, CONV_FIXED = 1, CONV_EPS = 2 };
constexpr int N1 = 7;   // pass 1: N, sum p (3), sum m (3)
constexpr int N2 = 11;  // pass 2: H (9, row-major), sigma, sum d2

SFM_REG_INLINE bool fin(double x) { return x - x == 0.0; }
SFM_REG_INLINE double inf_d() {
  const uint64_t u = 0x7FF0000000000000ull;
  double d;
  memcpy(&d, &u, 8);
  return d;
}
SFM_REG_INLINE double qnan_d() {  // (0 / 0 has the sign bit set on x86 and clear on the device: one NaN for both)
  const uint64_t u = 0x7FF8000000000000ull;
  double d;
  memcpy(&d, &u, 8);
  return d;
}

SFM_REG_INLINE Opts default_opts() {
  Opts o;
  o.max_iters = 50, o.with_scale = 0, o.min_pairs = 3, o.reserved = 0;
  o.max_dist = inf_d(), o.eps = 0.0;
  return o;
}
SFM_REG_INLINE Transform identity() {
  Transform T;
  for (int i = 0; i < 9; ++i) T.R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  T.t[0] = T.t[1] = T.t[2] = 0.0;
  T.scale = 1.0;
  return T;
}
// rule 1
SFM_REG_INLINE bool valid_transform(const Transform& T) {
  bool ok = fin(T.scale) && T.scale > 0.0;
  for (int i = 0; i < 9; ++i) ok = ok && fin(T.R[i]);
  for (int i = 0; i < 3; ++i) ok = ok && fin(T.t[i]);
  return ok;
}
SFM_REG_INLINE bool valid_max_dist(double md) { return md > 0.0; }  // (NaN fails; +inf passes)
SFM_REG_INLINE bool valid_opts(const Opts& o) {
  return valid_max_dist(o.max_dist) && o.eps >= 0.0 && o.max_iters >= 0 && o.min_pairs >= 3;
}
// f-18's batch of starts: rule 1 for every one of them, 1 .. MAX_BATCH starts (host)
constexpr int MAX_BATCH = 1024;
inline bool valid_batch(const Opts& o, const Transform* inits, int n_init) {
  if (!valid_opts(o) || !inits || n_init < 1 || n_init > MAX_BATCH) return false;
  for (int b = 0; b < n_init; ++b)
    if (!valid_transform(inits[b])) return false;
  return true;
}

// rule 2: q = (float)(scale ((R x + R y) + R z) + t) in f64; false when the point has no image
SFM_REG_INLINE bool move(const Transform& T, float x, float y, float z, float q[3]) {
  const double xd = (double)x, yd = (double)y, zd = (double)z;
  for (int r = 0; r < 3; ++r) q[r] = (float)(T.scale * ((T.R[3 * r] * xd + T.R[3 * r + 1] * yd) + T.R[3 * r + 2] * zd) + T.t[r]);
  return sfmcloud::finite3(x, y, z) && sfmcloud::finite3(q[0], q[1], q[2]);
}
// rule 3: the pair test's bound, squared in f64
SFM_REG_INLINE float max_d2(double max_dist) { return (float)(max_dist * max_dist); }
SFM_REG_INLINE bool keep(float d2, float md2) { return d2 <= md2; }

// rule 4: a point's terms of the two sums (idx < 0: +0.0 in every slot); p the source float, m the matched target float
SFM_REG_INLINE void terms1(bool paired, const float p[3], const float m[3], double v[N1]) {
  v[0] = paired ? 1.0 : 0.0;
  for (int a = 0; a < 3; ++a) v[1 + a] = paired ? (double)p[a] : 0.0, v[4 + a] = paired ? (double)m[a] : 0.0;
}
SFM_REG_INLINE void terms2(bool paired, const float p[3], const float m[3], float d2, const double mu_p[3], const double mu_m[3], double v[N2]) {
  for (int k = 0; k < N2; ++k) v[k] = 0.0;
  if (!paired) return;
  double dp[3], dm[3];
  for (int a = 0; a < 3; ++a) dp[a] = (double)p[a] - mu_p[a], dm[a] = (double)m[a] - mu_m[a];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) v[3 * r + c] = dm[r] * dp[c];
  v[9] = (dp[0] * dp[0] + dp[1] * dp[1]) + dp[2] * dp[2];
  v[10] = (double)d2;
}
// mu_p, mu_m of pass 1's sums (not read when N is 0)
SFM_REG_INLINE void means(const double s1[N1], double mu_p[3], double mu_m[3]) {
  for (int a = 0; a < 3; ++a) mu_p[a] = s1[1 + a] / s1[0], mu_m[a] = s1[4 + a] / s1[0];
}
SFM_REG_INLINE double mse_of(const double s1[N1], const double s2[N2]) { return s1[0] > 0.0 ? s2[10] / s1[0] : qnan_d(); }

// rule 5: the next transform from the sums; returns 0 or F_DEGENERATE (then `next` is not to be used)
SFM_REG_INLINE int estimate(const double s1[N1], const double s2[N2], int with_scale, const Transform& cur, Transform& next) {
  double U[9], W[3], Vt[9], mu_p[3], mu_m[3];
  means(s1, mu_p, mu_m);
  const int svd_flags = sfmpose::svd3(s2, U, W, Vt);
  const double d = sfmpose::det3(U) * sfmpose::det3(Vt) >= 0.0 ? 1.0 : -1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) next.R[3 * r + c] = (U[3 * r] * Vt[c] + U[3 * r + 1] * Vt[3 + c]) + (d * U[3 * r + 2]) * Vt[6 + c];
  const double sigma = s2[9];
  next.scale = with_scale ? ((W[0] + W[1]) + d * W[2]) / sigma : cur.scale;
  for (int r = 0; r < 3; ++r)
    next.t[r] = mu_m[r] - next.scale * ((next.R[3 * r] * mu_p[0] + next.R[3 * r + 1] * mu_p[1]) + next.R[3 * r + 2] * mu_p[2]);
  const bool bad = svd_flags != 0 || sigma == 0.0 || W[1] <= 1e-12 * W[0] || !(fin(next.scale) && next.scale > 0.0) || !valid_transform(next);
  return bad ? F_DEGENERATE : 0;
}

// rule 6's eps test: no entry of scale R and t moved by more than eps
SFM_REG_INLINE bool within_eps(const Transform& a, const Transform& b, double eps) {
  bool ok = true;
  for (int i = 0; i < 9; ++i) ok = ok && !(fabs(a.scale * a.R[i] - b.scale * b.R[i]) > eps);
  for (int i = 0; i < 3; ++i) ok = ok && !(fabs(a.t[i] - b.t[i]) > eps);
  return ok;
}

// rule 6, step k: the state the loop carries, and the decision once C_k's sums are known.  `changed`: C_k differs from
// C_{k-1} (not read at k = 0).  Returns true when the loop stops; res is complete then.  Else T becomes T_{k+1}.
struct Loop {
  Transform T, prev;
  int32_t k, stop;
  Result res;
};
SFM_REG_INLINE void loop_init(Loop& L, const Transform& init) {
  L.T = init, L.prev = init;
  L.k = 0, L.stop = 0;
  memset(&L.res, 0, sizeof L.res);
}
SFM_REG_INLINE bool loop_step(Loop& L, const Opts& o, bool changed, const double s1[N1], const double s2[N2]) {
  Result& r = L.res;
  r.T = L.T;
  r.iterations = L.k;
  r.pairs = (int32_t)s1[0];
  r.mse = mse_of(s1, s2);
  r.converged = CONV_LIMIT;
  r.flags = 0;
  bool stop = true;
  Transform next = L.T;
  if (r.pairs < o.min_pairs) r.flags = F_FEW;
  else if (L.k > 0 && !changed) r.converged = CONV_FIXED;
  else if (L.k > 0 && o.eps > 0.0 && within_eps(L.T, L.prev, o.eps)) r.converged = CONV_EPS;
  else if (L.k == o.max_iters) r.converged = CONV_LIMIT;
  else {
    r.flags = estimate(s1, s2, o.with_scale, L.T, next);
    stop = r.flags != 0;
  }
  if (!stop) {
    L.prev = L.T;
    L.T = next;
    L.k += 1;
  }
  L.stop = stop ? 1 : 0;
  return stop;
}

}  // namespace sfmreg

#ifndef __HIPCC__
// ---- the whole call on the host: what the device is checked against
#include <algorithm>
#include <cmath>
#include <vector>

namespace sfmreg {

// a uniform grid over the finite target points: about 8 per cell.  nearest() returns the least (d2, index) whatever the
// cells are: a ring is left only when every point outside it is farther (by the plain distance to the ring's box, less a
// slack far above the rounding of a float d2) than what is held, or than the bound the caller gives
struct HostGrid {
  int n = 0, nv = 0, D[3] = {1, 1, 1};
  const float* xyz = nullptr;
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // the box of the nv finite points (f-22 rule 8 takes its centre from here)
  double o[3] = {0, 0, 0}, cell = 1;
  std::vector<int> start, order;
  void build(int n_, const float* xyz_) {
    n = n_, xyz = xyz_, nv = 0;
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = 0;
    for (int i = 0; i < n; ++i) {
      if (!sfmcloud::finite3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
      for (int a = 0; a < 3; ++a) {
        const double v = xyz[3 * i + a];
        lo[a] = nv ? std::min(lo[a], v) : v, hi[a] = nv ? std::max(hi[a], v) : v;
      }
      ++nv;
    }
    double ext = 0;
    for (int a = 0; a < 3; ++a) ext = std::max(ext, hi[a] - lo[a]), o[a] = lo[a];
    cell = ext > 0 ? ext / std::max(1.0, std::min(256.0, std::cbrt((double)nv / 2.0))) : 1.0;
    for (int a = 0; a < 3; ++a) D[a] = (int)std::floor((hi[a] - lo[a]) / cell) + 1;
    const size_t nc = (size_t)D[0] * D[1] * D[2];
    start.assign(nc + 1, 0);
    order.resize(nv);
    std::vector<int> key(n, -1);
    for (int i = 0; i < n; ++i) {
      if (!sfmcloud::finite3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2])) continue;
      int c[3];
      cells(&xyz[3 * i], c);
      key[i] = (c[2] * D[1] + c[1]) * D[0] + c[0];
      ++start[key[i] + 1];
    }
    for (size_t c = 0; c < nc; ++c) start[c + 1] += start[c];
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i)
      if (key[i] >= 0) order[fill[key[i]]++] = i;
  }
  void cells(const float* q, int c[3]) const {
    for (int a = 0; a < 3; ++a) {
      double f = std::floor(((double)q[a] - o[a]) / cell);
      f = f < 0 ? 0 : f > D[a] - 1 ? D[a] - 1 : f;
      c[a] = (int)f;
    }
  }
  // the pair of q: idx (-1: none) and d2 (+inf: none).  exact: search until the nearest is known also beyond md2
  void nearest(const float q[3], float md2, bool exact, int& idx, float& d2) const {
    float bd = sfmcloud::bits_f(0x7F800000u);
    int bi = INT_MAX;
    if (nv > 0) {
      int c[3];
      cells(q, c);
      const int Rmax = std::max(D[0], std::max(D[1], D[2]));
      auto scan = [&](int z, int y, int xa, int xb) {
        for (int x = xa; x <= xb; ++x) {
          const size_t cl = ((size_t)z * D[1] + y) * D[0] + x;
          for (int s = start[cl]; s < start[cl + 1]; ++s) {
            const int j = order[s];
            const float dd = sfmcloud::dist2(q[0], q[1], q[2], xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
            if (sfmcloud::knn_less(dd, j, bd, bi)) bd = dd, bi = j;
          }
        }
      };
      for (int R = 0; R <= Rmax; ++R) {
        for (int z = std::max(c[2] - R, 0); z <= std::min(c[2] + R, D[2] - 1); ++z)
          for (int y = std::max(c[1] - R, 0); y <= std::min(c[1] + R, D[1] - 1); ++y) {
            if (std::abs(z - c[2]) == R || std::abs(y - c[1]) == R) {
              scan(z, y, std::max(c[0] - R, 0), std::min(c[0] + R, D[0] - 1));
            } else {  // (the inside of the ring was searched: its two x faces)
              if (c[0] - R >= 0) scan(z, y, c[0] - R, c[0] - R);
              if (c[0] + R <= D[0] - 1) scan(z, y, c[0] + R, c[0] + R);
            }
          }
        // the least distance from q to a point outside the ring's cells
        double b = inf_d();
        for (int a = 0; a < 3; ++a) {
          if (c[a] - R > 0) b = std::min(b, std::max(0.0, (double)q[a] - (o[a] + (double)(c[a] - R) * cell)));
          if (c[a] + R < D[a] - 1) b = std::min(b, std::max(0.0, (o[a] + (double)(c[a] + R + 1) * cell) - (double)q[a]));
        }
        if (b == inf_d()) break;
        const double bs = b * (1.0 - 1.0 / 1024.0) - 1e-9 * (cell + std::fabs((double)q[0]) + std::fabs((double)q[1]) + std::fabs((double)q[2]));
        if (bs > 0.0) {
          if (bi != INT_MAX && bs * bs > (double)bd) break;
          if (!exact && bs * bs > (double)md2) break;
        }
      }
    }
    const bool got = bi != INT_MAX;
    d2 = got ? bd : sfmcloud::bits_f(0x7F800000u);
    idx = got && keep(bd, md2) ? bi : -1;
  }
};

// rules 2 + 3 for every source point under T (the search exact: a rejected pair keeps its d2)
inline void nearest_host(const HostGrid& g, int n_src, const float* src, const Transform& T, float md2, bool exact, int32_t* idx, float* d2) {
  for (int i = 0; i < n_src; ++i) {
    float q[3];
    int bi = -1;
    float bd = sfmcloud::bits_f(0x7F800000u);
    if (move(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], q)) g.nearest(q, md2, exact, bi, bd);
    idx[i] = bi, d2[i] = bd;
  }
}

// rule 4's fixed-order sum of Q slots: blocks of 256 source indices by block_sum.h's tree, the partials in ascending order
template <int Q, class Terms>
inline void sum_host(int n_src, Terms terms, double out[Q]) {
  for (int k = 0; k < Q; ++k) out[k] = 0.0;
  std::vector<double> v((size_t)Q * sfmsum::CHUNK);
  for (int i0 = 0; i0 < n_src; i0 += sfmsum::CHUNK) {
    for (int t = 0; t < sfmsum::CHUNK; ++t) {
      double w[Q];
      for (int k = 0; k < Q; ++k) w[k] = 0.0;
      if (i0 + t < n_src) terms(i0 + t, w);
      for (int k = 0; k < Q; ++k) v[(size_t)k * sfmsum::CHUNK + t] = w[k];
    }
    for (int k = 0; k < Q; ++k) out[k] = out[k] + sfmsum::chunk_tree(&v[(size_t)k * sfmsum::CHUNK]);
  }
}

// rule 8 on the host: the image of every point (a non-finite point stays)
inline void transform_host(int n, const float* xyz, const Transform& T, float* out) {
  for (int i = 0; i < n; ++i) {
    float q[3];
    move(T, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], q);
    const bool f = sfmcloud::finite3(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    for (int a = 0; a < 3; ++a) out[3 * i + a] = f ? q[a] : xyz[3 * i + a];
  }
}

}  // namespace sfmreg

// the whole call (run_host, run_host_batch) is register_icp.h's one loop with metric 0 and no rejector: that header is built
// on the rules above and this one ends by including it, so either of the two can be included alone
#include "register_icp.h"
#endif
