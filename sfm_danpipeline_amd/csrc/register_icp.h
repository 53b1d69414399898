// register_icp.h -- the rules of the second registration entry (point-to-plane, trimmed and one-to-one ICP) as
// code that hipcc and a plain g++ both compile, on top of register.h: the options' refusals, the no-plane test, the one-to-one
// slot, the trim count, the row and the sums of the point-to-plane step, its Cholesky solve, the Cayley increment and the loop's
// decision.  The device code (register.hip) and the CPU test stub (tests/stub/register_icp_capi.cpp) share these bodies, so the
// device result is checked bit for bit against a CPU build.  Compile with -ffp-contract=off.  Below the shared part is the host
// form of the whole call: ONE loop (iterate_host, loop_host) behind f-17's run_host, f-18's run_host_batch and f-22's run_host_icp
// and run_host_icp_batch, which differ in their rule 1 and in the struct they hand back.  Every product below is bracketed as
// written: that bracketing is the contract.
#pragma once
#include "register.h"

namespace sfmreg {

// the C ABI's structs (include/sfmhip.h), field for field
struct IcpOpts {
  int32_t max_iters, with_scale, min_pairs, metric, one_to_one, normal_stride;
  double max_dist, eps, trim;
};
struct IcpResult {
  Transform T;
  int32_t iterations, pairs, converged, flags;
  double mse, plane_mse, trim_d2;
};
enum { METRIC_POINT = 0, METRIC_PLANE = 1 };
constexpr int NU = 7;                              // unknowns of the plane step: omega (3), translation (3), sigma
constexpr int NTRI = NU * (NU + 1) / 2;            // the upper triangle of a^T a, row-major: 28
constexpr int NP = 1 + NTRI + NU + 2;              // N, a^T a, a^T r, sum r^2, sum d2: 38
constexpr int P_ATA = 1, P_ATR = 1 + NTRI, P_RR = P_ATR + NU, P_D2 = P_RR + 1;
constexpr uint64_t SLOT_EMPTY = 0xFFFFFFFFFFFFFFFFull;  // rule 4: a target slot nobody chose

SFM_REG_INLINE IcpOpts default_icp_opts() {
  IcpOpts o;
  o.max_iters = 50, o.with_scale = 0, o.min_pairs = 3, o.metric = METRIC_POINT, o.one_to_one = 0, o.normal_stride = 4;
  o.max_dist = inf_d(), o.eps = 0.0, o.trim = 1.0;
  return o;
}
SFM_REG_INLINE int unknowns(const IcpOpts& o) { return o.metric == METRIC_PLANE ? (o.with_scale ? 7 : 6) : 3; }
// rule 1 (NaN fails every comparison)
SFM_REG_INLINE bool valid_icp_opts(const IcpOpts& o, bool have_normals) {
  bool ok = valid_max_dist(o.max_dist) && o.eps >= 0.0 && o.max_iters >= 0;
  ok = ok && o.trim > 0.0 && o.trim <= 1.0;
  ok = ok && (o.metric == METRIC_POINT || o.metric == METRIC_PLANE) && (o.one_to_one == 0 || o.one_to_one == 1);
  ok = ok && (o.normal_stride == 3 || o.normal_stride == 4);
  if (ok && o.metric == METRIC_PLANE) ok = have_normals && o.eps > 0.0;
  return ok && o.min_pairs >= unknowns(o);
}
inline bool valid_icp_batch(const IcpOpts& o, bool have_normals, const Transform* inits, int n_init) {
  if (!valid_icp_opts(o, have_normals) || !inits || n_init < 1 || n_init > MAX_BATCH) return false;
  for (int b = 0; b < n_init; ++b)
    if (!valid_transform(inits[b])) return false;
  return true;
}
// f-17's options of the same call: what metric 0 hands to loop_step
SFM_REG_INLINE Opts point_opts(const IcpOpts& o) {
  Opts p;
  p.max_iters = o.max_iters, p.with_scale = o.with_scale, p.min_pairs = o.min_pairs, p.reserved = 0;
  p.max_dist = o.max_dist, p.eps = o.eps;
  return p;
}
// ... and its inverse: f-17's call as the loop sees it (rule 7: metric 0, no rejector)
SFM_REG_INLINE IcpOpts icp_opts(const Opts& p) {
  IcpOpts o = default_icp_opts();
  o.max_iters = p.max_iters, o.with_scale = p.with_scale, o.min_pairs = p.min_pairs;
  o.max_dist = p.max_dist, o.eps = p.eps;
  return o;
}

// rule 3: a target normal that gives a plane
SFM_REG_INLINE bool has_plane(float nx, float ny, float nz) {
  return sfmcloud::finite3(nx, ny, nz) && !(nx == 0.0f && ny == 0.0f && nz == 0.0f);
}
// rule 4: the slot value of source i at distance d2 (finite or +inf, >= 0: the bits are ordered); the least wins
SFM_REG_INLINE uint64_t slot_of(float d2, int i) {
  uint32_t b;
  memcpy(&b, &d2, 4);
  return ((uint64_t)b << 32) | (uint32_t)i;
}
SFM_REG_INLINE int slot_source(uint64_t s) { return (int)(uint32_t)(s & 0xFFFFFFFFull); }
// a loser of rule 4 keeps its target in the candidate array (so the slot can be cleared): -(j + 2)
SFM_REG_INLINE int lost(int j) { return -(j + 2); }
SFM_REG_INLINE int lost_target(int c) { return -c - 2; }
// rule 5: K of N survivors
SFM_REG_INLINE uint32_t trim_count(double trim, uint32_t n) {
  if (n == 0) return 0;
  double k = ceil(trim * (double)n);
  k = k < 1.0 ? 1.0 : k;
  k = k > (double)n ? (double)n : k;
  return (uint32_t)k;
}
SFM_REG_INLINE uint32_t d2_bits(float d2) {
  uint32_t b;
  memcpy(&b, &d2, 4);
  return b;
}
SFM_REG_INLINE float inf_f() { return sfmcloud::bits_f(0x7F800000u); }

// rule 8: c, the midpoint of the target's finite box (lo, hi the exact floats widened; no finite point: 0)
SFM_REG_INLINE void box_centre(int n_valid, const double lo[3], const double hi[3], double c[3]) {
  for (int a = 0; a < 3; ++a) c[a] = n_valid > 0 ? 0.5 * (lo[a] + hi[a]) : 0.0;
}
// rule 8: a kept pair's terms of the one sum.  q the moved source float, m the target float, n its normal.
//   r = (n0 (q0 - m0) + n1 (q1 - m1)) + n2 (q2 - m2);  qt = q - c
//   a = (qt1 n2 - qt2 n1, qt2 n0 - qt0 n2, qt0 n1 - qt1 n0, n0, n1, n2, with_scale ? (n0 qt0 + n1 qt1) + n2 qt2 : 0)
//   v = N | a_i a_j (i <= j, row-major) | a_i r | r r | (double)d2
SFM_REG_INLINE void plane_terms(bool kept, const float q[3], const float m[3], const float n[3], float d2, const double c[3], int with_scale,
                                double v[NP]) {
#pragma unroll
  for (int k = 0; k < NP; ++k) v[k] = 0.0;
  if (!kept) return;
  double nd[3], qt[3], e[3], a[NU];
  for (int k = 0; k < 3; ++k) nd[k] = (double)n[k], qt[k] = (double)q[k] - c[k], e[k] = (double)q[k] - (double)m[k];
  const double r = (nd[0] * e[0] + nd[1] * e[1]) + nd[2] * e[2];
  a[0] = qt[1] * nd[2] - qt[2] * nd[1];
  a[1] = qt[2] * nd[0] - qt[0] * nd[2];
  a[2] = qt[0] * nd[1] - qt[1] * nd[0];
  a[3] = nd[0], a[4] = nd[1], a[5] = nd[2];
  a[6] = with_scale ? (nd[0] * qt[0] + nd[1] * qt[1]) + nd[2] * qt[2] : 0.0;
  v[0] = 1.0;
#pragma unroll
  for (int i = 0; i < NU; ++i) {
#pragma unroll
    for (int j = i; j < NU; ++j) v[P_ATA + (i * NU - i * (i - 1) / 2) + (j - i)] = a[i] * a[j];  // (row i starts after NU + ... + (NU - i + 1))
  }
#pragma unroll
  for (int i = 0; i < NU; ++i) v[P_ATR + i] = a[i] * r;
  v[P_RR] = r * r;
  v[P_D2] = (double)d2;
}

// rule 8: (a^T a) x = -(a^T r) over the first U unknowns by Cholesky, row by row in one order.  A pivot p_j = A_jj - sum_k<j
// L_jk^2 (subtracted in ascending k) must be finite and > 1e-12 * the largest diagonal entry of A.  false: DEGENERATE
SFM_REG_INLINE bool plane_solve(const double s[NP], int U, double x[NU]) {
  double L[NU][NU], y[NU];
  double dmax = 0.0;
  int at = P_ATA;
  for (int i = 0; i < NU; ++i)
    for (int j = i; j < NU; ++j) L[j][i] = s[at++];  // the lower triangle holds A
  bool ok = true;
  for (int i = 0; i < U; ++i) ok = ok && fin(L[i][i]), dmax = L[i][i] > dmax ? L[i][i] : dmax;
  for (int j = 0; j < U && ok; ++j) {
    double p = L[j][j];
    for (int k = 0; k < j; ++k) p = p - L[j][k] * L[j][k];
    if (!(fin(p) && p > 1e-12 * dmax)) {
      ok = false;
      break;
    }
    const double d = sqrt(p);
    L[j][j] = d;
    for (int i = j + 1; i < U; ++i) {
      double t = L[i][j];
      for (int k = 0; k < j; ++k) t = t - L[i][k] * L[j][k];
      L[i][j] = t / d;
    }
  }
  for (int i = 0; i < NU; ++i) x[i] = 0.0;
  if (!ok) return false;
  for (int i = 0; i < U; ++i) {  // L y = -(a^T r)
    double t = -s[P_ATR + i];
    for (int k = 0; k < i; ++k) t = t - L[i][k] * y[k];
    y[i] = t / L[i][i];
  }
  for (int i = U - 1; i >= 0; --i) {  // L^T x = y
    double t = y[i];
    for (int k = i + 1; k < U; ++k) t = t - L[k][i] * x[k];
    x[i] = t / L[i][i];
  }
  for (int i = 0; i < U; ++i) ok = ok && fin(x[i]);
  return ok;
}

// rule 8: the Cayley increment of omega: v = omega / 2, vv = (v0 v0 + v1 v1) + v2 v2, s = 1 / (1 + vv),
// dR[r][c] = I[r][c] + (2 s) (K[r][c] + (v_r v_c - I[r][c] vv)), K = [v]x.  One division, no trigonometry.
SFM_REG_INLINE void cayley(const double w[3], double dR[9]) {
  const double v[3] = {w[0] / 2.0, w[1] / 2.0, w[2] / 2.0};
  const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  const double s2 = 2.0 * (1.0 / (1.0 + vv));
  const double K[9] = {0.0, -v[2], v[1], v[2], 0.0, -v[0], -v[1], v[0], 0.0};
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double eye = r == c ? 1.0 : 0.0;
      dR[3 * r + c] = eye + s2 * (K[3 * r + c] + (v[r] * v[c] - eye * vv));
    }
}
// rule 8: the next transform from the sums; 0 or F_DEGENERATE (then `next` is not to be used).
//   g = 1 + sigma;  scale' = scale g;  R'[r][c] = (dR[r][0] R[0][c] + dR[r][1] R[1][c]) + dR[r][2] R[2][c]
//   u = t - c;  t'_r = (g ((dR[r][0] u0 + dR[r][1] u1) + dR[r][2] u2) + c_r) + x_{3+r}
SFM_REG_INLINE int plane_estimate(const double s[NP], int with_scale, const double c[3], const Transform& cur, Transform& next) {
  double x[NU], dR[9];
  if (!plane_solve(s, with_scale ? 7 : 6, x)) return F_DEGENERATE;
  const double g = 1.0 + (with_scale ? x[6] : 0.0);
  if (!(fin(g) && g > 0.0)) return F_DEGENERATE;
  cayley(x, dR);
  next.scale = cur.scale * g;
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) next.R[3 * r + k] = (dR[3 * r] * cur.R[k] + dR[3 * r + 1] * cur.R[3 + k]) + dR[3 * r + 2] * cur.R[6 + k];
  const double u[3] = {cur.t[0] - c[0], cur.t[1] - c[1], cur.t[2] - c[2]};
  for (int r = 0; r < 3; ++r) next.t[r] = (g * ((dR[3 * r] * u[0] + dR[3 * r + 1] * u[1]) + dR[3 * r + 2] * u[2]) + c[r]) + x[3 + r];
  return valid_transform(next) ? 0 : F_DEGENERATE;
}

// what the plane metric adds to a loop's record
struct IcpExtra {
  double plane_mse, trim_d2;
};
// rule 9, step k, once C_k's sums are known (register.h's Loop; no fixed-point stop).  true: the loop stops, L.res and ex are complete
SFM_REG_INLINE bool plane_loop_step(Loop& L, IcpExtra& ex, const IcpOpts& o, const double c[3], const double s[NP]) {
  Result& r = L.res;
  r.T = L.T;
  r.iterations = L.k;
  r.pairs = (int32_t)s[0];
  r.mse = s[0] > 0.0 ? s[P_D2] / s[0] : qnan_d();
  ex.plane_mse = s[0] > 0.0 ? s[P_RR] / s[0] : qnan_d();
  r.converged = CONV_LIMIT;
  r.flags = 0;
  bool stop = true;
  Transform next = L.T;
  if (r.pairs < o.min_pairs) r.flags = F_FEW;
  else if (L.k > 0 && within_eps(L.T, L.prev, o.eps)) r.converged = CONV_EPS;
  else if (L.k == o.max_iters) r.converged = CONV_LIMIT;
  else {
    r.flags = plane_estimate(s, o.with_scale, c, L.T, next);
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
SFM_REG_INLINE IcpResult icp_result(const Result& r, const IcpExtra& ex) {
  IcpResult o;
  o.T = r.T;
  o.iterations = r.iterations, o.pairs = r.pairs, o.converged = r.converged, o.flags = r.flags;
  o.mse = r.mse, o.plane_mse = ex.plane_mse, o.trim_d2 = ex.trim_d2;
  return o;
}
// f-17's result of the loop's
SFM_REG_INLINE Result point_result(const IcpResult& r) {
  Result o;
  o.T = r.T;
  o.iterations = r.iterations, o.pairs = r.pairs, o.converged = r.converged, o.flags = r.flags;
  o.mse = r.mse;
  return o;
}

}  // namespace sfmreg

#ifndef __HIPCC__
// ---- the whole call on the host: what the device is checked against
namespace sfmreg {

// rules 3 - 5 on one problem's pairs: idx (rule 2's, -1 without) becomes the kept set; returns tau
inline float reject_host(int n_tgt, int n_src, const IcpOpts& o, const float* normals, std::vector<int32_t>& idx, const std::vector<float>& d2) {
  if (o.metric == METRIC_PLANE)
    for (int i = 0; i < n_src; ++i)
      if (idx[i] >= 0) {
        const float* n = normals + (size_t)o.normal_stride * idx[i];
        if (!has_plane(n[0], n[1], n[2])) idx[i] = -1;
      }
  if (o.one_to_one) {
    std::vector<uint64_t> slot((size_t)std::max(n_tgt, 1), SLOT_EMPTY);
    for (int i = 0; i < n_src; ++i)
      if (idx[i] >= 0) slot[idx[i]] = std::min(slot[idx[i]], slot_of(d2[i], i));
    for (int i = 0; i < n_src; ++i)
      if (idx[i] >= 0 && slot_source(slot[idx[i]]) != i) idx[i] = -1;
  }
  float tau = inf_f();
  if (o.trim < 1.0) {
    std::vector<float> live;
    for (int i = 0; i < n_src; ++i)
      if (idx[i] >= 0) live.push_back(d2[i]);
    const uint32_t K = trim_count(o.trim, (uint32_t)live.size());
    if (K > 0) {
      std::nth_element(live.begin(), live.begin() + (K - 1), live.end());
      tau = live[K - 1];
    }
    for (int i = 0; i < n_src; ++i)
      if (idx[i] >= 0 && !(d2[i] <= tau)) idx[i] = -1;
  }
  return tau;
}

// one step of the loop on the host, for every entry: the search under L.T, the rejectors (without an active one idx stays rule
// 2's), then metric 0's two sums and f-17's decision or the plane's one sum and rule 9's.  prev: scratch for C_{k-1}
inline bool iterate_host(const HostGrid& g, const float* tgt, const float* normals, int n_src, const float* src, const IcpOpts& o, float md2,
                         const double c[3], Loop& L, IcpExtra& ex, std::vector<int32_t>& idx, std::vector<int32_t>& prev, std::vector<float>& d2) {
  prev = idx;
  nearest_host(g, n_src, src, L.T, md2, false, idx.data(), d2.data());
  ex.trim_d2 = (double)reject_host(g.n, n_src, o, normals, idx, d2);
  if (o.metric == METRIC_PLANE) {
    double s[NP];
    const Transform T = L.T;
    sum_host<NP>(n_src, [&](int i, double* v) {
      const bool kept = idx[i] >= 0;
      float q[3] = {0, 0, 0}, m[3] = {0, 0, 0}, n[3] = {0, 0, 0};
      if (kept) {
        move(T, src[3 * i], src[3 * i + 1], src[3 * i + 2], q);
        for (int a = 0; a < 3; ++a) m[a] = tgt[3 * (size_t)idx[i] + a], n[a] = normals[(size_t)o.normal_stride * idx[i] + a];
      }
      plane_terms(kept, q, m, n, kept ? d2[i] : 0.0f, c, o.with_scale, v);
    }, s);
    return plane_loop_step(L, ex, o, c, s);
  }
  bool changed = false;
  for (int i = 0; i < n_src; ++i) changed = changed || idx[i] != prev[i];
  double s1[N1], s2[N2], mu_p[3], mu_m[3];
  auto pm = [&](int i, float p[3], float m[3]) {
    const bool paired = idx[i] >= 0;
    for (int a = 0; a < 3; ++a) p[a] = src[3 * i + a], m[a] = paired ? tgt[3 * (size_t)idx[i] + a] : 0.0f;
    return paired;
  };
  sum_host<N1>(n_src, [&](int i, double* v) {
    float p[3], m[3];
    const bool paired = pm(i, p, m);
    terms1(paired, p, m, v);
  }, s1);
  means(s1, mu_p, mu_m);
  sum_host<N2>(n_src, [&](int i, double* v) {
    float p[3], m[3];
    const bool paired = pm(i, p, m);
    terms2(paired, p, m, d2[i], mu_p, mu_m, v);
  }, s2);
  ex.plane_mse = qnan_d();
  return loop_step(L, point_opts(o), changed, s1, s2);
}

// the one loop: n_init starts in lock step over one grid, a record per problem; a problem that has stopped is left alone.
// results[b] and row b of idx_out (n_init x n_src, or NULL) are what a single call from inits[b] gives.  Refuses nothing: every
// entry below applies its own rule 1 first
inline void loop_host(int n_tgt, const float* tgt, const float* normals, int n_src, const float* src, const IcpOpts& o, const Transform* inits,
                      int n_init, IcpResult* results, int32_t* idx_out) {
  HostGrid g;
  g.build(n_tgt, tgt);
  double c[3];
  box_centre(g.nv, g.lo, g.hi, c);
  const float md2 = max_d2(o.max_dist);
  const size_t n1 = (size_t)std::max(n_src, 1);
  std::vector<std::vector<int32_t>> idx((size_t)n_init, std::vector<int32_t>(n1, -2));
  std::vector<int32_t> prev;
  std::vector<float> d2(n1);  // (a problem's d2 is read only inside its own step)
  std::vector<Loop> L((size_t)n_init);
  std::vector<IcpExtra> ex((size_t)n_init);
  for (int b = 0; b < n_init; ++b) loop_init(L[b], inits[b]), ex[b].plane_mse = qnan_d(), ex[b].trim_d2 = inf_d();
  for (int round = 0, open = n_init; open > 0 && round <= o.max_iters; ++round)
    for (int b = 0; b < n_init; ++b)
      if (!L[b].stop && iterate_host(g, tgt, normals, n_src, src, o, md2, c, L[b], ex[b], idx[b], prev, d2)) --open;
  for (int b = 0; b < n_init; ++b) {
    results[b] = icp_result(L[b].res, ex[b]);
    if (idx_out)
      for (int i = 0; i < n_src; ++i) idx_out[(size_t)b * n_src + i] = idx[b][i];
  }
}

// f-22's two entries (a single call is a batch of one).  false: refused, nothing written
inline bool run_host_icp_batch(int n_tgt, const float* tgt, const float* normals, int n_src, const float* src, const IcpOpts& o,
                               const Transform* inits, int n_init, IcpResult* results, int32_t* idx_out) {
  if (!valid_icp_batch(o, normals != nullptr, inits, n_init)) return false;
  loop_host(n_tgt, tgt, normals, n_src, src, o, inits, n_init, results, idx_out);
  return true;
}
inline bool run_host_icp(int n_tgt, const float* tgt, const float* normals, int n_src, const float* src, const IcpOpts& o, const Transform* init,
                         IcpResult& res, int32_t* idx_out) {
  const Transform T0 = init ? *init : identity();
  return run_host_icp_batch(n_tgt, tgt, normals, n_src, src, o, &T0, 1, &res, idx_out);
}

// f-17's and f-18's entries: the loop with metric 0 and no rejector (f-22 rule 7).  results[b] and row b of idx_out are run_host's
// from inits[b]; `longest` (nullable): the iterations of the problem that ran longest.  false: refused, nothing written
inline bool run_host_batch(int n_tgt, const float* tgt, int n_src, const float* src, const Opts& o, const Transform* inits, int n_init,
                           Result* results, int32_t* idx_out, int* longest = nullptr) {
  if (!valid_batch(o, inits, n_init)) return false;
  std::vector<IcpResult> r((size_t)n_init);
  loop_host(n_tgt, tgt, nullptr, n_src, src, icp_opts(o), inits, n_init, r.data(), idx_out);
  int most = 0;
  for (int b = 0; b < n_init; ++b) results[b] = point_result(r[b]), most = std::max(most, (int)r[b].iterations);
  if (longest) *longest = most;
  return true;
}
inline bool run_host(int n_tgt, const float* tgt, int n_src, const float* src, const Opts& o, const Transform* init, Result& res, int32_t* idx_out) {
  const Transform T0 = init ? *init : identity();
  return run_host_batch(n_tgt, tgt, n_src, src, o, &T0, 1, &res, idx_out);
}

}  // namespace sfmreg
#endif
