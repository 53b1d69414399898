// ground.h -- the arithmetic of the ground-plane fit (the dominant plane of a cloud by RANSAC, refitted and
// oriented so that the trees stand on it: the vertical frame dendro.h measures in) as __host__ __device__ code that hipcc
// and a plain g++ both compile with -ffp-contract=off.  The device code (ground.hip) and the CPU test stub
// (tests/stub/ground_capi.cpp) share these bodies, and run_host() at the end is the whole call in plain loops: the device
// result is checked bit for bit against it.  The contract is the rule list of f-12 (copied at the declaration in
// include/sfmhip.h).  Every f64 expression is written in one order; sqrt and / are the correctly rounded ones; cos is
// called once, on the host, for the tilt limit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "block_sum.h"  // chunk_tree (f-11 rule 6's fixed-order sum)
#include "cloud.h"
#include "dendro.h"  // dnan, finite_d, parallel_for
#include "draw_hash.h"
#include "jacobi.h"

#ifdef __HIPCC__
#define SFM_GND_INLINE __host__ __device__ __forceinline__
#else
#define SFM_GND_INLINE inline __attribute__((always_inline))
#endif

namespace sfmground {

using sfmsum::chunk_tree;
using sfmdendro::dnan;
using sfmdendro::finite_d;

constexpr int MAX_ITERS = 4096;          // rule 1
constexpr int MAX_REFIT = 8;             // rule 1
constexpr int CHUNK = 256;               // slots of a fixed-order sum = threads of a workgroup
constexpr uint32_t STREAM = 0x67726E64;  // rule 3: the hash's second word ("grnd")

enum Flags { F_FEW = 1, F_NO_PLANE = 2, F_REFIT_KEPT = 4, F_NORTH_REPLACED = 8 };

struct Opts {
  double inlier_tol, inlier_rel, below_max;
  double up_hint[3];
  double max_tilt_deg;
  double north_hint[3];
  int32_t ransac_iters, min_inliers, refit_rounds;
  uint32_t seed;
};

struct Result {
  double up[3], north[3];
  double offset, rms, tol;
  int32_t n_selected, inliers, below, above, winner, flags;
};

struct P3 {  // a point of the selection list
  float x, y, z;
};

struct Hyp {  // rule 3: a point of the plane and its unit normal; ok = 0: the iteration is skipped
  double a[3], n[3];
  int32_t ok, pad;
};

struct Counts {  // rule 4
  uint32_t inl, pos, neg;
};

struct Plane {  // the plane between the stages: the winner, then each refit's
  double a[3], n[3];  // n oriented by rule 5
  int32_t winner, flags;
};

struct Prep {  // the options once checked (rule 1)
  double hint[3];   // unit, or 0 when there is none
  double cos_tilt;  // -1 without a hint
  int has_hint;
};

inline Opts default_opts() {
  Opts o;
  o.inlier_tol = 0.0;
  o.inlier_rel = 0.005;
  o.below_max = 0.01;
  o.up_hint[0] = o.up_hint[1] = o.up_hint[2] = 0.0;
  o.max_tilt_deg = 180.0;
  o.north_hint[0] = 0.0, o.north_hint[1] = 1.0, o.north_hint[2] = 0.0;
  o.ransac_iters = 512;
  o.min_inliers = 100;
  o.refit_rounds = 2;
  o.seed = 1;
  return o;
}

SFM_GND_INLINE double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// rule 1: the refusals; the hint normalised, the tilt limit as a cosine
inline bool prepare(const Opts& o, Prep& p) {
  if (o.ransac_iters < 1 || o.ransac_iters > MAX_ITERS) return false;
  if (!(o.inlier_tol >= 0.0) || !finite_d(o.inlier_tol) || !(o.inlier_rel >= 0.0) || !finite_d(o.inlier_rel)) return false;
  if (!(o.below_max >= 0.0 && o.below_max <= 1.0)) return false;
  for (int a = 0; a < 3; ++a)
    if (!finite_d(o.up_hint[a]) || !finite_d(o.north_hint[a])) return false;
  if (!(o.max_tilt_deg > 0.0 && o.max_tilt_deg <= 180.0)) return false;
  if (o.refit_rounds < 0 || o.refit_rounds > MAX_REFIT || o.min_inliers < 3) return false;
  const double hh = std::sqrt(dot3(o.up_hint, o.up_hint));
  p.has_hint = hh > 0.0 && finite_d(hh) ? 1 : 0;
  for (int a = 0; a < 3; ++a) p.hint[a] = p.has_hint ? o.up_hint[a] / hh : 0.0;
  p.cos_tilt = p.has_hint ? std::cos(o.max_tilt_deg * (sfmcloud::PI / 180.0)) : -1.0;
  return true;
}

// rule 2: the tolerance from the selection's float bounding box
inline double tolerance(const Opts& o, const float lo[3], const float hi[3]) {
  if (o.inlier_tol > 0.0) return o.inlier_tol;
  const double dx = (double)hi[0] - (double)lo[0], dy = (double)hi[1] - (double)lo[1], dz = (double)hi[2] - (double)lo[2];
  return o.inlier_rel * std::sqrt((dx * dx + dy * dy) + dz * dz);
}

// rule 3
SFM_GND_INLINE Hyp hypothesis(const P3* pts, int n_sel, uint32_t seed, int j, const double hint[3], double cos_tilt, int has_hint) {
  Hyp h;
  for (int k = 0; k < 3; ++k) h.a[k] = h.n[k] = 0.0;
  h.ok = h.pad = 0;
  const uint32_t ia = sfmdraw::draw_index(seed, STREAM, (uint32_t)j, 0u, (uint32_t)n_sel);
  const uint32_t ib = sfmdraw::draw_index(seed, STREAM, (uint32_t)j, 1u, (uint32_t)n_sel);
  const uint32_t ic = sfmdraw::draw_index(seed, STREAM, (uint32_t)j, 2u, (uint32_t)n_sel);
  if (ia == ib || ia == ic || ib == ic) return h;
  const P3 a = pts[ia], b = pts[ib], c = pts[ic];
  const double ux = (double)b.x - (double)a.x, uy = (double)b.y - (double)a.y, uz = (double)b.z - (double)a.z;
  const double vx = (double)c.x - (double)a.x, vy = (double)c.y - (double)a.y, vz = (double)c.z - (double)a.z;
  const double m0 = uy * vz - uz * vy, m1 = uz * vx - ux * vz, m2 = ux * vy - uy * vx;
  const double mm = (m0 * m0 + m1 * m1) + m2 * m2;
  if (mm == 0.0 || !finite_d(mm)) return h;
  const double len = sqrt(mm);
  h.n[0] = m0 / len;
  h.n[1] = m1 / len;
  h.n[2] = m2 / len;
  if (has_hint && fabs(dot3(h.n, hint)) < cos_tilt) return h;
  h.a[0] = (double)a.x;
  h.a[1] = (double)a.y;
  h.a[2] = (double)a.z;
  h.ok = 1;
  return h;
}

// rule 4: the signed distance of a point to the plane (a, n)
SFM_GND_INLINE double signed_dist(const double a[3], const double n[3], double x, double y, double z) {
  return (n[0] * (x - a[0]) + n[1] * (y - a[1])) + n[2] * (z - a[2]);
}

// rule 5: +1 keeps n, -1 flips it.  cpos / cneg: camera centres with s > 0 / s < 0; pos / neg: rule 4's counts
SFM_GND_INLINE int orientation(const double n[3], int cpos, int cneg, uint32_t pos, uint32_t neg) {
  if (cpos != cneg) return cpos > cneg ? 1 : -1;
  if (pos != neg) return pos > neg ? 1 : -1;
  const double f = n[0] != 0.0 ? n[0] : (n[1] != 0.0 ? n[1] : n[2]);
  return f < 0.0 ? -1 : 1;
}
SFM_GND_INLINE void camera_sides(const Hyp& h, const double* cams, int n_cam, int& cpos, int& cneg) {
  cpos = cneg = 0;
  for (int c = 0; c < n_cam; ++c) {
    const double s = signed_dist(h.a, h.n, cams[3 * c], cams[3 * c + 1], cams[3 * c + 2]);
    cpos += s > 0.0 ? 1 : 0;
    cneg += s < 0.0 ? 1 : 0;
  }
}

// rule 6: the key of hypothesis j (0: not admissible) and its orientation
SFM_GND_INLINE unsigned long long hyp_key(const Hyp& h, const Counts& k, int j, const double* cams, int n_cam, int min_inliers,
                                          long long below_cap, int& sign) {
  sign = 1;
  if (!h.ok) return 0ull;
  int cpos, cneg;
  camera_sides(h, cams, n_cam, cpos, cneg);
  sign = orientation(h.n, cpos, cneg, k.pos, k.neg);
  const uint32_t below = sign > 0 ? k.neg : k.pos;
  if ((long long)k.inl < (long long)min_inliers || (long long)below > below_cap) return 0ull;
  return ((unsigned long long)k.inl << 32) | (unsigned long long)(unsigned)(MAX_ITERS - 1 - j);
}
SFM_GND_INLINE int key_iter(unsigned long long key) { return MAX_ITERS - 1 - (int)(key & 0xFFFFFFFFull); }
inline long long below_cap(double below_max, int n_sel) { return (long long)std::floor(below_max * (double)n_sel); }

SFM_GND_INLINE void plane_from(const Hyp& h, int sign, int j, Plane& p) {
  for (int k = 0; k < 3; ++k) {
    p.a[k] = h.a[k];
    p.n[k] = sign > 0 ? h.n[k] : -h.n[k];
  }
  p.winner = j;
  p.flags = 0;
}

// rule 7: the terms one inlier adds to the first pass (the centroid) and to the second (the covariance about it)
SFM_GND_INLINE void cov_terms(double dx, double dy, double dz, double s[6]) {
  s[0] = dx * dx;
  s[1] = dx * dy;
  s[2] = dx * dz;
  s[3] = dy * dy;
  s[4] = dy * dz;
  s[5] = dz * dz;
}
// ... and the plane from the sums: cen = the centroid, cs = the six covariance sums, N inliers.  w: 21 doubles of work
// space (the device passes LDS: jacobi_svd indexes its rows at run time).  false: the round keeps the previous plane.
SFM_GND_INLINE bool refit_plane(const double cen[3], const double cs[6], double N, double* w, Plane& p) {
  double *At = w, *W = w + 9, *Vt = w + 12;
  At[0] = cs[0] / N, At[1] = cs[1] / N, At[2] = cs[2] / N;
  At[3] = cs[1] / N, At[4] = cs[3] / N, At[5] = cs[4] / N;
  At[6] = cs[2] / N, At[7] = cs[4] / N, At[8] = cs[5] / N;
  sfmjacobi::jacobi_svd<3, 3, 3, 3>(At, W, Vt);
  const double v[3] = {Vt[6], Vt[7], Vt[8]};  // the singular vector of the least singular value
  const double len = sqrt(dot3(v, v));
  double n[3] = {v[0] / len, v[1] / len, v[2] / len};
  if (!finite_d(n[0]) || !finite_d(n[1]) || !finite_d(n[2]) || !finite_d(cen[0]) || !finite_d(cen[1]) || !finite_d(cen[2])) return false;
  const bool flip = dot3(n, p.n) < 0.0;
  for (int k = 0; k < 3; ++k) {
    p.n[k] = flip ? -n[k] : n[k];
    p.a[k] = cen[k];
  }
  return true;
}

// rule 8: north from the hint; true when the hint was replaced by a coordinate axis
inline bool make_north(const double up[3], const double hint_in[3], double north[3]) {
  double h[3] = {hint_in[0], hint_in[1], hint_in[2]};
  const double hh = std::sqrt(dot3(h, h));
  bool replaced = !(hh > 0.0) || !finite_d(hh);
  double n[3] = {0, 0, 0}, nn = 0.0;
  if (!replaced) {
    for (int a = 0; a < 3; ++a) h[a] = h[a] / hh;
    const double d = dot3(h, up);
    for (int a = 0; a < 3; ++a) n[a] = h[a] - d * up[a];
    nn = std::sqrt(dot3(n, n));
    replaced = !(nn > 1e-6);
  }
  if (replaced) {
    int ax = 0;
    for (int a = 1; a < 3; ++a)
      if (std::fabs(up[a]) < std::fabs(up[ax])) ax = a;
    h[0] = h[1] = h[2] = 0.0;
    h[ax] = 1.0;
    const double d = dot3(h, up);
    for (int a = 0; a < 3; ++a) n[a] = h[a] - d * up[a];
    nn = std::sqrt(dot3(n, n));
  }
  for (int a = 0; a < 3; ++a) north[a] = n[a] / nn;
  return replaced;
}

inline void empty_result(Result& r, int n_sel, double tol, int flags) {
  for (int a = 0; a < 3; ++a) r.up[a] = r.north[a] = dnan();
  r.offset = r.rms = dnan();
  r.tol = tol;
  r.n_selected = n_sel;
  r.inliers = r.below = r.above = 0;
  r.winner = -1;
  r.flags = flags;
}

// what the host does after the last stage, shared with ground.hip: the frame from the final plane and its counts
inline void finish(const Opts& o, const Plane& p, int n_sel, double tol, uint32_t inl, uint32_t above, uint32_t below, double rms, Result& r) {
  r.n_selected = n_sel;
  r.tol = tol;
  r.winner = p.winner;
  r.flags = p.flags;
  for (int a = 0; a < 3; ++a) r.up[a] = p.n[a];
  r.offset = dot3(p.n, p.a);
  if (make_north(p.n, o.north_hint, r.north)) r.flags |= F_NORTH_REPLACED;
  r.inliers = (int32_t)inl;
  r.above = (int32_t)above;
  r.below = (int32_t)below;
  r.rms = rms;
}

// the hand-over to dendro.h: up, north and ground = offset * scale (metres).  false: the result has no plane, or no scale.
inline bool opts_from_ground(const Result& g, sfmdendro::Opts& io) {
  if (g.winner < 0 || !(io.scale > 0.0) || !finite_d(io.scale)) return false;
  for (int a = 0; a < 3; ++a) {
    io.up[a] = g.up[a];
    io.north[a] = g.north[a];
  }
  io.ground = g.offset * io.scale;
  return true;
}

// ------------------------------------------------------------------------------------------------ host: the whole call
// the fixed-order sums of one pass over the list: q sums of term(i) over the inliers of plane p
template <int Q, typename Term>
inline void list_sums(const P3* pts, int n_sel, const Plane& p, double tol, Term term, double sum[Q]) {
  std::vector<double> acc((size_t)Q * CHUNK, 0.0);
  double t[Q];
  for (int i = 0; i < n_sel; ++i) {
    const double x = (double)pts[i].x, y = (double)pts[i].y, z = (double)pts[i].z;
    const double s = signed_dist(p.a, p.n, x, y, z);
    if (!(fabs(s) <= tol)) continue;
    term(x, y, z, s, t);
    for (int q = 0; q < Q; ++q) acc[(size_t)q * CHUNK + i % CHUNK] = acc[(size_t)q * CHUNK + i % CHUNK] + t[q];
  }
  for (int q = 0; q < Q; ++q) sum[q] = chunk_tree(&acc[(size_t)q * CHUNK]);
}
inline void count_sides(const P3* pts, int n_sel, const double a[3], const double n[3], double tol, Counts& k) {
  k.inl = k.pos = k.neg = 0;
  for (int i = 0; i < n_sel; ++i) {
    const double s = signed_dist(a, n, (double)pts[i].x, (double)pts[i].y, (double)pts[i].z);
    k.inl += fabs(s) <= tol ? 1u : 0u;
    k.pos += s > tol ? 1u : 0u;
    k.neg += s < -tol ? 1u : 0u;
  }
}

// rule 7, one round on the host
inline void refit_round(const P3* pts, int n_sel, double tol, Plane& p) {
  Counts k;
  count_sides(pts, n_sel, p.a, p.n, tol, k);
  if (k.inl < 3u) {
    p.flags |= F_REFIT_KEPT;
    return;
  }
  const double N = (double)k.inl;
  double s3[3], cen[3], cs[6], w[21];
  list_sums<3>(pts, n_sel, p, tol, [](double x, double y, double z, double, double t[3]) { t[0] = x, t[1] = y, t[2] = z; }, s3);
  for (int a = 0; a < 3; ++a) cen[a] = s3[a] / N;
  list_sums<6>(pts, n_sel, p, tol, [&](double x, double y, double z, double, double t[6]) { cov_terms(x - cen[0], y - cen[1], z - cen[2], t); }, cs);
  if (!refit_plane(cen, cs, N, w, p)) p.flags |= F_REFIT_KEPT;
}

// the whole call on the host.  false: the options are refused.  cams: 3 n_cam doubles or nullptr.
inline bool run_host(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts& o, const double* cams, int n_cam,
                     int threads, Result& res) {
  Prep pr;
  if (!prepare(o, pr) || n_cam < 0 || (n_cam > 0 && !cams)) return false;
  // rule 1: the list, and its float bounding box
  std::vector<P3> pts;
  uint32_t klo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, khi[3] = {0u, 0u, 0u};
  for (int i = 0; i < n; ++i) {
    const float* v = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(v[0], v[1], v[2]) || (labels && labels[i] != label)) continue;
    P3 p;
    p.x = v[0], p.y = v[1], p.z = v[2];
    pts.push_back(p);
    for (int a = 0; a < 3; ++a) {
      const uint32_t key = sfmcloud::ord_key(v[a]);
      klo[a] = key < klo[a] ? key : klo[a];
      khi[a] = key > khi[a] ? key : khi[a];
    }
  }
  const int n_sel = (int)pts.size();
  if (n_sel < 3) {
    empty_result(res, n_sel, dnan(), F_FEW);
    return true;
  }
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = sfmcloud::ord_val(klo[a]), hi[a] = sfmcloud::ord_val(khi[a]);
  const double tol = tolerance(o, lo, hi);
  // rules 3 - 6
  const int J = o.ransac_iters;
  const long long cap = below_cap(o.below_max, n_sel);
  std::vector<unsigned long long> keys((size_t)J, 0ull);
  std::vector<int> signs((size_t)J, 1);
  sfmdendro::parallel_for(J, threads, [&](int j) {
    const Hyp h = hypothesis(pts.data(), n_sel, o.seed, j, pr.hint, pr.cos_tilt, pr.has_hint);
    if (!h.ok) return;
    Counts k;
    count_sides(pts.data(), n_sel, h.a, h.n, tol, k);
    keys[j] = hyp_key(h, k, j, cams, n_cam, o.min_inliers, cap, signs[j]);
  });
  unsigned long long best = 0ull;
  for (int j = 0; j < J; ++j) best = keys[j] > best ? keys[j] : best;
  if (best == 0ull) {
    empty_result(res, n_sel, tol, F_NO_PLANE);
    return true;
  }
  const int jw = key_iter(best);
  Plane p;
  plane_from(hypothesis(pts.data(), n_sel, o.seed, jw, pr.hint, pr.cos_tilt, pr.has_hint), signs[jw], jw, p);
  // rule 7
  for (int r = 0; r < o.refit_rounds; ++r) refit_round(pts.data(), n_sel, tol, p);
  Counts k;
  count_sides(pts.data(), n_sel, p.a, p.n, tol, k);
  double s2;
  list_sums<1>(pts.data(), n_sel, p, tol, [](double, double, double, double s, double t[1]) { t[0] = s * s; }, &s2);
  const double rms = k.inl ? std::sqrt(s2 / (double)k.inl) : dnan();
  finish(o, p, n_sel, tol, k.inl, k.pos, k.neg, rms, res);
  return true;
}

}  // namespace sfmground
