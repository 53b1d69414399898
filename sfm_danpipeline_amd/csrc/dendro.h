// dendro.h -- the arithmetic of the dendrometry step (tree height, DBH, stem profile, crown base, crown
// spread on a tree's cloud) as __host__ __device__ code that hipcc and a plain g++ both compile with -ffp-contract=off.
// The device code (dendro.hip) and the CPU test stub (tests/stub/dendro_capi.cpp) share these bodies, and run_host() at
// the end is the whole call in plain loops: the device result is checked bit for bit against it.  The reference has
// no implementation to match (its Dendrometry::estimate prints blanks, src/DendrometryE.cpp:3-29); the contract is the
// rule list of f-11.  Every f64 expression is written in one order; sqrt and / are the correctly rounded ones.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>
#include "block_sum.h"
#include "cloud.h"
#include "draw_hash.h"

#ifdef __HIPCC__
#define SFM_DND_INLINE __host__ __device__ __forceinline__
#else
#define SFM_DND_INLINE inline __attribute__((always_inline))
#endif

namespace sfmdendro {

constexpr int MAX_SLICES = 4096;  // rule 4
constexpr int MAX_ITERS = 4096;   // rule 1
constexpr int SECTORS = 16;       // rule 5
constexpr int BINS = 1024;        // rule 8
constexpr int GN_STEPS = 10;      // rule 6
constexpr int CHUNK = 256;        // slots of a fixed-order sum = threads of a workgroup

enum Flags { F_EMPTY = 1, F_DBH_ONE = 2, F_DBH_NONE = 4, F_NO_CROWN = 8 };

struct Opts {  // rule 1 (lengths in metres)
  double up[3], north[3];
  double scale, ground, dbh_height, slice, inlier_tol, r_min, r_max, extent_q, extent_bin, crown_factor;
  int ransac_iters, min_inliers, min_sectors, crown_run, min_slice_pts;
  uint32_t seed;
};

struct Frame {  // rule 3 and the lengths of rule 1 in cloud units
  double east[3], north[3], up[3];
  double t, tol, r_min, r_max, bin, dbh_h;
};

struct P2 {  // (e, n) of a point of a slice
  float x, y;
};

struct Circle {
  double cx, cy, r;
  int ok;
};

struct Slice {  // one row of the stem profile (cloud units)
  int32_t count, stem, inliers, mask;
  double ce, cn, radius, rms, extent;
};

struct Result {  // metres
  double total_height, dbh, dbh_e, dbh_n, crown_base_height, live_crown, spread_ns, spread_ew, ground;
  int32_t n_selected, n_slices, crown_base_slice, flags;
};

SFM_DND_INLINE double dnan() {
  const uint64_t u = 0x7FF8000000000000ull;
  double d;
  memcpy(&d, &u, 8);
  return d;
}
SFM_DND_INLINE bool finite_d(double x) { return x - x == 0.0; }

inline Opts default_opts() {
  Opts o;
  o.up[0] = 0, o.up[1] = 0, o.up[2] = 1;
  o.north[0] = 0, o.north[1] = 1, o.north[2] = 0;
  o.scale = 1.0;
  o.ground = dnan();
  o.dbh_height = 1.3;
  o.slice = 0.1;
  o.inlier_tol = 0.02;
  o.r_min = 0.02;
  o.r_max = 1.5;
  o.extent_q = 0.95;
  o.extent_bin = 0.05;
  o.crown_factor = 3.0;
  o.ransac_iters = 256;
  o.min_inliers = 20;
  o.min_sectors = 6;
  o.crown_run = 3;
  o.min_slice_pts = 10;
  o.seed = 1;
  return o;
}

// rule 1: the refusals, and the frame.  north is projected off up and normalised; east = north x up.
inline bool make_frame(const Opts& o, Frame& f) {
  const double uu = (o.up[0] * o.up[0] + o.up[1] * o.up[1]) + o.up[2] * o.up[2];
  if (!(std::fabs(uu - 1.0) <= 2e-6)) return false;  // (|up| within 1e-6 of 1)
  if (!(o.scale > 0.0) || !finite_d(o.scale) || !(o.slice > 0.0) || !finite_d(o.slice)) return false;
  if (o.ransac_iters < 1 || o.ransac_iters > MAX_ITERS) return false;
  if (!(o.inlier_tol >= 0.0) || !(o.r_min >= 0.0) || !(o.r_max >= o.r_min) || !(o.extent_bin > 0.0) || !finite_d(o.extent_bin)) return false;
  if (!(o.extent_q > 0.0 && o.extent_q <= 1.0) || !(o.crown_factor > 0.0) || !finite_d(o.dbh_height)) return false;
  if (o.min_inliers < 1 || o.min_sectors < 0 || o.min_sectors > SECTORS || o.crown_run < 1 || o.min_slice_pts < 3) return false;
  if (!(o.ground != o.ground) && !finite_d(o.ground)) return false;  // NaN or a number
  const double d = (o.north[0] * o.up[0] + o.north[1] * o.up[1]) + o.north[2] * o.up[2];
  double n[3];
  for (int a = 0; a < 3; ++a) n[a] = o.north[a] - d * o.up[a];
  const double nn = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(nn > 1e-9) || !finite_d(nn)) return false;  // parallel to up
  for (int a = 0; a < 3; ++a) {
    f.up[a] = o.up[a];
    f.north[a] = n[a] / nn;
  }
  f.east[0] = f.north[1] * f.up[2] - f.north[2] * f.up[1];
  f.east[1] = f.north[2] * f.up[0] - f.north[0] * f.up[2];
  f.east[2] = f.north[0] * f.up[1] - f.north[1] * f.up[0];
  f.t = o.slice / o.scale;
  f.tol = o.inlier_tol / o.scale;
  f.r_min = o.r_min / o.scale;
  f.r_max = o.r_max / o.scale;
  f.bin = o.extent_bin / o.scale;
  f.dbh_h = o.dbh_height / o.scale;
  return true;
}

// rules 2 and 3: (e, n, h) of a point as float32; NaN for a point that is not selected (not finite, another label, or a
// frame coordinate that leaves float32's range)
SFM_DND_INLINE bool frame_point(const Frame& f, const float* p, bool label_ok, float out[3]) {
  bool ok = label_ok && sfmcloud::finite3(p[0], p[1], p[2]);
  if (ok) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    out[0] = (float)((f.east[0] * x + f.east[1] * y) + f.east[2] * z);
    out[1] = (float)((f.north[0] * x + f.north[1] * y) + f.north[2] * z);
    out[2] = (float)((f.up[0] * x + f.up[1] * y) + f.up[2] * z);
    ok = sfmcloud::finite3(out[0], out[1], out[2]);
  }
  if (!ok) out[0] = out[1] = out[2] = sfmcloud::qnan();
  return ok;
}

// rule 4: the slice of height h among S slices (-1: below the ground or not selected)
SFM_DND_INLINE int slice_of(float h, double h0, double t, int S) {
  const double d = (double)h - h0;
  if (!(d >= 0.0)) return -1;
  double k = floor(d / t);
  if (k > (double)(S - 1)) k = (double)(S - 1);
  return (int)k;
}
inline int slice_count(float hmax, double h0, double t) {
  const double d = (double)hmax - h0;
  if (!(d >= 0.0)) return 0;
  double k = std::floor(d / t);
  if (k > (double)(MAX_SLICES - 1)) k = (double)(MAX_SLICES - 1);
  return (int)k + 1;
}

// rule 5, the draw: draw_hash.h's counter-based hash of (seed, slice, iteration, draw)
using sfmdraw::draw_hash;
using sfmdraw::mix32;
SFM_DND_INLINE int draw_index(uint32_t seed, int k, int j, int d, int nk) {
  return (int)sfmdraw::draw_index(seed, (uint32_t)k, (uint32_t)j, (uint32_t)d, (uint32_t)nk);
}

// rule 5, the model: the circumcircle of three points relative to the first
SFM_DND_INLINE Circle circumcircle(float x1, float y1, float x2, float y2, float x3, float y3, double r_min, double r_max) {
  Circle c;
  c.cx = c.cy = c.r = 0.0;
  c.ok = 0;
  const double bx = (double)x2 - (double)x1, by = (double)y2 - (double)y1;
  const double cx = (double)x3 - (double)x1, cy = (double)y3 - (double)y1;
  const double det = 2.0 * (bx * cy - by * cx);
  if (det == 0.0 || det != det) return c;
  const double b2 = bx * bx + by * by, c2 = cx * cx + cy * cy;
  const double ux = (cy * b2 - by * c2) / det, uy = (bx * c2 - cx * b2) / det;
  const double r = sqrt(ux * ux + uy * uy);
  if (!(r >= r_min && r <= r_max)) return c;
  c.cx = (double)x1 + ux;
  c.cy = (double)y1 + uy;
  c.r = r;
  c.ok = (c.cx - c.cx == 0.0 && c.cy - c.cy == 0.0) ? 1 : 0;
  return c;
}
SFM_DND_INLINE Circle hypothesis(const P2* pts, int nk, uint32_t seed, int k, int j, double r_min, double r_max) {
  const int a = draw_index(seed, k, j, 0, nk), b = draw_index(seed, k, j, 1, nk), c = draw_index(seed, k, j, 2, nk);
  if (a == b || a == c || b == c) {
    Circle z;
    z.cx = z.cy = z.r = 0.0;
    z.ok = 0;
    return z;
  }
  return circumcircle(pts[a].x, pts[a].y, pts[b].x, pts[b].y, pts[c].x, pts[c].y, r_min, r_max);
}

// rule 5, inliers and arc cover
SFM_DND_INLINE bool is_inlier(double dx, double dy, double r, double tol) {
  const double d = sqrt(dx * dx + dy * dy);
  return fabs(d - r) <= tol;
}
// the sector (0 .. 15, 22.5 degrees each, counter-clockwise from +e) of a direction: signs, one comparison of |dx| with
// |dy| and one of the smaller with tan(22.5 deg) times the larger
SFM_DND_INLINE int sector_of(double dx, double dy) {
  const double ax = fabs(dx), ay = fabs(dy);
  const bool steep = ay > ax;
  const double lo = steep ? ax : ay, hi = steep ? ay : ax;
  const bool half = lo > hi * 0.41421356237309503;
  const int s = steep ? (half ? 2 : 3) : (half ? 1 : 0);
  if (dx >= 0.0) return dy >= 0.0 ? s : 15 - s;
  return dy >= 0.0 ? 7 - s : 8 + s;
}
// rule 5, the winner: one integer key per hypothesis with at least one inlier; the largest key wins (the mask rides below j:
// it is a function of (k, j), so it never decides)
SFM_DND_INLINE unsigned long long winner_key(int count, int j, unsigned mask) {
  return ((unsigned long long)(unsigned)count << 32) | ((unsigned long long)(unsigned)(MAX_ITERS - 1 - j) << 16) | (unsigned long long)(mask & 0xFFFFu);
}
SFM_DND_INLINE int key_count(unsigned long long key) { return (int)(key >> 32); }
SFM_DND_INLINE int key_iter(unsigned long long key) { return MAX_ITERS - 1 - (int)((key >> 16) & 0xFFFFu); }
SFM_DND_INLINE int key_mask(unsigned long long key) { return (int)(key & 0xFFFFu); }
SFM_DND_INLINE int popcount16(int m) {
  int c = 0;
  for (int b = 0; b < SECTORS; ++b) c += (m >> b) & 1;
  return c;
}
SFM_DND_INLINE bool is_stem(unsigned long long key, int min_inliers, int min_sectors) {
  return key != 0ull && key_count(key) >= min_inliers && popcount16(key_mask(key)) >= min_sectors;
}

// rule 6: the terms of one point.  Kasa: u, v relative to the RANSAC centre, z = u^2 + v^2
SFM_DND_INLINE void kasa_terms(double u, double v, double s[8]) {
  const double z = u * u + v * v;
  s[0] = u * u;
  s[1] = u * v;
  s[2] = v * v;
  s[3] = u;
  s[4] = v;
  s[5] = u * z;
  s[6] = v * z;
  s[7] = z;
}
// Gauss-Newton on d_i - r: p = (u - a) / d, q = (v - b) / d (0 when d is 0), res = d - r
SFM_DND_INLINE void gn_terms(double u, double v, double a, double b, double r, double s[8]) {
  const double du = u - a, dv = v - b;
  const double d = sqrt(du * du + dv * dv);
  const double p = d > 0.0 ? du / d : 0.0, q = d > 0.0 ? dv / d : 0.0;
  const double res = d - r;
  s[0] = p * p;
  s[1] = p * q;
  s[2] = q * q;
  s[3] = p;
  s[4] = q;
  s[5] = p * res;
  s[6] = q * res;
  s[7] = res;
}
SFM_DND_INLINE double res2_term(double u, double v, double a, double b, double r) {
  const double du = u - a, dv = v - b;
  const double res = sqrt(du * du + dv * dv) - r;
  return res * res;
}
// both solves reduce the 3 x 3 normal equations to 2 x 2 with the count N
SFM_DND_INLINE bool kasa_solve(const double s[8], double N, double& a, double& b, double& r) {
  const double cuu = s[0] - s[3] * s[3] / N, cuv = s[1] - s[3] * s[4] / N, cvv = s[2] - s[4] * s[4] / N;
  const double cuz = s[5] - s[3] * s[7] / N, cvz = s[6] - s[4] * s[7] / N;
  const double det = cuu * cvv - cuv * cuv;
  if (!(det > 0.0)) return false;
  const double ka = (cuz * cvv - cvz * cuv) / (2.0 * det), kb = (cvz * cuu - cuz * cuv) / (2.0 * det);
  const double c = -((s[7] - 2.0 * ka * s[3]) - 2.0 * kb * s[4]) / N;
  const double r2 = (ka * ka + kb * kb) - c;
  if (!(r2 > 0.0) || !finite_d(r2) || !finite_d(ka) || !finite_d(kb)) return false;
  a = ka;
  b = kb;
  r = sqrt(r2);
  return true;
}
SFM_DND_INLINE bool gn_solve(const double s[8], double N, double& a, double& b, double& r) {
  const double mpp = s[0] - s[3] * s[3] / N, mpq = s[1] - s[3] * s[4] / N, mqq = s[2] - s[4] * s[4] / N;
  const double gp = s[5] - s[3] * s[7] / N, gq = s[6] - s[4] * s[7] / N;
  const double det = mpp * mqq - mpq * mpq;
  if (!(det > 0.0)) return false;
  const double da = (gp * mqq - gq * mpq) / det, db = (gq * mpp - gp * mpq) / det;
  const double dr = ((s[7] - s[3] * da) - s[4] * db) / N;
  const double na = a + da, nb = b + db, nr = r + dr;
  if (!finite_d(na) || !finite_d(nb) || !finite_d(nr) || !(nr > 0.0)) return false;
  a = na;
  b = nb;
  r = nr;
  return true;
}

// rule 8
SFM_DND_INLINE int extent_bin_of(double de, double dn, double bin) {
  double b = floor(sqrt(de * de + dn * dn) / bin);
  if (!(b < (double)(BINS - 1))) b = (double)(BINS - 1);
  return (int)b;
}
SFM_DND_INLINE int extent_need(double q, int nk) {
  double need = ceil(q * (double)nk);
  if (need < 1.0) need = 1.0;
  if (need > (double)nk) need = (double)nk;
  return (int)need;
}

// ------------------------------------------------------------------------------------------------ host: the whole call
// the fixed-order sum: slot i mod 256 in ascending i, then four 64-entry trees (strides 32 .. 1), then (w0 + w1) + (w2 + w3)
using sfmsum::chunk_tree;  // (block_sum.h)

template <typename F>
inline void parallel_for(int n, int threads, F f) {
  if (threads <= 1 || n < 2) {
    for (int i = 0; i < n; ++i) f(i);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < threads; ++t)
    th.emplace_back([&, t] {
      for (int i = t; i < n; i += threads) f(i);
    });
  for (auto& x : th) x.join();
}

// rule 5 for one slice of nk >= min_slice_pts points: the winner's key, 0 when no iteration had an inlier
inline unsigned long long ransac_slice(const P2* pts, int nk, int k, const Opts& o, const Frame& f) {
  unsigned long long best = 0;
  for (int j = 0; j < o.ransac_iters; ++j) {
    const Circle c = hypothesis(pts, nk, o.seed, k, j, f.r_min, f.r_max);
    if (!c.ok) continue;
    int cnt = 0;
    unsigned mask = 0;
    for (int i = 0; i < nk; ++i) {
      const double dx = (double)pts[i].x - c.cx, dy = (double)pts[i].y - c.cy;
      if (is_inlier(dx, dy, c.r, f.tol)) {
        ++cnt;
        mask |= 1u << sector_of(dx, dy);
      }
    }
    if (cnt > 0) {
      const unsigned long long key = winner_key(cnt, j, mask);
      if (key > best) best = key;
    }
  }
  return best;
}

// rules 5 and 6 for one slice of nk points (ascending input index); fills every field of `s` but extent
inline void fit_slice(const P2* pts, int nk, int k, const Opts& o, const Frame& f, Slice& s) {
  s.count = nk;
  s.stem = s.inliers = s.mask = 0;
  s.ce = s.cn = s.radius = s.rms = s.extent = dnan();
  if (nk < o.min_slice_pts) return;
  const unsigned long long best = ransac_slice(pts, nk, k, o, f);
  if (best != 0ull) {
    s.inliers = key_count(best);
    s.mask = key_mask(best);
  }
  if (!is_stem(best, o.min_inliers, o.min_sectors)) return;
  s.stem = 1;
  const Circle c = hypothesis(pts, nk, o.seed, k, key_iter(best), f.r_min, f.r_max);
  const double N = (double)s.inliers;
  double a = 0.0, b = 0.0, r = c.r;
  double acc[8][CHUNK], sum[8], term[8];
  for (int pass = 0; pass <= GN_STEPS + 1; ++pass) {  // Kasa, the Gauss-Newton steps, the residual
    for (int q = 0; q < 8; ++q)
      for (int t = 0; t < CHUNK; ++t) acc[q][t] = 0.0;
    for (int i = 0; i < nk; ++i) {
      const double dx = (double)pts[i].x - c.cx, dy = (double)pts[i].y - c.cy;
      if (!is_inlier(dx, dy, c.r, f.tol)) continue;
      if (pass == 0)
        kasa_terms(dx, dy, term);
      else if (pass <= GN_STEPS)
        gn_terms(dx, dy, a, b, r, term);
      else
        term[0] = res2_term(dx, dy, a, b, r);
      const int nq = pass <= GN_STEPS ? 8 : 1;
      for (int q = 0; q < nq; ++q) acc[q][i % CHUNK] = acc[q][i % CHUNK] + term[q];
    }
    for (int q = 0; q < 8; ++q) sum[q] = chunk_tree(acc[q]);
    if (pass == 0)
      kasa_solve(sum, N, a, b, r);
    else if (pass <= GN_STEPS)
      gn_solve(sum, N, a, b, r);
    else
      s.rms = sqrt(sum[0] / N);
  }
  s.ce = c.cx + a;
  s.cn = c.cy + b;
  s.radius = r;
}

// rule 7 over the slice table: radius and centre at the DBH height (cloud units); returns the flag bits
inline int dbh_from_slices(const Slice* sl, int S, const Frame& f, double& r, double& ce, double& cn) {
  const double x = f.dbh_h / f.t - 0.5;
  const double kf = std::floor(x);
  r = ce = cn = dnan();
  if (!(kf >= -1.0 && kf < (double)MAX_SLICES)) return F_DBH_NONE;
  const int lo = (int)kf, hi = lo + 1;
  const bool slo = lo >= 0 && lo < S && sl[lo].stem, shi = hi >= 0 && hi < S && sl[hi].stem;
  if (slo && shi) {
    const double w = x - kf;
    r = sl[lo].radius + w * (sl[hi].radius - sl[lo].radius);
    ce = sl[lo].ce + w * (sl[hi].ce - sl[lo].ce);
    cn = sl[lo].cn + w * (sl[hi].cn - sl[lo].cn);
    return 0;
  }
  if (slo || shi) {
    const Slice& s = slo ? sl[lo] : sl[hi];
    r = s.radius;
    ce = s.ce;
    cn = s.cn;
    return F_DBH_ONE;
  }
  return F_DBH_NONE;
}

// rule 9 over the slice table (extents filled): the crown base slice, -1 if none
inline int crown_base(const Slice* sl, int S, const Opts& o, const Frame& f, double r_dbh) {
  if (!(r_dbh == r_dbh)) return -1;
  const double lim = o.crown_factor * r_dbh;
  for (int k = 0; k + o.crown_run <= S; ++k) {
    if (!(((double)k + 0.5) * f.t > f.dbh_h)) continue;
    bool ok = true;
    for (int m = k; m < k + o.crown_run && ok; ++m) ok = sl[m].count >= o.min_slice_pts && sl[m].extent > lim;
    if (ok) return k;
  }
  return -1;
}

inline void empty_result(Result& res) {
  res.total_height = res.dbh = res.dbh_e = res.dbh_n = res.crown_base_height = res.live_crown = res.spread_ns = res.spread_ew = res.ground = dnan();
  res.n_selected = res.n_slices = 0;
  res.crown_base_slice = -1;
  res.flags = F_EMPTY;
}

// what the host does between the device's stages, shared with dendro.hip: the scalars once the table is complete
// (mn / mx: float32 min / max of e and n over the points at or above the crown base, read only when cb >= 0)
inline void finish(const Opts& o, const Frame& f, double h0, float hmax, int n_sel, int S, int dbh_flags, double r_dbh, double ce, double cn,
                   int cb, const float mn[2], const float mx[2], Result& res) {
  res.n_selected = n_sel;
  res.n_slices = S;
  res.flags = dbh_flags;
  res.ground = h0 * o.scale;
  res.total_height = ((double)hmax - h0) * o.scale;
  res.dbh = 2.0 * r_dbh * o.scale;
  res.dbh_e = ce * o.scale;
  res.dbh_n = cn * o.scale;
  res.crown_base_slice = cb;
  if (cb >= 0) {
    res.crown_base_height = (double)cb * f.t * o.scale;
    res.live_crown = res.total_height - res.crown_base_height;
    res.spread_ew = ((double)mx[0] - (double)mn[0]) * o.scale;
    res.spread_ns = ((double)mx[1] - (double)mn[1]) * o.scale;
  } else {
    res.crown_base_height = res.live_crown = res.spread_ew = res.spread_ns = dnan();
    res.flags |= F_NO_CROWN;
  }
}

// the whole call on the host.  false: the options are refused.  frame_out (3 n floats, nullable): the frame buffer.
inline bool run_host(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts& o, int threads, Result& res,
                     std::vector<Slice>& slices, float* frame_out = nullptr) {
  Frame f;
  if (!make_frame(o, f)) return false;
  slices.clear();
  std::vector<float> fr((size_t)3 * (n > 0 ? n : 1));
  parallel_for(threads, threads, [&](int t) {
    for (int i = t; i < n; i += threads) frame_point(f, xyz + 3 * (size_t)i, !labels || labels[i] == label, &fr[3 * (size_t)i]);
  });
  if (frame_out) memcpy(frame_out, fr.data(), sizeof(float) * 3 * (size_t)n);
  int n_sel = 0;
  uint32_t lo = 0xFFFFFFFFu, hi = 0u;
  for (int i = 0; i < n; ++i) {
    const float h = fr[3 * (size_t)i + 2];
    if (h != h) continue;
    ++n_sel;
    const uint32_t key = sfmcloud::ord_key(h);
    lo = key < lo ? key : lo;
    hi = key > hi ? key : hi;
  }
  empty_result(res);
  if (!n_sel) return true;
  const float hmax = sfmcloud::ord_val(hi);
  const double h0 = o.ground != o.ground ? (double)sfmcloud::ord_val(lo) : o.ground / o.scale;
  const int S = slice_count(hmax, h0, f.t);
  if (!S) return true;
  // rule 4: the points of every slice in ascending input index
  std::vector<int> start((size_t)S + 1, 0);
  for (int i = 0; i < n; ++i) {
    const int k = slice_of(fr[3 * (size_t)i + 2], h0, f.t, S);
    if (k >= 0) ++start[(size_t)k + 1];
  }
  for (int k = 0; k < S; ++k) start[(size_t)k + 1] += start[k];
  std::vector<P2> pts((size_t)start[S] + 1);
  {
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i) {
      const int k = slice_of(fr[3 * (size_t)i + 2], h0, f.t, S);
      if (k < 0) continue;
      P2 p;
      p.x = fr[3 * (size_t)i];
      p.y = fr[3 * (size_t)i + 1];
      pts[(size_t)at[k]++] = p;
    }
  }
  slices.resize((size_t)S);
  parallel_for(S, threads, [&](int k) { fit_slice(pts.data() + start[k], start[(size_t)k + 1] - start[k], k, o, f, slices[k]); });
  double r_dbh, ce, cn;
  const int dflags = dbh_from_slices(slices.data(), S, f, r_dbh, ce, cn);
  if (!(dflags & F_DBH_NONE))
    parallel_for(S, threads, [&](int k) {
      const int nk = slices[k].count;
      if (!nk) return;
      std::vector<int> hist(BINS, 0);
      for (int i = start[k]; i < start[(size_t)k + 1]; ++i) ++hist[extent_bin_of((double)pts[i].x - ce, (double)pts[i].y - cn, f.bin)];
      const int need = extent_need(o.extent_q, nk);
      int cum = 0;
      for (int b = 0; b < BINS; ++b) {
        cum += hist[b];
        if (cum >= need) {
          slices[k].extent = (double)(b + 1) * f.bin;
          break;
        }
      }
    });
  const int cb = crown_base(slices.data(), S, o, f, r_dbh);
  float mn[2] = {0, 0}, mx[2] = {0, 0};
  if (cb >= 0) {
    uint32_t klo[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, khi[2] = {0u, 0u};
    const double hb = h0 + (double)cb * f.t;
    for (int i = 0; i < n; ++i) {
      if (!((double)fr[3 * (size_t)i + 2] >= hb)) continue;
      for (int a = 0; a < 2; ++a) {
        const uint32_t key = sfmcloud::ord_key(fr[3 * (size_t)i + a]);
        klo[a] = key < klo[a] ? key : klo[a];
        khi[a] = key > khi[a] ? key : khi[a];
      }
    }
    for (int a = 0; a < 2; ++a) {
      mn[a] = sfmcloud::ord_val(klo[a]);
      mx[a] = sfmcloud::ord_val(khi[a]);
    }
  }
  finish(o, f, h0, hmax, n_sel, S, dflags, r_dbh, ce, cn, cb, mn, mx, res);
  return true;
}

}  // namespace sfmdendro
