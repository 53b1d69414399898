// crowns.h -- the arithmetic of the crown delineation (tree tops as variable-window maxima of the smoothed
// canopy raster, crowns by steepest ascent with window merging, a tree number per point) as __host__ __device__ code that hipcc
// and a plain g++ both compile with -ffp-contract=off.  The device code (crowns.hip) and the CPU test stub
// (tests/stub/crowns_capi.cpp) share these bodies, and run_host() at the end is the whole call in plain loops: the device result
// is checked byte for byte against it.  The contract is the rule list of f-21 (copied at the declaration in include/sfmhip.h).
// Every quantity is a pure function of the raster: a comparison of float32 values, a comparison of integers, or an f64
// expression written in one order; no result depends on the order in which cells are visited.
//
// What the rules do not do: this is a steepest-ascent partition with window merging, not a flooding watershed.  Two crowns that
// touch are split along the valley of the smoothed raster.  A minor summit goes to the tree of the highest cell in its window,
// which can leave a crown in two pieces.  A tree shorter than a taller neighbour's window away from it is absorbed.  PCL and the
// reference have nothing comparable: there is no parity to pin.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "cloud.h"
#include "dendro.h"  // finite_d
#include "terrain.h"  // Dims, cell_of (f-20 rule 3) for rule 10

#ifdef __HIPCC__
#define SFM_CRN_INLINE __host__ __device__ __forceinline__
#else
#define SFM_CRN_INLINE inline __attribute__((always_inline))
#endif

namespace sfmcrowns {

using sfmdendro::finite_d;

constexpr int TILE = 64;                 // cells a wave takes from one raster row (crowns.hip): the tests' edge shapes hang on it
constexpr int BATCH = 4;                 // doubling rounds between two reads of the counters (crowns.hip)
constexpr int MAX_PASSES = 64;           // rule 1
constexpr int MAX_TREES = 65536;         // rule 1
constexpr double WINDOW_CAP = 64.0;      // rule 1: a window's radius in cells
constexpr double CELL_CAP = 16777216.0;  // rule 2: 2^24 cells

enum Flags { F_NO_CANOPY = 1, F_OVERFLOW = 4 };

struct Opts {  // rule 1 (lengths in metres)
  double scale, min_height, win_a, win_b, r_min, r_max, crown_frac, max_crown_radius, ground_clear;
  int32_t smooth_passes, max_trees;
};

struct Top {  // rule 11
  double e, n, area;
  float height, height_smooth;
  int32_t cell_id, ix, iy, R2, cells, points;
};

struct Result {  // rule 11
  double c;
  float e_min, n_min;
  int32_t De, Dn, n_canopy, n_summits, n_trees, n_labelled_cells, n_labelled, max_depth, flags, pad;
};

struct Prep {  // the options once checked: lengths in cloud units where the rules use them so
  double scale, c, min_h, win_a, win_b, r_min, r_max, crown_frac, mr2, ground_clear;
  int32_t smooth_passes, max_trees;
};

inline Opts default_opts() {
  Opts o;
  o.scale = 1.0;
  o.min_height = 2.0;
  o.win_a = 0.6;
  o.win_b = 0.06;
  o.r_min = 0.6;
  o.r_max = 5.0;
  o.crown_frac = 0.3;
  o.max_crown_radius = 10.0;
  o.ground_clear = 0.3;
  o.smooth_passes = 2;
  o.max_trees = 4096;
  return o;
}

// rule 1: the refusals, and the lengths the rules use in cloud units.  c: the cell in cloud units.
inline bool prepare(const Opts& o, double c, Prep& p) {
  const double all[9] = {o.scale, o.min_height, o.win_a, o.win_b, o.r_min, o.r_max, o.crown_frac, o.max_crown_radius, o.ground_clear};
  for (double v : all)
    if (!finite_d(v)) return false;
  if (!(o.scale > 0.0) || !(o.min_height > 0.0) || !(o.r_min > 0.0) || !(o.max_crown_radius > 0.0)) return false;
  if (o.r_max < o.r_min || o.win_b < 0.0 || o.crown_frac < 0.0 || o.crown_frac > 1.0 || o.ground_clear < 0.0) return false;
  if (o.smooth_passes < 0 || o.smooth_passes > MAX_PASSES || o.max_trees < 1 || o.max_trees > MAX_TREES) return false;
  if (!(c > 0.0) || !finite_d(c)) return false;
  p.scale = o.scale, p.c = c;
  p.min_h = o.min_height / o.scale;
  p.win_a = o.win_a, p.win_b = o.win_b, p.r_min = o.r_min, p.r_max = o.r_max, p.crown_frac = o.crown_frac;
  const double mr = (o.max_crown_radius / o.scale) / c;
  p.mr2 = std::floor(mr * mr);
  p.ground_clear = o.ground_clear / o.scale;
  p.smooth_passes = o.smooth_passes, p.max_trees = o.max_trees;
  if (!finite_d(p.min_h) || !finite_d(p.ground_clear) || !(p.mr2 == p.mr2)) return false;  // (a scale that takes a length out of f64's range)
  return (o.r_max / o.scale) / c <= WINDOW_CAP;  // the window's cap in cells
}

// rule 3: one pass at cell (x, y).  An empty cell stays empty.
SFM_CRN_INLINE float smooth_value(const float* H, int x, int y, int De, int Dn) {
  const float own = H[(size_t)y * De + x];
  if (own != own) return own;
  double S = 0.0, W = 0.0;
  for (int j = 0; j < 9; ++j) {
    const int dx = j % 3 - 1, dy = j / 3 - 1;
    const int xx = x + dx, yy = y + dy;
    if (xx < 0 || yy < 0 || xx >= De || yy >= Dn) continue;
    const float v = H[(size_t)yy * De + xx];
    if (v != v) continue;
    const double k = (double)((dx == 0 ? 2 : 1) * (dy == 0 ? 2 : 1));
    S = S + k * (double)v;
    W = W + k;
  }
  return (float)(S / W);
}

// rule 4
SFM_CRN_INLINE bool is_canopy(float h, double min_h) { return h - h == 0.0f && (double)h >= min_h; }

// rule 5: the key of (ha, a) exceeds that of (hb, b)
SFM_CRN_INLINE bool key_greater(float ha, int a, float hb, int b) { return ha > hb || (ha == hb && a < b); }

// rule 6: up(q) of a canopy cell
SFM_CRN_INLINE int up_of(const float* H, int x, int y, int De, int Dn, double min_h) {
  int best = y * De + x;
  float hb = H[best];
  for (int j = 0; j < 9; ++j) {
    const int xx = x + j % 3 - 1, yy = y + j / 3 - 1;
    if (xx < 0 || yy < 0 || xx >= De || yy >= Dn) continue;
    const int r = yy * De + xx;
    const float v = H[r];
    if (is_canopy(v, min_h) && key_greater(v, r, hb, best)) best = r, hb = v;
  }
  return best;
}

// rule 7: a summit's window
SFM_CRN_INLINE int window_R2(float hs, const Prep& p) {
  const double w = p.win_a + p.win_b * ((double)hs * p.scale);
  const double lo = p.r_min > w ? p.r_min : w;
  const double r = p.r_max < lo ? p.r_max : lo;
  const double rc = (r / p.scale) / p.c;
  const int R2 = (int)floor(rc * rc);
  return R2 > 2 ? R2 : 2;
}
// the largest integer whose square is at most R2 (R2 <= 4096)
SFM_CRN_INLINE int int_radius(int R2) {
  int r = 0;
  while ((r + 1) * (r + 1) <= R2) ++r;
  return r;
}

// rule 9 for a canopy cell (x, y) of height h whose top (tx, ty) has the height ht
SFM_CRN_INLINE bool in_crown(float h, float ht, int x, int y, int tx, int ty, const Prep& p) {
  const long long dx = x - tx, dy = y - ty;
  return (double)h >= p.crown_frac * (double)ht && (double)(dx * dx + dy * dy) <= p.mr2;
}

// rule 10: point i's height lets it belong to a tree
SFM_CRN_INLINE bool above_clear(float hag, double ground_clear) { return hag - hag == 0.0f && (double)hag >= ground_clear; }

// rule 11: a top's row but for its counts
SFM_CRN_INLINE void fill_top(Top& t, int q, int De, float e_min, float n_min, double c, float z, float h, int R2) {
  t.cell_id = q, t.ix = q % De, t.iy = q / De;
  t.e = (double)e_min + ((double)t.ix + 0.5) * c;
  t.n = (double)n_min + ((double)t.iy + 0.5) * c;
  t.height = z, t.height_smooth = h;
  t.R2 = R2;
}
SFM_CRN_INLINE double top_area(int cells, double c) { return (double)cells * (c * c); }

inline void empty_result(Result& r, double c, float e_min, float n_min, int De, int Dn) {
  r.c = c, r.e_min = e_min, r.n_min = n_min, r.De = De, r.Dn = Dn;
  r.n_canopy = r.n_summits = r.n_trees = r.n_labelled_cells = r.n_labelled = r.max_depth = 0;
  r.flags = F_NO_CANOPY;
  r.pad = 0;
}

// ------------------------------------------------------------------------------------------------ host: the whole call
struct HostOut {
  std::vector<float> smooth;     // De Dn: H
  std::vector<int32_t> labels;   // De Dn
  std::vector<int32_t> tree_of;  // n (cloud entry)
  std::vector<Top> tops;         // min(n_trees, max_trees)
  Result res;
};

// rules 2 - 9 and 11 on a host raster.  false: refused.
inline bool run_host_raster(const float* Z, int De, int Dn, double c, float e_min, float n_min, const Opts& o, HostOut& out) {
  Prep p;
  if (De < 0 || Dn < 0 || !prepare(o, c, p)) return false;
  if (!((double)De * (double)Dn <= CELL_CAP)) return false;
  Result& res = out.res;
  empty_result(res, c, e_min, n_min, De, Dn);
  const size_t nc = (size_t)De * Dn;
  out.smooth.assign(Z, Z + nc);
  out.labels.assign(nc, -1);
  out.tops.clear();
  out.tree_of.clear();
  if (nc == 0) return true;
  // rule 3
  std::vector<float>& H = out.smooth;
  std::vector<float> H2(nc);
  for (int s = 0; s < p.smooth_passes; ++s) {
    for (int y = 0; y < Dn; ++y)
      for (int x = 0; x < De; ++x) H2[(size_t)y * De + x] = smooth_value(H.data(), x, y, De, Dn);
    H.swap(H2);
  }
  // rules 4 - 6
  std::vector<int32_t> up(nc, -1), root(nc, -1);
  for (size_t q = 0; q < nc; ++q) {
    if (!is_canopy(H[q], p.min_h)) continue;
    ++res.n_canopy;
    up[q] = up_of(H.data(), (int)(q % De), (int)(q / De), De, Dn, p.min_h);
  }
  if (res.n_canopy == 0) return true;
  res.flags = 0;
  for (size_t q = 0; q < nc; ++q) {
    if (up[q] < 0) continue;
    int r = (int)q;
    while (up[r] != r) r = up[r];
    root[q] = r;
  }
  // rule 7
  std::vector<int32_t> parent(nc, -1), R2s(nc, 0);
  for (size_t s = 0; s < nc; ++s) {
    if (up[s] != (int)s) continue;
    ++res.n_summits;
    const int R2 = R2s[s] = window_R2(H[s], p), rad = int_radius(R2);
    const int sx = (int)(s % De), sy = (int)(s / De);
    int dom = (int)s;
    for (int yy = std::max(sy - rad, 0); yy <= std::min(sy + rad, Dn - 1); ++yy)
      for (int xx = std::max(sx - rad, 0); xx <= std::min(sx + rad, De - 1); ++xx) {
        if ((xx - sx) * (xx - sx) + (yy - sy) * (yy - sy) > R2) continue;
        const int r = yy * De + xx;
        if (is_canopy(H[r], p.min_h) && key_greater(H[r], r, H[dom], dom)) dom = r;
      }
    parent[s] = root[dom];
  }
  // rule 8 (and the longest chain of rule 7)
  std::vector<int32_t> number(nc, -1);
  for (size_t s = 0; s < nc; ++s) {
    if (up[s] != (int)s) continue;
    if (parent[s] == (int)s) {
      if (res.n_trees < p.max_trees) number[s] = res.n_trees;
      ++res.n_trees;
      continue;
    }
    int depth = 0;
    for (int t = (int)s; parent[t] != t; t = parent[t]) ++depth;
    res.max_depth = std::max(res.max_depth, depth);
  }
  if (res.n_trees > p.max_trees) res.flags |= F_OVERFLOW;
  const int kept = std::min(res.n_trees, p.max_trees);
  out.tops.resize((size_t)kept);
  for (size_t s = 0; s < nc; ++s) {
    if (number[s] < 0) continue;
    Top& t = out.tops[(size_t)number[s]];
    fill_top(t, (int)s, De, e_min, n_min, c, Z[s], H[s], R2s[s]);
    t.cells = t.points = 0;
  }
  // rule 9
  for (size_t q = 0; q < nc; ++q) {
    if (root[q] < 0) continue;
    int t = root[q];
    while (parent[t] != t) t = parent[t];
    const int j = number[t];
    if (j < 0) continue;
    if (!in_crown(H[q], H[t], (int)(q % De), (int)(q / De), t % De, t / De, p)) continue;
    out.labels[q] = j;
    ++out.tops[(size_t)j].cells;
    ++res.n_labelled_cells;
  }
  for (Top& t : out.tops) t.area = top_area(t.cells, c);
  return true;
}

// rule 10 after run_host_raster on a terrain call's canopy raster: enh (3 n) and hag (n) are that call's
inline void points_host(int n, const float* enh, const float* hag, const sfmterrain::Dims& d, const Opts& o, HostOut& out) {
  const double clear = o.ground_clear / o.scale;
  out.tree_of.assign((size_t)n, -1);
  const int nc = d.De * d.Dn;
  for (int i = 0; i < n; ++i) {
    const float e = enh[3 * (size_t)i], nn = enh[3 * (size_t)i + 1], h = enh[3 * (size_t)i + 2];
    if (!(h == h) || !above_clear(hag[i], clear)) continue;
    const int q = sfmterrain::cell_of(e, nn, d, out.res.c);
    if (q < 0 || q >= nc) continue;  // (never: the raster was sized by these points)
    const int j = out.labels[(size_t)q];
    if (j < 0) continue;
    out.tree_of[(size_t)i] = j;
    ++out.tops[(size_t)j].points;
    ++out.res.n_labelled;
  }
}

}  // namespace sfmcrowns
