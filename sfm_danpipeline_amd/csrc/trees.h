// trees.h -- the arithmetic of the individual-tree extraction (from the levelled cloud, the stems in a
// height band and, for every point above the ground, the number of the tree it belongs to) as __host__ __device__ code that
// hipcc and a plain g++ both compile with -ffp-contract=off.  The device code (trees.hip) and the CPU test stub
// (tests/stub/trees_capi.cpp) share these bodies, and run_host() at the end is the whole call in plain loops: the device
// result is checked byte for byte against it.  There is no reference implementation; the contract is the rule list of f-13
// (copied at the declaration in include/sfmhip.h).  Every result is an integer or an f64 expression of integers written in
// one order, and none depends on the order of evaluation: counts, minima of integer keys, the unique fixed point of rule 8.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <queue>
#include <vector>
#include "cloud.h"
#include "dendro.h"  // Frame, make_frame, frame_point (f-11 rules 1 - 3), finite_d, parallel_for
#include "ground.h"  // the ground result the frame comes from

#ifdef __HIPCC__
#define SFM_TRS_INLINE __host__ __device__ __forceinline__
#else
#define SFM_TRS_INLINE inline __attribute__((always_inline))
#endif

namespace sfmtrees {

using sfmdendro::finite_d;

constexpr int MAX_TREES = 4096;               // rule 1
constexpr double CELL_CAP = 16777216.0;       // rule 4: 2^24 stem cells
constexpr double VOXEL_CAP = 2147483648.0;    // rule 6: 2^31 voxels
constexpr int STEPS = 26;                     // rule 6: the 26-neighbourhood
constexpr unsigned long long UNREACHED = ~0ull;

enum Flags { F_NONE_ABOVE = 1, F_NO_STEM = 2, F_MAX_TREES = 4 };
enum Class { C_OUT = 0, C_BELOW = 1, C_ABOVE = 2, C_BAND = 3 };  // not selected; selected; in A; in B (and in A)

struct Opts {  // rule 1 (lengths in metres)
  double up[3], north[3];
  double scale, ground, ground_clear, band_lo, band_hi, stem_cell, max_stem_width, voxel, max_path;
  int32_t min_cell_pts, min_stem_pts, max_trees, pad;
};

struct Stem {  // one row of the stem table (cloud units)
  double e, n, foot[3];
  int32_t cell_id, band_points, band_cells, points;
};

struct Result {
  int32_t n_selected, n_above, n_band, n_trees, n_voxels, n_labelled, max_cost, flags;
};

struct Prep {  // the options once checked, lengths in cloud units
  sfmdendro::Frame f;
  double h0, clear, lo, hi, c, w, v, cap;  // cap: the largest cost a labelled voxel may have (rule 8), -1 for none
};

struct Dims {  // rules 4 and 6: the origins and the sizes of the two grids
  float e_min, n_min;
  int32_t De, Dn, Dx, Dy, Dz, pad;
};

struct StemSums {  // rule 5: what a component adds up to, all integers
  long long Se, Sn, N;
  int32_t cells, cell_id;
};

inline Opts default_opts() {
  Opts o;
  o.up[0] = 0, o.up[1] = 0, o.up[2] = 1;
  o.north[0] = 0, o.north[1] = 1, o.north[2] = 0;
  o.scale = 1.0;
  o.ground = sfmdendro::dnan();  // required: the caller sets it
  o.ground_clear = 0.3;
  o.band_lo = 1.0;
  o.band_hi = 1.6;
  o.stem_cell = 0.05;
  o.max_stem_width = 1.5;
  o.voxel = 0.15;
  o.max_path = 0.0;
  o.min_cell_pts = 2;
  o.min_stem_pts = 30;
  o.max_trees = MAX_TREES;
  o.pad = 0;
  return o;
}

// rule 1: the refusals, the frame (f-11 rule 1's) and the lengths in cloud units
inline bool prepare(const Opts& o, Prep& p) {
  sfmdendro::Opts d = sfmdendro::default_opts();
  for (int a = 0; a < 3; ++a) d.up[a] = o.up[a], d.north[a] = o.north[a];
  d.scale = o.scale;
  if (!sfmdendro::make_frame(d, p.f)) return false;
  if (!finite_d(o.ground)) return false;
  if (!(o.ground_clear >= 0.0) || !(o.band_lo >= o.ground_clear) || !(o.band_hi > o.band_lo) || !finite_d(o.band_hi)) return false;
  if (!(o.stem_cell > 0.0) || !(o.voxel > 0.0) || !(o.max_stem_width > 0.0) || !(o.max_path >= 0.0)) return false;
  if (!finite_d(o.stem_cell) || !finite_d(o.voxel) || !finite_d(o.max_stem_width) || !finite_d(o.max_path)) return false;
  if (o.min_cell_pts < 1 || o.min_stem_pts < 1 || o.max_trees < 1 || o.max_trees > MAX_TREES) return false;
  p.h0 = o.ground / o.scale;
  p.clear = o.ground_clear / o.scale;
  p.lo = o.band_lo / o.scale;
  p.hi = o.band_hi / o.scale;
  p.c = o.stem_cell / o.scale;
  p.w = o.max_stem_width / o.scale;
  p.v = o.voxel / o.scale;
  p.cap = o.max_path > 0.0 ? std::floor(10.0 * (o.max_path / o.scale) / p.v) : -1.0;
  // (a scale that takes a length out of f64's range)
  return finite_d(p.h0) && finite_d(p.hi) && p.c > 0.0 && finite_d(p.c) && p.v > 0.0 && finite_d(p.v) && p.w > 0.0 && finite_d(p.w) && finite_d(p.cap);
}

// rule 3
SFM_TRS_INLINE int classify(bool selected, float h, double h0, double clear, double lo, double hi) {
  if (!selected) return C_OUT;
  const double d = (double)h - h0;
  if (!(d >= clear)) return C_BELOW;
  return d >= lo && d < hi ? C_BAND : C_ABOVE;
}

// rules 4 and 6: the index of x along an axis that starts at `origin` with steps of `step`
SFM_TRS_INLINE int axis_index(float x, double origin, double step) { return (int)floor(((double)x - origin) / step); }
inline double axis_count(float x_max, double origin, double step) { return std::floor(((double)x_max - origin) / step) + 1.0; }

// the sizes from the float32 minima and maxima of (e, n, h) over A; false: a cap is exceeded (rules 4 and 6)
inline bool make_dims(const Prep& p, const float lo[3], const float hi[3], Dims& d) {
  const double De = axis_count(hi[0], (double)lo[0], p.c), Dn = axis_count(hi[1], (double)lo[1], p.c);
  if (!(De * Dn <= CELL_CAP)) return false;
  const double Dx = axis_count(hi[0], (double)lo[0], p.v), Dy = axis_count(hi[1], (double)lo[1], p.v), Dz = axis_count(hi[2], p.h0, p.v);
  if (!((Dx * Dy) * Dz < VOXEL_CAP)) return false;
  d.e_min = lo[0], d.n_min = lo[1];
  d.De = (int32_t)De, d.Dn = (int32_t)Dn, d.Dx = (int32_t)Dx, d.Dy = (int32_t)Dy, d.Dz = (int32_t)Dz;
  d.pad = 0;
  return true;
}

SFM_TRS_INLINE int cell_of(const float enh[3], const Dims& d, double c) {
  return axis_index(enh[1], (double)d.n_min, c) * d.De + axis_index(enh[0], (double)d.e_min, c);
}
SFM_TRS_INLINE int voxel_of(const float enh[3], const Dims& d, double h0, double v) {
  const int vx = axis_index(enh[0], (double)d.e_min, v), vy = axis_index(enh[1], (double)d.n_min, v), vz = axis_index(enh[2], h0, v);
  return (vz * d.Dy + vy) * d.Dx + vx;
}

// rule 5: a component of N band points in the cell box [x0, x1] x [y0, y1]
SFM_TRS_INLINE bool is_stem(long long N, int x0, int x1, int y0, int y1, int min_stem_pts, double c, double w) {
  return N >= (long long)min_stem_pts && (double)(x1 - x0 + 1) * c <= w && (double)(y1 - y0 + 1) * c <= w;
}
inline void stem_row(const StemSums& s, const Prep& p, const Dims& d, Stem& r) {
  r.e = (double)d.e_min + (p.c * (double)s.Se) / (double)(2 * s.N);
  r.n = (double)d.n_min + (p.c * (double)s.Sn) / (double)(2 * s.N);
  for (int a = 0; a < 3; ++a) r.foot[a] = (r.e * p.f.east[a] + r.n * p.f.north[a]) + p.h0 * p.f.up[a];
  r.cell_id = s.cell_id;
  r.band_points = (int32_t)s.N;
  r.band_cells = s.cells;
  r.points = 0;
}

// rule 6: step k of the 26 (dz slowest, dx fastest, the centre left out) and its weight
SFM_TRS_INLINE void step_delta(int k, int& dx, int& dy, int& dz) {
  const int q = k < 13 ? k : k + 1;
  dx = q % 3 - 1;
  dy = (q / 3) % 3 - 1;
  dz = q / 9 - 1;
}
SFM_TRS_INLINE int step_weight(int k) {
  int dx, dy, dz;
  step_delta(k, dx, dy, dz);
  const int m = (dx != 0) + (dy != 0) + (dz != 0);
  return m == 1 ? 10 : (m == 2 ? 14 : 17);
}
// the key of voxel `key`'s neighbour along step k, -1 outside the grid
SFM_TRS_INLINE int neighbour_key(int key, int k, const Dims& d) {
  int dx, dy, dz;
  step_delta(k, dx, dy, dz);
  const int x = key % d.Dx + dx, y = (key / d.Dx) % d.Dy + dy, z = key / (d.Dx * d.Dy) + dz;
  if (x < 0 || y < 0 || z < 0 || x >= d.Dx || y >= d.Dy || z >= d.Dz) return -1;
  return (z * d.Dy + y) * d.Dx + x;
}
// the position of `key` in the ascending list of the occupied voxels' keys, -1 when it is not there
SFM_TRS_INLINE int find_voxel(const int* keys, int n, int key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo < n && keys[lo] == key ? lo : -1;
}

// rule 8: key = cost << 16 | stem; one relaxation along an edge of weight w
SFM_TRS_INLINE unsigned long long relax(unsigned long long key_u, int w) { return key_u == UNREACHED ? UNREACHED : key_u + ((unsigned long long)w << 16); }
SFM_TRS_INLINE long long key_cost(unsigned long long key) { return (long long)(key >> 16); }
SFM_TRS_INLINE int key_stem(unsigned long long key) { return (int)(key & 0xFFFFull); }
// the tree of a voxel from its final key (-1: no seed reaches it, or only further than max_path)
SFM_TRS_INLINE int voxel_tree(unsigned long long key, double cap) {
  if (key == UNREACHED) return -1;
  if (cap >= 0.0 && (double)key_cost(key) > cap) return -1;
  return key_stem(key);
}

inline void empty_result(Result& r, int flags) {
  r.n_selected = r.n_above = r.n_band = r.n_trees = r.n_voxels = r.n_labelled = r.max_cost = 0;
  r.flags = flags;
}

// the hand-over from ground.h: up, north and ground = offset * scale (metres).  false: the result has no plane, or no scale.
inline bool opts_from_ground(const sfmground::Result& g, Opts& io) {
  if (g.winner < 0 || !(io.scale > 0.0) || !finite_d(io.scale)) return false;
  for (int a = 0; a < 3; ++a) {
    io.up[a] = g.up[a];
    io.north[a] = g.north[a];
  }
  io.ground = g.offset * io.scale;
  return true;
}

// ------------------------------------------------------------------------------------------------ host: the whole call
// rule 5 on the host: the least cell id of each occupied cell's 8-connected component (-1: not occupied)
inline void components(const std::vector<int32_t>& count, int De, int Dn, int min_cell_pts, std::vector<int32_t>& root) {
  const size_t nc = (size_t)De * Dn;
  root.assign(nc, -1);
  std::vector<int32_t> stack;
  for (size_t c0 = 0; c0 < nc; ++c0) {
    if (count[c0] < min_cell_pts || root[c0] >= 0) continue;
    root[c0] = (int32_t)c0;  // (ascending scan: the first cell met is the component's least id)
    stack.push_back((int32_t)c0);
    while (!stack.empty()) {
      const int32_t c = stack.back();
      stack.pop_back();
      const int x = c % De, y = c / De;
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          const int xx = x + dx, yy = y + dy;
          if (xx < 0 || yy < 0 || xx >= De || yy >= Dn) continue;
          const int32_t q = yy * De + xx;
          if (count[q] < min_cell_pts || root[q] >= 0) continue;
          root[q] = (int32_t)c0;
          stack.push_back(q);
        }
    }
  }
}

// the whole call on the host.  false: the options are refused, or a grid cap is exceeded.  tree_of: n entries; stems: the
// first min(cap, T) rows are written.
inline bool run_host(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts& o, int threads, int32_t* tree_of, int cap,
                     Stem* stems, Result& res) {
  Prep p;
  if (!prepare(o, p)) return false;
  empty_result(res, F_NONE_ABOVE);
  // rules 2, 3
  std::vector<float> enh((size_t)3 * std::max(n, 1));
  std::vector<signed char> cls((size_t)std::max(n, 1), C_OUT);
  sfmdendro::parallel_for(n, threads, [&](int i) {
    const bool sel = sfmdendro::frame_point(p.f, xyz + 3 * (size_t)i, !labels || labels[i] == label, &enh[3 * (size_t)i]);
    cls[i] = (signed char)classify(sel, enh[3 * (size_t)i + 2], p.h0, p.clear, p.lo, p.hi);
  });
  uint32_t klo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, khi[3] = {0u, 0u, 0u};
  for (int i = 0; i < n; ++i) {
    tree_of[i] = -1;
    res.n_selected += cls[i] != C_OUT;
    res.n_band += cls[i] == C_BAND;
    if (cls[i] < C_ABOVE) continue;
    ++res.n_above;
    for (int a = 0; a < 3; ++a) {
      const uint32_t key = sfmcloud::ord_key(enh[3 * (size_t)i + a]);
      klo[a] = key < klo[a] ? key : klo[a];
      khi[a] = key > khi[a] ? key : khi[a];
    }
  }
  if (res.n_above == 0) return true;
  res.flags = 0;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = sfmcloud::ord_val(klo[a]), hi[a] = sfmcloud::ord_val(khi[a]);
  Dims d;
  if (!make_dims(p, lo, hi, d)) return false;
  // rules 4, 5
  std::vector<int32_t> count((size_t)d.De * d.Dn, 0), root;
  for (int i = 0; i < n; ++i)
    if (cls[i] == C_BAND) ++count[cell_of(&enh[3 * (size_t)i], d, p.c)];
  components(count, d.De, d.Dn, o.min_cell_pts, root);
  struct Comp {
    StemSums s;
    int x0, x1, y0, y1;
  };
  std::vector<Comp> comps;  // in ascending component id
  std::vector<int32_t> comp_of(count.size(), -1), stem_of(count.size(), -1);  // by root cell
  for (size_t q = 0; q < count.size(); ++q) {
    if (root[q] < 0) continue;
    const int x = (int)(q % d.De), y = (int)(q / d.De);
    if (root[q] == (int32_t)q) {
      comp_of[q] = (int32_t)comps.size();
      comps.push_back(Comp{{0, 0, 0, 0, (int32_t)q}, x, x, y, y});
    }
    Comp& k = comps[comp_of[root[q]]];
    k.s.Se += (long long)count[q] * (2 * x + 1);
    k.s.Sn += (long long)count[q] * (2 * y + 1);
    k.s.N += count[q];
    ++k.s.cells;
    k.x0 = std::min(k.x0, x), k.x1 = std::max(k.x1, x), k.y0 = std::min(k.y0, y), k.y1 = std::max(k.y1, y);
  }
  std::vector<StemSums> sums;
  int T_all = 0;
  for (const Comp& k : comps) {
    if (!is_stem(k.s.N, k.x0, k.x1, k.y0, k.y1, o.min_stem_pts, p.c, p.w)) continue;
    if (T_all < o.max_trees) {
      stem_of[k.s.cell_id] = T_all;
      sums.push_back(k.s);
    }
    ++T_all;
  }
  const int T = (int)sums.size();
  if (T_all > T) res.flags |= F_MAX_TREES;
  res.n_trees = T;
  if (T == 0) {
    res.flags |= F_NO_STEM;
    return true;
  }
  // rule 6: the occupied voxels in ascending key order
  std::vector<int32_t> vkey((size_t)n, -1);
  std::vector<int32_t> keys;
  for (int i = 0; i < n; ++i)
    if (cls[i] >= C_ABOVE) keys.push_back(vkey[i] = voxel_of(&enh[3 * (size_t)i], d, p.h0, p.v));
  std::sort(keys.begin(), keys.end());
  keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
  const int nv = (int)keys.size();
  res.n_voxels = nv;
  std::vector<int32_t> pvox((size_t)n, -1), vpts((size_t)nv, 0);
  std::vector<unsigned long long> key((size_t)nv, UNREACHED);
  // rule 7
  for (int i = 0; i < n; ++i) {
    if (cls[i] < C_ABOVE) continue;
    const int v = pvox[i] = find_voxel(keys.data(), nv, vkey[i]);
    ++vpts[v];
    if (cls[i] != C_BAND) continue;
    const int32_t r = root[cell_of(&enh[3 * (size_t)i], d, p.c)];
    if (r >= 0 && stem_of[r] >= 0) key[v] = std::min(key[v], (unsigned long long)stem_of[r]);
  }
  // rule 8: the fixed point, reached in ascending key order (Dijkstra on the 64-bit keys: an edge only adds to a key)
  typedef std::pair<unsigned long long, int> QE;
  std::priority_queue<QE, std::vector<QE>, std::greater<QE>> q;
  for (int v = 0; v < nv; ++v)
    if (key[v] != UNREACHED) q.push(QE(key[v], v));
  while (!q.empty()) {
    const QE top = q.top();
    q.pop();
    if (top.first != key[top.second]) continue;
    for (int k = 0; k < STEPS; ++k) {
      const int nk = neighbour_key(keys[top.second], k, d);
      const int u = nk < 0 ? -1 : find_voxel(keys.data(), nv, nk);
      if (u < 0) continue;
      const unsigned long long cand = relax(top.first, step_weight(k));
      if (cand < key[u]) {
        key[u] = cand;
        q.push(QE(cand, u));
      }
    }
  }
  // rule 9
  std::vector<int32_t> pts((size_t)T, 0);
  long long max_cost = 0;
  for (int v = 0; v < nv; ++v) {
    const int s = voxel_tree(key[v], p.cap);
    if (s < 0) continue;
    pts[s] += vpts[v];
    res.n_labelled += vpts[v];
    max_cost = std::max(max_cost, key_cost(key[v]));
  }
  res.max_cost = (int32_t)max_cost;
  for (int i = 0; i < n; ++i)
    if (pvox[i] >= 0) tree_of[i] = voxel_tree(key[pvox[i]], p.cap);
  for (int s = 0; s < T && s < cap; ++s) {
    stem_row(sums[s], p, d, stems[s]);
    stems[s].points = pts[s];
  }
  return true;
}

}  // namespace sfmtrees
