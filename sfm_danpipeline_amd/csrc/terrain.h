// terrain.h -- the arithmetic of the terrain model (the ground points of a levelled cloud by a progressive
// morphological filter on a raster, the digital terrain model rasterised from them, and every point's height above it) as
// __host__ __device__ code that hipcc and a plain g++ both compile with -ffp-contract=off.  The device code (terrain.hip) and
// the CPU test stub (tests/stub/terrain_capi.cpp) share these bodies, and run_host() at the end is the whole call in plain
// loops: the device result is checked byte for byte against it.  The contract is the rule list of f-20 (copied at the
// declaration in include/sfmhip.h).  Every step is a min, a max or a comparison of float32 or f64 values, or an f64
// expression written in one order.  PARITY UNPINNED: the window and threshold tables are a reading of PCL 1.8.1's
// ApproximateProgressiveMorphologicalFilter from memory.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#include "cloud.h"
#include "dendro.h"  // Frame, make_frame, frame_point (f-11 rules 1 - 3), finite_d
#include "ground.h"  // the ground result the frame comes from

#ifdef __HIPCC__
#define SFM_TER_INLINE __host__ __device__ __forceinline__
#else
#define SFM_TER_INLINE inline __attribute__((always_inline))
#endif

namespace sfmterrain {

using sfmdendro::finite_d;

constexpr int TILE = 64;                  // the width of the opening's LDS tile (terrain.hip): the tests' edge shapes hang on it
constexpr int MAX_WINDOWS = 32;           // rule 5
constexpr int SLOTS = 64;                 // rule 8: slots of a cell's sum = lanes of a wave
constexpr int MAX_FILL = 4096;            // rule 1
constexpr int MAX_RELAX = 1024;           // rule 1
constexpr double CELL_CAP = 16777216.0;   // rule 3: 2^24 cells
constexpr int K_CAP = 1 << 24;            // a half-width beyond any raster axis opens like this one

enum Flags { F_NONE_SELECTED = 1, F_UNFILLED = 2, F_NO_WINDOW = 4 };
enum Kind { K_EMPTY = 0, K_GROUND = 1, K_FILLED = 2 };

struct Opts {  // rule 1 (lengths in metres)
  double up[3], north[3];
  double scale, cell, max_window, slope, initial_distance, max_distance;
  int32_t base, exponential, fill_rounds, relax_sweeps;
};

struct Result {
  double c;                                // the cell in cloud units
  float e_min, n_min, t_min, t_max, hag_max;
  int32_t De, Dn, n_selected, n_ground, n_windows, n_kind1, n_kind2, n_kind0, fill_rounds, flags, pad;
};

struct Prep {  // the options once checked, lengths in cloud units
  sfmdendro::Frame f;
  double c, wmax, slope, d0, dmax;
  int32_t base, exponential, fill_rounds, relax_sweeps;
};

struct Dims {  // rule 3
  float e_min, n_min;
  int32_t De, Dn;
};

struct Windows {  // rule 5: kd the half-widths (integers held in f64, exact below 2^53), k the same capped at K_CAP
  int32_t n, k[MAX_WINDOWS];
  double kd[MAX_WINDOWS], dh[MAX_WINDOWS];
};

SFM_TER_INLINE float pinf() { return sfmcloud::bits_f(0x7F800000u); }
SFM_TER_INLINE float ninf() { return sfmcloud::bits_f(0xFF800000u); }

inline Opts default_opts() {
  Opts o;
  o.up[0] = 0, o.up[1] = 0, o.up[2] = 1;
  o.north[0] = 0, o.north[1] = 1, o.north[2] = 0;
  o.scale = 1.0;
  o.cell = 0.5;
  o.max_window = 9.0;
  o.slope = 1.0;
  o.initial_distance = 0.15;
  o.max_distance = 2.5;
  o.base = 2;
  o.exponential = 1;
  o.fill_rounds = 64;
  o.relax_sweeps = 32;
  return o;
}

// rule 1: the refusals, the frame (f-11 rule 1's) and the lengths in cloud units
inline bool prepare(const Opts& o, Prep& p) {
  sfmdendro::Opts d = sfmdendro::default_opts();
  for (int a = 0; a < 3; ++a) d.up[a] = o.up[a], d.north[a] = o.north[a];
  d.scale = o.scale;
  if (!sfmdendro::make_frame(d, p.f)) return false;
  if (!(o.cell > 0.0) || !(o.initial_distance > 0.0) || !(o.max_distance > 0.0)) return false;
  if (!finite_d(o.cell) || !finite_d(o.initial_distance) || !finite_d(o.max_distance)) return false;
  if (!(o.max_window >= 0.0) || !(o.slope >= 0.0) || !finite_d(o.max_window) || !finite_d(o.slope)) return false;
  if (o.base < 2 || o.fill_rounds < 0 || o.fill_rounds > MAX_FILL || o.relax_sweeps < 0 || o.relax_sweeps > MAX_RELAX) return false;
  p.c = o.cell / o.scale;
  p.wmax = o.max_window / o.scale;
  p.slope = o.slope;
  p.d0 = o.initial_distance / o.scale;
  p.dmax = o.max_distance / o.scale;
  p.base = o.base, p.exponential = o.exponential, p.fill_rounds = o.fill_rounds, p.relax_sweeps = o.relax_sweeps;
  // (a scale that takes a length out of f64's range)
  return p.c > 0.0 && finite_d(p.c) && finite_d(p.wmax) && p.d0 > 0.0 && finite_d(p.d0) && p.dmax > 0.0 && finite_d(p.dmax);
}

// rule 3: the index of x along an axis that starts at `origin` with steps of `c`
SFM_TER_INLINE int axis_index(float x, double origin, double c) { return (int)floor(((double)x - origin) / c); }
inline double axis_count(float x_max, double origin, double c) { return std::floor(((double)x_max - origin) / c) + 1.0; }

// the raster from the float32 minima and maxima of (e, n) over the selection; false: more than 2^24 cells
inline bool make_dims(const Prep& p, const float lo[2], const float hi[2], Dims& d) {
  const double De = axis_count(hi[0], (double)lo[0], p.c), Dn = axis_count(hi[1], (double)lo[1], p.c);
  if (!(De * Dn <= CELL_CAP)) return false;
  d.e_min = lo[0], d.n_min = lo[1];
  d.De = (int32_t)De, d.Dn = (int32_t)Dn;
  return true;
}

SFM_TER_INLINE int cell_of(float e, float n, const Dims& d, double c) {
  return axis_index(n, (double)d.n_min, c) * d.De + axis_index(e, (double)d.e_min, c);
}

// rule 5: the windows and their height thresholds
inline void make_windows(const Prep& p, Windows& w) {
  const double cells = p.wmax / p.c;
  w.n = 0;
  double kd = p.exponential ? 1.0 : (double)p.base;
  for (int i = 0; i < MAX_WINDOWS; ++i) {
    if (!(2.0 * kd + 1.0 <= cells)) break;
    w.kd[i] = kd;
    w.k[i] = kd < (double)K_CAP ? (int32_t)kd : K_CAP;
    if (i == 0) {
      w.dh[i] = p.d0;
    } else {
      const double v = p.slope * ((2.0 * (kd - w.kd[i - 1])) * p.c) + p.d0;
      w.dh[i] = v < p.dmax ? v : p.dmax;
    }
    w.n = i + 1;
    kd = p.exponential ? kd * (double)p.base : (double)(i + 2) * (double)p.base;
  }
}

// rule 7
SFM_TER_INLINE bool below_threshold(float h, float opened, double dh) { return (double)h - (double)opened <= dh; }

// rule 9: what an empty cell takes from its 8 neighbours as they are before the round; false: none of them holds a value
SFM_TER_INLINE bool fill_value(const float* T, const uint8_t* kind, int x, int y, int De, int Dn, float& out) {
  double s = 0.0;
  int m = 0;
  for (int j = 0; j < 8; ++j) {
    const int q = j < 4 ? j : j + 1;  // (dx fastest, the centre left out)
    const int xx = x + q % 3 - 1, yy = y + q / 3 - 1;
    if (xx < 0 || yy < 0 || xx >= De || yy >= Dn) continue;
    const int r = yy * De + xx;
    if (kind[r] == K_EMPTY) continue;
    s = s + (double)T[r];
    ++m;
  }
  if (m == 0) return false;
  out = (float)(s / (double)m);
  return true;
}

// rule 10: one Jacobi step of a filled cell
SFM_TER_INLINE float relax_value(const float* T, const uint8_t* kind, int x, int y, int De, int Dn) {
  const int q = y * De + x;
  const double own = (double)T[q];
  const double W = x > 0 && kind[q - 1] != K_EMPTY ? (double)T[q - 1] : own;
  const double E = x + 1 < De && kind[q + 1] != K_EMPTY ? (double)T[q + 1] : own;
  const double S = y > 0 && kind[q - De] != K_EMPTY ? (double)T[q - De] : own;
  const double N = y + 1 < Dn && kind[q + De] != K_EMPTY ? (double)T[q + De] : own;
  return (float)(((W + E) + (S + N)) / 4.0);
}

// rule 11: the stencil along one axis
SFM_TER_INLINE void stencil(float x, double origin, double c, int D, int& i0, int& i1, double& f) {
  const double u = ((double)x - origin) / c - 0.5;
  double fl = floor(u);
  fl = fl < 0.0 ? 0.0 : fl;
  fl = fl > (double)(D - 1) ? (double)(D - 1) : fl;
  i0 = (int)fl;
  i1 = i0 + 1 < D ? i0 + 1 : D - 1;
  double t = u - fl;
  t = t < 0.0 ? 0.0 : t;
  f = t > 1.0 ? 1.0 : t;
}
// the height above the terrain of a selected point (e, n, h) in cell q
SFM_TER_INLINE float height_above(float e, float n, float h, int q, const Dims& d, double c, const float* T, const uint8_t* kind) {
  if (kind[q] == K_EMPTY) return sfmcloud::qnan();
  int x0, x1, y0, y1;
  double fx, fy;
  stencil(e, (double)d.e_min, c, d.De, x0, x1, fx);
  stencil(n, (double)d.n_min, c, d.Dn, y0, y1, fy);
  const int i00 = y0 * d.De + x0, i01 = y0 * d.De + x1, i10 = y1 * d.De + x0, i11 = y1 * d.De + x1;
  const double own = (double)T[q];
  const double T00 = kind[i00] != K_EMPTY ? (double)T[i00] : own, T01 = kind[i01] != K_EMPTY ? (double)T[i01] : own;
  const double T10 = kind[i10] != K_EMPTY ? (double)T[i10] : own, T11 = kind[i11] != K_EMPTY ? (double)T[i11] : own;
  const double g = ((T00 * (1.0 - fx) + T01 * fx) * (1.0 - fy)) + ((T10 * (1.0 - fx) + T11 * fx) * fy);
  return (float)((double)h - g);
}

inline void empty_result(Result& r, const Prep& p, int flags) {
  r.c = p.c;
  r.e_min = r.n_min = 0.0f;
  r.t_min = r.t_max = r.hag_max = sfmcloud::qnan();
  r.De = r.Dn = r.n_selected = r.n_ground = r.n_windows = r.n_kind1 = r.n_kind2 = r.n_kind0 = r.fill_rounds = 0;
  r.flags = flags;
  r.pad = 0;
}

// the hand-over from ground.h: up and north.  false: the result has no plane.
inline bool opts_from_ground(const sfmground::Result& g, Opts& io) {
  if (g.winner < 0) return false;
  for (int a = 0; a < 3; ++a) {
    io.up[a] = g.up[a];
    io.north[a] = g.north[a];
  }
  return true;
}

// what the last sfmhip_cloud_terrain call left on a handle, for the stages after it (crowns.hip): device pointers to the canopy
// raster (De Dn cells; null when nothing was selected), the frame coordinates (3 n) and the heights above ground (n), the
// raster and the cell.  Defined in terrain.hip; false: no call yet (or the last one was refused).
struct LastCall {
  const float *chm, *enh, *hag;
  Dims d;
  double c;
  int32_t n;
};
}  // namespace sfmterrain
struct sfmhip_cloud;
namespace sfmterrain {
bool last_call(sfmhip_cloud* c, LastCall& out);

// ------------------------------------------------------------------------------------------------ host: the whole call
// one pass of rule 6 along the lines of a raster (stride `step` between a line's elements): the least (or largest) value within
// k of each element, the window clipped at the line's ends.  Empty cells are +inf in `in` and in `out`.
inline void line_pass(const float* in, float* out, int L, int step, int k, bool largest) {
  k = std::min(k, L - 1);
  for (int x = 0; x < L; ++x) {
    float best = largest ? ninf() : pinf();
    for (int xx = std::max(x - k, 0); xx <= std::min(x + k, L - 1); ++xx) {
      float v = in[(size_t)xx * step];
      if (largest && v == pinf()) v = ninf();
      best = largest ? (v > best ? v : best) : (v < best ? v : best);
    }
    out[(size_t)x * step] = best == ninf() ? pinf() : best;
  }
}
// rule 6: the opening of Z (De x Dn, +inf for an empty cell) by the window of half-width k
inline void open_host(const std::vector<float>& Z, int De, int Dn, int k, std::vector<float>& O) {
  std::vector<float> a(Z.size()), b(Z.size());
  for (int y = 0; y < Dn; ++y) line_pass(&Z[(size_t)y * De], &a[(size_t)y * De], De, 1, k, false);
  for (int x = 0; x < De; ++x) line_pass(&a[x], &b[x], Dn, De, k, false);
  for (int y = 0; y < Dn; ++y) line_pass(&b[(size_t)y * De], &a[(size_t)y * De], De, 1, k, true);
  O.resize(Z.size());
  for (int x = 0; x < De; ++x) line_pass(&a[x], &O[x], Dn, De, k, true);
}

struct HostOut {  // per point: is_ground, hag, norm (3 each); per cell: T, kind, chm
  std::vector<int32_t> is_ground;
  std::vector<float> hag, norm, T, chm;
  std::vector<uint8_t> kind;
  Result res;
};

// the whole call on the host.  false: the options are refused, or the raster exceeds its cap.
inline bool run_host(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts& o, HostOut& out) {
  Prep p;
  if (!prepare(o, p)) return false;
  Result& res = out.res;
  empty_result(res, p, F_NONE_SELECTED);
  out.is_ground.assign((size_t)n, 0);
  out.hag.assign((size_t)n, sfmcloud::qnan());
  out.norm.assign((size_t)3 * n, sfmcloud::qnan());
  out.T.clear(), out.chm.clear(), out.kind.clear();
  // rule 2
  std::vector<float> enh((size_t)3 * std::max(n, 1));
  std::vector<char> sel((size_t)std::max(n, 1), 0);
  uint32_t klo[2] = {0xFFFFFFFFu, 0xFFFFFFFFu}, khi[2] = {0u, 0u};
  for (int i = 0; i < n; ++i) {
    sel[i] = sfmdendro::frame_point(p.f, xyz + 3 * (size_t)i, !labels || labels[i] == label, &enh[3 * (size_t)i]);
    if (!sel[i]) continue;
    ++res.n_selected;
    for (int a = 0; a < 2; ++a) {
      const uint32_t key = sfmcloud::ord_key(enh[3 * (size_t)i + a]);
      klo[a] = key < klo[a] ? key : klo[a];
      khi[a] = key > khi[a] ? key : khi[a];
    }
  }
  if (res.n_selected == 0) return true;
  res.flags = 0;
  // rule 3
  float lo[2], hi[2];
  for (int a = 0; a < 2; ++a) lo[a] = sfmcloud::ord_val(klo[a]), hi[a] = sfmcloud::ord_val(khi[a]);
  Dims d;
  if (!make_dims(p, lo, hi, d)) return false;
  res.e_min = d.e_min, res.n_min = d.n_min, res.De = d.De, res.Dn = d.Dn;
  const size_t nc = (size_t)d.De * d.Dn;
  std::vector<int32_t> cell((size_t)n, -1);
  // rule 4
  std::vector<float> Z(nc, pinf());
  std::vector<int32_t> start(nc + 1, 0), run((size_t)res.n_selected);  // a cell's run: its selected points in ascending input index
  for (int i = 0; i < n; ++i) {
    if (!sel[i]) continue;
    const int q = cell[i] = cell_of(enh[3 * (size_t)i], enh[3 * (size_t)i + 1], d, p.c);
    ++start[q + 1];
    const float h = enh[3 * (size_t)i + 2];
    Z[q] = h < Z[q] ? h : Z[q];
  }
  for (size_t q = 0; q < nc; ++q) start[q + 1] += start[q];
  {
    std::vector<int32_t> at(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i)
      if (sel[i]) run[at[cell[i]]++] = i;
  }
  // rules 5 - 7
  Windows w;
  make_windows(p, w);
  res.n_windows = w.n;
  if (w.n == 0) res.flags |= F_NO_WINDOW;
  for (int i = 0; i < n; ++i) out.is_ground[i] = sel[i] ? 1 : 0;
  std::vector<float> O;
  for (int i = 0; i < w.n; ++i) {
    open_host(Z, d.De, d.Dn, w.k[i], O);
    for (int j = 0; j < n; ++j)
      if (sel[j] && !below_threshold(enh[3 * (size_t)j + 2], O[cell[j]], w.dh[i])) out.is_ground[j] = 0;
    Z.swap(O);
  }
  // rule 8
  std::vector<float> T(nc, sfmcloud::qnan()), T2(nc);
  std::vector<uint8_t> kind(nc, K_EMPTY), kind2(nc);
  for (size_t q = 0; q < nc; ++q) {
    if (start[q + 1] == start[q]) continue;
    double slot[SLOTS];
    for (int s = 0; s < SLOTS; ++s) slot[s] = 0.0;
    int m = 0;
    for (int j = 0; j < start[q + 1] - start[q]; ++j) {
      const int i = run[start[q] + j];
      if (!out.is_ground[i]) continue;
      slot[j % SLOTS] = slot[j % SLOTS] + (double)enh[3 * (size_t)i + 2];
      ++m;
    }
    if (m == 0) continue;
    for (int stride = SLOTS / 2; stride >= 1; stride >>= 1)
      for (int s = 0; s < stride; ++s) slot[s] = slot[s] + slot[s + stride];
    T[q] = (float)(slot[0] / (double)m);
    kind[q] = K_GROUND;
    res.n_ground += m;
  }
  // rule 9
  for (int r = 1; r <= p.fill_rounds; ++r) {
    int filled = 0;
    for (int y = 0; y < d.Dn; ++y)
      for (int x = 0; x < d.De; ++x) {
        const size_t q = (size_t)y * d.De + x;
        T2[q] = T[q], kind2[q] = kind[q];
        float v;
        if (kind[q] == K_EMPTY && fill_value(T.data(), kind.data(), x, y, d.De, d.Dn, v)) T2[q] = v, kind2[q] = K_FILLED, ++filled;
      }
    T.swap(T2), kind.swap(kind2);
    res.fill_rounds = r;
    if (!filled) break;
  }
  // rule 10
  for (int s = 0; s < p.relax_sweeps; ++s) {
    for (int y = 0; y < d.Dn; ++y)
      for (int x = 0; x < d.De; ++x) {
        const size_t q = (size_t)y * d.De + x;
        T2[q] = kind[q] == K_FILLED ? relax_value(T.data(), kind.data(), x, y, d.De, d.Dn) : T[q];
      }
    T.swap(T2);
  }
  uint32_t tlo = 0xFFFFFFFFu, thi = 0u;
  for (size_t q = 0; q < nc; ++q) {
    res.n_kind1 += kind[q] == K_GROUND, res.n_kind2 += kind[q] == K_FILLED, res.n_kind0 += kind[q] == K_EMPTY;
    if (kind[q] == K_EMPTY) continue;
    const uint32_t key = sfmcloud::ord_key(T[q]);
    tlo = key < tlo ? key : tlo, thi = key > thi ? key : thi;
  }
  if (res.n_kind0) res.flags |= F_UNFILLED;
  if (thi) res.t_min = sfmcloud::ord_val(tlo), res.t_max = sfmcloud::ord_val(thi);
  // rules 11 - 13
  std::vector<uint32_t> ckey(nc, 0u);
  uint32_t hmax = 0u;
  for (int i = 0; i < n; ++i) {
    if (!sel[i]) continue;
    const float e = enh[3 * (size_t)i], nn = enh[3 * (size_t)i + 1], h = enh[3 * (size_t)i + 2];
    const float g = height_above(e, nn, h, cell[i], d, p.c, T.data(), kind.data());
    out.hag[i] = g;
    if (!(g - g == 0.0f)) continue;
    out.norm[3 * (size_t)i] = e, out.norm[3 * (size_t)i + 1] = nn, out.norm[3 * (size_t)i + 2] = g;
    const uint32_t key = sfmcloud::ord_key(g);
    ckey[cell[i]] = key > ckey[cell[i]] ? key : ckey[cell[i]];
    hmax = key > hmax ? key : hmax;
  }
  out.chm.resize(nc);
  for (size_t q = 0; q < nc; ++q) out.chm[q] = ckey[q] ? sfmcloud::ord_val(ckey[q]) : sfmcloud::qnan();
  if (hmax) res.hag_max = sfmcloud::ord_val(hmax);
  out.T.swap(T), out.kind.swap(kind);
  return true;
}

}  // namespace sfmterrain
