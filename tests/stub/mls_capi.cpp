// mls_capi.cpp -- a C surface over csrc/mls.h for tests/test_mls_cpu.py and tests/test_gpu_mls.py (built with g++ -O2
// -ffp-contract=off -pthread) and, with -DMLS_MAIN, a stand-alone driver that runs the smoothing on clouds of its own under the
// sanitizers.  The neighbour search here is the CPU's own (brute force, or a hash grid of its own cells whose result the
// tests compare with brute force), independent of mls.hip's walk over the radius grid; a point's neighbours are then sorted
// by (M2's key, input index).  Only the key function and the arithmetic come from the shared headers.  Status codes are
// include/sfmhip.h's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <utility>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/mls.h"

namespace {

constexpr int OK = 0, ERR_ARG = -3;

template <typename F>
void parallel(int n, F f) {
  const int T = n < 4096 ? 1 : 16;
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      for (int i = t; i < n; i += T) f(i);
    });
  for (auto& x : th) x.join();
}

bool finite_pt(const float* p) { return sfmcloud::finite3(p[0], p[1], p[2]); }

// M2's grid for radius r over the finite points; returns their count
int geometry(int n, const float* xyz, double r, sfmcloud::GridGeom& g) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  int nv = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!finite_pt(p)) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = nv ? std::min(lo[a], (double)p[a]) : (double)p[a];
      hi[a] = nv ? std::max(hi[a], (double)p[a]) : (double)p[a];
    }
    ++nv;
  }
  sfmcloud::grid_geometry(lo, hi, nv, sfmcloud::radius_cell(r), g);
  return nv;
}

struct HashGrid {  // cells of its own size and origin (0), coordinates clamped: a far point joins a border cell
  double cell = 1;
  std::unordered_map<long long, std::vector<int>> cells;
  static long long pack(long long x, long long y, long long z) {
    return ((x + (1ll << 20)) << 42) | ((y + (1ll << 20)) << 21) | (z + (1ll << 20));
  }
  long long coord(float v) const {
    double f = std::floor((double)v / cell);
    f = std::max(-(double)(1 << 20) + 1, std::min((double)(1 << 20) - 1, f));
    return (long long)f;
  }
  void build(int n, const float* xyz, double c) {
    cell = c;
    for (int i = 0; i < n; ++i) {
      const float* p = xyz + 3 * (size_t)i;
      if (finite_pt(p)) cells[pack(coord(p[0]), coord(p[1]), coord(p[2]))].push_back(i);
    }
  }
};

struct Row {
  float xyz[3], n4[4];
  int status, count;
};

template <int O>
void polynomial(const float* xyz, const std::vector<std::pair<int, int>>& nb, double g, sfmmls::Plane& pl, double q[3], double nrm[3],
                int& status) {
  sfmmls::Fit<O> f;
  sfmmls::fit_zero(f);
  sfmmls::frame(pl);
  for (const auto& kn : nb) {
    const float* x = xyz + 3 * (size_t)kn.second;
    sfmmls::fit_add<O>(f, pl, g, (double)x[0], (double)x[1], (double)x[2]);
  }
  double c[sfmmls::Fit<O>::NC];
  if (sfmmls::fit_solve<O>(f, c)) {
    sfmmls::fit_apply<O>(pl, c, q, nrm);
    status = sfmmls::ST_FIT;
  } else {
    status = sfmmls::ST_FIT_FAILED;
  }
}

// M3 - M5 on the neighbours nb (key, index), sorted
void fit_point(const float* xyz, int i, std::vector<std::pair<int, int>>& nb, int order, double g, Row& row) {
  std::sort(nb.begin(), nb.end());
  row.count = (int)nb.size();
  row.status = sfmmls::ST_DROPPED;
  if (row.count < sfmmls::MIN_NEIGHBOURS) return;
  sfmmls::Accu acc;
  sfmmls::accu_zero(acc);
  for (const auto& kn : nb) {
    const float* x = xyz + 3 * (size_t)kn.second;
    sfmmls::accu_add(acc, (double)x[0], (double)x[1], (double)x[2]);
  }
  const double p[3] = {(double)xyz[3 * (size_t)i], (double)xyz[3 * (size_t)i + 1], (double)xyz[3 * (size_t)i + 2]};
  sfmmls::Plane pl;
  sfmmls::plane_fit(acc, row.count, p, pl);
  if (pl.degenerate) {
    row.status = sfmmls::ST_DEGENERATE;
    sfmmls::write_degenerate(p, row.xyz, row.n4);
    return;
  }
  double q[3] = {pl.q[0], pl.q[1], pl.q[2]}, nrm[3] = {pl.n[0], pl.n[1], pl.n[2]};
  row.status = sfmmls::ST_PLANE;
  if (order > 0) {
    if (row.count < sfmmls::n_coeff(order)) row.status = sfmmls::ST_PLANE_ONLY;
    else if (order == 1) polynomial<1>(xyz, nb, g, pl, q, nrm, row.status);
    else polynomial<2>(xyz, nb, g, pl, q, nrm, row.status);
  }
  sfmmls::write_row(q, nrm, pl.curv, false, row.xyz, row.n4);
}

}  // namespace

extern "C" {

// exp_neg over an array (M6)
void mls_exp(int n, const double* x, double* y) {
  for (int i = 0; i < n; ++i) y[i] = sfmmls::exp_neg(x[i]);
}

// M2's grid for radius r: cell, D[3]; keys[i] = the cell key of point i, -1 for a non-finite point (keys may be NULL)
int mls_grid(int n, const float* xyz, double r, double* cell, int32_t* D, int32_t* keys) {
  sfmcloud::GridGeom g;
  geometry(n, xyz, r, g);
  *cell = g.cell;
  for (int a = 0; a < 3; ++a) D[a] = g.D[a];
  for (int i = 0; keys && i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    keys[i] = finite_pt(p) ? sfmcloud::cell_key(g, p[0], p[1], p[2]) : -1;
  }
  return OK;
}

// sfmhip_cloud_mls without the handle.  search: 0 = brute force up to 2048 points and the hash grid above, 1 = brute force,
// 2 = the hash grid.  stats6: n_out, n_dropped, n_plane_only, n_degenerate, n_fit_failed, max_neighbours (may be NULL, as
// out_xyz, out_n4 and src_index may)
int mls_run(int n, const float* xyz, double radius, int order, int compute_normals, double sqr_gauss, int search, float* out_xyz,
            float* out_n4, int32_t* src_index, int32_t* n_out, int32_t* stats6) {
  if (n < 0 || !n_out || !(radius > 0.0) || !sfmmls::finite_d(radius) || order < 0 || order > 2 || !sfmmls::finite_d(sqr_gauss))
    return ERR_ARG;
  sfmcloud::GridGeom geom;
  geometry(n, xyz, radius, geom);
  const float r2 = sfmcloud::radius2(radius);
  const double g = sfmmls::gauss_param(sqr_gauss, radius);
  std::vector<int> key((size_t)n, -1);
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (finite_pt(p)) key[i] = sfmcloud::cell_key(geom, p[0], p[1], p[2]);
  }
  const bool brute = search == 1 || (search == 0 && n <= 2048);
  HashGrid hg;
  if (!brute) hg.build(n, xyz, radius * 1.01);
  std::vector<Row> rows((size_t)n);
  parallel(n, [&](int i) {
    const float* p = xyz + 3 * (size_t)i;
    rows[i].status = -1;
    rows[i].count = 0;
    if (!finite_pt(p)) return;
    std::vector<std::pair<int, int>> nb;
    auto test = [&](int j) {
      const float* q = xyz + 3 * (size_t)j;
      if (finite_pt(q) && sfmcloud::in_radius(sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]), r2)) nb.emplace_back(key[j], j);
    };
    if (brute) {
      for (int j = 0; j < n; ++j) test(j);
    } else {
      const long long cx = hg.coord(p[0]), cy = hg.coord(p[1]), cz = hg.coord(p[2]);
      for (long long z = cz - 1; z <= cz + 1; ++z)
        for (long long y = cy - 1; y <= cy + 1; ++y)
          for (long long x = cx - 1; x <= cx + 1; ++x) {
            auto it = hg.cells.find(HashGrid::pack(x, y, z));
            if (it == hg.cells.end()) continue;
            for (int j : it->second) test(j);
          }
    }
    fit_point(xyz, i, nb, order, g, rows[i]);
  });
  int32_t st[6] = {0, 0, 0, 0, 0, 0};
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const Row& r = rows[i];
    if (r.status < 0) continue;
    st[5] = std::max(st[5], r.count);
    if (r.status == sfmmls::ST_DROPPED) {
      ++st[1];
      continue;
    }
    st[2] += r.status == sfmmls::ST_PLANE_ONLY;
    st[3] += r.status == sfmmls::ST_DEGENERATE;
    st[4] += r.status == sfmmls::ST_FIT_FAILED;
    for (int a = 0; a < 3 && out_xyz; ++a) out_xyz[3 * (size_t)m + a] = r.xyz[a];
    for (int a = 0; a < 4 && out_n4 && compute_normals; ++a) out_n4[4 * (size_t)m + a] = r.n4[a];
    if (src_index) src_index[m] = i;
    ++m;
  }
  st[0] = m;
  *n_out = m;
  for (int a = 0; a < 6 && stats6; ++a) stats6[a] = st[a];
  return OK;
}

}  // extern "C"

#ifdef MLS_MAIN
// The smoothing on clouds made here: a noisy sheet with NaN and infinite rows at the three orders by both searches, the
// tiny clouds, clusters at the minimum counts and the coefficient edges, one cell of 129 points, identical and collinear
// points, a singular fit, a far outlier, a tiny radius on a wide box, a Gaussian whose far weights underflow, the refusals.
// Prints a digest of each.
namespace {
uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
float unit(uint32_t& s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

int run(const char* name, const std::vector<float>& xyz, double r, int order, double gauss, int search) {
  const int n = (int)(xyz.size() / 3);
  std::vector<float> o3((size_t)3 * n + 3), o4((size_t)4 * n + 4);
  std::vector<int32_t> src((size_t)n + 1);
  int32_t m = -1, st[6];
  const int rc = mls_run(n, xyz.data(), r, order, 1, gauss, search, o3.data(), o4.data(), src.data(), &m, st);
  double sum = 0;
  for (int i = 0; i < 3 * m; ++i) sum += o3[i];
  std::printf("%s: order %d search %d rc %d out %d dropped %d plane_only %d degenerate %d failed %d max %d sum %.9g\n", name, order, search,
              rc, (int)m, (int)st[1], (int)st[2], (int)st[3], (int)st[4], (int)st[5], sum);
  return rc;
}
}  // namespace

int main() {
  uint32_t seed = 11;
  const int n = 5000;
  std::vector<float> sheet((size_t)3 * n);
  for (int i = 0; i < n; ++i) {
    const float x = unit(seed), y = unit(seed);
    sheet[3 * i] = x, sheet[3 * i + 1] = y, sheet[3 * i + 2] = 0.2f * x * x - 0.1f * x * y + 0.004f * (unit(seed) - 0.5f);
    if (i % 97 == 0) sheet[3 * i + (i % 3)] = NAN;
    if (i % 211 == 0) sheet[3 * i + 1] = (i & 1) ? INFINITY : -INFINITY;
  }
  for (int order = 0; order <= 2; ++order)
    for (int search = 1; search <= 2; ++search)
      if (run("sheet", sheet, 0.05, order, 0.0, search) != 0) return 1;
  if (run("gauss", sheet, 0.05, 2, 1e-7, 0) != 0) return 1;
  if (run("tiny radius", sheet, 1e-5, 2, 0.0, 0) != 0) return 1;
  for (int k = 0; k <= 2; ++k)
    if (run("tiny cloud", std::vector<float>(sheet.begin() + 3, sheet.begin() + 3 + 3 * k), 0.5, 2, 0.0, 0) != 0) return 1;
  for (int k : {2, 3, 5, 6, 63, 64, 65, 129}) {
    std::vector<float> c((size_t)3 * k);
    for (int i = 0; i < 3 * k; ++i) c[i] = 0.01f * unit(seed);
    for (int order = 1; order <= 2; ++order)
      if (run("cluster", c, 0.5, order, 0.0, 0) != 0) return 1;
  }
  std::vector<float> same((size_t)3 * 70, 0.25f), line((size_t)3 * 40, 0.0f), sing, far(sheet.begin() + 3, sheet.begin() + 303);
  for (int i = 0; i < 40; ++i) line[3 * i] = 0.01f * (float)i;
  for (int i = -4; i <= 4; ++i) sing.insert(sing.end(), {0.0f, 0.01f * (float)i, 0.0f});  // a cross: u v = 0 at every neighbour of its centre
  for (int i = -4; i <= 4; ++i)
    if (i) sing.insert(sing.end(), {0.01f * (float)i, 0.0f, 0.0f});
  far.insert(far.end(), {1e6f, -1e6f, 3e5f});
  if (run("same", same, 0.1, 2, 0.0, 0) != 0 || run("line", line, 0.1, 2, 0.0, 0) != 0 || run("singular", sing, 1.0, 2, 0.0, 0) != 0 ||
      run("far", far, 0.2, 2, 0.0, 0) != 0)
    return 1;
  int32_t m = 0;
  std::printf("refusals %d %d %d %d %d\n", mls_run(3, sheet.data() + 3, 0.0, 2, 1, 0.0, 0, nullptr, nullptr, nullptr, &m, nullptr),
              mls_run(3, sheet.data() + 3, INFINITY, 2, 1, 0.0, 0, nullptr, nullptr, nullptr, &m, nullptr),
              mls_run(3, sheet.data() + 3, 0.1, 3, 1, 0.0, 0, nullptr, nullptr, nullptr, &m, nullptr),
              mls_run(3, sheet.data() + 3, 0.1, 2, 1, NAN, 0, nullptr, nullptr, nullptr, &m, nullptr),
              mls_run(3, sheet.data() + 3, 0.1, 2, 1, 0.0, 0, nullptr, nullptr, nullptr, nullptr, nullptr));
  std::printf("done\n");
  return 0;
}
#endif
