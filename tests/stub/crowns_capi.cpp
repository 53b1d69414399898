// crowns_capi.cpp -- a C surface over csrc/crowns.h for tests/test_crowns_cpu.py and tests/test_gpu_crowns.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off -pthread): the whole call in the header's plain loops (run_host_raster, points_host), the
// pieces the rule cases look at one by one, and, with -DCROWNS_MAIN, a driver that runs rasters of its own making under the
// sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/crowns.h"

using namespace sfmcrowns;

static HostOut g_last;  // the last crn_run that was not refused, for crn_points

extern "C" {

void crn_default_opts(Opts* o) { *o = default_opts(); }
int crn_sizes(int* opts, int* top, int* result) {
  *opts = (int)sizeof(Opts);
  *top = (int)sizeof(Top);
  *result = (int)sizeof(Result);
  return 0;
}
int crn_tile() { return TILE; }
int crn_batch() { return BATCH; }

// 0: done; 1: refused.  labels, smooth: De Dn entries; tops: cap rows, of which min(cap, n_trees, max_trees) are written.
int crn_run(const float* Z, int De, int Dn, double c, float e_min, float n_min, const Opts* o, int32_t* labels, float* smooth, int cap,
            Top* tops, Result* res) {
  if (!run_host_raster(Z, De, Dn, c, e_min, n_min, *o, g_last)) return 1;
  for (size_t q = 0; q < g_last.labels.size(); ++q) labels[q] = g_last.labels[q], smooth[q] = g_last.smooth[q];
  for (size_t j = 0; j < g_last.tops.size() && (int)j < cap; ++j) tops[j] = g_last.tops[j];
  *res = g_last.res;
  return 0;
}

// rule 10 on the last crn_run, whose raster was a terrain call's canopy: enh (3 n; the normalised cloud serves) and hag (n) are
// that call's, (e_min, n_min, De, Dn) its raster.  Writes tree_of (n), the rows again and the result again.
int crn_points(int n, const float* enh, const float* hag, const Opts* o, int32_t* tree_of, int cap, Top* tops, Result* res) {
  sfmterrain::Dims d;
  d.e_min = g_last.res.e_min, d.n_min = g_last.res.n_min, d.De = g_last.res.De, d.Dn = g_last.res.Dn;
  for (Top& t : g_last.tops) t.points = 0;
  g_last.res.n_labelled = 0;
  points_host(n, enh, hag, d, *o, g_last);
  for (int i = 0; i < n; ++i) tree_of[i] = g_last.tree_of[(size_t)i];
  for (size_t j = 0; j < g_last.tops.size() && (int)j < cap; ++j) tops[j] = g_last.tops[j];
  *res = g_last.res;
  return 0;
}

// rule 7's window of a summit of smoothed height h: R2, -1 when the options are refused
int crn_window(const Opts* o, double c, float h) {
  Prep p;
  if (!prepare(*o, c, p)) return -1;
  return window_R2(h, p);
}
}

#ifdef CROWNS_MAIN
// rasters that walk every branch: paraboloid crowns apart and touching on a ground of noise, with empty cells, through several
// option sets; 1 x 1, one-row, empty, all-empty and no-canopy rasters; a plateau; the tree cap; the points of rule 10; the
// refusals and the window's cap
static uint32_t rng_state = 1357u;
static double rnd() {
  rng_state = sfmdraw::mix32(rng_state + 0x9E3779B9u);
  return (double)rng_state / 4294967296.0;
}
static std::vector<float> plot(const double (*trees)[4], int nt, double c, int D) {
  std::vector<float> Z((size_t)D * D);
  for (int y = 0; y < D; ++y)
    for (int x = 0; x < D; ++x) {
      const double px = (x + 0.5) * c - 0.5 * D * c, py = (y + 0.5) * c - 0.5 * D * c;
      double z = 0.05 * rnd();
      for (int k = 0; k < nt; ++k) {
        const double r2 = ((px - trees[k][0]) * (px - trees[k][0]) + (py - trees[k][1]) * (py - trees[k][1])) / (trees[k][3] * trees[k][3]);
        if (r2 <= 1.0) z = std::max(z, 0.4 * trees[k][2] + 0.6 * trees[k][2] * (1.0 - r2) + 0.05 * (rnd() - 0.5));
      }
      Z[(size_t)y * D + x] = rnd() < 0.03 ? NAN : (float)z;
    }
  return Z;
}
static void summary(const char* what, const Result& r) {
  std::printf("%s: raster %d x %d canopy %d summits %d trees %d cells %d points %d depth %d flags %d\n", what, r.De, r.Dn, r.n_canopy,
              r.n_summits, r.n_trees, r.n_labelled_cells, r.n_labelled, r.max_depth, r.flags);
}
static bool consistent(const HostOut& out, int max_trees = MAX_TREES) {
  const size_t nc = (size_t)out.res.De * out.res.Dn;
  if (out.labels.size() != nc || out.smooth.size() != nc) return false;
  std::vector<int> cells(out.tops.size(), 0);
  int labelled = 0;
  for (int32_t l : out.labels) {
    if (l < -1 || l >= (int)out.tops.size()) return false;
    if (l >= 0) ++cells[(size_t)l], ++labelled;
  }
  for (size_t j = 0; j < out.tops.size(); ++j)
    if (cells[j] != out.tops[j].cells || (j && out.tops[j].cell_id <= out.tops[j - 1].cell_id)) return false;
  return labelled == out.res.n_labelled_cells && (int)out.tops.size() == std::min(out.res.n_trees, max_trees);
}
int main() {
  const double APART[6][4] = {{-9, -8, 18, 3.0}, {8, -9, 9, 1.5}, {0, 0, 24, 4.0}, {-8, 9, 12, 2.0}, {9, 8, 15, 2.5}, {0, -10.5, 6, 1.2}};
  const double TOUCHING[5][4] = {{-4, 0, 18, 3.0}, {1.2, 0, 12, 2.2}, {4.6, 0.5, 9, 1.5}, {0, 5, 22, 3.5}, {-5.5, 5, 8, 1.4}};
  HostOut out;
  for (int scene = 0; scene < 2; ++scene)
    for (int variant = 0; variant < 7; ++variant) {
      Opts v = default_opts();
      double c = 0.5;
      if (variant == 1) c = 0.25;
      if (variant == 2) v.smooth_passes = 0, c = 0.1;
      if (variant == 3) v.smooth_passes = 64;
      if (variant == 4) v.scale = 0.5, c = 1.0;                            // every length doubles in cloud units
      if (variant == 5) v.r_min = v.r_max = 5.0, v.crown_frac = 0.9, v.max_crown_radius = 1.0;
      if (variant == 6) v.max_trees = 2, v.win_a = 0.0, v.win_b = 0.0, v.r_min = 0.1, v.r_max = 0.1, v.smooth_passes = 0;
      const int D = (int)(28.0 / (c * v.scale));
      double trees[6][4];
      const int nt = scene ? 5 : 6;
      for (int k = 0; k < nt; ++k)
        for (int a = 0; a < 4; ++a) trees[k][a] = (scene ? TOUCHING[k][a] : APART[k][a]) / v.scale;
      std::vector<float> Z = plot(trees, nt, c, D);
      if (!run_host_raster(Z.data(), D, D, c, -3.0f, 7.5f, v, out) || !consistent(out, v.max_trees)) return 1;
      if (variant == 6 && (!(out.res.flags & F_OVERFLOW) || out.tops.size() != 2)) return 1;
      if (variant == 0 && out.res.n_trees != nt) return 1;
      // rule 10: a point in the middle of every cell, at the cell's raw height, and two points that have none
      std::vector<float> enh, hag;
      for (int q = 0; q < D * D; ++q) {
        enh.push_back((float)(-3.0 + (q % D + 0.5) * c)), enh.push_back((float)(7.5 + (q / D + 0.5) * c)), enh.push_back(Z[(size_t)q]);
        hag.push_back(Z[(size_t)q]);
      }
      enh.push_back(0.f), enh.push_back(0.f), enh.push_back(NAN), hag.push_back(NAN);
      enh.push_back(-3.f), enh.push_back(7.5f), enh.push_back(1.f), hag.push_back(INFINITY);
      sfmterrain::Dims d = {-3.0f, 7.5f, D, D};
      points_host((int)hag.size(), enh.data(), hag.data(), d, v, out);
      int pts = 0;
      for (const Top& t : out.tops) pts += t.points;
      if (pts != out.res.n_labelled || out.res.n_labelled > out.res.n_labelled_cells || out.tree_of.size() != hag.size()) return 1;
      char name[48];
      std::snprintf(name, sizeof name, "scene %d variant %d", scene, variant);
      summary(name, out.res);
    }
  {
    Opts v = default_opts();
    const float one[1] = {5.0f};
    if (!run_host_raster(one, 1, 1, 0.5, 0.f, 0.f, v, out) || out.res.n_trees != 1 || out.labels[0] != 0 || out.tops[0].cells != 1) return 2;
    summary("one cell", out.res);
    std::vector<float> row(300);
    for (int x = 0; x < 300; ++x) row[(size_t)x] = x % 37 == 5 ? NAN : (float)(3.0 + 2.0 * std::sin(x / 9.0));
    if (!run_host_raster(row.data(), 300, 1, 0.5, 0.f, 0.f, v, out) || !consistent(out) || out.res.n_trees < 2) return 2;
    summary("one row", out.res);
    if (!run_host_raster(row.data(), 1, 300, 0.5, 0.f, 0.f, v, out) || !consistent(out)) return 2;
    summary("one column", out.res);
    if (!run_host_raster(nullptr, 0, 0, 0.5, 0.f, 0.f, v, out) || out.res.flags != F_NO_CANOPY) return 2;
    if (!run_host_raster(nullptr, 0, 5, 0.5, 0.f, 0.f, v, out) || out.res.flags != F_NO_CANOPY) return 2;
    std::vector<float> none(64, NAN), low(64, 1.0f), flat(40 * 40, 7.0f);
    if (!run_host_raster(none.data(), 8, 8, 0.5, 0.f, 0.f, v, out) || out.res.flags != F_NO_CANOPY || out.res.n_canopy) return 2;
    if (!run_host_raster(low.data(), 8, 8, 0.5, 0.f, 0.f, v, out) || out.res.flags != F_NO_CANOPY) return 2;
    if (!run_host_raster(flat.data(), 40, 40, 0.5, 0.f, 0.f, v, out) || !consistent(out) || out.tops[0].cell_id != 0) return 2;
    summary("plateau", out.res);
    v.r_max = 40.0;  // the window's cap: 80 cells
    if (run_host_raster(flat.data(), 40, 40, 0.5, 0.f, 0.f, v, out)) return 3;
    v.r_max = 32.0;  // 64 cells: the cap itself
    if (!run_host_raster(flat.data(), 40, 40, 0.5, 0.f, 0.f, v, out) || out.res.n_trees != 1) return 3;
    summary("cap", out.res);
  }
  const float z4[4] = {3.f, 4.f, 5.f, 6.f};
  Opts bad = default_opts();
  bad.scale = 0.0;
  if (run_host_raster(z4, 2, 2, 0.5, 0.f, 0.f, bad, out)) return 4;
  bad = default_opts(), bad.win_b = -0.1;
  if (run_host_raster(z4, 2, 2, 0.5, 0.f, 0.f, bad, out)) return 4;
  bad = default_opts(), bad.crown_frac = NAN;
  if (run_host_raster(z4, 2, 2, 0.5, 0.f, 0.f, bad, out)) return 4;
  bad = default_opts(), bad.smooth_passes = MAX_PASSES + 1;
  if (run_host_raster(z4, 2, 2, 0.5, 0.f, 0.f, bad, out)) return 4;
  bad = default_opts(), bad.max_trees = 0;
  if (run_host_raster(z4, 2, 2, 0.5, 0.f, 0.f, bad, out)) return 4;
  bad = default_opts(), bad.r_max = 0.1;
  if (run_host_raster(z4, 2, 2, 0.5, 0.f, 0.f, bad, out)) return 4;
  if (run_host_raster(z4, 2, 2, 0.0, 0.f, 0.f, default_opts(), out)) return 4;
  if (run_host_raster(z4, 5000, 5000, 0.5, 0.f, 0.f, default_opts(), out)) return 4;  // rule 2's cap, refused before the raster is read
  std::printf("done\n");
  return 0;
}
#endif
