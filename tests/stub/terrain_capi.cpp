// terrain_capi.cpp -- a C surface over csrc/terrain.h for tests/test_terrain_cpu.py and tests/test_gpu_terrain.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off -pthread): the whole call in the header's plain loops (run_host), the pieces the rule
// cases look at one by one, and, with -DTERRAIN_MAIN, a driver that runs plots of its own making under the sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/terrain.h"

using namespace sfmterrain;

static HostOut g_last;  // the rasters of the last ter_run, for ter_raster

extern "C" {

void ter_default_opts(Opts* o) { *o = default_opts(); }
int ter_sizes(int* opts, int* result) {
  *opts = (int)sizeof(Opts);
  *result = (int)sizeof(Result);
  return 0;
}
int ter_tile() { return TILE; }

// 0: done; 1: the options are refused or the raster exceeds its cap.  is_ground, hag: n entries; norm: 3 n.
int ter_run(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts* o, int32_t* is_ground, float* hag, float* norm,
            Result* res) {
  if (!run_host(n, xyz, labels, label, *o, g_last)) return 1;
  for (int i = 0; i < n; ++i) {
    is_ground[i] = g_last.is_ground[i];
    hag[i] = g_last.hag[i];
    for (int a = 0; a < 3; ++a) norm[3 * (size_t)i + a] = g_last.norm[3 * (size_t)i + a];
  }
  *res = g_last.res;
  return 0;
}

// the rasters of the last ter_run that was not refused (De Dn entries each); returns their size
int ter_raster(float* T, uint8_t* kind, float* chm) {
  for (size_t q = 0; q < g_last.T.size(); ++q) T[q] = g_last.T[q], kind[q] = g_last.kind[q], chm[q] = g_last.chm[q];
  return (int)g_last.T.size();
}

// rule 5: the table (32 entries each); returns the number of windows, -1 when the options are refused
int ter_windows(const Opts* o, int32_t* k, double* kd, double* dh) {
  Prep p;
  if (!prepare(*o, p)) return -1;
  Windows w;
  make_windows(p, w);
  for (int i = 0; i < w.n; ++i) k[i] = w.k[i], kd[i] = w.kd[i], dh[i] = w.dh[i];
  return w.n;
}

// rule 6 on a De x Dn raster whose empty cells are +inf
void ter_open(const float* Z, int De, int Dn, int k, float* O) {
  std::vector<float> z(Z, Z + (size_t)De * Dn), o;
  open_host(z, De, Dn, k, o);
  for (size_t i = 0; i < o.size(); ++i) O[i] = o[i];
}

// the hand-over from the ground plane (0: done; 1: refused)
int ter_opts_from_ground(const sfmground::Result* g, Opts* io) { return opts_from_ground(*g, *io) ? 0 : 1; }
}

#ifdef TERRAIN_MAIN
// plots that walk every branch: trunks and crowns on an undulating slope with holes under the crowns, rotated, with NaN points
// and labels; every option off its default; no window; a hole the fill does not close; 0, 1 and 3 points; a one-row raster;
// the cap and the refusals
static uint32_t rng_state = 2468u;
static double rnd() {
  rng_state = sfmdraw::mix32(rng_state + 0x9E3779B9u);
  return (double)rng_state / 4294967296.0;
}
static double gauss() {
  double s = 0;
  for (int i = 0; i < 12; ++i) s += rnd();
  return s - 6.0;
}
static void summary(const char* what, const Result& r) {
  std::printf("%s: raster %d x %d selected %d ground %d windows %d kinds %d %d %d rounds %d flags %d\n", what, r.De, r.Dn, r.n_selected,
              r.n_ground, r.n_windows, r.n_kind1, r.n_kind2, r.n_kind0, r.fill_rounds, r.flags);
}
int main() {
  const double PI = 3.14159265358979323846;
  std::vector<float> xyz;
  std::vector<int32_t> lab;
  const double c = std::cos(0.7), s = std::sin(0.7);
  auto push = [&](double x, double y, double z, int l) {  // a fixed rotation about x, so that no axis is special
    xyz.push_back((float)x);
    xyz.push_back((float)(c * y - s * z));
    xyz.push_back((float)(s * y + c * z));
    lab.push_back(l);
  };
  auto terrain = [](double x, double y) { return 0.25 * x + std::sin(x / 4) * std::cos(y / 5); };
  const double trees[3][2] = {{-5, -4}, {4, -3}, {0, 5}};
  for (int i = 0; i < 12000; ++i) {  // ground on a 24 m square, noise 0.01, no ground within 1.5 of a stem
    const double x = 24 * rnd() - 12, y = 24 * rnd() - 12;
    bool hole = false;
    for (auto& t : trees) hole = hole || (x - t[0]) * (x - t[0]) + (y - t[1]) * (y - t[1]) < 2.25;
    if (!hole) push(x, y, terrain(x, y) + 0.01 * gauss(), 0);
  }
  for (int k = 0; k < 3; ++k) {
    const double cx = trees[k][0], cy = trees[k][1], z0 = terrain(cx, cy);
    for (int i = 0; i < 1500; ++i) {  // trunk 0 .. 4, radius 0.15
      const double a = 2 * PI * rnd();
      push(cx + 0.15 * std::cos(a), cy + 0.15 * std::sin(a), z0 + 4.0 * rnd(), k == 2 ? 1 : 0);
    }
    for (int i = 0; i < 3000; ++i) {  // crown shell around 6.5
      const double a = 2 * PI * rnd(), q = 2 * rnd() - 1, r = std::sqrt(1 - q * q);
      push(cx + 2.0 * r * std::cos(a), cy + 1.5 * r * std::sin(a), z0 + 6.5 + 2.5 * q, k == 2 ? 1 : 0);
    }
  }
  push(NAN, 0, 0, 0);
  push(0, INFINITY, 1, 0);
  const int n = (int)lab.size();
  Opts o = default_opts();
  o.up[0] = 0, o.up[1] = -s, o.up[2] = c;
  o.north[0] = 0, o.north[1] = c, o.north[2] = s;
  HostOut out;
  for (int variant = 0; variant < 9; ++variant) {
    Opts v = o;
    const int32_t* l = nullptr;
    if (variant == 1) l = lab.data();
    if (variant == 2) v.cell = 0.25;
    if (variant == 3) v.exponential = 0, v.base = 3;
    if (variant == 4) v.scale = 0.5;             // every length doubles in cloud units
    if (variant == 5) v.max_window = 1.0;        // no window
    if (variant == 6) v.fill_rounds = 1, v.cell = 0.2;  // the holes stay open
    if (variant == 7) v.fill_rounds = 0, v.relax_sweeps = 0;
    if (variant == 8) v.relax_sweeps = 0, v.slope = 0.0, v.max_window = 40.0;
    if (!run_host(n, xyz.data(), l, 0, v, out)) return 1;
    char name[32];
    std::snprintf(name, sizeof name, "variant %d", variant);
    summary(name, out.res);
    const size_t nc = (size_t)out.res.De * out.res.Dn;
    if (out.T.size() != nc || out.kind.size() != nc || out.chm.size() != nc) return 5;
    int ground = 0;
    for (int i = 0; i < n; ++i) ground += out.is_ground[i];
    if (ground != out.res.n_ground || out.res.n_kind0 + out.res.n_kind1 + out.res.n_kind2 != (int)nc) return 5;
  }
  if (!run_host(0, xyz.data(), nullptr, 0, o, out) || out.res.flags != F_NONE_SELECTED) return 2;
  if (!run_host(n, xyz.data(), lab.data(), 7, o, out) || out.res.flags != F_NONE_SELECTED || out.res.De != 0) return 2;  // nobody has label 7
  {
    const float pts[9] = {0.f, 0.f, 0.f, 0.1f, 0.1f, 0.05f, 7.f, 0.2f, 3.f};
    Opts v = default_opts();
    if (!run_host(1, pts, nullptr, 0, v, out) || out.res.De != 1 || out.res.Dn != 1 || out.res.n_ground != 1) return 3;
    summary("one point", out.res);
    if (!run_host(3, pts, nullptr, 0, v, out) || out.res.Dn != 1 || out.res.De != 15) return 3;  // a one-row raster
    summary("three points", out.res);
    v.cell = 1e-9;  // rule 3's cap
    if (run_host(3, pts, nullptr, 0, v, out)) return 4;
  }
  Opts bad = o;
  bad.cell = 0.0;
  if (run_host(n, xyz.data(), nullptr, 0, bad, out)) return 4;
  bad = o, bad.base = 1;
  if (run_host(n, xyz.data(), nullptr, 0, bad, out)) return 4;
  bad = o, bad.fill_rounds = MAX_FILL + 1;
  if (run_host(n, xyz.data(), nullptr, 0, bad, out)) return 4;
  bad = o, bad.slope = NAN;
  if (run_host(n, xyz.data(), nullptr, 0, bad, out)) return 4;
  bad = o, bad.up[2] = 2.0;
  if (run_host(n, xyz.data(), nullptr, 0, bad, out)) return 4;
  std::printf("done\n");
  return 0;
}
#endif
