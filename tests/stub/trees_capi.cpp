// trees_capi.cpp -- a C surface over csrc/trees.h for tests/test_trees_cpu.py and tests/test_gpu_trees.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off -pthread): the whole call in the header's plain loops (run_host), the pieces the rule
// cases look at one by one, and, with -DTREES_MAIN, a driver that runs plots of its own making under the sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/trees.h"

using namespace sfmtrees;

extern "C" {

void trs_default_opts(Opts* o) { *o = default_opts(); }
int trs_sizes(int* opts, int* stem, int* result) {
  *opts = (int)sizeof(Opts);
  *stem = (int)sizeof(Stem);
  *result = (int)sizeof(Result);
  return 0;
}

// 0: done; 1: the options are refused or a grid cap is exceeded
int trs_run(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts* o, int threads, int32_t* tree_of, int cap, Stem* stems,
            Result* res) {
  return run_host(n, xyz, labels, label, *o, threads < 1 ? 1 : threads, tree_of, cap, stems, *res) ? 0 : 1;
}

// rule 5 on a De x Dn table of band counts: the least cell id of each occupied cell's component (-1: not occupied)
void trs_components(const int32_t* count, int De, int Dn, int min_cell_pts, int32_t* root) {
  std::vector<int32_t> c(count, count + (size_t)De * Dn), r;
  components(c, De, Dn, min_cell_pts, r);
  for (size_t i = 0; i < r.size(); ++i) root[i] = r[i];
}

// rule 6: the 26 steps and their weights
void trs_steps(int32_t* dxyz, int32_t* weight) {
  for (int k = 0; k < STEPS; ++k) {
    int dx, dy, dz;
    step_delta(k, dx, dy, dz);
    dxyz[3 * k] = dx, dxyz[3 * k + 1] = dy, dxyz[3 * k + 2] = dz;
    weight[k] = step_weight(k);
  }
}

// the hand-over from the ground plane (0: done; 1: refused)
int trs_opts_from_ground(const sfmground::Result* g, Opts* io) { return opts_from_ground(*g, *io) ? 0 : 1; }
}

#ifdef TREES_MAIN
// plots that walk every branch: trees on a ground disc, rotated, with NaN points and labels; touching crowns; a pole; the
// three flags; 0 and 1 points; max_trees, max_path, both caps and the refusals
static uint32_t rng_state = 9876u;
static double rnd() {
  rng_state = sfmdraw::mix32(rng_state + 0x9E3779B9u);
  return (double)rng_state / 4294967296.0;
}
static double gauss() {
  double s = 0;
  for (int i = 0; i < 12; ++i) s += rnd();
  return s - 6.0;
}
static void summary(const char* what, const Result& r, const Stem* st) {
  std::printf("%s: selected %d above %d band %d trees %d voxels %d labelled %d max_cost %d flags %d", what, r.n_selected, r.n_above, r.n_band,
              r.n_trees, r.n_voxels, r.n_labelled, r.max_cost, r.flags);
  if (r.n_trees > 0) std::printf(" stem0 cell %d points %d", st[0].cell_id, st[0].points);
  std::printf("\n");
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
  auto tree = [&](double cx, double cy, int nt, int l) {
    for (int i = 0; i < nt; ++i) {  // trunk 0 .. 4, radius 0.15
      const double a = 2 * PI * rnd();
      push(cx + 0.15 * std::cos(a), cy + 0.15 * std::sin(a), 4.0 * rnd(), l);
    }
    for (int i = 0; i < 2 * nt; ++i) {  // crown shell around 6.5
      const double a = 2 * PI * rnd(), q = 2 * rnd() - 1, r = std::sqrt(1 - q * q);
      push(cx + 2.0 * r * std::cos(a), cy + 1.5 * r * std::sin(a), 6.5 + 2.5 * q, l);
    }
  };
  for (int i = 0; i < 8000; ++i) {  // ground disc, noise 0.01
    const double a = 2 * PI * rnd(), r = 8.0 * std::sqrt(rnd());
    push(r * std::cos(a), r * std::sin(a), 0.01 * gauss(), 0);
  }
  tree(-2.5, -2.5, 2000, 0);
  tree(2.5, -2.5, 2000, 0);
  tree(-1.0, 2.0, 2000, 0);
  tree(2.2, 2.0, 2000, 1);  // touches the third's crown; its own label
  push(NAN, 0, 0, 0);
  push(0, INFINITY, 1, 0);
  const int n = (int)lab.size();
  Opts o = default_opts();
  o.up[0] = 0, o.up[1] = -s, o.up[2] = c;
  o.north[0] = 0, o.north[1] = c, o.north[2] = s;
  o.ground = 0.0;
  std::vector<int32_t> tree_of((size_t)n);
  std::vector<Stem> stems(MAX_TREES);
  Result res;
  for (int variant = 0; variant < 8; ++variant) {
    Opts v = o;
    const int32_t* l = nullptr;
    int threads = 1, cap = MAX_TREES;
    if (variant == 1) l = lab.data(), threads = 4;
    if (variant == 2) v.max_trees = 2, cap = 1;
    if (variant == 3) v.max_path = 3.0;
    if (variant == 4) v.voxel = 0.4, v.stem_cell = 0.1, v.min_cell_pts = 1;
    if (variant == 5) v.scale = 0.5, v.ground = 0.0;  // every length doubles in cloud units
    if (variant == 6) v.min_stem_pts = 100000;        // no stem
    if (variant == 7) v.ground = 100.0;               // nothing above
    if (!run_host(n, xyz.data(), l, 0, v, threads, tree_of.data(), cap, stems.data(), res)) return 1;
    char name[32];
    std::snprintf(name, sizeof name, "variant %d", variant);
    summary(name, res, stems.data());
    for (int i = 0; i < n; ++i)
      if (tree_of[i] < -1 || tree_of[i] >= res.n_trees) return 5;
  }
  if (!run_host(0, xyz.data(), nullptr, 0, o, 1, tree_of.data(), 0, nullptr, res) || res.flags != F_NONE_ABOVE) return 2;
  if (!run_host(n, xyz.data(), lab.data(), 7, o, 1, tree_of.data(), 0, nullptr, res) || res.flags != F_NONE_ABOVE) return 2;  // nobody has label 7
  {  // one point, in the band: one cell, one voxel
    const float one[3] = {0.f, (float)(-s * 1.2), (float)(c * 1.2)};
    Opts v = o;
    v.min_cell_pts = 1, v.min_stem_pts = 1;
    if (!run_host(1, one, nullptr, 0, v, 1, tree_of.data(), 1, stems.data(), res) || res.n_trees != 1 || tree_of[0] != 0) return 2;
    summary("one point", res, stems.data());
  }
  {  // a pole: the sweep goes to the top
    std::vector<float> p;
    for (int i = 0; i < 4000; ++i) {
      const double a = 2 * PI * rnd();
      p.push_back((float)(0.1 * std::cos(a))), p.push_back((float)(0.1 * std::sin(a))), p.push_back((float)(20.0 * rnd()));
    }
    Opts v = default_opts();
    v.ground = 0.0;
    if (!run_host(4000, p.data(), nullptr, 0, v, 2, tree_of.data(), 1, stems.data(), res) || res.n_trees != 1) return 3;
    summary("pole", res, stems.data());
    v.stem_cell = 1e-9;  // rule 4's cap
    if (run_host(4000, p.data(), nullptr, 0, v, 1, tree_of.data(), 1, stems.data(), res)) return 4;
    v = default_opts(), v.ground = 0.0, v.voxel = 1e-4;  // rule 6's cap
    if (run_host(4000, p.data(), nullptr, 0, v, 1, tree_of.data(), 1, stems.data(), res)) return 4;
  }
  Opts bad = o;
  bad.ground = NAN;
  if (run_host(n, xyz.data(), nullptr, 0, bad, 1, tree_of.data(), 0, nullptr, res)) return 4;
  bad = o, bad.band_hi = bad.band_lo;
  if (run_host(n, xyz.data(), nullptr, 0, bad, 1, tree_of.data(), 0, nullptr, res)) return 4;
  bad = o, bad.max_trees = MAX_TREES + 1;
  if (run_host(n, xyz.data(), nullptr, 0, bad, 1, tree_of.data(), 0, nullptr, res)) return 4;
  bad = o, bad.up[2] = 2.0;
  if (run_host(n, xyz.data(), nullptr, 0, bad, 1, tree_of.data(), 0, nullptr, res)) return 4;
  std::printf("done\n");
  return 0;
}
#endif
