// dendro_capi.cpp -- a C surface over csrc/dendro.h for tests/test_dendro_cpu.py and tests/test_gpu_dendro.py (built with
// g++ -O2 -ffp-contract=off -pthread): the whole call in the header's plain loops (run_host), the pieces the rule cases
// look at one by one, and, with -DDENDRO_MAIN, a driver that runs clouds of its own making under the sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/dendro.h"

using namespace sfmdendro;

extern "C" {

void dnd_default_opts(Opts* o) { *o = default_opts(); }
int dnd_sizes(int* opts, int* slice, int* result) {
  *opts = (int)sizeof(Opts);
  *slice = (int)sizeof(Slice);
  *result = (int)sizeof(Result);
  return 0;
}

// 0: done; 1: the options are refused.  slices: cap rows; frame: 3 n floats or NULL.
int dnd_run(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts* o, int threads, Result* res, int cap,
            Slice* slices, int32_t* n_slices, float* frame) {
  std::vector<Slice> rows;
  if (!run_host(n, xyz, labels, label, *o, threads < 1 ? 1 : threads, *res, rows, frame)) return 1;
  *n_slices = (int32_t)rows.size();
  for (size_t k = 0; k < rows.size() && (int)k < cap; ++k) slices[k] = rows[k];
  return 0;
}

// rules 5 and 6 on one hand-made slice k of nk (e, n) pairs, lengths in cloud units of scale 1
int dnd_fit_slice(const float* en, int nk, int k, const Opts* o, Slice* s) {
  Frame f;
  if (!make_frame(*o, f)) return 1;
  fit_slice((const P2*)en, nk, k, *o, f, *s);
  return 0;
}

// rule 5 alone on the same slice: the winning iteration, -1 when no iteration had an inlier (or the slice is too small)
int dnd_winner(const float* en, int nk, int k, const Opts* o) {
  Frame f;
  if (!make_frame(*o, f) || nk < o->min_slice_pts) return -1;
  const unsigned long long key = ransac_slice((const P2*)en, nk, k, *o, f);
  return key ? key_iter(key) : -1;
}

uint32_t dnd_hash(uint32_t seed, uint32_t k, uint32_t j, uint32_t d) { return draw_hash(seed, k, j, d); }
int dnd_sector(double dx, double dy) { return sector_of(dx, dy); }
unsigned long long dnd_key(int count, int j, unsigned mask) { return winner_key(count, j, mask); }
int dnd_circle(const float* xy6, double r_min, double r_max, double* out3) {
  const Circle c = circumcircle(xy6[0], xy6[1], xy6[2], xy6[3], xy6[4], xy6[5], r_min, r_max);
  out3[0] = c.cx;
  out3[1] = c.cy;
  out3[2] = c.r;
  return c.ok;
}
}

#ifdef DENDRO_MAIN
// clouds that walk every branch: a planted tree, NaN points, labels, a pole, tiny and degenerate slices, refusals
static uint32_t rng_state = 12345u;
static double rnd() {
  rng_state = mix32(rng_state + 0x9E3779B9u);
  return (double)rng_state / 4294967296.0;
}
int main() {
  const double PI = 3.14159265358979323846;
  std::vector<float> xyz;
  std::vector<int32_t> lab;
  auto push = [&](double x, double y, double z, int l) {
    xyz.push_back((float)x);
    xyz.push_back((float)y);
    xyz.push_back((float)z);
    lab.push_back(l);
  };
  for (int i = 0; i < 12000; ++i) {  // trunk
    const double a = 2 * PI * rnd(), z = 4.0 * rnd(), r = 0.15 + 0.005 * (rnd() - 0.5);
    push(r * std::cos(a), r * std::sin(a), z, 0);
  }
  for (int i = 0; i < 20000; ++i) {  // crown shell
    const double a = 2 * PI * rnd(), c = 2 * rnd() - 1, s = std::sqrt(1 - c * c);
    push(2.0 * s * std::cos(a), 1.5 * s * std::sin(a), 6.5 + 2.5 * c, 0);
  }
  for (int i = 0; i < 500; ++i) push(5 + rnd(), 5 + rnd(), rnd(), 1);  // a second object
  push(NAN, 0, 0, 0);
  push(0, INFINITY, 1, 0);
  for (int i = 0; i < 7; ++i) push(0.1, 0.1, 9.5, 0);  // identical points in a thin slice
  const int n = (int)lab.size();
  Opts o = default_opts();
  Result res;
  std::vector<Slice> rows;
  for (int variant = 0; variant < 5; ++variant) {
    Opts v = o;
    if (variant == 1) v.ransac_iters = 1;
    if (variant == 2) v.ransac_iters = 4096, v.slice = 5.0;
    if (variant == 3) v.scale = 0.37, v.ground = -0.2;
    if (variant == 4) v.up[0] = 1, v.up[2] = 0, v.north[1] = 1;  // the tree lies on its side: no stem
    if (!run_host(n, xyz.data(), variant == 4 ? nullptr : lab.data(), 0, v, variant == 2 ? 4 : 1, res, rows)) return 1;
    std::printf("variant %d: slices %d height %.6f dbh %.6f crown base %.6f spread %.6f %.6f flags %d\n", variant, res.n_slices,
                res.total_height, res.dbh, res.crown_base_height, res.spread_ns, res.spread_ew, res.flags);
  }
  if (!run_host(n, xyz.data(), lab.data(), 7, o, 1, res, rows) || res.flags != F_EMPTY) return 2;  // nobody has label 7
  if (!run_host(0, xyz.data(), nullptr, 0, o, 1, res, rows) || res.flags != F_EMPTY) return 2;
  Opts bad = o;
  bad.up[2] = 2;
  if (run_host(n, xyz.data(), nullptr, 0, bad, 1, res, rows)) return 3;
  bad = o;
  bad.north[0] = 0, bad.north[1] = 0, bad.north[2] = 1;
  if (run_host(n, xyz.data(), nullptr, 0, bad, 1, res, rows)) return 3;
  // hand-made slices: sizes around the wave and the chunk, collinear, identical
  Frame f;
  make_frame(o, f);
  for (int nk : {0, 1, 2, 3, 9, 64, 65, 256, 257, 1025}) {
    std::vector<P2> p((size_t)nk + 1);
    for (int i = 0; i < nk; ++i) {
      p[i].x = (float)(0.2 * std::cos(2 * PI * i / nk));
      p[i].y = (float)(0.2 * std::sin(2 * PI * i / nk));
    }
    Slice s;
    fit_slice(p.data(), nk, 3, o, f, s);
    std::printf("ring %d: stem %d inliers %d radius %.9f\n", nk, s.stem, s.inliers, s.radius);
    for (int i = 0; i < nk; ++i) p[i].y = 2 * p[i].x;
    fit_slice(p.data(), nk, 3, o, f, s);
    for (int i = 0; i < nk; ++i) p[i] = p[0];
    fit_slice(p.data(), nk, 3, o, f, s);
    if (s.stem) return 4;
  }
  std::printf("done\n");
  return 0;
}
#endif
