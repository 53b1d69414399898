// register_capi.cpp -- a C surface over csrc/register.h for tests/test_register_cpu.py and tests/test_gpu_register.py (built
// with g++ -O2 -std=c++17 -ffp-contract=off): the whole call in the header's plain loops (run_host), the pieces the rule
// cases look at one by one, and, with -DREGISTER_MAIN, a driver that runs clouds of its own making under the sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/register.h"

using namespace sfmreg;

extern "C" {

void reg_default_opts(Opts* o) { *o = default_opts(); }
int reg_sizes(int* transform, int* opts, int* result) {
  *transform = (int)sizeof(Transform);
  *opts = (int)sizeof(Opts);
  *result = (int)sizeof(Result);
  return 0;
}

// rules 2 + 3 + 7 (0: done; 1: refused)
int reg_nearest(int n_tgt, const float* tgt, int n_src, const float* src, const Transform* T, double max_dist, int32_t* idx, float* d2) {
  const Transform T0 = T ? *T : identity();
  if (!valid_max_dist(max_dist) || !valid_transform(T0)) return 1;
  HostGrid g;
  g.build(n_tgt, tgt);
  nearest_host(g, n_src, src, T0, max_d2(max_dist), true, idx, d2);
  return 0;
}

// rule 6 (0: done; 1: refused)
int reg_run(int n_tgt, const float* tgt, int n_src, const float* src, const Opts* o, const Transform* init, Result* res, int32_t* idx) {
  const Opts oo = o ? *o : default_opts();
  return run_host(n_tgt, tgt, n_src, src, oo, init, *res, idx) ? 0 : 1;
}

// rules 4 + 5 on exact pairs p[i] <-> m[i]: the flags of the estimate (FEW without a pair), `next` from `cur`
int reg_estimate(int n, const float* p, const float* m, int with_scale, const Transform* cur, Transform* next) {
  double s1[N1], s2[N2], mu_p[3], mu_m[3];
  sum_host<N1>(n, [&](int i, double* v) { terms1(true, p + 3 * i, m + 3 * i, v); }, s1);
  if (n < 1) return F_FEW;
  means(s1, mu_p, mu_m);
  sum_host<N2>(n, [&](int i, double* v) { terms2(true, p + 3 * i, m + 3 * i, 0.0f, mu_p, mu_m, v); }, s2);
  return estimate(s1, s2, with_scale, *cur, *next);
}

// rule 8
int reg_transform(int n, const float* xyz, const Transform* T, float* out) {
  if (!valid_transform(*T)) return 1;
  transform_host(n, xyz, *T, out);
  return 0;
}
}

#ifdef REGISTER_MAIN
// clouds that walk every branch: a box of points with duplicates and NaN rows against sources inside, outside and far
// outside it; a planted motion with and without scale; a partial overlap under max_dist; the loop's edges; the refusals
static uint32_t rng_state = 8765u;
static double rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) / 16777216.0;
}
static Transform motion(double deg, double tr, double scale) {
  const double PI = 3.14159265358979323846, a = deg * PI / 180.0;
  double ax[3] = {0.3, -0.2, 0.93};
  const double l = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  for (double& v : ax) v /= l;
  const double c = std::cos(a), s = std::sin(a), C = 1 - c;
  Transform T;
  const double R[9] = {c + ax[0] * ax[0] * C,         ax[0] * ax[1] * C - ax[2] * s, ax[0] * ax[2] * C + ax[1] * s,
                       ax[1] * ax[0] * C + ax[2] * s, c + ax[1] * ax[1] * C,         ax[1] * ax[2] * C - ax[0] * s,
                       ax[2] * ax[0] * C - ax[1] * s, ax[2] * ax[1] * C + ax[0] * s, c + ax[2] * ax[2] * C};
  for (int i = 0; i < 9; ++i) T.R[i] = R[i];
  T.t[0] = tr, T.t[1] = -0.7 * tr, T.t[2] = 0.5 * tr;
  T.scale = scale;
  return T;
}
int main() {
  // scene 1: nearest
  std::vector<float> tgt, src;
  for (int i = 0; i < 500; ++i)
    for (int a = 0; a < 3; ++a) tgt.push_back((float)(rnd() * (a == 2 ? 0.5 : 2.0)));
  for (int i = 0; i < 20; ++i)
    for (int a = 0; a < 3; ++a) tgt[3 * (480 + i) + a] = tgt[3 * (7 * i) + a];
  for (int i = 0; i < 5; ++i) tgt[3 * (100 * i + 3) + (i % 3)] = NAN;
  for (int i = 0; i < 300; ++i)
    for (int a = 0; a < 3; ++a) {
      double v = rnd() * 2.0;
      if (i >= 200 && i < 227) {  // outside: beyond each face, edge and corner, near and far
        const int k = i - 200, d = (k / (a == 0 ? 1 : a == 1 ? 3 : 9)) % 3 - 1;
        v = d == 0 ? v : d < 0 ? -0.2 * (1 + 99 * (i & 1)) : 2.0 + 0.2 * (1 + 99 * (i & 1));
      }
      src.push_back((float)v);
    }
  src[3 * 5 + 1] = NAN, src[3 * 77] = INFINITY;
  std::vector<int32_t> idx(300);
  std::vector<float> d2(300);
  for (double md : {(double)INFINITY, 0.25, 0.01}) {
    if (reg_nearest(500, tgt.data(), 300, src.data(), nullptr, md, idx.data(), d2.data())) return 1;
    int kept = 0;
    for (int i = 0; i < 300; ++i) {  // against the plain loop
      int bi = -1;
      float bd = INFINITY;
      if (sfmcloud::finite3(src[3 * i], src[3 * i + 1], src[3 * i + 2]))
        for (int j = 0; j < 500; ++j) {
          if (!sfmcloud::finite3(tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2])) continue;
          const float dd = sfmcloud::dist2(src[3 * i], src[3 * i + 1], src[3 * i + 2], tgt[3 * j], tgt[3 * j + 1], tgt[3 * j + 2]);
          if (dd < bd) bd = dd, bi = j;
        }
      if (!(bd <= max_d2(md))) bi = -1;
      if (bi != idx[i] || bd != d2[i]) return 1;
      kept += bi >= 0;
    }
    std::printf("nearest max_dist %g: kept %d\n", md, kept);
  }
  if (!reg_nearest(500, tgt.data(), 300, src.data(), nullptr, 0.0, idx.data(), d2.data())) return 1;
  // scenes 3 / 4: a planted motion, the whole and a part with strangers above it
  std::vector<float> plot, part;
  for (int i = 0; i < 6000; ++i) {
    const double u = rnd(), v = rnd(), w = rnd();
    if (i % 3 == 0) plot.push_back((float)(16 * u - 8)), plot.push_back((float)(16 * v - 8)), plot.push_back((float)(0.05 * w + 0.3 * std::sin(u * 7) * std::cos(v * 5)));
    else plot.push_back((float)(3 * std::cos(6.28 * u) * (0.2 + v) + (i % 2 ? 3 : -4))), plot.push_back((float)(3 * std::sin(6.28 * u) * (0.2 + v) - 2)), plot.push_back((float)(9 * w));
  }
  for (int variant = 0; variant < 6; ++variant) {
    const Transform M = motion(variant < 3 ? 4.0 : 2.0, variant < 3 ? 0.3 : 0.1, variant % 3 == 1 ? 1.04 : variant % 3 == 2 ? 0.95 : 1.0);
    // the source is the target moved by the inverse: x = R^T (y - t) / scale
    part.clear();
    for (int i = 0; i < 6000; i += 3) {
      if (variant >= 3 && !(plot[3 * i] < 1.0f)) continue;
      double y[3];
      for (int a = 0; a < 3; ++a) y[a] = (plot[3 * i + a] - M.t[a]) / M.scale;
      for (int a = 0; a < 3; ++a) part.push_back((float)(M.R[a] * y[0] + M.R[3 + a] * y[1] + M.R[6 + a] * y[2]));
    }
    if (variant >= 3)
      for (int i = 0; i < 400; ++i) part.push_back((float)(-8 * rnd())), part.push_back((float)(16 * rnd() - 8)), part.push_back((float)(12 + 2 * rnd()));
    Opts o = default_opts();
    o.with_scale = variant % 3 != 0;
    o.max_dist = variant >= 3 ? 0.5 : variant == 0 ? INFINITY : 1.0;
    Transform init = identity();
    init.scale = o.with_scale ? 1.0 : M.scale;
    Result res;
    const int n_src = (int)part.size() / 3;
    std::vector<int32_t> pidx(n_src);
    if (reg_run(6000, plot.data(), n_src, part.data(), &o, &init, &res, pidx.data())) return 2;
    std::printf("variant %d: n_src %d iterations %d pairs %d converged %d flags %d rmse %.3g scale %.6f\n", variant, n_src, res.iterations,
                res.pairs, res.converged, res.flags, std::sqrt(res.mse), res.T.scale);
    if (res.flags != 0 || res.converged != CONV_FIXED) return 2;
  }
  // scene 5: the loop's edges
  {
    Opts o = default_opts();
    Result res;
    const int np = (int)part.size() / 3;
    o.max_iters = 0;
    if (reg_run(6000, plot.data(), np, part.data(), &o, nullptr, &res, nullptr) || res.iterations != 0) return 3;
    o.max_iters = 1;
    if (reg_run(6000, plot.data(), np, part.data(), &o, nullptr, &res, nullptr) || res.iterations != 1) return 3;
    o.max_iters = 50, o.eps = 1e-3;
    if (reg_run(6000, plot.data(), np, part.data(), &o, nullptr, &res, nullptr)) return 3;
    std::printf("eps: iterations %d converged %d\n", res.iterations, res.converged);
    o = default_opts();
    if (reg_run(6000, plot.data(), 6000, plot.data(), &o, nullptr, &res, nullptr) || res.converged != CONV_FIXED || res.iterations != 1 || res.mse != 0.0)
      return 3;
    if (reg_run(6000, plot.data(), 0, part.data(), &o, nullptr, &res, nullptr) || res.flags != F_FEW || res.mse == res.mse) return 3;
    if (reg_run(0, plot.data(), 100, part.data(), &o, nullptr, &res, nullptr) || res.flags != F_FEW || res.pairs != 0) return 3;
    const float nan3[6] = {NAN, 0, 0, 0, NAN, 0};
    if (reg_run(2, nan3, 100, part.data(), &o, nullptr, &res, nullptr) || res.flags != F_FEW) return 3;
    const float line[12] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3};
    if (reg_run(4, line, 4, line, &o, nullptr, &res, nullptr) || res.flags != F_DEGENERATE) return 3;
    const float same[12] = {1, 2, 3, 1, 2, 3, 1, 2, 3, 1, 2, 3};
    if (reg_run(4, same, 4, same, &o, nullptr, &res, nullptr) || res.flags != F_DEGENERATE) return 3;
    o.max_dist = 0.01;  // a source wholly outside, farther than max_dist
    std::vector<float> far(part.begin(), part.begin() + 300);
    for (int i = 0; i < 100; ++i) far[3 * i] += 100.0f;
    if (reg_run(6000, plot.data(), 100, far.data(), &o, nullptr, &res, nullptr) || res.flags != F_FEW || res.pairs != 0) return 3;
  }
  // the refusals
  {
    Opts o = default_opts();
    Result res;
    Transform bad = identity();
    bad.scale = 0;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, &bad, &res, nullptr)) return 4;
    bad = identity(), bad.R[4] = NAN;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, &bad, &res, nullptr)) return 4;
    o.max_dist = -1;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, nullptr, &res, nullptr)) return 4;
    o = default_opts(), o.max_dist = NAN;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, nullptr, &res, nullptr)) return 4;
    o = default_opts(), o.eps = -1e-9;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, nullptr, &res, nullptr)) return 4;
    o = default_opts(), o.max_iters = -1;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, nullptr, &res, nullptr)) return 4;
    o = default_opts(), o.min_pairs = 2;
    if (!reg_run(6000, plot.data(), 100, part.data(), &o, nullptr, &res, nullptr)) return 4;
  }
  std::printf("done\n");
  return 0;
}
#endif
