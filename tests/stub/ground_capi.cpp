// ground_capi.cpp -- a C surface over csrc/ground.h for tests/test_ground_cpu.py and tests/test_gpu_ground.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off -pthread): the whole call in the header's plain loops (run_host), the pieces the rule
// cases look at one by one, and, with -DGROUND_MAIN, a driver that runs clouds of its own making under the sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/ground.h"

using namespace sfmground;

extern "C" {

void gnd_default_opts(Opts* o) { *o = default_opts(); }
int gnd_sizes(int* opts, int* result) {
  *opts = (int)sizeof(Opts);
  *result = (int)sizeof(Result);
  return 0;
}

// 0: done; 1: the options are refused
int gnd_run(int n, const float* xyz, const int32_t* labels, int32_t label, const Opts* o, const double* cams, int n_cam, int threads,
            Result* res) {
  return run_host(n, xyz, labels, label, *o, cams, n_cam, threads < 1 ? 1 : threads, *res) ? 0 : 1;
}

// rule 3 on a list of n_sel points: out6 = a, n; returns ok (-1: the options are refused)
int gnd_hypothesis(const float* pts, int n_sel, const Opts* o, int j, double* out6) {
  Prep pr;
  if (!prepare(*o, pr)) return -1;
  const Hyp h = hypothesis((const P3*)pts, n_sel, o->seed, j, pr.hint, pr.cos_tilt, pr.has_hint);
  for (int k = 0; k < 3; ++k) out6[k] = h.a[k], out6[3 + k] = h.n[k];
  return h.ok;
}

// rule 4 on the same list against the plane (a, n): inliers, pos, neg
void gnd_count(const float* pts, int n_sel, const double* a, const double* n, double tol, uint32_t* out3) {
  Counts k;
  count_sides((const P3*)pts, n_sel, a, n, tol, k);
  out3[0] = k.inl, out3[1] = k.pos, out3[2] = k.neg;
}

int gnd_orientation(const double* n, int cpos, int cneg, uint32_t pos, uint32_t neg) { return orientation(n, cpos, cneg, pos, neg); }

// rule 8: 1 when the hint was replaced
int gnd_north(const double* up, const double* hint, double* north) { return make_north(up, hint, north) ? 1 : 0; }

// the hand-over to the dendrometry's options (0: done; 1: refused)
int gnd_opts_from_ground(const Result* g, sfmdendro::Opts* io) { return opts_from_ground(*g, *io) ? 0 : 1; }

// jacobi_svd<3, 3, 3, 3> on a row-major 3 x 3: W (3) and Vt (9)
void gnd_svd3(const double* m, double* W, double* Vt) {
  double At[9];
  for (int i = 0; i < 9; ++i) At[i] = m[i];
  sfmjacobi::jacobi_svd<3, 3, 3, 3>(At, W, Vt);
}
}

#ifdef GROUND_MAIN
// clouds that walk every branch: a ground disc with a tree on it, NaN points, labels, walls, a sphere, 0 .. 3 points,
// collinear and identical points, camera centres, hints, the refusals
static uint32_t rng_state = 4321u;
static double rnd() {
  rng_state = sfmdraw::mix32(rng_state + 0x9E3779B9u);
  return (double)rng_state / 4294967296.0;
}
static double gauss() {
  double s = 0;
  for (int i = 0; i < 12; ++i) s += rnd();
  return s - 6.0;
}
int main() {
  const double PI = 3.14159265358979323846;
  std::vector<float> xyz;
  std::vector<int32_t> lab;
  auto push = [&](double x, double y, double z, int l) {
    // a fixed rotation, so that no axis is special
    const double c = std::cos(0.7), s = std::sin(0.7);
    const double y2 = c * y - s * z, z2 = s * y + c * z;
    xyz.push_back((float)(c * x + s * z2));
    xyz.push_back((float)y2);
    xyz.push_back((float)(-s * x + c * z2));
    lab.push_back(l);
  };
  for (int i = 0; i < 9000; ++i) {  // ground disc, noise 0.01
    const double a = 2 * PI * rnd(), r = 6.0 * std::sqrt(rnd());
    push(r * std::cos(a), r * std::sin(a), 0.01 * gauss(), 0);
  }
  for (int i = 0; i < 3000; ++i) {  // trunk
    const double a = 2 * PI * rnd();
    push(0.15 * std::cos(a), 0.15 * std::sin(a), 4.0 * rnd(), 0);
  }
  for (int i = 0; i < 5000; ++i) {  // crown shell
    const double a = 2 * PI * rnd(), c = 2 * rnd() - 1, s = std::sqrt(1 - c * c);
    push(2.0 * s * std::cos(a), 1.5 * s * std::sin(a), 6.5 + 2.5 * c, 0);
  }
  for (int i = 0; i < 12000; ++i) push(5.9, 12 * rnd() - 6, 8 * rnd(), 1);  // a wall at the edge, its own label
  push(NAN, 0, 0, 0);
  push(0, INFINITY, 1, 0);
  const int n = (int)lab.size();
  const double cams[6] = {1.0, 2.0, 3.0, -2.0, 1.0, 2.5};
  Opts o = default_opts();
  Result res;
  for (int variant = 0; variant < 7; ++variant) {
    Opts v = o;
    const int32_t* l = lab.data();
    const double* cm = nullptr;
    int nc = 0, threads = 1;
    if (variant == 1) v.ransac_iters = 1, v.refit_rounds = 0;
    if (variant == 2) v.ransac_iters = 4096, v.refit_rounds = 8, threads = 4;
    if (variant == 3) l = nullptr;                       // the wall is in: it has more points than the ground
    if (variant == 4) l = nullptr, cm = cams, nc = 2;    // (the centres are not rotated: this only walks the branch)
    if (variant == 5) v.up_hint[2] = 2.0, v.max_tilt_deg = 60.0, v.inlier_tol = 0.03;
    if (variant == 6) v.north_hint[0] = 0, v.north_hint[1] = 0, v.north_hint[2] = 0;
    if (!run_host(n, xyz.data(), l, 0, v, cm, nc, threads, res)) return 1;
    std::printf("variant %d: selected %d inliers %d below %d above %d winner %d flags %d rms %.6f tol %.6f up %.4f %.4f %.4f\n", variant,
                res.n_selected, res.inliers, res.below, res.above, res.winner, res.flags, res.rms, res.tol, res.up[0], res.up[1], res.up[2]);
  }
  if (!run_host(n, xyz.data(), lab.data(), 7, o, nullptr, 0, 1, res) || res.flags != F_FEW) return 2;  // nobody has label 7
  if (!run_host(0, xyz.data(), nullptr, 0, o, nullptr, 0, 1, res) || res.flags != F_FEW) return 2;
  for (int m = 1; m <= 3; ++m) {  // 1, 2, 3 points
    Opts v = o;
    v.min_inliers = 3;
    if (!run_host(m, xyz.data(), nullptr, 0, v, nullptr, 0, 1, res)) return 2;
    if ((m < 3) != (res.flags == F_FEW)) return 2;
    std::printf("points %d: flags %d inliers %d\n", m, res.flags, res.inliers);
  }
  {  // a sphere shell, collinear points, identical points: no plane
    std::vector<float> s;
    for (int i = 0; i < 4000; ++i) {
      const double a = 2 * PI * rnd(), c = 2 * rnd() - 1, q = std::sqrt(1 - c * c);
      s.push_back((float)(q * std::cos(a))), s.push_back((float)(q * std::sin(a))), s.push_back((float)c);
    }
    if (!run_host(4000, s.data(), nullptr, 0, o, nullptr, 0, 2, res) || res.flags != F_NO_PLANE) return 3;
    for (int i = 0; i < 4000; ++i) s[3 * i] = (float)i, s[3 * i + 1] = (float)(2 * i), s[3 * i + 2] = (float)(-i);
    if (!run_host(4000, s.data(), nullptr, 0, o, nullptr, 0, 1, res) || res.flags != F_NO_PLANE) return 3;
    for (int i = 0; i < 4000; ++i) s[3 * i] = s[3 * i + 1] = s[3 * i + 2] = 0.5f;
    if (!run_host(4000, s.data(), nullptr, 0, o, nullptr, 0, 1, res) || res.flags != F_NO_PLANE) return 3;
  }
  Opts bad = o;
  bad.ransac_iters = 0;
  if (run_host(n, xyz.data(), nullptr, 0, bad, nullptr, 0, 1, res)) return 4;
  bad = o;
  bad.max_tilt_deg = 0.0;
  if (run_host(n, xyz.data(), nullptr, 0, bad, nullptr, 0, 1, res)) return 4;
  if (run_host(n, xyz.data(), nullptr, 0, o, nullptr, 2, 1, res)) return 4;
  std::printf("done\n");
  return 0;
}
#endif
