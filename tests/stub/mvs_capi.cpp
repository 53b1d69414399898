// C entry points over sfm_danpipeline_amd/csrc/mvs.h for the CPU tests (tests/test_mvs_cpu.py) and for the GPU tests'
// bit-for-bit comparison: the g++ build of the header the device code is compiled from.
// -DMVS_MAIN: a driver for the sanitizer run (reads a scene from a file).
#include "../../sfm_danpipeline_amd/csrc/mvs.h"
#include <cstdio>

using namespace sfmmvs;

struct MvsOpts {
  int32_t n_planes, window, n_src, n_best, min_views, pad;
  double ncc_min, eps, var_min;
};
static Opts to_opts(const MvsOpts* o) { return Opts{o->n_planes, o->window, o->n_src, o->n_best, o->min_views, o->ncc_min, o->eps, o->var_min}; }

extern "C" {

void mvs_default_opts(MvsOpts* o) {
  const Opts r = default_opts();
  o->n_planes = r.n_planes, o->window = r.window, o->n_src = r.n_src, o->n_best = r.n_best, o->min_views = r.min_views, o->pad = 0;
  o->ncc_min = r.ncc_min, o->eps = r.eps, o->var_min = r.var_min;
}

// rule 3 on one pixel
int mvs_sample(const uint8_t* img, int rows, int cols, const double* H, int x, int y) { return warp_sample(img, rows, cols, H, x, y); }

// rule 4 as the plain double loop over two side x side windows of 12-bit samples (0xFFFF: invalid); 0: no NCC
int mvs_ncc_window(const uint16_t* r, const uint16_t* q, int side, double* out) {
  uint32_t sr = 0, srr = 0, sq = 0, sqq = 0, srq = 0;
  for (int y = 0; y < side; ++y)
    for (int x = 0; x < side; ++x) {
      const uint32_t a = r[y * side + x], b = q[y * side + x];
      if (a == (uint32_t)INVALID || b == (uint32_t)INVALID) return 0;
      sr += a, srr += a * a, sq += b, sqq += b * b, srq += a * b;
    }
  return ncc(side * side, sr, var_term(side * side, sr, srr), sq, sqq, srq, out) ? 1 : 0;
}

int mvs_sources(const double* poses, int n_views, int ref, int n_src, int32_t* src) { return choose_sources(poses, n_views, ref, n_src, src); }

// rule 2: H[k][s][9]
int mvs_homographies(const double* K9, const double* poses, int ref, int n_src, const int32_t* src, int D, double dmin, double dmax, double* H) {
  double inv_far, step;
  plane_range(dmin, dmax, D, &inv_far, &step);
  std::vector<double> h;
  make_homographies(Cam{K9[0], K9[4], K9[2], K9[5]}, poses, ref, n_src, src, D, inv_far, step, h);
  memcpy(H, h.data(), h.size() * 8);
  return 0;
}

// null: the arguments are refused
void* mvs_create(int n_views, int rows, int cols, const uint8_t* const* gray, const uint8_t* const* bgr, const double* K9, const double* poses,
                 int level) {
  host::Scene* S = new host::Scene();
  if (!host::build(*S, n_views, rows, cols, gray, bgr, K9, poses, level)) {
    delete S;
    return nullptr;
  }
  return S;
}
void mvs_free(void* h) { delete (host::Scene*)h; }

void mvs_level(void* h, int32_t* rows, int32_t* cols, double* K9, int view, uint8_t* gray, uint8_t* bgr) {
  const host::Scene* S = (const host::Scene*)h;
  const size_t px = (size_t)S->rows * S->cols;
  *rows = S->rows, *cols = S->cols;
  const double k[9] = {S->K.fx, 0, S->K.cx, 0, S->K.fy, S->K.cy, 0, 0, 1};
  if (K9) memcpy(K9, k, sizeof k);
  if (view >= 0 && gray) memcpy(gray, &S->gray[px * view], px);
  if (view >= 0 && bgr && S->colour) memcpy(bgr, &S->bgr[3 * px * view], 3 * px);
}

// -3 (the library's SFMHIP_ERR_ARG) for refused arguments
int mvs_depthmap(void* h, int ref, int n_src, const int32_t* src, double dmin, double dmax, const MvsOpts* o, int32_t* idx, float* depth,
                 float* score, int threads) {
  return host::depthmap(*(host::Scene*)h, ref, n_src, src, dmin, dmax, to_opts(o), idx, depth, score, threads) ? 0 : -3;
}

int mvs_set_depthmap(void* h, int view, const float* depth) {
  host::Scene* S = (host::Scene*)h;
  if (view < 0 || view >= S->n) return -3;
  const size_t px = (size_t)S->rows * S->cols;
  memcpy(&S->depth[px * view], depth, px * sizeof(float));
  return 0;
}

// the points, or -3
int mvs_fuse(void* h, const MvsOpts* o) { return opts_valid(to_opts(o)) ? host::fuse(*(host::Scene*)h, to_opts(o)) : -3; }
int mvs_run(void* h, const double* dmin, const double* dmax, const MvsOpts* o, int threads) {
  const int n = host::run(*(host::Scene*)h, dmin, dmax, to_opts(o), threads);
  return n < 0 ? -3 : n;
}
void mvs_download(void* h, float* xyz, float* nrm, uint32_t* rgb) {
  const host::Scene* S = (const host::Scene*)h;
  if (xyz && !S->xyz.empty()) memcpy(xyz, S->xyz.data(), S->xyz.size() * 4);
  if (nrm && !S->nrm.empty()) memcpy(nrm, S->nrm.data(), S->nrm.size() * 4);
  if (rgb && !S->rgb.empty()) memcpy(rgb, S->rgb.data(), S->rgb.size() * 4);
}

}  // extern "C"

#ifdef MVS_MAIN
// file: int32 n, rows, cols, colour; K9; poses 12 n; dmin n; dmax n (doubles); gray n rows cols; bgr (if colour)
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[4];
  if (fread(hd, 4, 4, f) != 4) return 2;
  const int n = hd[0], rows = hd[1], cols = hd[2];
  const size_t px = (size_t)rows * cols;
  std::vector<double> d(9 + 14 * (size_t)n);
  std::vector<uint8_t> g(px * n), c(hd[3] ? 3 * px * n : 0);
  if (fread(d.data(), 8, d.size(), f) != d.size() || fread(g.data(), 1, g.size(), f) != g.size()) return 2;
  if (!c.empty() && fread(c.data(), 1, c.size(), f) != c.size()) return 2;
  fclose(f);
  std::vector<const uint8_t*> gp, cp;
  for (int v = 0; v < n; ++v) gp.push_back(&g[px * v]), cp.push_back(c.empty() ? nullptr : &c[3 * px * v]);
  const double *K = d.data(), *poses = K + 9, *dmin = poses + 12 * n, *dmax = dmin + n;
  MvsOpts o;
  for (int level = 0; level <= 1; ++level)
    for (int w : {1, 3, 7}) {
      void* h = mvs_create(n, rows, cols, gp.data(), c.empty() ? nullptr : cp.data(), K, poses, level);
      if (!h) return 1;
      mvs_default_opts(&o);
      o.window = w, o.n_planes = level ? 3 : 17;
      const int m = mvs_run(h, dmin, dmax, &o, 3);
      std::vector<float> xyz(3 * (size_t)std::max(m, 1)), nrm(xyz.size());
      std::vector<uint32_t> rgb((size_t)std::max(m, 1));
      mvs_download(h, xyz.data(), nrm.data(), rgb.data());
      printf("level %d window %d: %d points\n", level, w, m);
      mvs_free(h);
    }
  {  // one source, n_best above it, an odd size through the pyramid, a black view
    std::fill(g.begin(), g.begin() + px, 0);
    void* h = mvs_create(n, rows - 1, cols - 1, gp.data(), nullptr, K, poses, 1);
    if (!h) return 1;
    mvs_default_opts(&o);
    o.n_planes = 5, o.n_src = 1, o.n_best = 2, o.min_views = 1;
    printf("starved: %d points\n", mvs_run(h, dmin, dmax, &o, 2));
    o.n_best = 1;
    printf("one source: %d points\n", mvs_run(h, dmin, dmax, &o, 2));
    mvs_free(h);
  }
  return 0;
}
#endif
