// C entry points over sfm_danpipeline_amd/csrc/poisson.h for the CPU tests (tests/test_poisson_cpu.py) and for the GPU
// tests' bit-for-bit comparison: the g++ build of the header the device code is compiled from.
// -DPOISSON_MAIN: a driver for the sanitizer run (reads n, xyz, normals from a file).
#include "../../sfm_danpipeline_amd/csrc/poisson.h"
#include <cstdio>

using namespace sfmpoisson;

struct PsnOpts {
  int depth;
  double scale, point_weight, cg_rtol;
  int cg_max_iter;
};
static Opts to_opts(const PsnOpts* o) { return Opts{o->depth, o->scale, o->point_weight, o->cg_rtol, o->cg_max_iter}; }

extern "C" {

double psn_bspline(double t) { return bspline(t); }

// cloud.h's ordered keys as poisson.h sees them: key[i] = ord_key(f[i]), back[i] = ord_val(key[i])
void psn_ord_keys(int n, const float* f, uint32_t* key, float* back) {
  for (int i = 0; i < n; ++i) {
    key[i] = sfmcloud::ord_key(f[i]);
    back[i] = sfmcloud::ord_val(key[i]);
  }
}

void psn_default_opts(PsnOpts* o) {
  const Opts r = reference_opts();
  o->depth = r.depth, o->scale = r.scale, o->point_weight = r.point_weight, o->cg_rtol = r.cg_rtol, o->cg_max_iter = r.cg_max_iter;
}

// -3 (the library's SFMHIP_ERR_ARG) for options out of range
int psn_reconstruct(int n, const float* xyz, const float* nrm, int stride, const PsnOpts* o, int threads, void** out) {
  *out = nullptr;
  if (n < 0 || (stride != 3 && stride != 4) || !opts_valid(to_opts(o))) return -3;
  host::Result* R = new host::Result();
  host::reconstruct(n, xyz, nrm, stride, to_opts(o), *R, threads);
  *out = R;
  return 0;
}
// info: n_vertices, n_triangles, iterations, samples, N
void psn_counts(void* h, int* info) {
  const host::Result* R = (const host::Result*)h;
  info[0] = (int)(R->verts.size() / 3), info[1] = (int)(R->tris.size() / 3), info[2] = R->iterations, info[3] = R->m, info[4] = R->g.N;
}
// d: iso, rr, bb, origin x y z, h; chi may be null
void psn_get(void* h, float* verts, int* tris, double* chi, double* d) {
  const host::Result* R = (const host::Result*)h;
  if (verts && !R->verts.empty()) memcpy(verts, R->verts.data(), R->verts.size() * 4);
  if (tris && !R->tris.empty()) memcpy(tris, R->tris.data(), R->tris.size() * 4);
  if (chi && !R->chi.empty()) memcpy(chi, R->chi.data(), R->chi.size() * 8);
  if (d) {
    d[0] = R->iso, d[1] = R->rr, d[2] = R->bb;
    for (int a = 0; a < 3; ++a) d[3 + a] = R->g.o[a];
    d[6] = R->g.h;
  }
}
void psn_free(void* h) { delete (host::Result*)h; }

// rules 1-4: V (3 N^3), W, rhs (N^3 each); cube: origin x y z, h; returns the samples used
int psn_splat(int n, const float* xyz, const float* nrm, int stride, const PsnOpts* o, int threads, double* V, double* W, double* rhs,
              double* cube) {
  host::Samples S;
  host::make_samples(n, xyz, nrm, stride, to_opts(o), S);
  std::vector<double> v, w, b;
  host::splat_rhs(S, v, w, b, threads);
  memcpy(V, v.data(), v.size() * 8);
  memcpy(W, w.data(), w.size() * 8);
  memcpy(rhs, b.data(), b.size() * 8);
  for (int a = 0; a < 3; ++a) cube[a] = S.g.o[a];
  cube[3] = S.g.h;
  return S.m;
}

// rule 5 from a given right-hand side; rr_bb: the final and the initial squared residual; returns the iterations
int psn_solve(int depth, const double* rhs, const double* W, double point_weight, double rtol, int max_iter, int threads, double* chi,
              double* rr_bb) {
  std::vector<double> x;
  const int it = host::solve(1 << depth, rhs, W, point_weight, rtol, max_iter, x, &rr_bb[0], &rr_bb[1], threads);
  memcpy(chi, x.data(), x.size() * 8);
  return it;
}

// rule 6 for a given chi
double psn_iso(int n, const float* xyz, const float* nrm, int stride, const PsnOpts* o, int threads, const double* chi) {
  host::Samples S;
  host::make_samples(n, xyz, nrm, stride, to_opts(o), S);
  return host::iso_value(S, chi, threads);
}

// rule 7 from a given field on an N^3 grid (any N >= 2)
void* psn_extract(int N, const double* chi, double iso, const double* origin, double h) {
  host::Result* R = new host::Result();
  R->g.N = N;
  host::extract(chi, N, iso, origin, h, R->verts, R->tris);
  return R;
}

// the fixed-order sum of a list
double psn_sum(const double* v, int n) {
  std::vector<double> part(((size_t)n + CHUNK - 1) / CHUNK);
  for (size_t c = 0; c < part.size(); ++c) {
    double w[CHUNK];
    for (int t = 0; t < CHUNK; ++t) w[t] = c * CHUNK + t < (size_t)n ? v[c * CHUNK + t] : 0.0;
    part[c] = chunk_tree(w);
  }
  return sum_partials(part.data(), part.size());
}

}  // extern "C"

#ifdef POISSON_MAIN
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<float> xyz(3 * (size_t)n + 3), nrm(3 * (size_t)n + 3);
  if (fread(xyz.data(), 4, 3 * (size_t)n, f) != 3 * (size_t)n || fread(nrm.data(), 4, 3 * (size_t)n, f) != 3 * (size_t)n) return 2;
  fclose(f);
  PsnOpts o;
  psn_default_opts(&o);
  for (int depth = 1; depth <= 5; ++depth) {
    o.depth = depth;
    void* h = nullptr;
    if (psn_reconstruct(n, xyz.data(), nrm.data(), 3, &o, 4, &h)) return 1;
    int info[5];
    psn_counts(h, info);
    printf("depth %d: %d vertices %d triangles %d iterations %d samples\n", depth, info[0], info[1], info[2], info[3]);
    psn_free(h);
  }
  o.depth = 3;
  for (int m : {0, 1, 2}) {  // no sample, one, two
    void* h = nullptr;
    if (psn_reconstruct(m, xyz.data(), nrm.data(), 3, &o, 2, &h)) return 1;
    int info[5];
    psn_counts(h, info);
    printf("n %d: %d vertices %d triangles\n", m, info[0], info[1]);
    psn_free(h);
  }
  return 0;
}
#endif
