// register_icp_capi.cpp -- a C surface over csrc/register_icp.h for tests/test_register_icp_cpu.py and
// tests/test_gpu_register_icp.py (built with g++ -O2 -std=c++17 -ffp-contract=off): the whole call in the header's plain loops
// (run_host_icp, run_host_icp_batch), the pieces the rule cases look at one by one, and, with -DREGISTER_ICP_MAIN, a driver that
// runs clouds of its own making under the sanitizers.
#include "../../sfm_danpipeline_amd/csrc/register_icp.h"

using namespace sfmreg;

extern "C" {

void icp_default_opts(IcpOpts* o) { *o = default_icp_opts(); }
int icp_sizes(int* opts, int* result) {
  *opts = (int)sizeof(IcpOpts);
  *result = (int)sizeof(IcpResult);
  return 0;
}

// the whole call (0: done; 1: refused)
int icp_run(int n_tgt, const float* tgt, const float* normals, int n_src, const float* src, const IcpOpts* o, const Transform* init, IcpResult* res,
            int32_t* idx) {
  const IcpOpts oo = o ? *o : default_icp_opts();
  return run_host_icp(n_tgt, tgt, normals, n_src, src, oo, init, *res, idx) ? 0 : 1;
}
int icp_run_batch(int n_tgt, const float* tgt, const float* normals, int n_src, const float* src, const IcpOpts* o, const Transform* inits, int n_init,
                  IcpResult* res, int32_t* idx) {
  const IcpOpts oo = o ? *o : default_icp_opts();
  return run_host_icp_batch(n_tgt, tgt, normals, n_src, src, oo, inits, n_init, res, idx) ? 0 : 1;
}

// rule 8's increment: R_out = dR(omega) R_in, bracketed as plane_estimate's
void icp_cayley_step(const double omega[3], const double R_in[9], double R_out[9]) {
  double dR[9];
  cayley(omega, dR);
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) R_out[3 * r + k] = (dR[3 * r] * R_in[k] + dR[3 * r + 1] * R_in[3 + k]) + dR[3 * r + 2] * R_in[6 + k];
}

// rule 5's count
uint32_t icp_trim_count(double trim, uint32_t n) { return trim_count(trim, n); }
}

#ifdef REGISTER_ICP_MAIN
// a driver for the sanitizers: a ground patch with four stems and their true normals against an independent sample moved by a
// small yaw and shift, through both metrics with every rejector, single and batched; rows without a plane; a partial overlap
// under the trim; one plane; empty inputs; the refusals
#include <cstdio>
static uint32_t rng_state = 4321u;
static double rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) / 16777216.0;
}
static void make_cloud(int ng, int ns, std::vector<float>& xyz, std::vector<float>* nrm, const Transform* back) {
  const double PI = 3.14159265358979323846, cx[4] = {2, 7.5, 5, 1.5}, cy[4] = {2.5, 1.5, 5.2, 8};
  auto put = [&](double x, double y, double z, double nx, double ny, double nz) {
    if (back) {  // the point whose image under *back is (x, y, z): R^T (p - t), scale 1
      const double d[3] = {x - back->t[0], y - back->t[1], z - back->t[2]};
      x = back->R[0] * d[0] + back->R[3] * d[1] + back->R[6] * d[2], y = back->R[1] * d[0] + back->R[4] * d[1] + back->R[7] * d[2];
      z = back->R[2] * d[0] + back->R[5] * d[1] + back->R[8] * d[2];
    }
    xyz.insert(xyz.end(), {(float)x, (float)y, (float)z});
    if (nrm) nrm->insert(nrm->end(), {(float)nx, (float)ny, (float)nz, 0.5f});
  };
  for (int i = 0; i < ng; ++i) put(10 * rnd(), 10 * rnd(), 0.02 * (rnd() - 0.5), 0, 0, 1);
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < ns; ++i) {
      const double a = 2 * PI * rnd();
      put(cx[k] + 0.15 * std::cos(a), cy[k] + 0.15 * std::sin(a), 5 * rnd(), std::cos(a), std::sin(a), 0);
    }
}
int main() {
  Transform M = identity();
  const double a = 3.0 * 3.14159265358979323846 / 180.0;
  M.R[0] = std::cos(a), M.R[1] = -std::sin(a), M.R[3] = std::sin(a), M.R[4] = std::cos(a);
  M.t[0] = 0.25, M.t[1] = -0.2, M.t[2] = 0.05;
  std::vector<float> tgt, nrm, src;
  make_cloud(1500, 150, tgt, &nrm, nullptr);
  make_cloud(600, 60, src, nullptr, &M);
  const int nt = (int)tgt.size() / 3, ns = (int)src.size() / 3;
  std::vector<int32_t> idx((size_t)5 * ns);
  IcpResult res[5];
  for (int metric = 0; metric < 2; ++metric)
    for (int o2o = 0; o2o < 2; ++o2o)
      for (double trim : {1.0, 0.5, 1.0 / ns})
        for (int ws = 0; ws < 2; ++ws) {
          IcpOpts o = default_icp_opts();
          o.metric = metric, o.one_to_one = o2o, o.trim = trim, o.with_scale = ws, o.max_dist = 1.0, o.max_iters = 12;
          if (metric) o.eps = 1e-6, o.min_pairs = ws ? 7 : 6;
          if (icp_run(nt, tgt.data(), nrm.data(), ns, src.data(), &o, nullptr, &res[0], idx.data())) return 1;
          std::printf("metric %d one_to_one %d trim %.4g scale %d: iterations %d pairs %d converged %d flags %d tau %.3g t %.4f %.4f %.4f\n", metric,
                      o2o, trim, ws, res[0].iterations, res[0].pairs, res[0].converged, res[0].flags, res[0].trim_d2, res[0].T.t[0], res[0].T.t[1],
                      res[0].T.t[2]);
          Transform inits[5] = {identity(), M, identity(), M, identity()};
          inits[2].t[0] = 500.0, inits[4].t[1] = 0.1;
          IcpResult one;
          if (icp_run_batch(nt, tgt.data(), nrm.data(), ns, src.data(), &o, inits, 5, res, idx.data())) return 1;
          for (int b = 0; b < 5; ++b)
            if (icp_run(nt, tgt.data(), nrm.data(), ns, src.data(), &o, &inits[b], &one, nullptr) || memcmp(&one, &res[b], sizeof one)) return 2;
          if (res[2].flags != F_FEW || res[2].pairs != 0) return 2;
        }
  {  // the plane metric finds the planted motion; rows without a plane take no part; a partial overlap under the trim
    IcpOpts o = default_icp_opts();
    o.metric = 1, o.eps = 1e-6, o.min_pairs = 6, o.max_dist = 1.0;
    if (icp_run(nt, tgt.data(), nrm.data(), ns, src.data(), &o, nullptr, &res[0], idx.data()) || res[0].flags || res[0].converged != CONV_EPS) return 3;
    if (std::fabs(res[0].T.t[0] - 0.25) > 0.02 || std::fabs(res[0].T.t[1] + 0.2) > 0.02 || std::fabs(res[0].T.t[2] - 0.05) > 0.02) return 3;
    std::vector<float> holes = nrm;
    for (int j = 0; j < nt; j += 3) holes[4 * j] = NAN;
    for (int j = 1; j < nt; j += 3) holes[4 * j] = holes[4 * j + 1] = holes[4 * j + 2] = 0.0f;
    o.max_iters = 0;
    if (icp_run(nt, tgt.data(), holes.data(), ns, src.data(), &o, nullptr, &res[0], idx.data())) return 3;
    for (int i = 0; i < ns; ++i)
      if (idx[i] >= 0 && idx[i] % 3 != 2) return 3;
    std::printf("no plane: pairs %d of %d\n", res[0].pairs, ns);
    std::vector<float> part;
    for (int i = 0; i < ns; ++i)
      if (src[3 * i] < 6.0f) part.insert(part.end(), src.begin() + 3 * i, src.begin() + 3 * i + 3);
    o.max_iters = 30, o.trim = 0.5, o.max_dist = inf_d();
    if (icp_run(nt, tgt.data(), nrm.data(), (int)part.size() / 3, part.data(), &o, nullptr, &res[0], idx.data()) || res[0].flags) return 3;
    std::printf("partial: iterations %d pairs %d tau %.3g\n", res[0].iterations, res[0].pairs, res[0].trim_d2);
  }
  {  // one plane; empty inputs; the refusals
    IcpOpts o = default_icp_opts();
    o.metric = 1, o.eps = 1e-6, o.min_pairs = 6;
    if (icp_run(1500, tgt.data(), nrm.data(), 600, src.data(), &o, nullptr, &res[0], nullptr) || res[0].flags != F_DEGENERATE) return 4;
    for (int pass = 0; pass < 2; ++pass) {
      o.trim = pass ? 0.5 : 1.0, o.one_to_one = pass;
      if (icp_run(nt, tgt.data(), nrm.data(), 0, src.data(), &o, nullptr, &res[0], idx.data()) || res[0].flags != F_FEW) return 4;
      if (icp_run(0, tgt.data(), nrm.data(), ns, src.data(), &o, nullptr, &res[0], idx.data()) || res[0].flags != F_FEW || res[0].pairs != 0) return 4;
    }
    o = default_icp_opts(), o.trim = 0.0;
    if (!icp_run(nt, tgt.data(), nrm.data(), ns, src.data(), &o, nullptr, &res[0], nullptr)) return 5;
    o = default_icp_opts(), o.metric = 1;  // eps 0
    if (!icp_run(nt, tgt.data(), nrm.data(), ns, src.data(), &o, nullptr, &res[0], nullptr)) return 5;
    o.eps = 1e-6, o.min_pairs = 6;
    if (!icp_run(nt, tgt.data(), nullptr, ns, src.data(), &o, nullptr, &res[0], nullptr)) return 5;
    o.min_pairs = 5;
    if (!icp_run(nt, tgt.data(), nrm.data(), ns, src.data(), &o, nullptr, &res[0], nullptr)) return 5;
  }
  std::printf("done\n");
  return 0;
}
#endif
