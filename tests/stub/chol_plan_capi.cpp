// C entry points over csrc/ba_chol_plan.h for tests/test_chol_plan.py (host only, no HIP): the launch shape, the decode of a
// range of trailing tiles, the dense schedule, the separator's grid and the packing of a set of chains.
#include "../../sfm_danpipeline_amd/csrc/ba_chol_plan.h"

extern "C" void c2plan_constants(int* out /*8*/) {
  const int v[8] = {c2plan::CB,
                    c2plan::C2_WAVES,
                    c2plan::MAX_CHAINS,
                    c2plan::DENSE_XB,
                    c2plan::DENSE_XB_MIN_NT,
                    c2plan::DENSE_DEFER4_MIN_NT,
                    c2plan::DENSE_SWITCH_M2,
                    c2plan::DENSE_TPW8_ROUNDS};
  for (int i = 0; i < 8; ++i) out[i] = v[i];
}

// out: m2, npanel, xlo, nx, ntile, mx, total
extern "C" void c2plan_shape(int nt, int nxc, int k2, int xb, int dfr, int* out /*7*/) {
  const c2plan::Shape s = c2plan::shape(nt, nxc, k2, xb, dfr);
  out[0] = s.m2, out[1] = s.npanel, out[2] = s.xlo, out[3] = s.nx, out[4] = s.ntile, out[5] = s.mx, out[6] = s.total;
}

// out: (kind, rb, cb, pair0, npend) for every t in [t0, t1)
extern "C" void c2plan_decode(int nt, int nxc, int k2, int xb, int dfr, int catchup, int t0, int t1, int* out) {
  const c2plan::Shape s = c2plan::shape(nt, nxc, k2, xb, dfr);
  for (int t = t0; t < t1; ++t, out += 5) {
    const c2plan::Tile tl = c2plan::decode(s, k2, dfr, catchup, t);
    out[0] = tl.kind, out[1] = tl.rb, out[2] = tl.cb, out[3] = tl.pair0, out[4] = tl.npend;
  }
}

// out: (k2, xb, dfr, catchup, tpw, grid) per launch, at most cap of them; returns the number of launches
extern "C" int c2plan_dense_schedule(int nt, int n_cu, int* out, int cap) {
  const std::vector<c2plan::Launch> L = c2plan::dense_schedule(nt, n_cu);
  for (int i = 0; i < (int)L.size() && i < cap; ++i, out += 6)
    out[0] = L[i].k2, out[1] = L[i].xb, out[2] = L[i].dfr, out[3] = L[i].catchup, out[4] = L[i].tpw, out[5] = L[i].grid;
  return (int)L.size();
}

extern "C" int c2plan_dense_xb(int nt) { return c2plan::dense_xb(nt); }

// out: tpw, grid
extern "C" void c2plan_launch_grid(int nt, int nxc, int k2, int n_cu, int* out /*2*/) {
  const c2plan::Grid g = c2plan::launch_grid(nt, nxc, k2, n_cu);
  out[0] = g.tpw, out[1] = g.grid;
}

// header: n, tpw, total; chain: MAX_CHAINS ints; pan0, trl0: MAX_CHAINS + 1 ints each
extern "C" void c2plan_pack_chains(int n_chains, const int* nt, const int* nxc, int k2, int n_cu, int* header /*3*/, int* chain,
                                   int* pan0, int* trl0) {
  const c2plan::ChainLaunch L = c2plan::pack_chains(n_chains, nt, nxc, k2, n_cu);
  header[0] = L.n, header[1] = L.tpw, header[2] = L.total;
  for (int j = 0; j < L.n; ++j) chain[j] = L.chain[j];
  for (int j = 0; j <= L.n; ++j) pan0[j] = L.pan0[j], trl0[j] = L.trl0[j];
}
