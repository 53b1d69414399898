// C entry point over csrc/ba_chains_plan.h for tests/test_chains_plan.py (host only, no HIP): the plan and its flat form.
#include "../../sfm_danpipeline_amd/csrc/ba_chains_plan.h"
#include <cstring>

// header: ok, chains, NS, max_ni, separator cameras, violations, jobs, ints of all inv maps.  cams: the separator's cameras, then
// every chain's; n_cams: their counts in that order.  dims: (ni, N, ld), offs: (offM, offX, offy) per chain and for the
// separator, offs[3 (n + 1)] the total.  inv: the chains' maps, then the separator's.
extern "C" int cplan_build_flat(int nc, const unsigned long long* adj, int wpr, int dense_tiles, int n_cu, int force, int* header /*8*/,
                                double* cost, int* cams, int* n_cams, int* dims, long long* offs, int* col0, int* inv, int inv_cap,
                                int* jobs, int jobs_cap) {
  static_assert(sizeof(bsetup::I4) == 4 * sizeof(int), "a job is four ints");
  const cplan::Plan P = cplan::build_plan(nc, adj, wpr, dense_tiles, n_cu, force != 0);
  header[0] = P.ok ? 1 : 0;
  *cost = P.cost;
  if (!P.ok) return 0;
  const cplan::Flat fl = cplan::flatten(P, nc);
  if (fl.n != (int)P.chains.size() || fl.n > cplan::CP_MAX) return -2;
  size_t n_inv = 0;
  for (int i = 0; i <= fl.n; ++i) n_inv += fl.inv[i].size();
  header[1] = fl.n;
  header[2] = fl.NS;
  header[3] = fl.max_ni;
  header[4] = (int)P.sep.size();
  header[5] = cplan::violations(P, nc, adj, wpr);
  header[6] = (int)fl.jobs.size();
  header[7] = (int)n_inv;
  if ((int)n_inv > inv_cap || (int)fl.jobs.size() > jobs_cap) return -1;
  *n_cams++ = (int)P.sep.size();
  for (int c : P.sep) *cams++ = c;
  for (const auto& ch : P.chains) {
    *n_cams++ = (int)ch.size();
    for (int c : ch) *cams++ = c;
  }
  for (int i = 0; i <= fl.n; ++i) {
    dims[3 * i] = fl.c[i].ni, dims[3 * i + 1] = fl.c[i].N, dims[3 * i + 2] = fl.c[i].ld;
    offs[3 * i] = (long long)fl.offM[i], offs[3 * i + 1] = (long long)fl.offX[i], offs[3 * i + 2] = (long long)fl.offy[i];
    col0[i] = fl.col0[i];
    memcpy(inv, fl.inv[i].data(), fl.inv[i].size() * sizeof(int));
    inv += fl.inv[i].size();
  }
  offs[3 * (fl.n + 1)] = (long long)fl.total;
  memcpy(jobs, fl.jobs.data(), fl.jobs.size() * sizeof(bsetup::I4));
  return 0;
}
