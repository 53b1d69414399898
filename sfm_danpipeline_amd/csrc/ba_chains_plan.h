// ba_chains_plan.h -- host-side plan of the "chains + separator" factorisation of the reduced camera system: one level of
// dissection, the fallback for camera graphs whose fronts do not fit the front tree (ba_front_plan.h).
//
// Order: reverse Cuthill-McKee positions pi; a cut at position p puts every camera at or behind p that sees a
// camera before p into the separator; what is left falls into connected components that do not see each
// other (interiors).  Cuts are chosen from a grid of positions (1..3 cuts) to minimise the number of
// two-panel launches on the dependency chain, max_i tiles_i / 2 + tiles_S / 2 + a constant for the gather /
// combine / three-step solve; the dense factorisation stays when that does not win by 20 %.
//
// Pure host C++ (no HIP): tests/test_chains_plan.py compiles it with g++ and checks the plan's index maps by running a
// numpy chains + separator solve over them against a dense solve.  ba.hip's kernels (nd_gather, chol_step2_chains,
// nd_combine, nd_xy, nd_w) walk the same maps.
#pragma once
#include <algorithm>
#include <cstddef>
#include <functional>
#include <map>
#include <vector>
#include "ba_setup.h"  // bsetup::I4, the layout of HIP's int4

namespace cplan {

constexpr int CP_MAX = 8;  // chains (the kernels' by-value tables hold this many and the separator)

struct Plan {
  bool ok = false;                       // false: no cut, more workgroups than one round, or no win over the dense factorisation
  double cost = 1e300;                   // two-panel launches on the dependency chain
  std::vector<int> sep;                  // cameras
  std::vector<std::vector<int>> chains;  // cameras of every chain, ascending
};

static inline std::vector<std::vector<int>> neighbours(int nc, const unsigned long long* adj, int wpr) {
  std::vector<std::vector<int>> nb(nc);
  for (int i = 0; i < nc; ++i)
    for (int j = 0; j < nc; ++j)
      if (j != i && ((adj[(size_t)i * wpr + (j >> 6)] >> (j & 63)) & 1ull)) nb[i].push_back(j);
  return nb;
}

// adj: nc x wpr bit rows; dense_tiles: 32-column tiles of the dense factorisation; force: take any plan that fits
static inline Plan build_plan(int nc, const unsigned long long* adj, int wpr, int dense_tiles, int n_cu, bool force) {
  const std::vector<std::vector<int>> nb = neighbours(nc, adj, wpr);
  // ---- RCM positions (every connected component from a pseudo-peripheral start)
  std::vector<int> order, pos(nc, -1), lvl(nc);
  order.reserve(nc);
  auto bfs = [&](int start, std::vector<int>& out) {
    out.clear();
    std::fill(lvl.begin(), lvl.end(), -1);
    out.push_back(start);
    lvl[start] = 0;
    for (size_t h = 0; h < out.size(); ++h) {
      const int u = out[h];
      std::vector<int> nx;
      for (int v : nb[u])
        if (lvl[v] < 0 && pos[v] < 0) {
          lvl[v] = lvl[u] + 1;
          nx.push_back(v);
        }
      std::sort(nx.begin(), nx.end(), [&](int a, int c) { return nb[a].size() != nb[c].size() ? nb[a].size() < nb[c].size() : a < c; });
      for (int v : nx) out.push_back(v);
    }
  };
  std::vector<int> comp;
  for (int s0 = 0; s0 < nc; ++s0) {
    if (pos[s0] >= 0) continue;
    int start = s0;
    for (int rep = 0; rep < 2; ++rep) {  // farthest vertex of the farthest vertex
      bfs(start, comp);
      start = comp.back();
    }
    bfs(start, comp);
    for (int v : comp) {
      pos[v] = (int)order.size();
      order.push_back(v);
    }
  }
  std::vector<int> minpos(nc);
  for (int v = 0; v < nc; ++v) {
    int m = pos[v];
    for (int u : nb[v]) m = std::min(m, pos[u]);
    minpos[v] = m;
  }
  // ---- evaluate a set of cuts: separator, components (chains by LPT when more than CP_MAX), launches
  auto evaluate = [&](const std::vector<int>& cuts, Plan& e) {
    std::vector<char> in_sep(nc, 0);
    for (int v = 0; v < nc; ++v)
      for (int p : cuts)
        if (pos[v] >= p && minpos[v] < p) in_sep[v] = 1;
    std::vector<int> root(nc);
    for (int v = 0; v < nc; ++v) root[v] = v;
    std::function<int(int)> find = [&](int x) {
      while (root[x] != x) x = root[x] = root[root[x]];
      return x;
    };
    for (int v = 0; v < nc; ++v)
      if (!in_sep[v])
        for (int u : nb[v])
          if (!in_sep[u]) root[find(u)] = find(v);
    std::map<int, std::vector<int>> comps;
    e.sep.clear();
    for (int v = 0; v < nc; ++v) {
      if (in_sep[v]) e.sep.push_back(v);
      else comps[find(v)].push_back(v);
    }
    if (comps.size() < 2) return;
    std::vector<std::vector<int>> cl;
    for (auto& kv : comps) cl.push_back(kv.second);
    std::sort(cl.begin(), cl.end(), [](const std::vector<int>& a, const std::vector<int>& c) {
      return a.size() != c.size() ? a.size() > c.size() : a[0] < c[0];
    });
    const int nch = (int)std::min<size_t>(cl.size(), CP_MAX);
    e.chains.assign(nch, {});
    for (auto& c : cl) {
      int best = 0;
      for (int k = 1; k < nch; ++k)
        if (e.chains[k].size() < e.chains[best].size()) best = k;
      e.chains[best].insert(e.chains[best].end(), c.begin(), c.end());
    }
    int max_t = 0;
    for (auto& c : e.chains) {
      std::sort(c.begin(), c.end());
      max_t = std::max(max_t, (int)((6 * c.size() + 63) / 64) * 2);
    }
    const int sep_t = (int)((6 * e.sep.size() + 1 + 63) / 64) * 2;
    e.cost = 0.5 * max_t + 0.5 * sep_t + 2.5;
    // the panel workgroups of a launch in one round of workgroups (a second round doubles the launch): launch 0
    // has N_i + 2 per chain
    int pan = 0;
    for (auto& c : e.chains) pan += (int)((6 * c.size() + 63) / 64) * 2 + sep_t + 2;
    if (pan > n_cu) e.cost = 1e300;
  };
  Plan best;
  {
    const int G = nc > 1024 ? 12 : 24;
    std::vector<int> grid;
    for (int k = 1; k < G; ++k) grid.push_back((int)((long long)nc * k / G));
    Plan e;
    for (size_t i = 0; i < grid.size(); ++i) {  // at most three cuts
      evaluate({grid[i]}, e);
      if (e.cost < best.cost) best = e;
      for (size_t j = i + 1; j < grid.size(); ++j) {
        evaluate({grid[i], grid[j]}, e);
        if (e.cost < best.cost) best = e;
        if (nc <= 1024)
          for (size_t k = j + 1; k < grid.size(); k += 2) {
            evaluate({grid[i], grid[j], grid[k]}, e);
            if (e.cost < best.cost) best = e;
          }
      }
    }
  }
  best.ok = !(best.chains.empty() || best.cost >= 1e299 || !(force || best.cost <= 0.8 * (0.5 * dense_tiles)));
  return best;
}

// the plan's invariants: a partition of the cameras, no edge between two chains (0 = they hold)
static inline int violations(const Plan& P, int nc, const unsigned long long* adj, int wpr) {
  const std::vector<std::vector<int>> nb = neighbours(nc, adj, wpr);
  std::vector<int> owner(nc, -2);
  int bad = 0;
  for (int c : P.sep) owner[c] = -1;
  for (int i = 0; i < (int)P.chains.size(); ++i)
    for (int c : P.chains[i]) {
      if (owner[c] != -2) ++bad;
      owner[c] = i;
    }
  for (int c = 0; c < nc; ++c) {
    if (owner[c] == -2) ++bad;
    for (int u : nb[c])
      if (owner[c] >= 0 && owner[u] >= 0 && owner[u] != owner[c]) ++bad;
  }
  return bad;
}

// ---------------------------------------------------------------- the plan as the device takes it
// Chain i is a dense square matrix of N = ni + NS tiles of 32 columns: its interior, then the separator (cameras, the focal
// last); index n is the separator itself (ni = N = NS).  One buffer of doubles holds M | X | y of every chain in turn.
struct Flat {
  int n = 0;  // chains
  int NS = 0, max_ni = 0;
  struct {
    int ni, N, ld;  // interior tiles (the separator: all of them); tiles; 32 N
  } c[CP_MAX + 1];
  std::vector<int> inv[CP_MAX + 1];  // 32 N: chain index -> index in S (the parameter's column), -1 = padding; inv[n] is the separator's
  size_t offM[CP_MAX + 1], offX[CP_MAX + 1], offy[CP_MAX + 1], total = 0;  // in doubles
  int col0[CP_MAX + 1];              // first interior column of chain i among all interior columns (col0[n]: their number)
  std::vector<bsetup::I4> jobs;      // nd_gather's: (chain, tile row, tile column, role)
};

static inline Flat flatten(const Plan& plan, int nc) {
  Flat fl;
  const int P = fl.n = (int)plan.chains.size();
  const int NS = fl.NS = (int)((6 * plan.sep.size() + 1 + 63) / 64) * 2;
  std::vector<int>& invS = fl.inv[P];
  invS.assign((size_t)NS * 32, -1);
  {
    int k = 0;
    for (int c : plan.sep)
      for (int j = 0; j < 6; ++j) invS[k++] = 6 * c + j;
    invS[k++] = 6 * nc;  // the focal
  }
  fl.col0[0] = 0;
  for (int i = 0; i <= P; ++i) {
    const int ni = i < P ? (int)((6 * plan.chains[i].size() + 63) / 64) * 2 : NS;
    const int N = i < P ? ni + NS : NS;
    if (i < P) {
      fl.inv[i].assign((size_t)N * 32, -1);
      int k = 0;
      for (int c : plan.chains[i])
        for (int j = 0; j < 6; ++j) fl.inv[i][k++] = 6 * c + j;
      for (int k2 = 0; k2 < NS * 32; ++k2) fl.inv[i][(size_t)ni * 32 + k2] = invS[k2];
      fl.max_ni = std::max(fl.max_ni, ni);
      fl.col0[i + 1] = fl.col0[i] + ni * 32;
    }
    fl.c[i] = {ni, N, N * 32};
    fl.offM[i] = fl.total;
    fl.total += (size_t)N * 32 * N * 32;
    fl.offX[i] = fl.total;
    fl.total += (size_t)N * 32 * N * 32;
    fl.offy[i] = fl.total;
    fl.total += (size_t)N * 32;
    for (int tr = 0; tr < N; ++tr) {
      for (int tc = 0; tc <= std::min(tr, ni - 1); ++tc) fl.jobs.push_back({i, tr, tc, 0});
      fl.jobs.push_back({i, tr, 0, 1});
      // what the factorisation reads before it writes: the lower right block of M (zero), the interior rows of X
      // (the identity; its tiles left of the diagonal are read too) -- no memset of the chain buffers
      for (int tc = ni; tc <= tr; ++tc) fl.jobs.push_back({i, tr, tc, 2});
      // (a chain's X is only formed up to its interior columns: nxc in chol_step2_chains)
      if (tr < ni)
        for (int tc = 0; tc < (i < P ? ni : N); ++tc) fl.jobs.push_back({i, tr, tc, 3});
    }
  }
  fl.jobs.push_back({0, 0, 0, 4});  // (ba_finalize's part, when it is deferred to the gather)
  return fl;
}

}  // namespace cplan
