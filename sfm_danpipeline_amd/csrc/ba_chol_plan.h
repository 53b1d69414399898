// ba_chol_plan.h -- the launch plan of the blocked Cholesky of the reduced camera system (chol_step2 / chol_step2_chains in
// ba.hip): how many panel, identity-row and trailing workgroups a launch has, which tile a trailing wave owns and which pending
// panel pairs it folds, and the schedule of launches (deferred trailing updates, the catch-up launch, tiles per workgroup) of
// the dense route, of a set of chains and of the separator.  The kernel and the host both take the counts from here.
//
// Everything is in units of tiles (CB columns) and panel pairs: launch k2 factors the panels 2 k2 and 2 k2 + 1 and folds "pair"
// p = the panels 2 p and 2 p + 1 of launch p into the tiles right of them.  No HIP runtime: tests/test_chol_plan.py compiles
// it with g++ and drives a numpy factorisation from the plan alone.
#pragma once
#include <vector>

#ifdef __HIPCC__
#define C2PLAN_HD __host__ __device__ __forceinline__
#else
#define C2PLAN_HD inline
#endif

namespace c2plan {

constexpr int CB = 32;        // tile width of the blocked Cholesky
constexpr int C2_WAVES = 11;  // waves of a chol_step2 workgroup: the most trailing tiles one workgroup takes
constexpr int MAX_CHAINS = 8; // chains of one chol_step2_chains launch (cplan::CP_MAX)
// Large dense systems (no dissection, nt >= DENSE_XB_MIN_NT -- 250 cameras: +3 % there, +5 % at 330, +55 % at 640): X is kept
// only inside diagonal blocks of DENSE_XB tile columns (chol_back_block in ba.hip).  The block width is not a knob:
// chol_back_block's registers and LDS and the sizes of its partial sums are built for DENSE_XB tile columns.
// From DENSE_DEFER4_MIN_NT tile columns on the trailing tiles are visited every 4th launch (every 2nd below), until
// DENSE_SWITCH_M2 tile rows are left; DENSE_TPW8_ROUNDS: see dense_schedule.
constexpr int DENSE_XB = 8, DENSE_XB_MIN_NT = 48, DENSE_DEFER4_MIN_NT = 100, DENSE_SWITCH_M2 = 40, DENSE_TPW8_ROUNDS = 4;

C2PLAN_HD int imin(int a, int b) { return a < b ? a : b; }
C2PLAN_HD int imax(int a, int b) { return a > b ? a : b; }

// Deferred trailing updates (dfr = D > 1, large matrices): a launch rewrites every trailing tile for 64 columns of update, and at
// 100+ tile rows that traffic -- not the MFMAs -- is what a launch waits for.  A tile column is only needed up to date when it becomes
// the panel, so launch k2 touches the columns whose distance to the panels, counted in column pairs, is a multiple of D, and folds
// the min(D, k2) pairs of panels they have missed (K = 64 D per visit): the columns next to the panels are among them every time.
// trail_tiles: the tiles of those columns (tc counted from the first column right of the panels), column by column.
C2PLAN_HD int trail_tiles(int m2, int D) {
  int n = 0;
  for (int tc = 0; tc < m2; tc += (tc & 1) ? 2 * D - 1 : 1) n += m2 - tc;
  return n;
}

// One launch on one matrix of nt tile columns (nxc: the tile columns of X that are wanted -- nt for a whole matrix, the interior
// tiles for a chain, whose X is only used up to there; xb: 0, or the width in tile columns (even) of the diagonal blocks of X
// that are wanted: the inverse of a diagonal block of L is made of that block alone).
// Workgroups [0, npanel): the owner of the diagonal tiles, the m2 tile rows below the panels, the rhs row; [npanel, npanel + nx):
// the rows xlo .. 2 k2 + 1 of the identity block X; then the trailing tiles, `total` of them: ntile of S (column by column
// when deferred, row by row otherwise), m2 of the rhs row, (2 k2 - xlo) x mx of X.
struct Shape {
  int m2;      // tile rows (and columns) right of / below the two panels
  int npanel;  // owner, m2 tile rows, rhs
  int xlo;     // first row block of X that takes part
  int nx;      // rows xlo .. 2 k2 + 1 of X, panel workgroups like any tile row
  int ntile;   // trailing tiles of S this launch visits
  int mx;      // column blocks of X right of the panels
  int total;   // trailing tiles of the launch (launch 0 has no pending pair: none)
};
// (the panel workgroups' part alone: they are a launch's critical path and do not wait for the tile counts, which with_tiles adds)
C2PLAN_HD Shape panel_shape(int nt, int k2, int xb) {
  Shape s;
  s.m2 = nt - 2 * k2 - 2;
  s.npanel = s.m2 + 2;
  s.xlo = xb ? 2 * k2 / xb * xb : 0;
  s.nx = 2 * k2 + 2 - s.xlo;
  s.ntile = s.mx = s.total = 0;
  return s;
}
C2PLAN_HD Shape with_tiles(Shape s, int nxc, int k2, int xb, int dfr) {
  if (xb) nxc = imin(nxc, s.xlo + xb);
  s.ntile = dfr > 1 ? trail_tiles(s.m2, dfr) : s.m2 * (s.m2 + 1) / 2;
  s.mx = imax(0, nxc - 2 * k2 - 2);
  s.total = k2 == 0 ? 0 : s.ntile + s.m2 + (2 * k2 - s.xlo) * s.mx;
  return s;
}
C2PLAN_HD Shape shape(int nt, int nxc, int k2, int xb, int dfr) { return with_tiles(panel_shape(nt, k2, xb), nxc, k2, xb, dfr); }

// Trailing tile t of a launch: tile (rb, cb) of S (rb >= cb > 2 k2 + 1), of the rhs row (rb = nt) or of X (row block rb of
// the identity), and the pairs pair0 .. pair0 + npend - 1 whose products the launch subtracts from it.
enum Kind { TILE_S = 0, TILE_RHS = 1, TILE_X = 2 };
struct Tile {
  int kind, rb, cb, pair0, npend;
};
// (catchup = D: the launch that ends a run of deferred updates -- itself undeferred -- visits every column and folds what each
// has missed: a column whose distance to the panels is r pairs was last visited when that distance was the next multiple of D
// above r)
C2PLAN_HD Tile decode(const Shape& s, int k2, int dfr, int catchup, int t) {
  const int m2 = s.m2, ntrail = s.ntile + m2;
  int ti_rel = 0;
  int rb_x = -1;
  int npend = 1;
  if (t >= ntrail) {
    t -= ntrail;
    rb_x = s.xlo + t / s.mx;
    t %= s.mx;
  } else if (dfr > 1) {
    if (t >= s.ntile) {
      t -= s.ntile;  // the rhs row: every column, every launch
      ti_rel = m2;
    } else {
      int tc = 0;
      while (t >= m2 - tc) {
        t -= m2 - tc;
        tc += (tc & 1) ? 2 * dfr - 1 : 1;
      }
      ti_rel = tc + t;
      t = tc;
      npend = imin(dfr, k2);
    }
  } else {
    while (true) {
      const int w = ti_rel < m2 ? ti_rel + 1 : m2;
      if (t < w) break;
      t -= w;
      ++ti_rel;
    }
    if (catchup > 1 && ti_rel < m2) npend = imin(catchup - (t / 2) % catchup, k2);
  }
  Tile tl;
  tl.kind = rb_x >= 0 ? TILE_X : ti_rel == m2 ? TILE_RHS : TILE_S;
  tl.rb = rb_x >= 0 ? rb_x : 2 * k2 + 2 + ti_rel;
  tl.cb = 2 * k2 + 2 + t;
  tl.pair0 = k2 - npend;
  tl.npend = npend;
  return tl;
}

// trailing tiles per workgroup (one wave each): the fewest, from four -- one wave per SIMD: a tile is 64 MFMAs -- that keep a
// launch of npan panel workgroups to one round of workgroups on the device (every workgroup of the kernel holds a CU's LDS)
inline int fit_tpw(int npan, int ntrail, int n_cu) {
  int tpw = 4;
  while (tpw < C2_WAVES && npan + (ntrail + tpw - 1) / tpw > n_cu) ++tpw;
  return tpw;
}

// ---- one undeferred matrix with all of its X (the separator of a dissected system)
struct Grid {
  int tpw, grid;
};
inline Grid launch_grid(int nt, int nxc, int k2, int n_cu) {
  const Shape s = shape(nt, nxc, k2, 0, 1);
  Grid g;
  g.tpw = fit_tpw(s.npanel + s.nx, s.total, n_cu);
  g.grid = s.npanel + s.nx + (s.total + g.tpw - 1) / g.tpw;
  return g;
}

// ---- the dense route: one entry per launch
struct Launch {
  int k2, xb, dfr, catchup, tpw, grid;
};
inline int dense_xb(int nt) { return nt >= DENSE_XB_MIN_NT ? DENSE_XB : 0; }
inline std::vector<Launch> dense_schedule(int nt, int n_cu) {
  std::vector<Launch> out;
  const int xb = dense_xb(nt), dfr0 = !xb ? 1 : nt >= DENSE_DEFER4_MIN_NT ? 4 : 2;
  // (measured, scripts/gpu_dense_sizes.py: worth it only behind visits of four pairs -- 640 cameras 624 -> 643 it/s at 40 tile
  // rows, 618 at 72; behind visits of two pairs the undeferred tail is slower: 400 cameras 1433 -> 1407)
  const int sw_m2 = dfr0 >= 4 ? DENSE_SWITCH_M2 : 0;
  bool deferred = false;  // some earlier launch of this factorisation left columns behind
  for (int k2 = 0; 2 * k2 < nt; ++k2) {
    const int m2 = nt - 2 * k2 - 2;
    // the updates are deferred while the trailing matrix is large; once a launch's visits of 64 dfr MFMAs would outlast its
    // panel chain (few tiles left: m2 <= DENSE_SWITCH_M2 tile rows) one launch catches every column up and the rest run undeferred
    const int dfr = m2 > sw_m2 ? dfr0 : 1;
    const int catchup = dfr == 1 && deferred ? dfr0 : 0;
    if (k2 > 0) deferred = dfr > 1;
    const Shape s = shape(nt, nt, k2, xb, dfr);
    const int npan = s.npanel + s.nx;
    int tpw = fit_tpw(npan, s.total, n_cu);
    // (deferred updates, K = 256 per visit: a workgroup of eleven such visits outlasts the panel workgroups twice over and
    // the launch ends on the stragglers of a second round -- four visits, one per SIMD, measured best: scripts/gpu_dense_sizes.py)
    if (dfr >= 4 || catchup >= 4) tpw = 4;
    // (... unless that makes many rounds of workgroups: then two visits per SIMD, one's loads under the other's MFMAs -- 1400
    // cameras 118.7 -> 125 it/s; at 640 cameras, under two rounds, the same choice loses 1-2 %)
    if (dfr >= 4 && (s.total + 3) / 4 > DENSE_TPW8_ROUNDS * n_cu) tpw = 8;
    out.push_back(Launch{k2, xb, dfr, catchup, tpw, npan + (s.total + tpw - 1) / tpw});
  }
  return out;
}

// ---- several independent matrices (chains) at the same pair k2 in ONE launch: ALL panel workgroups come first in the grid, the
// trailing workgroups after them.  Chain j of the launch is chain[j] of the caller's (those that still have panels at k2:
// 2 k2 < nxc); its panel workgroups are [pan0[j], pan0[j + 1]), its trailing workgroups pan0[n] + [trl0[j], trl0[j + 1]).
struct ChainLaunch {
  int n, tpw, total;
  int chain[MAX_CHAINS], pan0[MAX_CHAINS + 1], trl0[MAX_CHAINS + 1];
};
inline ChainLaunch pack_chains(int n_chains, const int* nt, const int* nxc, int k2, int n_cu) {
  ChainLaunch L;
  for (L.tpw = 4;; ++L.tpw) {
    L.n = 0;
    int pan = 0, trl = 0;
    for (int i = 0; i < n_chains && L.n < MAX_CHAINS; ++i) {
      if (2 * k2 >= nxc[i]) continue;
      const Shape s = shape(nt[i], nxc[i], k2, 0, 1);
      const int j = L.n++;
      L.chain[j] = i;
      L.pan0[j] = pan;
      L.trl0[j] = trl;
      pan += s.npanel + s.nx;
      trl += (s.total + L.tpw - 1) / L.tpw;
    }
    L.pan0[L.n] = pan;
    L.trl0[L.n] = trl;
    L.total = pan + trl;
    if (L.total <= n_cu || L.tpw >= C2_WAVES) break;
  }
  return L;
}

}  // namespace c2plan
