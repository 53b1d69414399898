// poisson.h -- the arithmetic of the screened Poisson surface reconstruction behind StructFromMotion::create_mesh
// (reference src/Sfm.cpp:1365-1381: pcl::Poisson at depth 7 on the cloud and its flipped normals), as __host__ __device__
// functions that poisson.hip compiles for gfx950 and tests/stub/poisson_capi.cpp compiles with g++.  The rules are
// DESIGN.md f-9's (copy at the declaration in include/sfmhip.h); PCL parity is UNPINNED: the grid is uniform at full
// depth where PCL's is an adaptive octree, the extraction is marching tetrahedra where PCL's is marching cubes.
//
// Everything is f64 without contraction (-ffp-contract=off on both compilers), and every sum runs in one fixed order:
//   * a splat cell adds its samples one by one: neighbour cells ascending in (z, y, x), samples ascending by input index;
//   * a sum over a list (the dot products of the solve, the iso-value) is sum_fixed below: chunks of 256 entries, each
//     reduced by a wave tree (64 entries, partner t + off for off = 32 .. 1) and then (w0 + w1) + (w2 + w3); the chunk
//     results are added per residue class mod 256 in ascending order, and the 256 classes by the same chunk tree.
//     For a grid vector the list is the bricks of brick_dims() in order, 256 slots per brick (unused slots are 0);
//   * the stencil is stencil() below, left to right.
// A wave (xor butterfly: lane 0 holds the tree's value), a workgroup and the host loops give the same bits.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "block_sum.h"
#include "cloud.h"
#ifndef __HIPCC__
#include <algorithm>
#include <thread>
#include <vector>
#endif

#ifdef __HIPCC__
#define SFM_PSN_INLINE __host__ __device__ __forceinline__
#else
#define SFM_PSN_INLINE inline __attribute__((always_inline))
#endif

namespace sfmpoisson {

constexpr int DEPTH_MIN = 1, DEPTH_MAX = 8;
constexpr int CHUNK = 256;  // entries per chunk of sum_fixed = threads per workgroup

struct Opts {
  int depth;
  double scale, point_weight, cg_rtol;
  int cg_max_iter;  // 0: 4 * 2^depth
};

// the reference's setters: setDepth(7), setPointWeight(4), setScale(1.1)
inline Opts reference_opts() { return Opts{7, 1.1, 4.0, 1e-8, 0}; }

inline bool opts_valid(const Opts& o) {
  return o.depth >= DEPTH_MIN && o.depth <= DEPTH_MAX && o.scale >= 1.0 && o.scale <= 16.0 && o.point_weight >= 0.0 &&
         o.point_weight <= 1e6 && o.cg_rtol >= 0.0 && o.cg_rtol < 1.0 && o.cg_max_iter >= 0 && o.cg_max_iter <= (1 << 20);
}

inline int max_iter_of(const Opts& o) { return o.cg_max_iter > 0 ? o.cg_max_iter : 4 * (1 << o.depth); }

struct Cube {
  double o[3], h;  // origin (the low corner), cell size
  int N;           // cells per side
};

// ---------------------------------------------------------------------------------------------- rule 1: samples
SFM_PSN_INLINE uint32_t f_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}
SFM_PSN_INLINE bool finite_f(float f) { return (f_bits(f) & 0x7F800000u) != 0x7F800000u; }
SFM_PSN_INLINE bool usable(const float* p, const float* nrm) {
  return finite_f(p[0]) && finite_f(p[1]) && finite_f(p[2]) && finite_f(nrm[0]) && finite_f(nrm[1]) && finite_f(nrm[2]) &&
         (nrm[0] != 0.f || nrm[1] != 0.f || nrm[2] != 0.f);
}
// the bounding box of the usable samples: cloud.h's ordered keys under integer atomicMin / atomicMax (order-free)

// ---------------------------------------------------------------------------------------------- rule 2: the cube
inline Cube make_cube(const float lo[3], const float hi[3], int depth, double scale) {
  Cube g;
  double ext = 0.0, c[3];
  for (int a = 0; a < 3; ++a) {
    c[a] = ((double)lo[a] + (double)hi[a]) * 0.5;
    const double e = (double)hi[a] - (double)lo[a];
    ext = e > ext ? e : ext;
  }
  const double side = ext > 0.0 ? scale * ext : 1.0;
  g.N = 1 << depth;
  g.h = side / (double)g.N;
  for (int a = 0; a < 3; ++a) g.o[a] = c[a] - side * 0.5;
  return g;
}

SFM_PSN_INLINE double u_coord(float p, double o, double h) { return ((double)p - o) / h - 0.5; }
// round(u): the cell the sample lies in, clamped to the cube
SFM_PSN_INLINE int cell_coord(float p, double o, double h, int N) {
  double f = floor(((double)p - o) / h);
  f = f < 0.0 ? 0.0 : f;
  f = f > (double)(N - 1) ? (double)(N - 1) : f;
  return (int)f;
}
SFM_PSN_INLINE int cell_key(const Cube& g, const float* p) {
  const int cx = cell_coord(p[0], g.o[0], g.h, g.N), cy = cell_coord(p[1], g.o[1], g.h, g.N),
            cz = cell_coord(p[2], g.o[2], g.h, g.N);
  return (cz * g.N + cy) * g.N + cx;
}

// ---------------------------------------------------------------------------------------------- rule 3: the splat
SFM_PSN_INLINE double bspline(double t) {
  const double a = fabs(t);
  if (a < 0.5) return 0.75 - a * a;
  if (a < 1.5) return 0.5 * ((1.5 - a) * (1.5 - a));
  return 0.0;
}

// pts4 / nrm4: the usable samples ordered by (cell, input index), 4 floats each (xyz + the input index's bits / 0);
// start / end: every cell's range in that order (empty: 0, 0).  out: Vx, Vy, Vz, W of the cell.
SFM_PSN_INLINE void splat_cell(const Cube& g, const float* pts4, const float* nrm4, const int* start, const int* end, int cx,
                               int cy, int cz, double out[4]) {
  double vx = 0.0, vy = 0.0, vz = 0.0, w = 0.0;
  const int N = g.N;
  for (int z = cz - 1; z <= cz + 1; ++z) {
    if (z < 0 || z >= N) continue;
    for (int y = cy - 1; y <= cy + 1; ++y) {
      if (y < 0 || y >= N) continue;
      for (int x = cx - 1; x <= cx + 1; ++x) {
        if (x < 0 || x >= N) continue;
        const size_t cell = ((size_t)z * N + y) * N + x;
        for (int s = start[cell]; s < end[cell]; ++s) {
          const float* p = pts4 + 4 * (size_t)s;
          const float* q = nrm4 + 4 * (size_t)s;
          const double bx = bspline(u_coord(p[0], g.o[0], g.h) - (double)cx);
          const double by = bspline(u_coord(p[1], g.o[1], g.h) - (double)cy);
          const double bz = bspline(u_coord(p[2], g.o[2], g.h) - (double)cz);
          const double wt = (bx * by) * bz;
          vx = vx + wt * (double)q[0];
          vy = vy + wt * (double)q[1];
          vz = vz + wt * (double)q[2];
          w = w + wt;
        }
      }
    }
  }
  out[0] = vx;
  out[1] = vy;
  out[2] = vz;
  out[3] = w;
}

// ---------------------------------------------------------------------------------------------- rule 4: the system
SFM_PSN_INLINE double at_or_zero(const double* v, int N, int x, int y, int z) {
  return (x < 0 || y < 0 || z < 0 || x >= N || y >= N || z >= N) ? 0.0 : v[((size_t)z * N + y) * N + x];
}
// -div V at a cell (central differences, V = 0 outside)
SFM_PSN_INLINE double rhs_cell(const double* vx, const double* vy, const double* vz, int N, int x, int y, int z) {
  double d = (at_or_zero(vx, N, x + 1, y, z) - at_or_zero(vx, N, x - 1, y, z)) * 0.5;
  d = d + (at_or_zero(vy, N, x, y + 1, z) - at_or_zero(vy, N, x, y - 1, z)) * 0.5;
  d = d + (at_or_zero(vz, N, x, y, z + 1) - at_or_zero(vz, N, x, y, z - 1)) * 0.5;
  return -d;
}
// (L + diag) p at a cell: dg = point_weight * W
SFM_PSN_INLINE double stencil(double pc, double xm, double xp, double ym, double yp, double zm, double zp, double dg) {
  return ((((((6.0 * pc - xm) - xp) - ym) - yp) - zm) - zp) + dg * pc;
}

// ---------------------------------------------------------------------------------------------- rule 5: fixed-order sums
struct Brick {
  int bx, by, bz;     // extent of a brick
  int nx, ny, nz, n;  // bricks per axis, in all
};
SFM_PSN_INLINE Brick brick_dims(int N) {
  Brick b;
  b.bx = N < 16 ? N : 16;
  b.by = N < 4 ? N : 4;
  b.bz = N < 4 ? N : 4;
  b.nx = N / b.bx;
  b.ny = N / b.by;
  b.nz = N / b.bz;
  b.n = b.nx * b.ny * b.nz;
  return b;
}
// slot t of brick `id` -> the cell, false for an unused slot
SFM_PSN_INLINE bool brick_cell(const Brick& b, int id, int t, int& x, int& y, int& z) {
  const int lx = t % b.bx, ly = (t / b.bx) % b.by, lz = t / (b.bx * b.by);
  x = (id % b.nx) * b.bx + lx;
  y = ((id / b.nx) % b.ny) * b.by + ly;
  z = (id / (b.nx * b.ny)) * b.bz + lz;
  return lz < b.bz;
}

using sfmsum::chunk_tree;  // block_sum.h: the tree of one chunk (v is overwritten)
// chunk results -> the sum
inline double sum_partials(const double* part, size_t n) {
  double v[CHUNK];
  for (int t = 0; t < CHUNK; ++t) {
    double a = 0.0;
    for (size_t j = (size_t)t; j < n; j += CHUNK) a = a + part[j];
    v[t] = a;
  }
  return chunk_tree(v);
}

// ---------------------------------------------------------------------------------------------- rule 6: the iso-value
// trilinear chi at a sample (chi = 0 outside the cube)
SFM_PSN_INLINE double trilinear(const double* chi, const Cube& g, const float* p) {
  int i0[3];
  double f[3];
  for (int a = 0; a < 3; ++a) {
    const double u = u_coord(p[a], g.o[a], g.h);
    double fl = floor(u);
    fl = fl < -1.0 ? -1.0 : fl;
    fl = fl > (double)(g.N - 1) ? (double)(g.N - 1) : fl;
    i0[a] = (int)fl;
    f[a] = u - fl;
  }
  const int N = g.N, x = i0[0], y = i0[1], z = i0[2];
  const double c00 = at_or_zero(chi, N, x, y, z) * (1.0 - f[0]) + at_or_zero(chi, N, x + 1, y, z) * f[0];
  const double c10 = at_or_zero(chi, N, x, y + 1, z) * (1.0 - f[0]) + at_or_zero(chi, N, x + 1, y + 1, z) * f[0];
  const double c01 = at_or_zero(chi, N, x, y, z + 1) * (1.0 - f[0]) + at_or_zero(chi, N, x + 1, y, z + 1) * f[0];
  const double c11 = at_or_zero(chi, N, x, y + 1, z + 1) * (1.0 - f[0]) + at_or_zero(chi, N, x + 1, y + 1, z + 1) * f[0];
  const double c0 = c00 * (1.0 - f[1]) + c10 * f[1];
  const double c1 = c01 * (1.0 - f[1]) + c11 * f[1];
  return c0 * (1.0 - f[2]) + c1 * f[2];
}

// ---------------------------------------------------------------------------------------------- rule 7: the extraction
// Cube corners are coded x + 2 y + 4 z.  Tetrahedron k of the Freudenthal split walks 0 -> 7 along the k-th permutation
// of the axes (lexicographic); an edge joins two corners a < b of one walk (a's bits a subset of b's), its class is
// (b - a) - 1 in 0..6 and its id (cell of a) * 7 + class.  A grid has N^3 points and (N - 1)^3 cubes; N need not be a
// power of two here.
struct TetTable {
  unsigned char corner[6][4];          // the walk of every tetrahedron
  unsigned char ntri[6][16];           // triangles of (tetrahedron, case); case bit i: corner[k][i] is inside
  unsigned char edge[6][16][2][3][2];  // (tetrahedron, case, triangle, vertex) -> the edge's corners (lower, upper)
};

inline void build_tet_table(TetTable& T) {
  static const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  memset(&T, 0, sizeof T);
  for (int k = 0; k < 6; ++k) {
    int c[4];
    c[0] = 0;
    c[1] = 1 << perm[k][0];
    c[2] = c[1] | (1 << perm[k][1]);
    c[3] = 7;
    for (int i = 0; i < 4; ++i) T.corner[k][i] = (unsigned char)c[i];
    for (int cs = 1; cs < 15; ++cs) {
      int in[4], out[4], ni = 0, no = 0;
      for (int i = 0; i < 4; ++i) {
        if (cs & (1 << i))
          in[ni++] = i;
        else
          out[no++] = i;
      }
      // the crossed edges as a cycle (pairs of walk positions: inside end, outside end)
      int cyc[4][2], nc = 0;
      if (ni == 1) {
        for (int j = 0; j < 3; ++j) cyc[nc][0] = in[0], cyc[nc][1] = out[j], ++nc;
      } else if (ni == 3) {
        for (int j = 0; j < 3; ++j) cyc[nc][0] = in[j], cyc[nc][1] = out[0], ++nc;
      } else {
        cyc[0][0] = in[0], cyc[0][1] = out[0];
        cyc[1][0] = in[0], cyc[1][1] = out[1];
        cyc[2][0] = in[1], cyc[2][1] = out[1];
        cyc[3][0] = in[1], cyc[3][1] = out[0];
        nc = 4;
      }
      // from the inside corners' centroid to the outside corners': the side the normals must face (scaled, exact)
      int dir[3] = {0, 0, 0};
      for (int a = 0; a < 3; ++a) {
        int so = 0, si = 0;
        for (int j = 0; j < no; ++j) so += (c[out[j]] >> a) & 1;
        for (int j = 0; j < ni; ++j) si += (c[in[j]] >> a) & 1;
        dir[a] = so * ni - si * no;
      }
      const int nt = nc - 2;
      T.ntri[k][cs] = (unsigned char)nt;
      for (int t = 0; t < nt; ++t) {
        int v[3] = {0, t + 1, t + 2};
        int m[3][3];  // twice the edges' midpoints
        for (int j = 0; j < 3; ++j)
          for (int a = 0; a < 3; ++a) m[j][a] = ((c[cyc[v[j]][0]] >> a) & 1) + ((c[cyc[v[j]][1]] >> a) & 1);
        int e1[3], e2[3];
        for (int a = 0; a < 3; ++a) e1[a] = m[1][a] - m[0][a], e2[a] = m[2][a] - m[0][a];
        const int nrm[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        if (nrm[0] * dir[0] + nrm[1] * dir[1] + nrm[2] * dir[2] < 0) {
          const int s = v[1];
          v[1] = v[2];
          v[2] = s;
        }
        for (int j = 0; j < 3; ++j) {
          const int p = cyc[v[j]][0], q = cyc[v[j]][1];
          T.edge[k][cs][t][j][0] = (unsigned char)c[p < q ? p : q];
          T.edge[k][cs][t][j][1] = (unsigned char)c[p < q ? q : p];
        }
      }
    }
  }
}

SFM_PSN_INLINE bool inside(double chi, double iso) { return chi < iso; }

// the crossed edges that start at grid point (x, y, z): bit k = class k
SFM_PSN_INLINE int edge_mask(const double* chi, int N, double iso, int x, int y, int z) {
  const bool a = inside(chi[((size_t)z * N + y) * N + x], iso);
  int m = 0;
  for (int k = 0; k < 7; ++k) {
    const int d = k + 1, X = x + (d & 1), Y = y + ((d >> 1) & 1), Z = z + (d >> 2);
    if (X >= N || Y >= N || Z >= N) continue;
    if (inside(chi[((size_t)Z * N + Y) * N + X], iso) != a) m |= 1 << k;
  }
  return m;
}
SFM_PSN_INLINE int popcount7(int m) {
  int n = 0;
  for (int k = 0; k < 7; ++k) n += (m >> k) & 1;
  return n;
}
// the vertex of edge (point, class): linear interpolation from the lower corner, cloud coordinates, float32
SFM_PSN_INLINE void edge_vertex(const double* chi, int N, double iso, const double o[3], double h, int x, int y, int z, int k,
                                float out[3]) {
  const int d = k + 1, dx = d & 1, dy = (d >> 1) & 1, dz = d >> 2;
  const double a = chi[((size_t)z * N + y) * N + x], b = chi[((size_t)(z + dz) * N + (y + dy)) * N + (x + dx)];
  const double t = (iso - a) / (b - a);
  out[0] = (float)(o[0] + (((double)x + 0.5) + t * (double)dx) * h);
  out[1] = (float)(o[1] + (((double)y + 0.5) + t * (double)dy) * h);
  out[2] = (float)(o[2] + (((double)z + 0.5) + t * (double)dz) * h);
}
// the 8 corners of cube (x, y, z): bit c = corner c is inside
SFM_PSN_INLINE int cube_mask(const double* chi, int N, double iso, int x, int y, int z) {
  int m = 0;
  for (int c = 0; c < 8; ++c)
    if (inside(chi[((size_t)(z + (c >> 2)) * N + (y + ((c >> 1) & 1))) * N + (x + (c & 1))], iso)) m |= 1 << c;
  return m;
}
SFM_PSN_INLINE int tet_case(const TetTable& T, int k, int cmask) {
  int cs = 0;
  for (int i = 0; i < 4; ++i) cs |= ((cmask >> T.corner[k][i]) & 1) << i;
  return cs;
}
SFM_PSN_INLINE int cube_triangles(const TetTable& T, int cmask) {
  if (cmask == 0 || cmask == 255) return 0;
  int n = 0;
  for (int k = 0; k < 6; ++k) n += T.ntri[k][tet_case(T, k, cmask)];
  return n;
}
// the triangles of cube (x, y, z) as vertex ids, 3 ints each, from the points' vertex offsets and crossed-edge masks
SFM_PSN_INLINE int cube_emit(const TetTable& T, int cmask, int N, int x, int y, int z, const int* voff, const unsigned char* vmask,
                             int* tri) {
  int n = 0;
  for (int k = 0; k < 6; ++k) {
    const int cs = tet_case(T, k, cmask);
    for (int t = 0; t < T.ntri[k][cs]; ++t) {
      for (int j = 0; j < 3; ++j) {
        const int lo = T.edge[k][cs][t][j][0], hi = T.edge[k][cs][t][j][1];
        const size_t p = ((size_t)(z + (lo >> 2)) * N + (y + ((lo >> 1) & 1))) * N + (x + (lo & 1));
        const int cls = (hi - lo) - 1;
        tri[3 * n + j] = voff[p] + popcount7(vmask[p] & ((1 << cls) - 1));
      }
      ++n;
    }
  }
  return n;
}

#ifndef __HIPCC__
// =============================================================================================== the host build
// The same pipeline with host loops (threads over slabs and bricks: the order inside a cell, a brick and a sum is the
// rule's, so the thread count does not change a bit).  This is what the device is compared against bit for bit.
namespace host {

template <class F>
inline void pfor(long long n, int threads, F f) {
  if (threads <= 1 || n < 2) {
    f(0ll, n);
    return;
  }
  const long long nt = std::min<long long>(threads, n), per = (n + nt - 1) / nt;
  std::vector<std::thread> th;
  for (long long t = 0; t < nt; ++t) {
    const long long a = t * per, b = std::min(n, a + per);
    if (a < b) th.emplace_back([=] { f(a, b); });
  }
  for (auto& t : th) t.join();
}

struct Samples {
  Cube g;
  int m = 0;
  std::vector<float> pts4, nrm4;
  std::vector<int> start, end;
};

// rule 1 + 2 and the ordering of rule 3
inline void make_samples(int n, const float* xyz, const float* nrm, int stride, const Opts& o, Samples& S) {
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  std::vector<int> idx;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!usable(p, nrm + (size_t)stride * i)) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = idx.empty() ? p[a] : std::min(lo[a], p[a]);
      hi[a] = idx.empty() ? p[a] : std::max(hi[a], p[a]);
    }
    idx.push_back(i);
  }
  S.m = (int)idx.size();
  S.g = make_cube(lo, hi, o.depth, o.scale);
  const size_t nc = (size_t)S.g.N * S.g.N * S.g.N;
  S.start.assign(nc, 0);
  S.end.assign(nc, 0);
  S.pts4.assign(4 * (size_t)std::max(S.m, 1), 0.f);
  S.nrm4.assign(4 * (size_t)std::max(S.m, 1), 0.f);
  if (S.m == 0) return;
  std::vector<int> key((size_t)S.m), cnt(nc + 1, 0);
  for (int s = 0; s < S.m; ++s) {
    key[s] = cell_key(S.g, xyz + 3 * (size_t)idx[s]);
    ++cnt[(size_t)key[s] + 1];
  }
  for (size_t c = 0; c < nc; ++c) cnt[c + 1] += cnt[c];
  for (size_t c = 0; c < nc; ++c)
    if (cnt[c + 1] > cnt[c]) S.start[c] = cnt[c], S.end[c] = cnt[c + 1];
  std::vector<int> fill(cnt.begin(), cnt.end() - 1);
  for (int s = 0; s < S.m; ++s) {  // (ascending input index inside a cell)
    const int d = fill[key[s]]++;
    const int i = idx[s];
    for (int a = 0; a < 3; ++a) {
      S.pts4[4 * (size_t)d + a] = xyz[3 * (size_t)i + a];
      S.nrm4[4 * (size_t)d + a] = nrm[(size_t)stride * i + a];
    }
    memcpy(&S.pts4[4 * (size_t)d + 3], &i, 4);
  }
}

// rules 3 + 4: V (3 N^3, axis-major), W, rhs
inline void splat_rhs(const Samples& S, std::vector<double>& V, std::vector<double>& W, std::vector<double>& rhs, int threads) {
  const int N = S.g.N;
  const size_t nc = (size_t)N * N * N;
  V.assign(3 * nc, 0.0);
  W.assign(nc, 0.0);
  rhs.assign(nc, 0.0);
  pfor(N, threads, [&](long long z0, long long z1) {
    for (int z = (int)z0; z < (int)z1; ++z)
      for (int y = 0; y < N; ++y)
        for (int x = 0; x < N; ++x) {
          double o4[4];
          splat_cell(S.g, S.pts4.data(), S.nrm4.data(), S.start.data(), S.end.data(), x, y, z, o4);
          const size_t c = ((size_t)z * N + y) * N + x;
          V[c] = o4[0];
          V[nc + c] = o4[1];
          V[2 * nc + c] = o4[2];
          W[c] = o4[3];
        }
  });
  pfor(N, threads, [&](long long z0, long long z1) {
    for (int z = (int)z0; z < (int)z1; ++z)
      for (int y = 0; y < N; ++y)
        for (int x = 0; x < N; ++x)
          rhs[((size_t)z * N + y) * N + x] = rhs_cell(V.data(), V.data() + nc, V.data() + 2 * nc, N, x, y, z);
  });
}

// sum of a(c) * b(c) over the grid in brick order
inline double dot_fixed(const double* a, const double* b, int N, std::vector<double>& part, int threads) {
  const Brick B = brick_dims(N);
  part.resize((size_t)B.n);
  pfor(B.n, threads, [&](long long b0, long long b1) {
    double v[CHUNK];
    for (int id = (int)b0; id < (int)b1; ++id) {
      for (int t = 0; t < CHUNK; ++t) {
        int x, y, z;
        v[t] = 0.0;
        if (brick_cell(B, id, t, x, y, z)) {
          const size_t c = ((size_t)z * N + y) * N + x;
          v[t] = a[c] * b[c];
        }
      }
      part[id] = chunk_tree(v);
    }
  });
  return sum_partials(part.data(), part.size());
}

// rule 5.  chi: N^3; returns the iterations; rr / bb: the final and the initial squared residual
inline int solve(int N, const double* rhs, const double* W, double point_weight, double rtol, int max_iter, std::vector<double>& chi,
                 double* rr_out, double* bb_out, int threads) {
  const size_t nc = (size_t)N * N * N;
  chi.assign(nc, 0.0);
  std::vector<double> r(rhs, rhs + nc), p(nc, 0.0), pn(nc, 0.0), q(nc, 0.0), dg(nc), part;
  for (size_t c = 0; c < nc; ++c) dg[c] = point_weight * W[c];
  double rr = dot_fixed(r.data(), r.data(), N, part, threads);
  const double bb = rr, tol2 = (rtol * rtol) * bb;
  double beta = 0.0;
  int it = 0;
  bool done = !(bb > 0.0);
  while (!done && it < max_iter) {
    pfor((long long)nc, threads, [&](long long a, long long b) {
      for (long long c = a; c < b; ++c) pn[c] = r[c] + beta * p[c];
    });
    p.swap(pn);
    pfor(N, threads, [&](long long z0, long long z1) {
      for (int z = (int)z0; z < (int)z1; ++z)
        for (int y = 0; y < N; ++y)
          for (int x = 0; x < N; ++x) {
            const size_t c = ((size_t)z * N + y) * N + x;
            q[c] = stencil(p[c], at_or_zero(p.data(), N, x - 1, y, z), at_or_zero(p.data(), N, x + 1, y, z),
                           at_or_zero(p.data(), N, x, y - 1, z), at_or_zero(p.data(), N, x, y + 1, z),
                           at_or_zero(p.data(), N, x, y, z - 1), at_or_zero(p.data(), N, x, y, z + 1), dg[c]);
          }
    });
    const double pq = dot_fixed(p.data(), q.data(), N, part, threads);
    const double alpha = rr / pq;
    pfor((long long)nc, threads, [&](long long a, long long b) {
      for (long long c = a; c < b; ++c) {
        chi[c] = chi[c] + alpha * p[c];
        r[c] = r[c] - alpha * q[c];
      }
    });
    const double rn = dot_fixed(r.data(), r.data(), N, part, threads);
    ++it;
    beta = rn / rr;
    rr = rn;
    if (rr <= tol2) done = true;
  }
  *rr_out = rr;
  *bb_out = bb;
  return it;
}

// rule 6
inline double iso_value(const Samples& S, const double* chi, int threads) {
  if (S.m == 0) return 0.0;
  const size_t nch = ((size_t)S.m + CHUNK - 1) / CHUNK;
  std::vector<double> part(nch);
  pfor((long long)nch, threads, [&](long long a, long long b) {
    double v[CHUNK];
    for (long long ch = a; ch < b; ++ch) {
      for (int t = 0; t < CHUNK; ++t) {
        const size_t s = (size_t)ch * CHUNK + t;
        v[t] = s < (size_t)S.m ? trilinear(chi, S.g, &S.pts4[4 * s]) : 0.0;
      }
      part[ch] = chunk_tree(v);
    }
  });
  return sum_partials(part.data(), nch) / (double)S.m;
}

// rule 7 on an N^3 grid of any N >= 2
inline void extract(const double* chi, int N, double iso, const double o[3], double h, std::vector<float>& verts,
                    std::vector<int>& tris) {
  verts.clear();
  tris.clear();
  if (N < 2) return;
  TetTable T;
  build_tet_table(T);
  const size_t nc = (size_t)N * N * N;
  std::vector<int> voff(nc);
  std::vector<unsigned char> vmask(nc);
  int nv = 0;
  for (int z = 0; z < N; ++z)
    for (int y = 0; y < N; ++y)
      for (int x = 0; x < N; ++x) {
        const size_t p = ((size_t)z * N + y) * N + x;
        const int m = edge_mask(chi, N, iso, x, y, z);
        vmask[p] = (unsigned char)m;
        voff[p] = nv;
        for (int k = 0; k < 7; ++k)
          if (m & (1 << k)) {
            float v[3];
            edge_vertex(chi, N, iso, o, h, x, y, z, k, v);
            verts.insert(verts.end(), v, v + 3);
            ++nv;
          }
      }
  for (int z = 0; z + 1 < N; ++z)
    for (int y = 0; y + 1 < N; ++y)
      for (int x = 0; x + 1 < N; ++x) {
        const int cm = cube_mask(chi, N, iso, x, y, z);
        if (cm == 0 || cm == 255) continue;
        int tri[36];
        const int n = cube_emit(T, cm, N, x, y, z, voff.data(), vmask.data(), tri);
        tris.insert(tris.end(), tri, tri + 3 * n);
      }
}

struct Result {
  Cube g;
  int m = 0, iterations = 0;
  double rr = 0, bb = 0, iso = 0;
  std::vector<double> chi;
  std::vector<float> verts;
  std::vector<int> tris;
};

inline void reconstruct(int n, const float* xyz, const float* nrm, int stride, const Opts& o, Result& R, int threads) {
  Samples S;
  make_samples(n, xyz, nrm, stride, o, S);
  R = Result();
  R.g = S.g;
  R.m = S.m;
  if (S.m < 1) return;
  std::vector<double> V, W, rhs;
  splat_rhs(S, V, W, rhs, threads);
  R.iterations = solve(S.g.N, rhs.data(), W.data(), o.point_weight, o.cg_rtol, max_iter_of(o), R.chi, &R.rr, &R.bb, threads);
  R.iso = iso_value(S, R.chi.data(), threads);
  extract(R.chi.data(), S.g.N, R.iso, S.g.o, S.g.h, R.verts, R.tris);
}

}  // namespace host
#endif  // !__HIPCC__

}  // namespace sfmpoisson
