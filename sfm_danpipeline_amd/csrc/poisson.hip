// poisson.hip -- the second half of StructFromMotion::create_mesh (reference src/Sfm.cpp:1365-1381: pcl::Poisson at
// depth 7 on the cloud and its flipped normals) on gfx950, on the device-resident cloud of cloud.hip.  The rules are
// DESIGN.md f-9's; the arithmetic is poisson.h's, which the CPU test stub compiles too, and every output is the same
// bits as that build's.  PCL parity is UNPINNED (uniform grid for PCL's octree, marching tetrahedra for its cubes).
//
// Samples: the usable points get their cell of the 2^depth cube as key (psn_keys), rocPRIM's stable radix sort orders
// them by (cell, input index) as cloud_grid.h's grids are ordered, psn_ranges records every cell's range.
// psn_splat: a thread per cell gathers the samples of its 27 neighbour cells in that order (no atomics).
// The solve is conjugate gradients on six f64 grid vectors.  One step is four launches:
//   psn_apply   a workgroup per brick of 16 x 4 x 4 cells: p = r + beta p for the brick and its face halo into LDS (p is
//               double-buffered: the neighbours' halo reads the old one), q = A p from the tile, the brick's part of p.q;
//   psn_reduce  one workgroup: the parts -> p.q, alpha;
//   psn_update  chi += alpha p, r -= alpha q, the brick's part of r.r;
//   psn_reduce  r.r, beta, the iteration count and the decision to stop, all in a record on the device.
// A stopped solve makes the remaining launches of a batch return at once; the host reads the record every CG_BATCH steps.
// Extraction: crossed edges per grid point and triangles per cube are counted, scanned (common.h) and written in place.
#include "common.h"
#include "cloud_grid.h"
#include "mesh_object.h"  // (sfmhip_mesh)
#include "poisson.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmpoisson;
using sfmgrid::blocks;
using sfmsum::block_tree;  // (block_sum.h: the chunk tree over the 256 threads of a workgroup)

namespace {

constexpr int CG_BATCH = 32;  // steps enqueued between two reads of the solve's record

struct Ctl {
  double rr, bb, pq, alpha, beta, tol2, sum;
  int iters, done, max_iter, pad;
};

// The device buffers of one call.  With a pool -- the cloud handle's: grow-only and freed with the handle, as its tmp /
// ibuf / cbuf are -- the k-th request of a call takes the pool's k-th block, which is replaced when it is too small: a
// repeat call on the handle allocates nothing (25 hipMalloc / hipFree pairs over 300 MB were 17 ms of a 44 ms call at
// depth 7).  The requests of sfmhip_cloud_poisson and sfmhip_cloud_poisson_splat come in the same order, so a block keeps
// its role.  Without a pool (the staged entries on a bare context) a block lives until the call ends.  Nothing relies on
// what a block holds when it is handed out.
struct Pool {  // on the cloud handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::POISSON;  // (its slot on the handle: stage<Pool>(cloud))
  std::vector<sfmgrid::Grow<unsigned char>> blk;
  double ms[4] = {0, 0, 0, 0};  // stage times of the last sfmhip_cloud_poisson call on the handle
};

struct Bufs {
  Pool* pool;
  size_t k = 0;
  DevBufs own;
  explicit Bufs(Pool* q = nullptr) : pool(q) {}
  template <typename T>
  int get(T** out, size_t n) {
    n = std::max(n, (size_t)1);
    if (!pool) return own.alloc(out, n);
    if (k == pool->blk.size()) pool->blk.emplace_back();
    SFM_TRY(pool->blk[k].need(n * sizeof(T)));
    *out = (T*)pool->blk[k++].p;
    return SFMHIP_OK;
  }
};

// ---------------------------------------------------------------------------------------------- samples
struct UsableSample {  // cloud_minmax's predicate: the points that are samples (rule 1)
  const float* nrm;
  int stride;
  __device__ bool operator()(long long i, const float* p) const {
    const float q[3] = {nrm[stride * i], nrm[stride * i + 1], nrm[stride * i + 2]};
    return usable(p, q);
  }
};

__global__ void psn_keys(const float* xyz, const float* nrm, int stride, int n, Cube g, int invalid, int* keys, int* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  const float q[3] = {nrm[(size_t)stride * i], nrm[(size_t)stride * i + 1], nrm[(size_t)stride * i + 2]};
  keys[i] = usable(p, q) ? cell_key(g, p) : invalid;
  vals[i] = i;
}

__global__ void psn_ranges(const float* xyz, const float* nrm, int stride, const int* keys, const int* vals, int m, int* start,
                           int* end, float4* pts, float4* nrs) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m) return;
  const int k = keys[s];
  if (s == 0 || keys[s - 1] != k) start[k] = s;
  if (s == m - 1 || keys[s + 1] != k) end[k] = s + 1;
  const size_t j = (size_t)vals[s];
  pts[s] = make_float4(xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2], __int_as_float((int)j));
  nrs[s] = make_float4(nrm[stride * j], nrm[stride * j + 1], nrm[stride * j + 2], 0.f);
}

// ---------------------------------------------------------------------------------------------- splat, right-hand side
// V4: Vx, Vy, Vz, W (nc each)
__global__ __launch_bounds__(256) void psn_splat(Cube g, const float* pts4, const float* nrm4, const int* start, const int* end,
                                                 double pw, double* V4, double* dg) {
  const size_t nc = (size_t)g.N * g.N * g.N;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int x = (int)(c % g.N), y = (int)((c / g.N) % g.N), z = (int)(c / ((size_t)g.N * g.N));
  double o4[4];
  splat_cell(g, pts4, nrm4, start, end, x, y, z, o4);
  V4[c] = o4[0];
  V4[nc + c] = o4[1];
  V4[2 * nc + c] = o4[2];
  V4[3 * nc + c] = o4[3];
  dg[c] = pw * o4[3];
}

__global__ __launch_bounds__(256) void psn_rhs(const double* V4, int N, double* rhs) {
  const size_t nc = (size_t)N * N * N;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int x = (int)(c % N), y = (int)((c / N) % N), z = (int)(c / ((size_t)N * N));
  rhs[c] = rhs_cell(V4, V4 + nc, V4 + 2 * nc, N, x, y, z);
}

__global__ __launch_bounds__(256) void psn_scale(const double* W, size_t nc, double pw, double* dg) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c < nc) dg[c] = pw * W[c];
}

// ---------------------------------------------------------------------------------------------- the solve
__global__ __launch_bounds__(256) void psn_dot_rr(const double* r, int N, Brick B, double* part) {
  __shared__ double sh4[4];
  int x, y, z;
  double v = 0.0;
  if (brick_cell(B, blockIdx.x, threadIdx.x, x, y, z)) {
    const double rv = r[((size_t)z * N + y) * N + x];
    v = rv * rv;
  }
  block_tree<1>(&v, &sh4);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// mode 0: r.r of the start (bb, the threshold, beta = 0); 1: p.q -> alpha; 2: r.r -> beta, the count, the decision; 3: a sum
__global__ __launch_bounds__(256) void psn_reduce(const double* part, int n, Ctl* ctl, int mode) {
  __shared__ double sh4[4];
  if ((mode == 1 || mode == 2) && ctl->done) return;
  double a = 0.0;
  for (int j = threadIdx.x; j < n; j += CHUNK) a = a + part[j];
  block_tree<1>(&a, &sh4);
  const double s = a;
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    ctl->rr = s;
    ctl->bb = s;
    ctl->tol2 = ctl->tol2 * s;  // (rtol * rtol) * bb
    ctl->beta = 0.0;
    ctl->iters = 0;
    ctl->done = (!(s > 0.0) || ctl->max_iter <= 0) ? 1 : 0;
  } else if (mode == 1) {
    ctl->pq = s;
    ctl->alpha = ctl->rr / s;
  } else if (mode == 2) {
    const int it = ctl->iters + 1;
    ctl->iters = it;
    ctl->beta = s / ctl->rr;
    ctl->rr = s;
    if (s <= ctl->tol2 || it >= ctl->max_iter) ctl->done = 1;
  } else {
    ctl->sum = s;
  }
}

// p_out = r + beta p_in on the brick, q = (L + dg) p_out, part = the brick's sum of p_out q
__global__ __launch_bounds__(256) void psn_apply(const double* __restrict__ r, const double* __restrict__ p_in,
                                                 double* __restrict__ p_out, double* __restrict__ q, const double* __restrict__ dg,
                                                 int N, Brick B, const Ctl* ctl, double* part) {
  __shared__ double tile[6 * 6 * 18];
  __shared__ double sh4[4];
  if (ctl->done) return;  // (uniform)
  const double beta = ctl->beta;
  const int id = blockIdx.x;
  const int x0 = (id % B.nx) * B.bx, y0 = ((id / B.nx) % B.ny) * B.by, z0 = (id / (B.nx * B.ny)) * B.bz;
  const int tx = B.bx + 2, ty = B.by + 2, tz = B.bz + 2;
  for (int i = threadIdx.x; i < tx * ty * tz; i += 256) {
    const int lx = i % tx - 1, ly = (i / tx) % ty - 1, lz = i / (tx * ty) - 1;
    const int outs = (lx < 0 || lx >= B.bx) + (ly < 0 || ly >= B.by) + (lz < 0 || lz >= B.bz);
    if (outs > 1) continue;  // (edges and corners of the halo: no stencil arm reads them)
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    double v = 0.0;
    if (gx >= 0 && gy >= 0 && gz >= 0 && gx < N && gy < N && gz < N) {
      const size_t c = ((size_t)gz * N + gy) * N + gx;
      v = r[c] + beta * p_in[c];
    }
    tile[i] = v;
  }
  __syncthreads();
  int x, y, z;
  double v = 0.0;
  if (brick_cell(B, id, threadIdx.x, x, y, z)) {
    const int lx = x - x0 + 1, ly = y - y0 + 1, lz = z - z0 + 1;
    const int i = (lz * ty + ly) * tx + lx;
    const size_t c = ((size_t)z * N + y) * N + x;
    const double pc = tile[i];
    const double qv = stencil(pc, tile[i - 1], tile[i + 1], tile[i - tx], tile[i + tx], tile[i - tx * ty], tile[i + tx * ty], dg[c]);
    p_out[c] = pc;
    q[c] = qv;
    v = pc * qv;
  }
  block_tree<1>(&v, &sh4);
  if (threadIdx.x == 0) part[id] = v;
}

__global__ __launch_bounds__(256) void psn_update(double* __restrict__ chi, double* __restrict__ r, const double* __restrict__ p,
                                                  const double* __restrict__ q, int N, Brick B, const Ctl* ctl, double* part) {
  __shared__ double sh4[4];
  if (ctl->done) return;  // (uniform)
  const double alpha = ctl->alpha;
  int x, y, z;
  double v = 0.0;
  if (brick_cell(B, blockIdx.x, threadIdx.x, x, y, z)) {
    const size_t c = ((size_t)z * N + y) * N + x;
    chi[c] = chi[c] + alpha * p[c];
    const double rv = r[c] - alpha * q[c];
    r[c] = rv;
    v = rv * rv;
  }
  block_tree<1>(&v, &sh4);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// ---------------------------------------------------------------------------------------------- iso-value
__global__ __launch_bounds__(256) void psn_iso_vals(const double* chi, Cube g, const float* pts4, int m, double* part) {
  __shared__ double sh4[4];
  const size_t s = (size_t)blockIdx.x * CHUNK + threadIdx.x;
  double v = s < (size_t)m ? trilinear(chi, g, pts4 + 4 * s) : 0.0;
  block_tree<1>(&v, &sh4);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}

// ---------------------------------------------------------------------------------------------- extraction
__global__ __launch_bounds__(256) void psn_classify_points(const double* chi, int N, double iso, int* vcnt, unsigned char* vmask) {
  const size_t nc = (size_t)N * N * N;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int x = (int)(c % N), y = (int)((c / N) % N), z = (int)(c / ((size_t)N * N));
  const int m = edge_mask(chi, N, iso, x, y, z);
  vmask[c] = (unsigned char)m;
  vcnt[c] = popcount7(m);
}

__global__ __launch_bounds__(256) void psn_classify_cubes(const double* chi, int N, double iso, const TetTable* T, int* tcnt) {
  const int M = N - 1;
  const size_t nq = (size_t)M * M * M;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nq) return;
  const int x = (int)(c % M), y = (int)((c / M) % M), z = (int)(c / ((size_t)M * M));
  tcnt[c] = cube_triangles(*T, cube_mask(chi, N, iso, x, y, z));
}

__global__ __launch_bounds__(256) void psn_emit_vertices(const double* chi, int N, double iso, Cube g, const int* voff,
                                                         const unsigned char* vmask, float* verts) {
  const size_t nc = (size_t)N * N * N;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nc) return;
  const int m = vmask[c];
  if (!m) return;
  const int x = (int)(c % N), y = (int)((c / N) % N), z = (int)(c / ((size_t)N * N));
  size_t o = (size_t)voff[c];
  for (int k = 0; k < 7; ++k)
    if (m & (1 << k)) {
      float v[3];
      edge_vertex(chi, N, iso, g.o, g.h, x, y, z, k, v);
      verts[3 * o] = v[0];
      verts[3 * o + 1] = v[1];
      verts[3 * o + 2] = v[2];
      ++o;
    }
}

__global__ __launch_bounds__(256) void psn_emit_triangles(const double* chi, int N, double iso, const TetTable* T, const int* toff,
                                                          const int* voff, const unsigned char* vmask, int* tris) {
  const int M = N - 1;
  const size_t nq = (size_t)M * M * M;
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= nq) return;
  const int x = (int)(c % M), y = (int)((c / M) % M), z = (int)(c / ((size_t)M * M));
  const int cm = cube_mask(chi, N, iso, x, y, z);
  if (cm == 0 || cm == 255) return;
  cube_emit(*T, cm, N, x, y, z, voff, vmask, tris + 3 * (size_t)toff[c]);
}

// ---------------------------------------------------------------------------------------------- host side
struct Samp {
  Cube g;
  int m = 0;
  float4* pts = nullptr;
  float4* nrs = nullptr;
  int* start = nullptr;
  int* end = nullptr;
};

Opts to_opts(const sfmhip_poisson_opts* o) { return Opts{o->depth, o->scale, o->point_weight, o->cg_rtol, o->cg_max_iter}; }

bool args_valid(const sfmhip_poisson_opts* o) { return o && (o->normal_stride == 3 || o->normal_stride == 4) && opts_valid(to_opts(o)); }

// rules 1-2 and the ordering of rule 3
int make_samples(sfmhip_cloud* c, const float* normals, int stride, const Opts& o, Bufs& B, Samp& S) {
  hipStream_t st = c->ctx->stream;
  const int n = c->n;
  float* d_nrm = nullptr;
  SFM_TRY(B.get(&d_nrm, (size_t)stride * n));
  unsigned mm[7];
  if (n > 0) SFM_HIP_TRY(hipMemcpyAsync(d_nrm, normals, sizeof(float) * (size_t)stride * n, hipMemcpyHostToDevice, st));
  SFM_TRY(sfmgrid::minmax(c, c->xyz, n, UsableSample{d_nrm, stride}, mm));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  S.m = (int)mm[6];
  if (S.m < 0 || S.m > n) return SFMHIP_ERR_STATE;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  if (S.m > 0)
    for (int a = 0; a < 3; ++a) lo[a] = sfmcloud::ord_val(mm[a]), hi[a] = sfmcloud::ord_val(mm[3 + a]);
  S.g = make_cube(lo, hi, o.depth, o.scale);
  if (S.m == 0) return SFMHIP_OK;
  const size_t nc = (size_t)S.g.N * S.g.N * S.g.N;
  SFM_TRY(sfmgrid::ensure_ibuf(c));  // keys in / out, points in / out: the arrays cloud_grid.h's cell sort uses
  int *kin = c->ibuf[0], *kout = c->ibuf[1], *vin = c->ibuf[2], *vout = c->ibuf[3];
  SFM_TRY(B.get(&S.start, nc));
  SFM_TRY(B.get(&S.end, nc));
  SFM_TRY(B.get(&S.pts, (size_t)S.m));
  SFM_TRY(B.get(&S.nrs, (size_t)S.m));
  SFM_HIP_TRY(hipMemsetAsync(S.start, 0, sizeof(int) * nc, st));
  SFM_HIP_TRY(hipMemsetAsync(S.end, 0, sizeof(int) * nc, st));
  hipLaunchKernelGGL(psn_keys, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, d_nrm, stride, n, S.g, (int)nc, kin, vin);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(sfmgrid::cell_sort(c, (long long)nc, kin, kout, vin, vout, n));
  hipLaunchKernelGGL(psn_ranges, dim3(blocks(S.m, 256)), dim3(256), 0, st, c->xyz, d_nrm, stride, kout, vout, S.m, S.start, S.end,
                     S.pts, S.nrs);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

// rules 3-4: V4 (Vx, Vy, Vz, W), dg = point_weight W, rhs
int splat_rhs(hipStream_t st, const Samp& S, double pw, double* V4, double* dg, double* rhs) {
  const size_t nc = (size_t)S.g.N * S.g.N * S.g.N;
  hipLaunchKernelGGL(psn_splat, dim3(blocks((long long)nc, 256)), dim3(256), 0, st, S.g, (const float*)S.pts, (const float*)S.nrs,
                     S.start, S.end, pw, V4, dg);
  hipLaunchKernelGGL(psn_rhs, dim3(blocks((long long)nc, 256)), dim3(256), 0, st, V4, S.g.N, rhs);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

// rule 5.  r holds the right-hand side and is overwritten; chi receives the solution
int solve(hipStream_t st, Bufs& B, int N, double* r, const double* dg, double rtol, int max_iter, double* chi, Ctl* out) {
  const size_t nc = (size_t)N * N * N;
  const Brick K = brick_dims(N);
  double *p0 = nullptr, *p1 = nullptr, *q = nullptr, *part = nullptr;
  Ctl* ctl = nullptr;
  SFM_TRY(B.get(&p0, nc));
  SFM_TRY(B.get(&p1, nc));
  SFM_TRY(B.get(&q, nc));
  SFM_TRY(B.get(&part, (size_t)K.n));
  SFM_TRY(B.get(&ctl, 1));
  Ctl h = {};
  h.tol2 = rtol * rtol;
  h.max_iter = max_iter;
  SFM_HIP_TRY(hipMemcpyAsync(ctl, &h, sizeof h, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(chi, 0, sizeof(double) * nc, st));
  SFM_HIP_TRY(hipMemsetAsync(p0, 0, sizeof(double) * nc, st));
  hipLaunchKernelGGL(psn_dot_rr, dim3((unsigned)K.n), dim3(256), 0, st, r, N, K, part);
  hipLaunchKernelGGL(psn_reduce, dim3(1), dim3(256), 0, st, part, K.n, ctl, 0);
  SFM_HIP_TRY(hipGetLastError());
  int launched = 0;
  for (;;) {
    for (int k = 0; k < CG_BATCH && launched < max_iter; ++k, ++launched) {
      double* pin = (launched & 1) ? p1 : p0;
      double* pout = (launched & 1) ? p0 : p1;
      hipLaunchKernelGGL(psn_apply, dim3((unsigned)K.n), dim3(256), 0, st, r, pin, pout, q, dg, N, K, ctl, part);
      hipLaunchKernelGGL(psn_reduce, dim3(1), dim3(256), 0, st, part, K.n, ctl, 1);
      hipLaunchKernelGGL(psn_update, dim3((unsigned)K.n), dim3(256), 0, st, chi, r, pout, q, N, K, ctl, part);
      hipLaunchKernelGGL(psn_reduce, dim3(1), dim3(256), 0, st, part, K.n, ctl, 2);
    }
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    if (h.done || launched >= max_iter) break;
  }
  *out = h;
  return SFMHIP_OK;
}

// rule 6
int iso_value(hipStream_t st, Bufs& B, const Samp& S, const double* chi, double* iso) {
  const int nch = (S.m + CHUNK - 1) / CHUNK;
  double* part = nullptr;
  Ctl* ctl = nullptr;
  SFM_TRY(B.get(&part, (size_t)nch));
  SFM_TRY(B.get(&ctl, 1));
  hipLaunchKernelGGL(psn_iso_vals, dim3((unsigned)nch), dim3(256), 0, st, chi, S.g, (const float*)S.pts, S.m, part);
  hipLaunchKernelGGL(psn_reduce, dim3(1), dim3(256), 0, st, part, nch, ctl, 3);
  SFM_HIP_TRY(hipGetLastError());
  Ctl h;
  SFM_HIP_TRY(hipMemcpyAsync(&h, ctl, sizeof h, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  *iso = h.sum / (double)S.m;
  return SFMHIP_OK;
}

// rule 7 on an N^3 grid (N >= 2)
int extract(hipStream_t st, Bufs& B, const double* chi, const Cube& g, double iso, sfmhip_mesh* mesh) {
  const int N = g.N, M = N - 1;
  const size_t nc = (size_t)N * N * N, nq = (size_t)M * M * M;
  TetTable T, *d_T = nullptr;
  build_tet_table(T);
  int *vcnt = nullptr, *voff = nullptr, *tcnt = nullptr, *toff = nullptr;
  unsigned char* vmask = nullptr;
  SFM_TRY(B.get(&d_T, 1));
  SFM_TRY(B.get(&vcnt, nc));
  SFM_TRY(B.get(&voff, nc));
  SFM_TRY(B.get(&vmask, nc));
  SFM_TRY(B.get(&tcnt, nq));
  SFM_TRY(B.get(&toff, nq));
  SFM_HIP_TRY(hipMemcpyAsync(d_T, &T, sizeof T, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(psn_classify_points, dim3(blocks((long long)nc, 256)), dim3(256), 0, st, chi, N, iso, vcnt, vmask);
  hipLaunchKernelGGL(psn_classify_cubes, dim3(blocks((long long)nq, 256)), dim3(256), 0, st, chi, N, iso, d_T, tcnt);
  SFM_HIP_TRY(hipGetLastError());
  long long nv = 0, nt = 0;
  auto scan = [&](const int* in, int* out, size_t n, long long* total) {  // (the temporary: one request to B per scan; n >= 1)
    size_t need = 0;
    unsigned char* tmp = nullptr;
    SFM_TRY(sfm_scan_bytes(n, st, &need));
    SFM_TRY(B.get(&tmp, need));
    return sfm_exclusive_scan(tmp, need, in, out, n, st, total);
  };
  SFM_TRY(scan(vcnt, voff, nc, &nv));
  SFM_TRY(scan(tcnt, toff, nq, &nt));
  if (nv < 0 || nt < 0 || nv > 7 * (long long)nc || nt > 12 * (long long)nq || 3 * nt > 0x7FFFFFFFll) return SFMHIP_ERR_STATE;
  mesh->verts.assign(3 * (size_t)nv, 0.f);
  mesh->tris.assign(3 * (size_t)nt, 0);
  if (nv == 0 || nt == 0) {
    mesh->verts.clear();
    mesh->tris.clear();
    return SFMHIP_OK;
  }
  float* verts = nullptr;
  int* tris = nullptr;
  SFM_TRY(B.get(&verts, 3 * (size_t)nv));
  SFM_TRY(B.get(&tris, 3 * (size_t)nt));
  hipLaunchKernelGGL(psn_emit_vertices, dim3(blocks((long long)nc, 256)), dim3(256), 0, st, chi, N, iso, g, voff, vmask, verts);
  hipLaunchKernelGGL(psn_emit_triangles, dim3(blocks((long long)nq, 256)), dim3(256), 0, st, chi, N, iso, d_T, toff, voff, vmask, tris);
  SFM_HIP_TRY(hipGetLastError());
  SFM_HIP_TRY(hipMemcpyAsync(mesh->verts.data(), verts, sizeof(float) * 3 * (size_t)nv, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(mesh->tris.data(), tris, sizeof(int) * 3 * (size_t)nt, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

void fill_summary(sfmhip_poisson_summary* s, const Samp& S, const Ctl& h, double iso, const sfmhip_mesh* mesh) {
  if (!s) return;
  s->n_samples = S.m;
  s->grid = S.g.N;
  s->n_vertices = mesh ? (int32_t)(mesh->verts.size() / 3) : 0;
  s->n_triangles = mesh ? (int32_t)(mesh->tris.size() / 3) : 0;
  s->cg_iterations = h.iters;
  s->cg_relative_residual = h.bb > 0.0 ? std::sqrt(h.rr / h.bb) : 0.0;
  s->iso_value = iso;
  for (int a = 0; a < 3; ++a) s->origin[a] = S.g.o[a];
  s->cell = S.g.h;
}

}  // namespace

extern "C" void sfmhip_poisson_default_opts(sfmhip_poisson_opts* o) {
  if (!o) return;
  const Opts r = reference_opts();
  o->depth = r.depth;
  o->scale = r.scale;
  o->point_weight = r.point_weight;
  o->cg_rtol = r.cg_rtol;
  o->cg_max_iter = r.cg_max_iter;
  o->normal_stride = 4;
}

extern "C" int sfmhip_cloud_poisson(sfmhip_cloud* c, const float* normals, const sfmhip_poisson_opts* opts, sfmhip_mesh** out,
                                    sfmhip_poisson_summary* summary) {
  if (!c || !out || !args_valid(opts) || (c->n > 0 && !normals)) return SFMHIP_ERR_ARG;
  *out = nullptr;
  const Opts o = to_opts(opts);
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  Pool* pool = sfmgrid::stage<Pool>(c);
  Bufs B(pool);
  Samp S;
  Ctl h = {};
  double iso = 0.0;
  sfmhip_mesh* mesh = new sfmhip_mesh();
  const double t0 = sfm_now_ms();
  double t1 = t0, t2 = t0;
  int rc = make_samples(c, normals, opts->normal_stride, o, B, S);
  if (rc == SFMHIP_OK && S.m > 0) {
    const size_t nc = (size_t)S.g.N * S.g.N * S.g.N;
    double *V4 = nullptr, *dg = nullptr, *r = nullptr, *chi = nullptr;
    if (rc == SFMHIP_OK) rc = B.get(&V4, 4 * nc);
    if (rc == SFMHIP_OK) rc = B.get(&dg, nc);
    if (rc == SFMHIP_OK) rc = B.get(&r, nc);
    if (rc == SFMHIP_OK) rc = B.get(&chi, nc);
    if (rc == SFMHIP_OK) rc = splat_rhs(st, S, o.point_weight, V4, dg, r);
    if (rc == SFMHIP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SFMHIP_ERR_HIP;
    t1 = sfm_now_ms();
    if (rc == SFMHIP_OK) rc = solve(st, B, S.g.N, r, dg, o.cg_rtol, max_iter_of(o), chi, &h);
    t2 = sfm_now_ms();
    if (rc == SFMHIP_OK) rc = iso_value(st, B, S, chi, &iso);
    if (rc == SFMHIP_OK) rc = extract(st, B, chi, S.g, iso, mesh);
  }
  const double t3 = sfm_now_ms();
  if (rc != SFMHIP_OK) {
    delete mesh;
    return rc;
  }
  pool->ms[0] = t1 - t0;
  pool->ms[1] = t2 - t1;
  pool->ms[2] = t3 - t2;
  pool->ms[3] = t3 - t0;
  fill_summary(summary, S, h, iso, mesh);
  *out = mesh;
  return SFMHIP_OK;
}

extern "C" int sfmhip_mesh_counts(const sfmhip_mesh* m, int32_t* n_vertices, int32_t* n_triangles) {
  if (!m || !n_vertices || !n_triangles) return SFMHIP_ERR_ARG;
  *n_vertices = (int32_t)(m->verts.size() / 3);
  *n_triangles = (int32_t)(m->tris.size() / 3);
  return SFMHIP_OK;
}

extern "C" int sfmhip_mesh_download(const sfmhip_mesh* m, float* vertices, int32_t* triangles) {
  if (!m || (!m->verts.empty() && !vertices) || (!m->tris.empty() && !triangles)) return SFMHIP_ERR_ARG;
  if (!m->verts.empty()) memcpy(vertices, m->verts.data(), m->verts.size() * sizeof(float));
  if (!m->tris.empty()) memcpy(triangles, m->tris.data(), m->tris.size() * sizeof(int32_t));
  return SFMHIP_OK;
}

extern "C" void sfmhip_mesh_destroy(sfmhip_mesh* m) { delete m; }

extern "C" int sfmhip_cloud_poisson_splat(sfmhip_cloud* c, const float* normals, const sfmhip_poisson_opts* opts, double* V, double* W,
                                          double* rhs, sfmhip_poisson_summary* summary) {
  if (!c || !args_valid(opts) || !V || !W || !rhs || (c->n > 0 && !normals)) return SFMHIP_ERR_ARG;
  const Opts o = to_opts(opts);
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  Bufs B(sfmgrid::stage<Pool>(c));
  Samp S;
  SFM_TRY(make_samples(c, normals, opts->normal_stride, o, B, S));
  const size_t nc = (size_t)S.g.N * S.g.N * S.g.N;
  if (S.m == 0) {
    memset(V, 0, sizeof(double) * 3 * nc);
    memset(W, 0, sizeof(double) * nc);
    memset(rhs, 0, sizeof(double) * nc);
  } else {
    double *V4 = nullptr, *dg = nullptr, *r = nullptr;
    SFM_TRY(B.get(&V4, 4 * nc));
    SFM_TRY(B.get(&dg, nc));
    SFM_TRY(B.get(&r, nc));
    SFM_TRY(splat_rhs(st, S, o.point_weight, V4, dg, r));
    SFM_HIP_TRY(hipMemcpyAsync(V, V4, sizeof(double) * 3 * nc, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(W, V4 + 3 * nc, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(rhs, r, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
  }
  fill_summary(summary, S, Ctl{}, 0.0, nullptr);
  return SFMHIP_OK;
}

extern "C" int sfmhip_poisson_solve(sfmhip_ctx* ctx, int depth, const double* rhs, const double* W, double point_weight, double cg_rtol,
                                    int cg_max_iter, double* chi, int32_t* iterations, double* rr_bb) {
  const Opts o{depth, 1.0, point_weight, cg_rtol, cg_max_iter};
  if (!ctx || !rhs || !W || !chi || !opts_valid(o)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = 1 << depth;
  const size_t nc = (size_t)N * N * N;
  Bufs B;
  double *r = nullptr, *w = nullptr, *dg = nullptr, *x = nullptr;
  SFM_TRY(B.get(&r, nc));
  SFM_TRY(B.get(&w, nc));
  SFM_TRY(B.get(&dg, nc));
  SFM_TRY(B.get(&x, nc));
  SFM_HIP_TRY(hipMemcpyAsync(r, rhs, sizeof(double) * nc, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(w, W, sizeof(double) * nc, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(psn_scale, dim3(blocks((long long)nc, 256)), dim3(256), 0, st, w, nc, point_weight, dg);
  SFM_HIP_TRY(hipGetLastError());
  Ctl h = {};
  SFM_TRY(solve(st, B, N, r, dg, cg_rtol, max_iter_of(o), x, &h));
  SFM_HIP_TRY(hipMemcpyAsync(chi, x, sizeof(double) * nc, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (iterations) *iterations = h.iters;
  if (rr_bb) rr_bb[0] = h.rr, rr_bb[1] = h.bb;
  return SFMHIP_OK;
}

extern "C" int sfmhip_poisson_extract(sfmhip_ctx* ctx, int n, const double* chi, double iso, const double* origin, double cell,
                                      sfmhip_mesh** out) {
  if (!ctx || n < 2 || n > (1 << DEPTH_MAX) || !chi || !origin || !out || !(cell > 0.0) || !(iso == iso)) return SFMHIP_ERR_ARG;
  *out = nullptr;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nc = (size_t)n * n * n;
  Bufs B;
  double* x = nullptr;
  SFM_TRY(B.get(&x, nc));
  SFM_HIP_TRY(hipMemcpyAsync(x, chi, sizeof(double) * nc, hipMemcpyHostToDevice, st));
  Cube g;
  g.N = n;
  g.h = cell;
  for (int a = 0; a < 3; ++a) g.o[a] = origin[a];
  sfmhip_mesh* mesh = new sfmhip_mesh();
  const int rc = extract(st, B, x, g, iso, mesh);
  if (rc != SFMHIP_OK) {
    delete mesh;
    return rc;
  }
  *out = mesh;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_poisson_last_timing(sfmhip_cloud* c, double* ms4) {
  if (!c || !ms4) return SFMHIP_ERR_ARG;
  const Pool* pool = sfmgrid::stage<Pool>(c);
  for (int i = 0; i < 4; ++i) ms4[i] = pool->ms[i];
  return SFMHIP_OK;
}
