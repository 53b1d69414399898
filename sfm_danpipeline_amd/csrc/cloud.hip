// cloud.hip -- map3D's step 10 (reference src/Sfm.cpp:94-102, bodies :1323-1383) on gfx950: PCL 1.8.1's PassThrough,
// RadiusOutlierRemoval and the k-nearest NormalEstimation, on a device-resident cloud (sfmhip_cloud) that uploads the
// points once and keeps one uniform grid per use.
//
// Spatial index: cell coordinates floor((x - lo) / cell) in double, clamped to the grid (a far outlier lands in a
// border cell instead of stretching the grid: clamping keeps two points whose true cells are adjacent in adjacent
// cells, so no neighbour is lost), the linear cell id x-fastest, then rocPRIM's radix sort of (cell, point) pairs and
// a pass that records each cell's [start, end) in sorted order.  Non-finite points get the key one past the last cell
// and are in no cell.  The radius grid has cells of r * (1 + 2^-10) (the margin covers the float rounding of d2 and
// the double rounding of the cell computation), so every neighbour lies in the 27 cells around a point, and the three
// cells of one x row are one contiguous range.  The k-NN grid is sized by density: about 16 points per occupied cell.
//
// cloud_radius_count: a workgroup of one wave per chunk of <= 64 points of one cell; the 9 row ranges around the cell are
// staged through LDS in tiles of 64 points and every lane tests its own point against the tile.  With a cap the wave
// leaves as soon as every lane has counted cap neighbours (counts are reported as min(count, cap)).
// cloud_knn (the k-NN lists, or the normals fused behind them): a lane per point in cell order; a ring search over the
// k-NN grid keeps a sorted (d2, index) list of KMAX slots in registers and stops once the nearest face of the searched
// block is farther than the k-th d2 (or the block covers the grid), so an unsearched point can neither be nearer nor
// tie; the covariance and the eigen step run on the final list.  Compaction (both filters): 0/1 flags, rocPRIM's
// exclusive scan, a scatter: input order kept.
// The arithmetic is cloud.h's, which the CPU test stub compiles too.
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmgrid;

namespace {

constexpr int KNN_BLOCK = 256;
constexpr double KNN_OCCUPANCY = 16.0;    // points per occupied cell the k-NN grid aims at

}  // namespace

int sfmgrid::grow_tmp(sfmhip_cloud* c, size_t bytes) { return c->tmp.need(bytes); }

int sfmgrid::scan(sfmhip_cloud* c, const int* in, int* out, size_t n, int* total) {
  size_t need = 0;
  long long t = 0;
  SFM_TRY(sfm_scan_bytes(n, c->ctx->stream, &need));
  SFM_TRY(grow_tmp(c, need));
  SFM_TRY(sfm_exclusive_scan(c->tmp.p, c->tmp.cap, in, out, n, c->ctx->stream, total ? &t : nullptr));
  if (total) *total = (int)t;
  return SFMHIP_OK;
}

int sfmgrid::cell_sort(sfmhip_cloud* c, long long ncell, int* keys_in, int* keys_out, int* vals_in, int* vals_out, int n) {
  unsigned bits = 1;
  while (bits < 31 && (1ll << bits) <= ncell) ++bits;
  size_t need = 0;
  SFM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, keys_in, keys_out, vals_in, vals_out, (unsigned)n, 0u, bits, c->ctx->stream));
  SFM_TRY(grow_tmp(c, need));
  SFM_HIP_TRY(rocprim::radix_sort_pairs(c->tmp.p, need, keys_in, keys_out, vals_in, vals_out, (unsigned)n, 0u, bits, c->ctx->stream));
  return SFMHIP_OK;
}

namespace {

__global__ void cloud_keys(const float* xyz, int n, GridDev g, int invalid, int* keys, int* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  int key = invalid;
  if (sfmcloud::finite3(x, y, z)) {
    const int cx = cell_of(x, g.o[0], g.cell, g.D[0]), cy = cell_of(y, g.o[1], g.cell, g.D[1]),
              cz = cell_of(z, g.o[2], g.cell, g.D[2]);
    key = (cz * g.D[1] + cy) * g.D[0] + cx;
  }
  keys[i] = key;
  vals[i] = i;
}

// per sorted point: the cell ranges, the sorted point record, and the count of occupied cells
__global__ void cloud_ranges(const float* xyz, const int* keys, const int* vals, int n_valid, int* start, int* end,
                             float4* pts, int* nonempty) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_valid) return;
  const int k = keys[i];
  const bool first = i == 0 || keys[i - 1] != k;
  if (first) {
    start[k] = i;
    atomicAdd(nonempty, 1);
  }
  if (i == n_valid - 1 || keys[i + 1] != k) end[k] = i + 1;
  const int j = vals[i];
  pts[i] = make_float4(xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], __int_as_float(j));
}

__global__ void cloud_chunk_counts(const int* start, const int* end, long long ncell, int* nch) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  nch[c] = (end[c] - start[c] + CHUNK - 1) / CHUNK;
}

__global__ void cloud_chunks(const int* start, const int* end, const int* nch, const int* off, long long ncell, int4* chunks) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncell) return;
  const int s = start[c], e = end[c];
  for (int j = 0; j < nch[c]; ++j) chunks[off[c] + j] = make_int4(s + j * CHUNK, min(CHUNK, e - s - j * CHUNK), (int)c, 0);
}

__global__ __launch_bounds__(CHUNK) void cloud_radius_count(GridDev g, const int4* chunks, float r2, int cap, int* counts) {
  __shared__ float4 tile[CHUNK];
  const int4 ch = chunks[blockIdx.x];
  const int lane = threadIdx.x;
  const bool live = lane < ch.y;
  const float4 p = g.pts[ch.x + (live ? lane : 0)];
  const int cx = ch.z % g.D[0], cy = (ch.z / g.D[0]) % g.D[1], cz = ch.z / (g.D[0] * g.D[1]);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.D[0] - 1);
  int cnt = 0;
  for (int z = max(cz - 1, 0); z <= min(cz + 1, g.D[2] - 1); ++z)
    for (int y = max(cy - 1, 0); y <= min(cy + 1, g.D[1] - 1); ++y) {
      const int row = (z * g.D[1] + y) * g.D[0];
      int s, e;
      row_span(g, row, x0, x1, &s, &e);
      for (int b = s; b < e; b += CHUNK) {
        __syncthreads();
        if (b + lane < e) tile[lane] = g.pts[b + lane];
        __syncthreads();
        const int m = min(CHUNK, e - b);
        for (int j = 0; j < m; ++j) {
          const float4 q = tile[j];
          cnt += sfmcloud::in_radius(sfmcloud::dist2(p.x, p.y, p.z, q.x, q.y, q.z), r2) ? 1 : 0;
        }
        if (cap > 0 && __all(!live || cnt >= cap)) goto done;  // (the workgroup is one wave: uniform)
      }
    }
done:
  if (live) counts[__float_as_int(p.w)] = cap > 0 ? min(cnt, cap) : cnt;
}

template <int N>
__device__ __forceinline__ void scan_cells(const GridDev& g, int row, int xa, int xb, const float4& p, float (&d)[N], int (&id)[N],
                                           int k, float& kd, int& ki) {
  int s, e;
  row_span(g, row, xa, xb, &s, &e);
  for (int j = s; j < e; ++j) {
    const float4 q = g.pts[j];
    const float dd = sfmcloud::dist2(p.x, p.y, p.z, q.x, q.y, q.z);
    const int qi = __float_as_int(q.w);
    if (sfmcloud::knn_less(dd, qi, kd, ki)) {
      sfmcloud::knn_insert<N>(d, id, dd, qi);
      sfmcloud::knn_kth<N>(d, id, k, kd, ki);
    }
  }
}

// mode 0: k-NN indices and d2; mode 1: normals (nx, ny, nz, curvature) of the k nearest
template <int N>
__global__ __launch_bounds__(KNN_BLOCK) void cloud_knn(GridDev g, double abs_eps, int k, int mode, const float* xyz, float vpx,
                                                       float vpy, float vpz, int* out_idx, float* out_d2, float* out4) {
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (i >= g.n_valid) return;
  const float4 p = g.pts[i];
  const int orig = __float_as_int(p.w);
  const int key = g.keys[i];
  const int c[3] = {key % g.D[0], (key / g.D[0]) % g.D[1], key / (g.D[0] * g.D[1])};
  float d[N];
  int id[N];
  sfmcloud::knn_init<N>(d, id);
  float kd = d[0];
  int ki = id[0];
  for (int R = 0;; ++R) {
    for (int z = max(c[2] - R, 0); z <= min(c[2] + R, g.D[2] - 1); ++z)
      for (int y = max(c[1] - R, 0); y <= min(c[1] + R, g.D[1] - 1); ++y) {
        const int row = (z * g.D[1] + y) * g.D[0];
        if (abs(z - c[2]) == R || abs(y - c[1]) == R) {
          scan_cells<N>(g, row, max(c[0] - R, 0), min(c[0] + R, g.D[0] - 1), p, d, id, k, kd, ki);
        } else {
          if (c[0] - R >= 0) scan_cells<N>(g, row, c[0] - R, c[0] - R, p, d, id, k, kd, ki);
          if (c[0] + R <= g.D[0] - 1) scan_cells<N>(g, row, c[0] + R, c[0] + R, p, d, id, k, kd, ki);
        }
      }
    const double b = block_bound(g, p, c, R);
    if (b == INFINITY) break;  // the block covers the grid
    if (ki != INT_MAX) {       // k entries: stop once every unsearched point is strictly farther than the k-th
      const double bs = b * (1.0 - 1.0 / 65536.0) - abs_eps;
      if (bs > 0.0 && bs * bs > (double)kd) break;
    }
  }
  const int kk = min(k, g.n_valid);
  if (mode == 0) {
#pragma unroll
    for (int s = 0; s < N; ++s)
      if (s < k) {
        out_idx[(size_t)orig * k + s] = s < kk ? id[s] : -1;
        out_d2[(size_t)orig * k + s] = s < kk ? d[s] : sfmcloud::bits_f(0x7F800000u);
      }
    return;
  }
  sfmcloud::Accu acc;
  sfmcloud::accu_zero(acc);
#pragma unroll
  for (int s = 0; s < N; ++s)
    if (s < kk) {
      const size_t j = (size_t)id[s];
      sfmcloud::accu_add(acc, xyz[3 * j], xyz[3 * j + 1], xyz[3 * j + 2]);
    }
  float cov[9], out[4];
  const float vp[3] = {vpx, vpy, vpz};
  if (kk >= 3) sfmcloud::accu_covariance(acc, kk, cov);
  sfmcloud::normal_from_cov(cov, kk, p.x, p.y, p.z, vp, out);
  *(float4*)(out4 + 4 * (size_t)orig) = make_float4(out[0], out[1], out[2], out[3]);
}

__global__ void cloud_flags_passthrough(const float* xyz, int n, int axis, float lo, float hi, int negative, int* flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = sfmcloud::passthrough_keep(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], axis, lo, hi,
                                        negative != 0) ? 1 : 0;
}

__global__ void cloud_flags_radius(const int* counts, int n, int min_pts, int* flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  flags[i] = sfmcloud::radius_keep(counts[i], min_pts) ? 1 : 0;  // (non-finite points count 0: removed)
}

__global__ void cloud_scatter(const int* flags, const int* off, int n, int* out, int* n_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (flags[i]) out[off[i]] = i;
  if (i == n - 1) *n_out = off[i] + flags[i];
}

}  // namespace

int sfmgrid::ensure_ibuf(sfmhip_cloud* c) {
  if (c->ibuf[0]) return SFMHIP_OK;
  for (int b = 0; b < 4; ++b) SFM_TRY(sfm_dev_alloc(&c->ibuf[b], (size_t)std::max(c->n, 1)));
  return SFMHIP_OK;
}

GridSrc sfmgrid::whole_cloud(const sfmhip_cloud* c) {
  GridSrc s;
  s.xyz = c->xyz;
  s.n = c->n;
  s.n_valid = c->n_valid;
  for (int a = 0; a < 3; ++a) {
    s.lo[a] = c->lo[a];
    s.hi[a] = c->hi[a];
  }
  return s;
}

int sfmgrid::grid_build(sfmhip_cloud* c, const GridSrc& src, Grid& g, double cell, bool chunks) {
  g.release();
  SFM_TRY(ensure_ibuf(c));
  hipStream_t st = c->ctx->stream;
  sfmcloud::GridGeom geom;
  sfmcloud::grid_geometry(src.lo, src.hi, src.n_valid, cell, geom);  // (cloud.h: the CPU stubs restate a walk's order from it)
  for (int a = 0; a < 3; ++a) g.o[a] = geom.o[a], g.D[a] = geom.D[a];
  g.cell = geom.cell;
  g.ncell = geom.ncell;
  SFM_TRY(sfm_dev_alloc(&g.start, (size_t)g.ncell));
  SFM_TRY(sfm_dev_alloc(&g.end, (size_t)g.ncell));
  SFM_TRY(sfm_dev_alloc(&g.keys, (size_t)std::max(src.n, 1)));
  SFM_TRY(sfm_dev_alloc(&g.pts, (size_t)std::max(src.n_valid, 1)));
  SFM_HIP_TRY(hipMemsetAsync(g.start, 0, sizeof(int) * g.ncell, st));
  SFM_HIP_TRY(hipMemsetAsync(g.end, 0, sizeof(int) * g.ncell, st));
  int* nonempty = c->ibuf[3];
  SFM_HIP_TRY(hipMemsetAsync(nonempty, 0, sizeof(int), st));
  if (src.n > 0) {
    int *kin = c->ibuf[0], *vin = c->ibuf[1], *vout = c->ibuf[2];
    GridDev gd = g.dev(src.n_valid);
    hipLaunchKernelGGL(cloud_keys, dim3(blocks(src.n, 256)), dim3(256), 0, st, src.xyz, src.n, gd, (int)g.ncell, kin, vin);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(cell_sort(c, g.ncell, kin, g.keys, vin, vout, src.n));
    if (src.n_valid > 0)
      hipLaunchKernelGGL(cloud_ranges, dim3(blocks(src.n_valid, 256)), dim3(256), 0, st, src.xyz, g.keys, vout, src.n_valid, g.start,
                         g.end, g.pts, nonempty);
    SFM_HIP_TRY(hipGetLastError());
  }
  SFM_HIP_TRY(hipMemcpyAsync(&g.nonempty, nonempty, sizeof(int), hipMemcpyDeviceToHost, st));
  if (chunks && src.n_valid > 0) {
    SFM_TRY(c->cbuf[0].need((size_t)g.ncell));
    SFM_TRY(c->cbuf[1].need((size_t)g.ncell));
    int *nch = c->cbuf[0].p, *off = c->cbuf[1].p;
    hipLaunchKernelGGL(cloud_chunk_counts, dim3(blocks(g.ncell, 256)), dim3(256), 0, st, g.start, g.end, g.ncell, nch);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(scan(c, nch, off, (size_t)g.ncell, &g.n_chunks));
    SFM_TRY(sfm_dev_alloc(&g.chunks, (size_t)std::max(g.n_chunks, 1)));
    hipLaunchKernelGGL(cloud_chunks, dim3(blocks(g.ncell, 256)), dim3(256), 0, st, g.start, g.end, nch, off, g.ncell, g.chunks);
    SFM_HIP_TRY(hipGetLastError());
  }
  SFM_HIP_TRY(hipStreamSynchronize(st));
  g.built = true;
  return SFMHIP_OK;
}

int sfmgrid::density_grid(sfmhip_cloud* c, const GridSrc& src, Grid& g, double occupancy) {
  double ext = 0, vol = 1;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, src.hi[a] - src.lo[a]);
  if (!(ext > 0)) ext = 1;
  for (int a = 0; a < 3; ++a) vol *= std::max(src.hi[a] - src.lo[a], ext * 1e-3);
  double cell = std::cbrt(vol * occupancy / std::max(src.n_valid, 1));
  SFM_TRY(grid_build(c, src, g, cell, false));
  for (int it = 0; it < 6 && g.nonempty > 0; ++it) {  // (a far outlier stretches the box: several rounds)
    const double occ = (double)src.n_valid / g.nonempty;
    if (occ <= 2 * occupancy) break;
    SFM_TRY(grid_build(c, src, g, g.cell * std::max(1e-3, std::sqrt(occupancy / occ)), false));
  }
  return SFMHIP_OK;
}

int sfmgrid::radius_grid(sfmhip_cloud* c, double radius) {
  if (c->rg.built && c->rg.param == radius) return SFMHIP_OK;
  SFM_TRY(grid_build(c, whole_cloud(c), c->rg, sfmcloud::radius_cell(radius), true));
  c->rg.param = radius;
  return SFMHIP_OK;
}

// the k-NN grid: about KNN_OCCUPANCY points per occupied cell
int sfmgrid::knn_grid(sfmhip_cloud* c) {
  if (c->kg.built) return SFMHIP_OK;
  return density_grid(c, whole_cloud(c), c->kg, KNN_OCCUPANCY);
}

double sfmgrid::knn_abs_eps(const sfmhip_cloud* c) {
  double mag = 0;
  for (int a = 0; a < 3; ++a) mag = std::max(mag, std::fabs(c->lo[a]) + std::fabs(c->hi[a]));
  return (mag + c->kg.cell) * 1e-12;  // (the double rounding of a cell coordinate, with room to spare)
}

int sfmgrid::compact(sfmhip_cloud* c, int32_t* idx_out, int32_t* n_out) {
  hipStream_t st = c->ctx->stream;
  int *flags = c->ibuf[0], *off = c->ibuf[1], *out = c->ibuf[2], *dn = c->ibuf[3];
  SFM_TRY(scan(c, flags, off, (size_t)c->n, nullptr));  // (c->n >= 1: the entry points return early on an empty cloud)
  hipLaunchKernelGGL(cloud_scatter, dim3(blocks(c->n, 256)), dim3(256), 0, st, flags, off, c->n, out, dn);
  SFM_HIP_TRY(hipGetLastError());
  int m = 0;
  SFM_HIP_TRY(hipMemcpyAsync(&m, dn, sizeof(int), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (m < 0 || m > c->n) return SFMHIP_ERR_STATE;
  if (m) SFM_HIP_TRY(hipMemcpyAsync(idx_out, out, sizeof(int) * m, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  *n_out = m;
  return SFMHIP_OK;
}

namespace {

int radius_counts_dev(sfmhip_cloud* c, double radius, int cap, int* d_counts) {
  SFM_TRY(radius_grid(c, radius));
  hipStream_t st = c->ctx->stream;
  SFM_HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(int) * c->n, st));
  if (c->rg.n_chunks > 0)
    hipLaunchKernelGGL(cloud_radius_count, dim3((unsigned)c->rg.n_chunks), dim3(CHUNK), 0, st, c->rg.dev(c->n_valid), c->rg.chunks,
                       sfmcloud::radius2(radius), cap, d_counts);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

int run_knn(sfmhip_cloud* c, int k, int mode, const float* vp, int* d_idx, float* d_d2, float* d_out4) {
  SFM_TRY(knn_grid(c));
  hipStream_t st = c->ctx->stream;
  const GridDev g = c->kg.dev(c->n_valid);
  const double abs_eps = knn_abs_eps(c);
  const float v0 = vp ? vp[0] : 0.f, v1 = vp ? vp[1] : 0.f, v2 = vp ? vp[2] : 0.f;
  if (c->n_valid > 0) {
    if (k <= 16)
      hipLaunchKernelGGL(cloud_knn<16>, dim3(blocks(c->n_valid, KNN_BLOCK)), dim3(KNN_BLOCK), 0, st, g, abs_eps, k, mode, c->xyz, v0,
                         v1, v2, d_idx, d_d2, d_out4);
    else
      hipLaunchKernelGGL(cloud_knn<sfmcloud::KMAX>, dim3(blocks(c->n_valid, KNN_BLOCK)), dim3(KNN_BLOCK), 0, st, g, abs_eps, k, mode,
                         c->xyz, v0, v1, v2, d_idx, d_d2, d_out4);
  }
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

// a device buffer of the context's scratch block 0 for one call's output
int out_buffer(sfmhip_cloud* c, size_t bytes, void** p) { return sfm_ctx_dev_scratch(c->ctx, 0, std::max(bytes, (size_t)4), p); }

}  // namespace

namespace {

int box_of(sfmhip_cloud* c) {
  unsigned mm[7] = {0u, 0u, 0u, 0u, 0u, 0u, 0u};
  if (c->n > 0) {
    SFM_TRY(minmax(c, c->xyz, c->n, FinitePoint(), mm));
    SFM_HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  }
  c->n_valid = (int)mm[6];
  for (int a = 0; a < 3; ++a) {
    c->lo[a] = c->n_valid ? (double)sfmcloud::ord_val(mm[a]) : 0.0;
    c->hi[a] = c->n_valid ? (double)sfmcloud::ord_val(mm[3 + a]) : 0.0;
  }
  return SFMHIP_OK;
}

}  // namespace

int sfmgrid::adopt_device(sfmhip_ctx* ctx, float* d_xyz, int n, sfmhip_cloud** out) {
  sfmhip_cloud* c = new sfmhip_cloud();
  c->ctx = ctx;
  c->n = n;
  c->xyz = d_xyz;
  int rc = sfm_dev_alloc(&c->mm, (size_t)7);
  if (rc == SFMHIP_OK) rc = box_of(c);
  if (rc != SFMHIP_OK) {
    sfmhip_cloud_destroy(c);
    return rc;
  }
  *out = c;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_create(sfmhip_ctx* ctx, int n, const float* xyz, sfmhip_cloud** out) {
  if (!ctx || !out || n < 0 || (n > 0 && !xyz)) return SFMHIP_ERR_ARG;
  *out = nullptr;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  float* d = nullptr;
  SFM_TRY(sfm_dev_alloc(&d, (size_t)3 * std::max(n, 1)));
  if (n > 0) {
    hipError_t e = hipMemcpyAsync(d, xyz, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
      g_sfmhip_last_hip_error = (int)e;
      hipFree(d);
      return SFMHIP_ERR_HIP;
    }
  }
  return adopt_device(ctx, d, n, out);
}

extern "C" void sfmhip_cloud_destroy(sfmhip_cloud* c) {
  if (!c) return;
  hipSetDevice(c->ctx->device);
  hipStreamSynchronize(c->ctx->stream);
  for (StageSlot& s : c->stage)
    if (s.p) s.free(s.p);
  hipFree(c->xyz);
  hipFree(c->mm);
  for (int b = 0; b < 4; ++b) hipFree(c->ibuf[b]);
  delete c;  // (the two grids, tmp and cbuf release themselves)
}

extern "C" int sfmhip_cloud_passthrough(sfmhip_cloud* c, int axis, float lo, float hi, int negative, int32_t* idx_out, int32_t* n_out) {
  if (!c || axis < 0 || axis > 2 || !n_out || (c->n > 0 && !idx_out)) return SFMHIP_ERR_ARG;
  *n_out = 0;
  if (c->n == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  SFM_TRY(ensure_ibuf(c));
  hipLaunchKernelGGL(cloud_flags_passthrough, dim3(blocks(c->n, 256)), dim3(256), 0, c->ctx->stream, c->xyz, c->n, axis, lo, hi,
                     negative, c->ibuf[0]);
  SFM_HIP_TRY(hipGetLastError());
  return compact(c, idx_out, n_out);
}

extern "C" int sfmhip_cloud_radius_count(sfmhip_cloud* c, double radius, int cap, int32_t* counts) {
  if (!c || !(radius > 0 && radius < 1e30) || (c->n > 0 && !counts)) return SFMHIP_ERR_ARG;
  if (c->n == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  void* d = nullptr;
  SFM_TRY(out_buffer(c, sizeof(int) * (size_t)c->n, &d));
  SFM_TRY(radius_counts_dev(c, radius, cap > 0 ? cap : 0, (int*)d));
  SFM_HIP_TRY(hipMemcpyAsync(counts, d, sizeof(int) * (size_t)c->n, hipMemcpyDeviceToHost, c->ctx->stream));
  SFM_HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_radius_outlier(sfmhip_cloud* c, double radius, int min_pts, int32_t* idx_out, int32_t* n_out) {
  if (!c || !(radius > 0 && radius < 1e30) || min_pts < 0 || min_pts == INT_MAX || !n_out || (c->n > 0 && !idx_out))
    return SFMHIP_ERR_ARG;
  *n_out = 0;
  if (c->n == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  SFM_TRY(ensure_ibuf(c));
  void* d = nullptr;
  SFM_TRY(out_buffer(c, sizeof(int) * (size_t)c->n, &d));
  SFM_TRY(radius_counts_dev(c, radius, min_pts + 1, (int*)d));  // (min(k, min_pts + 1) decides k <= min_pts)
  hipLaunchKernelGGL(cloud_flags_radius, dim3(blocks(c->n, 256)), dim3(256), 0, c->ctx->stream, (const int*)d, c->n, min_pts,
                     c->ibuf[0]);
  SFM_HIP_TRY(hipGetLastError());
  return compact(c, idx_out, n_out);
}

extern "C" int sfmhip_cloud_knn(sfmhip_cloud* c, int k, int32_t* idx, float* d2) {
  if (!c || k < 1 || k > sfmcloud::KMAX || (c->n > 0 && (!idx || !d2))) return SFMHIP_ERR_ARG;
  if (c->n == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  const size_t m = (size_t)c->n * k;
  void* d = nullptr;
  SFM_TRY(out_buffer(c, m * 8, &d));
  int* di = (int*)d;
  float* dd = (float*)((char*)d + m * 4);
  hipStream_t st = c->ctx->stream;
  SFM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)di, -1, m, st));  // non-finite points: -1 / +inf
  SFM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)dd, (int)0x7F800000, m, st));
  SFM_TRY(run_knn(c, k, 0, nullptr, di, dd, nullptr));
  SFM_HIP_TRY(hipMemcpyAsync(idx, di, m * 4, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(d2, dd, m * 4, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_normals(sfmhip_cloud* c, int k, const float* vp, float* out4) {
  if (!c || k < 1 || k > sfmcloud::KMAX || !vp || (c->n > 0 && !out4)) return SFMHIP_ERR_ARG;
  if (c->n == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  const size_t m = (size_t)c->n * 4;
  void* d = nullptr;
  SFM_TRY(out_buffer(c, m * 4, &d));
  hipStream_t st = c->ctx->stream;
  SFM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)d, (int)0x7FC00000, m, st));  // non-finite points: NaN
  SFM_TRY(run_knn(c, k, 1, vp, nullptr, nullptr, (float*)d));
  SFM_HIP_TRY(hipMemcpyAsync(out4, d, m * 4, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}
