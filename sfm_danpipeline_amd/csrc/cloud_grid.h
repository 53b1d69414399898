// cloud_grid.h -- the device-resident cloud (sfmhip_cloud), its uniform grids and the primitives the cloud family shares:
// cloud.hip (map3D's step 10), segment.hip (the colour region growing after it), poisson.hip (create_mesh), dendro.hip
// (the dendrometry after the segmentation), ground.hip (the ground plane that gives it its vertical), trees.hip (the trees of a plot) and, for blocks(), mvs.hip.  The bodies of the host functions declared here (grid builds, the handle's scan and cell sort) live
// in cloud.hip; the device helpers (cell_of, block_bound, row_span, the min / max kernel) are inline.
//
// Spatial index: cell coordinates floor((x - lo) / cell) in double, clamped to the grid (a far outlier lands in a
// border cell instead of stretching the grid: clamping keeps two points whose true cells are adjacent in adjacent
// cells, so no neighbour is lost), the linear cell id x-fastest, then rocPRIM's radix sort of (cell, point) pairs and
// a pass that records each cell's [start, end) in sorted order.  Non-finite points get the key one past the last cell
// and are in no cell.
#pragma once
#include "common.h"
#include "cloud.h"
#include <cmath>

namespace sfmgrid {

constexpr int CHUNK = 64;                 // points per radius_count workgroup (one wave)
constexpr long long AXIS_CAP = 1 << 12;   // cells per axis
constexpr long long CELL_CAP = 1 << 22;   // cells in all

struct GridDev {
  double o[3], cell;
  int D[3];
  int n_valid;
  const int* start;
  const int* end;
  const int* keys;    // sorted cell ids (n_valid)
  const float4* pts;  // sorted points, w = the input index's bits
};

struct Grid {
  bool built = false;
  double param = 0;  // the radius it was built for (radius grid)
  double o[3] = {0, 0, 0}, cell = 1;
  int D[3] = {1, 1, 1};
  long long ncell = 1;
  int nonempty = 0;
  int* start = nullptr;
  int* end = nullptr;
  int* keys = nullptr;
  float4* pts = nullptr;
  int4* chunks = nullptr;
  int n_chunks = 0;
  void release() {
    hipFree(start);
    hipFree(end);
    hipFree(keys);
    hipFree(pts);
    hipFree(chunks);
    start = end = keys = nullptr;
    pts = nullptr;
    chunks = nullptr;
    built = false;
    n_chunks = nonempty = 0;
  }
  GridDev dev(int n_valid) const {
    GridDev g;
    for (int a = 0; a < 3; ++a) {
      g.o[a] = o[a];
      g.D[a] = D[a];
    }
    g.cell = cell;
    g.n_valid = n_valid;
    g.start = start;
    g.end = end;
    g.keys = keys;
    g.pts = pts;
    return g;
  }
};

// the points a grid is built over: the handle's own cloud, or a subset gathered into an array of its own (at most as
// many points as the handle's cloud: the scratch arrays are sized by it)
struct GridSrc {
  const float* xyz;  // 3 n, on the device
  int n, n_valid;
  double lo[3], hi[3];  // box of the finite points
};

}  // namespace sfmgrid

struct sfmhip_cloud {
  sfmhip_ctx* ctx = nullptr;
  int n = 0, n_valid = 0;
  float* xyz = nullptr;          // 3 n, as given
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // box of the finite points
  sfmgrid::Grid rg, kg;          // radius grid, k-NN grid
  void* tmp = nullptr;           // rocPRIM temporary storage (grow-only)
  size_t tmp_bytes = 0;
  int* ibuf[4] = {nullptr, nullptr, nullptr, nullptr};  // 4 int scratch arrays of max(n, 1) (keys / values in, flags, scan)
  int* cbuf[2] = {nullptr, nullptr};                    // 2 int scratch arrays of ncell (chunk counts and offsets)
  long long cbuf_n = 0;
  void* seg = nullptr;           // segment.hip's state on this handle (the subset grid and its buffers), freed with it
  void (*seg_free)(void*) = nullptr;
  double psn_ms[4] = {0, 0, 0, 0};  // poisson.hip: stage times of the last sfmhip_cloud_poisson call on this handle
  void* psn = nullptr;           // poisson.hip's grow-only device blocks on this handle, freed with it
  void (*psn_free)(void*) = nullptr;
  void* dnd = nullptr;           // dendro.hip's state on this handle (frame, slice tables, stage times), freed with it
  void (*dnd_free)(void*) = nullptr;
  void* gnd = nullptr;           // ground.hip's state on this handle (selection list, hypotheses, counts, stage times), freed with it
  void (*gnd_free)(void*) = nullptr;
  void* trs = nullptr;           // trees.hip's state on this handle (frame coordinates, cell and voxel tables, keys, stage times), freed with it
  void (*trs_free)(void*) = nullptr;
  void* flt = nullptr;           // cloud_filter.hip's grow-only device blocks on this handle (run tables, attributes, mean distances), freed with it
  void (*flt_free)(void*) = nullptr;
  double flt_ms[4] = {0, 0, 0, 0};  // cloud_filter.hip: key + sort, voxel reduce (last voxel grid); neighbour means, threshold + compaction (last outlier call)
};

namespace sfmgrid {

inline unsigned blocks(long long n, int b) { return (unsigned)((n + b - 1) / b); }
int grow_tmp(sfmhip_cloud* c, size_t bytes);
int ensure_ibuf(sfmhip_cloud* c);
// common.h's exclusive scan of n >= 1 ints through the handle's tmp, on its stream; with `total`, the sum of `in`
int scan(sfmhip_cloud* c, const int* in, int* out, size_t n, int* total);
// rocPRIM's stable radix sort of n (cell id, point) pairs through the handle's tmp, over the bits that hold ids up to
// and including ncell (the key of a point that is in no cell)
int cell_sort(sfmhip_cloud* c, long long ncell, int* keys_in, int* keys_out, int* vals_in, int* vals_out, int n);
GridSrc whole_cloud(const sfmhip_cloud* c);
// build `g` over `src` with cells of `cell` (grown by 2 until the grid fits CELL_CAP); chunk list for the radius kernel if asked
int grid_build(sfmhip_cloud* c, const GridSrc& src, Grid& g, double cell, bool chunks);
// a grid sized by density: a first guess from the box volume, then rebuilds while the occupied cells hold far more
// points than `occupancy` (a surface fills few of the cells a volume estimate makes: cells shrink by the square root of
// the excess)
int density_grid(sfmhip_cloud* c, const GridSrc& src, Grid& g, double occupancy);
// the handle's k-NN grid (about 16 points per occupied cell), built on first use, and the slack its ring searches give
// the double rounding of a cell coordinate
int knn_grid(sfmhip_cloud* c);
double knn_abs_eps(const sfmhip_cloud* c);
// both filters' compaction: the 0/1 flags in ibuf[0] -> the kept indices, in input order, on the host
int compact(sfmhip_cloud* c, int32_t* idx_out, int32_t* n_out);
// a handle over n points that are on the device already (d_xyz: 3 max(n, 1) floats from sfm_dev_alloc; the handle owns
// it from here on, also when the call fails): the box by cloud_minmax, then n_valid
int adopt_device(sfmhip_ctx* ctx, float* d_xyz, int n, sfmhip_cloud** out);

#ifdef __HIPCC__
__device__ __forceinline__ int cell_of(double v, double o, double cell, int D) {
  double f = floor((v - o) / cell);
  f = f < 0.0 ? 0.0 : f;
  f = f > (double)(D - 1) ? (double)(D - 1) : f;
  return (int)f;
}

// distance from p to the nearest face of the block of cells [c - R, c + R] that has cells beyond it (+inf if none)
__device__ __forceinline__ double block_bound(const GridDev& g, const float4& p, const int c[3], int R) {
  const double pv[3] = {(double)p.x, (double)p.y, (double)p.z};
  double b = INFINITY;
  for (int a = 0; a < 3; ++a) {
    if (c[a] - R > 0) b = fmin(b, fmax(0.0, pv[a] - (g.o[a] + (double)(c[a] - R) * g.cell)));
    if (c[a] + R < g.D[a] - 1) b = fmin(b, fmax(0.0, (g.o[a] + (double)(c[a] + R + 1) * g.cell) - pv[a]));
  }
  return b;
}

// cells xa..xb of one x row merged into one span of sorted points [*s, *e) (the cells of a row are contiguous in
// sorted order; *s >= *e when all are empty)
__device__ __forceinline__ void row_span(const GridDev& g, int row, int xa, int xb, int* s, int* e) {
  *s = INT_MAX;
  *e = 0;
  for (int x = xa; x <= xb; ++x) {
    const int st = g.start[row + x], en = g.end[row + x];
    if (en > st) {
      *s = min(*s, st);
      *e = max(*e, en);
    }
  }
}

// the ordered keys (cloud.h) of the per-axis minima out[0..2] and maxima out[3..5] of the points ok(i, v) accepts
// (v: the three coordinates of point i) and their count out[6], by integer atomics: order-free
struct FinitePoint {  // cloud_minmax's predicate: the finite points
  __device__ bool operator()(long long, const float* v) const { return sfmcloud::finite3(v[0], v[1], v[2]); }
};

template <class Ok>
__global__ __launch_bounds__(256) void cloud_minmax(const float* xyz, int n, Ok ok, unsigned* out) {
  unsigned lo[3] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}, hi[3] = {0u, 0u, 0u}, cnt = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const float v[3] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]};
    if (!ok(i, v)) continue;
    ++cnt;
    for (int a = 0; a < 3; ++a) {
      const unsigned key = sfmcloud::ord_key(v[a]);
      lo[a] = min(lo[a], key);
      hi[a] = max(hi[a], key);
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    cnt += __shfl_xor(cnt, off);
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], (unsigned)__shfl_xor(lo[a], off));
      hi[a] = max(hi[a], (unsigned)__shfl_xor(hi[a], off));
    }
  }
  if ((threadIdx.x & 63) == 0 && cnt) {
    for (int a = 0; a < 3; ++a) {
      atomicMin(out + a, lo[a]);
      atomicMax(out + 3 + a, hi[a]);
    }
    atomicAdd(out + 6, cnt);
  }
}
#endif

}  // namespace sfmgrid
