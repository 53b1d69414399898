// cloud_grid.h -- the device-resident cloud (sfmhip_cloud), its uniform grids and everything the cloud family shares:
// cloud.hip (map3D's step 10), cloud_filter.hip (the voxel grid and the statistical outlier removal), register.hip (two clouds:
// nearest points and ICP, whose queries are not the grid's own points), align.hip (two levelled clouds: the pose vote), segment.hip (the colour
// region growing after it), poisson.hip (create_mesh), mesh.hip (the finishing of its mesh: queries that are the mesh's vertices), dendro.hip (the dendrometry after the segmentation), ground.hip (the
// ground plane that gives it its vertical), trees.hip (the trees of a plot), terrain.hip (the terrain under them), crowns.hip (the crowns
// on its canopy raster) and, for blocks(), mvs.hip.
// The handle plumbing is here once: a stage keeps its state in its slot of the handle's table (stage<S>(): made on first use,
// deleted with the handle, so a state owns its device memory through members with destructors -- DevBufs, Grow, Grid), a
// grow-only device array is a Grow<T>, and a min / max over points is minmax() into the handle's 7-word record.  A stage added
// to the family names itself in Stage, gives its state `static constexpr Stage slot`, and edits nothing else here.  The bodies of the host functions declared here (grid
// builds, the handle's scan and cell sort) live in cloud.hip; the device helpers (cell_of, block_bound, row_span, the min /
// max kernel) are inline.  The fixed-order block sum of f-9, f-11 and f-12 is block_sum.h's.
//
// Spatial index: cell coordinates floor((x - lo) / cell) in double, clamped to the grid (a far outlier lands in a
// border cell instead of stretching the grid: clamping keeps two points whose true cells are adjacent in adjacent
// cells, so no neighbour is lost), the linear cell id x-fastest, then rocPRIM's radix sort of (cell, point) pairs and
// a pass that records each cell's [start, end) in sorted order.  Non-finite points get the key one past the last cell
// and are in no cell.
#pragma once
#include "common.h"
#include "cloud.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace sfmgrid {

constexpr int CHUNK = 64;                 // points per radius_count workgroup (one wave)
using sfmcloud::AXIS_CAP;                 // cells per axis   (cloud.h: the grid geometry is shared with the CPU stubs)
using sfmcloud::CELL_CAP;                 // cells in all

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
  Grid() = default;
  Grid(const Grid&) = delete;
  Grid& operator=(const Grid&) = delete;
  ~Grid() { release(); }
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

// a grow-only device array: need(n) keeps the block when it holds n elements, else frees it and takes a new one from
// sfm_dev_alloc (so SFMHIP_POISON applies); old contents are never carried over.  Freed with its owner.
template <typename T>
struct Grow {
  T* p = nullptr;
  size_t cap = 0;
  Grow() = default;
  Grow(const Grow&) = delete;
  Grow& operator=(const Grow&) = delete;
  Grow(Grow&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }  // (for a std::vector of them)
  ~Grow() { hipFree(p); }
  int need(size_t n) {
    if (n <= cap && p) return SFMHIP_OK;
    hipFree(p);  // (synchronises: no launch of an earlier call still reads it)
    p = nullptr;
    cap = 0;
    SFM_TRY(sfm_dev_alloc(&p, n));
    cap = std::max(n, (size_t)1);
    return SFMHIP_OK;
  }
};

// the stages that keep state on the handle, and a stage's slot: the state and what deletes it
enum Stage { SEGMENT, POISSON, DENDRO, GROUND, TREES, FILTER, REGISTER, ALIGN, TERRAIN, CROWNS, MLS, MESH, N_STAGES };
struct StageSlot {
  void* p = nullptr;
  void (*free)(void*) = nullptr;
};

}  // namespace sfmgrid

struct sfmhip_cloud {
  sfmhip_ctx* ctx = nullptr;
  int n = 0, n_valid = 0;
  float* xyz = nullptr;          // 3 n, as given
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};  // box of the finite points
  sfmgrid::Grid rg, kg;          // radius grid, k-NN grid
  sfmgrid::Grow<unsigned char> tmp;  // rocPRIM temporary storage
  int* ibuf[4] = {nullptr, nullptr, nullptr, nullptr};  // 4 int scratch arrays of max(n, 1) (keys / values in, flags, scan)
  sfmgrid::Grow<int> cbuf[2];                           // 2 int scratch arrays of ncell (chunk counts and offsets)
  unsigned* mm = nullptr;        // 7 words: minmax()'s record, made and freed with the handle
  sfmgrid::StageSlot stage[sfmgrid::N_STAGES];  // the stages' state on this handle (stage<S>()), deleted with it
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
// the handle's radius grid for `radius` (cells of cloud.h's radius_cell(radius), with the chunk list: one entry per run of at
// most CHUNK points of one cell), kept until a call asks for another radius: radius_count, radius_outlier and mls.hip share it
int radius_grid(sfmhip_cloud* c, double radius);
double knn_abs_eps(const sfmhip_cloud* c);
// both filters' compaction: the 0/1 flags in ibuf[0] -> the kept indices, in input order, on the host
int compact(sfmhip_cloud* c, int32_t* idx_out, int32_t* n_out);
// a handle over n points that are on the device already (d_xyz: 3 max(n, 1) floats from sfm_dev_alloc; the handle owns
// it from here on, also when the call fails): the box by cloud_minmax, then n_valid
int adopt_device(sfmhip_ctx* ctx, float* d_xyz, int n, sfmhip_cloud** out);

// a struct of the C ABI and the header's struct it mirrors field for field: one as the other
template <class To, class From>
To mirror(const From& f) {
  static_assert(sizeof(To) == sizeof(From), "a struct of the C ABI mirrors the header's");
  To t;
  memcpy(&t, &f, sizeof t);
  return t;
}

// a stage's state on the handle, in the slot the state names (S::slot, so a state cannot be read out of another stage's
// slot): an S made on first use (stage times start at zero), deleted with the handle
template <class S>
S* stage(sfmhip_cloud* c) {
  StageSlot& s = c->stage[S::slot];
  if (!s.p) {
    s.p = new S();
    s.free = [](void* p) { delete (S*)p; };
  }
  return (S*)s.p;
}

#ifdef __HIPCC__
using sfmcloud::cell_of;  // (cloud.h's: one body for grid_build's kernel, the walks and the CPU stubs)

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

// the one min / max call: the start values into the handle's record, cloud_minmax<Ok> over the n points of xyz, the record
// into out[0..6], all on the handle's stream.  Does not wait: out is valid after the caller's next wait on the stream.  With
// no accepted point out[6] is 0 and out[0..5] are the start values, the keys of no float.
template <class Ok>
int minmax(sfmhip_cloud* c, const float* xyz, int n, Ok ok, unsigned out[7]) {
  static const unsigned init[7] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u, 0u};
  hipStream_t st = c->ctx->stream;
  SFM_HIP_TRY(hipMemcpyAsync(c->mm, init, sizeof init, hipMemcpyHostToDevice, st));
  if (n > 0) hipLaunchKernelGGL(cloud_minmax<Ok>, dim3(std::min(blocks(n, 256), 1024u)), dim3(256), 0, st, xyz, n, ok, c->mm);
  SFM_HIP_TRY(hipGetLastError());
  SFM_HIP_TRY(hipMemcpyAsync(out, c->mm, sizeof init, hipMemcpyDeviceToHost, st));
  return SFMHIP_OK;
}
#endif

}  // namespace sfmgrid
