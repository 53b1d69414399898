// trees.hip -- individual-tree extraction on gfx950 over the device-resident cloud of cloud.hip: the stems in a height band
// of the levelled cloud and, for every point above the ground, the number of the tree it belongs to.  The rules are
// DESIGN.md f-13's; the arithmetic is trees.h's, which the CPU test stub compiles too, and every output is the same bytes as
// that build's.
//
//   trs_frame     (e, n, h) of every point of A as float32, NaN elsewhere, and the counts of the selection and the band;
//   cloud_minmax  e_min, n_min and the maxima over A (cloud_grid.h: integer atomics on ordered keys);
//   trs_hist      the band histogram over the stem cells (integer atomics);
//   trs_cells / trs_hook / trs_flatten   the 8-connected components of the occupied cells: a union-find whose roots only move
//                 down (atomicMin), so that a component ends at its least cell id whatever the order;
//   trs_stats     per component the i64 sums, the cell count and the bounding box (integer atomics); trs_stem_flag and the
//                 handle's scan number the stems; trs_stem_emit writes one record per stem;
//   trs_vkeys     the voxel key of every point of A; the handle's cell sort; trs_heads + scan give the occupied voxels in
//                 ascending key order; trs_vox_emit the point -> voxel map, the key list and the seeds; trs_adj the 26
//                 neighbours of every voxel by binary search in the key list, once;
//   trs_sweep     the hot loop: a thread per voxel pulls min(key(u) + w) over its neighbours and stores it when it is
//                 smaller; only the voxel's own thread writes its key, keys only fall, and a sweep that changes nothing is
//                 rule 8's fixed point.  The host enqueues 16 sweeps, reads the counter of changed keys, and stops at 0;
//   trs_vlabel / trs_plabel   the tree of every voxel and point, the points per tree, the largest cost.
// No spin, no hand-off between workgroups, no float atomic.  Launches are ordered by the stream alone.
#include "common.h"
#include "cloud_grid.h"
#include "trees.h"
#include "union_find.h"
#include <algorithm>
#include <climits>
#include <cmath>

using namespace sfmtrees;
using sfmgrid::blocks;
using sfmgrid::mirror;  // (the options in, the defaults and the result out: size-checked)

static_assert(sizeof(sfmhip_tree_stem) == sizeof(Stem), "sfmhip_tree_stem mirrors sfmtrees::Stem");

namespace {

constexpr int BATCH = 16;  // sweeps between two reads of the counter

typedef unsigned long long u64;

struct Totals {  // trs_frame's and trs_vlabel's counts
  unsigned selected, band, labelled, pad;
  u64 max_cost;
};

struct TrsState {  // on the cloud handle, freed with it; the cloud's size never changes, so the blocks sized by it are made once
  static constexpr sfmgrid::Stage slot = sfmgrid::TREES;  // (its slot on the handle: stage<TrsState>(cloud))
  DevBufs B;
  bool ready = false;
  int* labels = nullptr;    // n
  float* enh = nullptr;     // 3 n
  int* tree_of = nullptr;   // n
  int* pvox = nullptr;      // n: the voxel of a point, -1 outside A
  int* head = nullptr;      // n
  int* hx = nullptr;        // n
  int* ukey = nullptr;      // n: the occupied voxels' keys, ascending
  int* vstart = nullptr;    // n + 1: a voxel's first position in sorted order
  int* vlabel = nullptr;    // n
  u64* key = nullptr;       // n: rule 8's keys
  long long* sums = nullptr;  // 3 n: Se, Sn, N per occupied cell's slot
  int* box = nullptr;       // 6 n: cells, x0, x1, y0, y1, root cell per slot
  int* sflag = nullptr;     // n
  int* sno = nullptr;       // n
  int* stem_of = nullptr;   // n: the stem of a slot, -1 for none
  StemSums* stems = nullptr;  // MAX_TREES
  int* pts = nullptr;       // MAX_TREES
  Totals* tot = nullptr;    // 1
  unsigned* changed = nullptr;  // 1
  sfmgrid::Grow<int> cells;  // 4 per stem cell: count, parent, occupied, slot
  sfmgrid::Grow<int> adj;    // 26 per voxel: adj[k nv + v]
  double ms[6] = {0, 0, 0, 0, 0, 0};
  int sweeps = 0;
};

int trs_alloc(sfmhip_cloud* c, TrsState* s) {
  if (s->ready) return SFMHIP_OK;
  const size_t n = (size_t)std::max(c->n, 1);
  SFM_TRY(s->B.alloc(&s->labels, n));
  SFM_TRY(s->B.alloc(&s->enh, 3 * n));
  SFM_TRY(s->B.alloc(&s->tree_of, n));
  SFM_TRY(s->B.alloc(&s->pvox, n));
  SFM_TRY(s->B.alloc(&s->head, n));
  SFM_TRY(s->B.alloc(&s->hx, n));
  SFM_TRY(s->B.alloc(&s->ukey, n));
  SFM_TRY(s->B.alloc(&s->vstart, n + 1));
  SFM_TRY(s->B.alloc(&s->vlabel, n));
  SFM_TRY(s->B.alloc(&s->key, n));
  SFM_TRY(s->B.alloc(&s->sums, 3 * n));
  SFM_TRY(s->B.alloc(&s->box, 6 * n));
  SFM_TRY(s->B.alloc(&s->sflag, n));
  SFM_TRY(s->B.alloc(&s->sno, n));
  SFM_TRY(s->B.alloc(&s->stem_of, n));
  SFM_TRY(s->B.alloc(&s->stems, (size_t)MAX_TREES));
  SFM_TRY(s->B.alloc(&s->pts, (size_t)MAX_TREES));
  SFM_TRY(s->B.alloc(&s->tot, 1));
  SFM_TRY(s->B.alloc(&s->changed, 1));
  s->ready = true;
  return SFMHIP_OK;
}

struct InA {  // cloud_minmax's predicate over the frame coordinates: trs_frame wrote NaN outside A
  __device__ bool operator()(long long, const float* v) const { return v[2] == v[2]; }
};

__global__ __launch_bounds__(256) void trs_frame(const float* xyz, const int* labels, int label, int n, Prep p, float* enh, Totals* tot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int cls = C_OUT;
  if (i < n) {
    const float q[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
    float o[3];
    const bool sel = sfmdendro::frame_point(p.f, q, !labels || labels[i] == label, o);
    cls = classify(sel, o[2], p.h0, p.clear, p.lo, p.hi);
    const bool in_a = cls >= C_ABOVE;
    enh[3 * (size_t)i] = in_a ? o[0] : sfmcloud::qnan();
    enh[3 * (size_t)i + 1] = in_a ? o[1] : sfmcloud::qnan();
    enh[3 * (size_t)i + 2] = in_a ? o[2] : sfmcloud::qnan();
  }
  const unsigned sel = (unsigned)__popcll(__ballot(cls != C_OUT)), band = (unsigned)__popcll(__ballot(cls == C_BAND));
  if ((threadIdx.x & 63) == 0) {
    if (sel) atomicAdd(&tot->selected, sel);
    if (band) atomicAdd(&tot->band, band);
  }
}

// the class of a point of the frame array (C_BELOW stands for everything outside A there)
__device__ __forceinline__ int class_of(const float* enh, int i, const Prep& p, float o[3]) {
  o[0] = enh[3 * (size_t)i], o[1] = enh[3 * (size_t)i + 1], o[2] = enh[3 * (size_t)i + 2];
  return classify(true, o[2], p.h0, p.clear, p.lo, p.hi);
}

__global__ __launch_bounds__(256) void trs_hist(const float* enh, int n, Prep p, Dims d, int ncell, int* count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float o[3];
  if (class_of(enh, i, p, o) != C_BAND) return;
  const int cell = cell_of(o, d, p.c);
  if (cell >= 0 && cell < ncell) atomicAdd(count + cell, 1);  // (always: the grid was sized by these points' own bounds)
}

__global__ __launch_bounds__(256) void trs_cells(const int* count, int ncell, int min_cell_pts, int* parent, int* occupied) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ncell) return;
  const bool occ = count[q] >= min_cell_pts;
  parent[q] = occ ? q : -1;
  occupied[q] = occ ? 1 : 0;
}

using sfmuf::root_of;  // (union_find.h: shared with tracks.hip)
using sfmuf::unite;

__global__ __launch_bounds__(256) void trs_hook(int* parent, int De, int Dn) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= De * Dn || parent[q] < 0) return;
  const int x = q % De, y = q / De;
  // the four neighbours after q in cell order; the other four hook q from their side
  if (x + 1 < De && parent[q + 1] >= 0) unite(parent, q, q + 1);
  if (y + 1 < Dn) {
    const int r = q + De;
    if (x > 0 && parent[r - 1] >= 0) unite(parent, q, r - 1);
    if (parent[r] >= 0) unite(parent, q, r);
    if (x + 1 < De && parent[r + 1] >= 0) unite(parent, q, r + 1);
  }
}

__global__ __launch_bounds__(256) void trs_flatten(int* parent, int ncell) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ncell || parent[q] < 0) return;
  const int r = root_of(parent, q);
  __hip_atomic_store(parent + q, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void trs_stats_init(int n_occ, long long* sums, int* box) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_occ) return;
  sums[3 * (size_t)j] = sums[3 * (size_t)j + 1] = sums[3 * (size_t)j + 2] = 0;
  int* b = box + 6 * (size_t)j;
  b[0] = 0, b[1] = INT_MAX, b[2] = -1, b[3] = INT_MAX, b[4] = -1, b[5] = -1;
}

__global__ __launch_bounds__(256) void trs_stats(const int* count, const int* parent, const int* slot, int ncell, int De, int n_occ,
                                                 long long* sums, int* box) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ncell || parent[q] < 0) return;
  const int r = parent[q], j = slot[r];
  if (j < 0 || j >= n_occ) return;  // (never: r is an occupied cell)
  const int x = q % De, y = q / De;
  const long long k = count[q];
  atomicAdd((u64*)(sums + 3 * (size_t)j), (u64)(k * (2 * x + 1)));
  atomicAdd((u64*)(sums + 3 * (size_t)j + 1), (u64)(k * (2 * y + 1)));
  atomicAdd((u64*)(sums + 3 * (size_t)j + 2), (u64)k);
  int* b = box + 6 * (size_t)j;
  atomicAdd(b, 1);
  atomicMin(b + 1, x);
  atomicMax(b + 2, x);
  atomicMin(b + 3, y);
  atomicMax(b + 4, y);
  if (q == r) b[5] = q;
}

__global__ __launch_bounds__(256) void trs_stem_flag(int n_occ, const long long* sums, const int* box, int min_stem_pts, double c, double w,
                                                     int* sflag) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_occ) return;
  const int* b = box + 6 * (size_t)j;  // (a slot that is no root holds N = 0 < min_stem_pts)
  sflag[j] = b[5] >= 0 && is_stem(sums[3 * (size_t)j + 2], b[1], b[2], b[3], b[4], min_stem_pts, c, w) ? 1 : 0;
}

__global__ __launch_bounds__(256) void trs_stem_emit(int n_occ, const int* sflag, const int* sno, int T, const long long* sums, const int* box,
                                                     StemSums* stems, int* stem_of) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n_occ) return;
  const int s = sflag[j] && sno[j] < T ? sno[j] : -1;
  stem_of[j] = s;
  if (s < 0) return;
  StemSums r;
  r.Se = sums[3 * (size_t)j], r.Sn = sums[3 * (size_t)j + 1], r.N = sums[3 * (size_t)j + 2];
  r.cells = box[6 * (size_t)j];
  r.cell_id = box[6 * (size_t)j + 5];
  stems[s] = r;
}

__global__ __launch_bounds__(256) void trs_vkeys(const float* enh, int n, Prep p, Dims d, int nvox, int* keys, int* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float o[3];
  int key = nvox;
  if (class_of(enh, i, p, o) >= C_ABOVE) {
    key = voxel_of(o, d, p.h0, p.v);
    if (key < 0 || key >= nvox) key = nvox;  // (never: the grid was sized by these points' own bounds)
  }
  keys[i] = key;
  vals[i] = i;
}

__global__ __launch_bounds__(256) void trs_heads(const int* keys, int n, int n_above, int nvox, int* head) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  head[i] = i < n_above && keys[i] < nvox && (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

// per sorted point of A: its voxel; at a voxel's first point the key and the start; rule 7's seeds
__global__ __launch_bounds__(256) void trs_vox_emit(const int* keys, const int* vals, const int* head, const int* hx, int n, int n_above,
                                                    int nvox, int nv, const float* enh, Prep p, Dims d, int ncell, const int* parent,
                                                    const int* slot, int n_occ, const int* stem_of, int* pvox, int* ukey, int* vstart, u64* key) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) vstart[nv] = n_above;
  if (i >= n_above || i >= n || keys[i] >= nvox) return;
  const int v = hx[i] + head[i] - 1, pt = vals[i];
  if (v < 0 || v >= nv || pt < 0 || pt >= n) return;  // (never)
  pvox[pt] = v;
  if (head[i]) {
    ukey[v] = keys[i];
    vstart[v] = i;
  }
  float o[3];
  if (class_of(enh, pt, p, o) != C_BAND) return;
  const int cell = cell_of(o, d, p.c);
  if (cell < 0 || cell >= ncell) return;  // (never)
  const int r = parent[cell];
  if (r < 0) return;
  const int j = slot[r];
  const int s = j >= 0 && j < n_occ ? stem_of[j] : -1;
  if (s >= 0) atomicMin(key + v, (u64)s);
}

__global__ __launch_bounds__(256) void trs_adj(const int* __restrict__ ukey, int nv, Dims d, int* __restrict__ adj) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x, k = blockIdx.y;
  if (v >= nv) return;
  const int nk = neighbour_key(ukey[v], k, d);
  adj[(size_t)k * nv + v] = nk < 0 ? -1 : find_voxel(ukey, nv, nk);
}

// one sweep of rule 8.  key[v] is written by v's thread alone; the neighbours' keys are read as they are at that moment, each
// the cost of a real path, so every store is an upper bound of the fixed point and lowers v's key.
__global__ __launch_bounds__(256) void trs_sweep(u64* key, const int* __restrict__ adj, int nv, unsigned* changed) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  bool moved = false;
  if (v < nv) {
    int u[STEPS];
#pragma unroll
    for (int k = 0; k < STEPS; ++k) u[k] = adj[(size_t)k * nv + v];
    const u64 own = __hip_atomic_load(key + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    u64 best = own;
#pragma unroll
    for (int k = 0; k < STEPS; ++k) {
      const u64 ku = __hip_atomic_load(key + (u[k] < 0 ? v : u[k]), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const u64 cand = relax(ku, step_weight(k));  // (u = v: own + w, never smaller)
      best = cand < best ? cand : best;
    }
    if (best < own) {
      __hip_atomic_store(key + v, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      moved = true;
    }
  }
  const unsigned m = (unsigned)__popcll(__ballot(moved));
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(changed, m);
}

__global__ __launch_bounds__(256) void trs_vlabel(const u64* key, const int* vstart, int nv, double cap, int T, int* vlabel, int* pts, Totals* tot) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned labelled = 0;
  u64 cost = 0;
  if (v < nv) {
    const u64 k = key[v];
    const int s = voxel_tree(k, cap);
    vlabel[v] = s;
    if (s >= 0 && s < T) {
      labelled = (unsigned)(vstart[v + 1] - vstart[v]);
      cost = (u64)key_cost(k);
      atomicAdd(pts + s, (int)labelled);
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    labelled += __shfl_xor(labelled, off);
    const u64 o = __shfl_xor(cost, off);
    cost = o > cost ? o : cost;
  }
  if ((threadIdx.x & 63) == 0 && labelled) {
    atomicAdd(&tot->labelled, labelled);
    atomicMax(&tot->max_cost, cost);
  }
}

__global__ __launch_bounds__(256) void trs_plabel(const int* pvox, const int* vlabel, int n, int nv, int* tree_of) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int v = pvox[i];
  tree_of[i] = v >= 0 && v < nv ? vlabel[v] : -1;
}

#define TRS_LAUNCH(kernel, grid, ...)                                              \
  do {                                                                             \
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, __VA_ARGS__);               \
    SFM_HIP_TRY(hipGetLastError());                                                \
  } while (0)

int run(sfmhip_cloud* c, const int32_t* labels, int32_t label, const Opts& o, int32_t* tree_of, int cap, Stem* stems, Result& res) {
  Prep p;
  if (!prepare(o, p)) return SFMHIP_ERR_ARG;
  TrsState* s = sfmgrid::stage<TrsState>(c);
  for (double& m : s->ms) m = 0;
  s->sweeps = 0;
  empty_result(res, F_NONE_ABOVE);
  const int n = c->n;
  if (n <= 0) return SFMHIP_OK;
  for (int i = 0; i < n; ++i) tree_of[i] = -1;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  SFM_TRY(sfmgrid::ensure_ibuf(c));
  SFM_TRY(trs_alloc(c, s));
  const double t0 = sfm_now_ms();
  double t1 = t0, t2 = t0, t3 = t0, t4 = t0;
  auto stamp = [&](double t5) {
    s->ms[0] = t1 - t0, s->ms[1] = t2 - t1, s->ms[2] = t3 - t2, s->ms[3] = t4 - t3, s->ms[4] = t5 - t4, s->ms[5] = t5 - t0;
  };
  const dim3 gn(blocks(n, 256));
  // rules 2, 3: the frame, the classes, the bounds of A
  if (labels) SFM_HIP_TRY(hipMemcpyAsync(s->labels, labels, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(s->tot, 0, sizeof(Totals), st));
  TRS_LAUNCH(trs_frame, gn, c->xyz, labels ? s->labels : nullptr, label, n, p, s->enh, s->tot);
  unsigned mm[7];
  Totals tot;
  SFM_TRY(sfmgrid::minmax(c, s->enh, n, InA(), mm));
  SFM_HIP_TRY(hipMemcpyAsync(&tot, s->tot, sizeof tot, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  res.n_selected = (int32_t)tot.selected;
  res.n_band = (int32_t)tot.band;
  res.n_above = (int32_t)mm[6];
  t1 = t2 = t3 = t4 = sfm_now_ms();
  stamp(t1);
  if (res.n_above == 0) return SFMHIP_OK;
  res.flags = 0;
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = sfmcloud::ord_val(mm[a]), hi[a] = sfmcloud::ord_val(mm[3 + a]);
  Dims d;
  if (!make_dims(p, lo, hi, d)) return SFMHIP_ERR_ARG;
  // rules 4, 5: the band histogram, the components, the stems
  const int ncell = d.De * d.Dn;
  SFM_TRY(s->cells.need(4 * (size_t)ncell));
  int *count = s->cells.p, *parent = count + ncell, *occupied = parent + ncell, *slot = occupied + ncell;
  const dim3 gc(blocks(ncell, 256));
  SFM_HIP_TRY(hipMemsetAsync(count, 0, sizeof(int) * (size_t)ncell, st));
  TRS_LAUNCH(trs_hist, gn, s->enh, n, p, d, ncell, count);
  TRS_LAUNCH(trs_cells, gc, count, ncell, o.min_cell_pts, parent, occupied);
  TRS_LAUNCH(trs_hook, gc, parent, d.De, d.Dn);
  TRS_LAUNCH(trs_flatten, gc, parent, ncell);
  int n_occ = 0, T_all = 0;
  SFM_TRY(sfmgrid::scan(c, occupied, slot, (size_t)ncell, &n_occ));
  if (n_occ > n) return SFMHIP_ERR_STATE;  // (never: an occupied cell holds a band point)
  if (n_occ > 0) {
    const dim3 go(blocks(n_occ, 256));
    TRS_LAUNCH(trs_stats_init, go, n_occ, s->sums, s->box);
    TRS_LAUNCH(trs_stats, gc, count, parent, slot, ncell, d.De, n_occ, s->sums, s->box);
    TRS_LAUNCH(trs_stem_flag, go, n_occ, s->sums, s->box, o.min_stem_pts, p.c, p.w, s->sflag);
    SFM_TRY(sfmgrid::scan(c, s->sflag, s->sno, (size_t)n_occ, &T_all));
  }
  const int T = std::min(T_all, o.max_trees);
  if (T_all > T) res.flags |= F_MAX_TREES;
  res.n_trees = T;
  t2 = t3 = t4 = sfm_now_ms();
  stamp(t2);
  if (T == 0) {
    res.flags |= F_NO_STEM;
    return SFMHIP_OK;
  }
  std::vector<StemSums> sums((size_t)T);
  TRS_LAUNCH(trs_stem_emit, dim3(blocks(n_occ, 256)), n_occ, s->sflag, s->sno, T, s->sums, s->box, s->stems, s->stem_of);
  SFM_HIP_TRY(hipMemcpyAsync(sums.data(), s->stems, sizeof(StemSums) * (size_t)T, hipMemcpyDeviceToHost, st));
  // rules 6, 7: the occupied voxels, the seeds, the neighbours
  const int nvox = d.Dx * d.Dy * d.Dz;  // (< 2^31: make_dims)
  int *keys_in = c->ibuf[0], *vals_in = c->ibuf[1], *keys_out = c->ibuf[2], *vals_out = c->ibuf[3];
  TRS_LAUNCH(trs_vkeys, gn, s->enh, n, p, d, nvox, keys_in, vals_in);
  SFM_TRY(sfmgrid::cell_sort(c, nvox, keys_in, keys_out, vals_in, vals_out, n));
  TRS_LAUNCH(trs_heads, gn, keys_out, n, res.n_above, nvox, s->head);
  int nv = 0;
  SFM_TRY(sfmgrid::scan(c, s->head, s->hx, (size_t)n, &nv));
  if (nv < 1 || nv > res.n_above) return SFMHIP_ERR_STATE;  // (never)
  res.n_voxels = nv;
  SFM_TRY(s->adj.need((size_t)STEPS * nv));
  SFM_HIP_TRY(hipMemsetAsync(s->key, 0xFF, sizeof(u64) * (size_t)nv, st));
  SFM_HIP_TRY(hipMemsetAsync(s->pvox, 0xFF, sizeof(int) * (size_t)n, st));
  TRS_LAUNCH(trs_vox_emit, gn, keys_out, vals_out, s->head, s->hx, n, res.n_above, nvox, nv, s->enh, p, d, ncell, parent, slot, n_occ,
             s->stem_of, s->pvox, s->ukey, s->vstart, s->key);
  const dim3 gv(blocks(nv, 256));
  TRS_LAUNCH(trs_adj, dim3(gv.x, STEPS), s->ukey, nv, d, s->adj.p);
  if (c->ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t3 = t4 = sfm_now_ms();
  // rule 8: sweeps in batches, until a batch changes no key.  A sweep that changes a key settles at least one more voxel
  // of some shortest path, so nv sweeps reach the fixed point and one more sees it.
  for (;;) {
    unsigned changed = 0;
    SFM_HIP_TRY(hipMemsetAsync(s->changed, 0, sizeof(unsigned), st));
    for (int b = 0; b < BATCH; ++b) TRS_LAUNCH(trs_sweep, gv, s->key, s->adj.p, nv, s->changed);
    SFM_HIP_TRY(hipMemcpyAsync(&changed, s->changed, sizeof changed, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    s->sweeps += BATCH;
    if (!changed) break;
    if (s->sweeps > nv + BATCH) return SFMHIP_ERR_STATE;  // (never)
  }
  t4 = sfm_now_ms();
  // rule 9
  std::vector<int32_t> pts((size_t)T);
  SFM_HIP_TRY(hipMemsetAsync(s->pts, 0, sizeof(int) * (size_t)T, st));
  SFM_HIP_TRY(hipMemsetAsync(s->tot, 0, sizeof(Totals), st));
  TRS_LAUNCH(trs_vlabel, gv, s->key, s->vstart, nv, p.cap, T, s->vlabel, s->pts, s->tot);
  TRS_LAUNCH(trs_plabel, gn, s->pvox, s->vlabel, n, nv, s->tree_of);
  SFM_HIP_TRY(hipMemcpyAsync(tree_of, s->tree_of, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(pts.data(), s->pts, sizeof(int) * (size_t)T, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(&tot, s->tot, sizeof tot, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  res.n_labelled = (int32_t)tot.labelled;
  res.max_cost = (int32_t)(long long)tot.max_cost;
  for (int k = 0; k < T && k < cap; ++k) {
    stem_row(sums[k], p, d, stems[k]);
    stems[k].points = pts[k];
  }
  stamp(sfm_now_ms());
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_trees_default_opts(sfmhip_trees_opts* o) {
  if (!o) return;
  *o = mirror<sfmhip_trees_opts>(default_opts());
}

extern "C" int sfmhip_trees_opts_from_ground(const sfmhip_ground_result* g, sfmhip_trees_opts* io) {
  if (!g || !io) return SFMHIP_ERR_ARG;
  Opts t = mirror<Opts>(*io);
  if (!opts_from_ground(mirror<sfmground::Result>(*g), t)) return SFMHIP_ERR_ARG;
  *io = mirror<sfmhip_trees_opts>(t);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_trees(sfmhip_cloud* c, const int32_t* labels_in, int32_t label, const sfmhip_trees_opts* opts, int32_t* tree_of,
                                  int cap, sfmhip_tree_stem* stems, sfmhip_trees_result* out) {
  if (!c || !opts || !out || cap < 0 || (cap > 0 && !stems) || (c->n > 0 && !tree_of)) return SFMHIP_ERR_ARG;
  Result res;
  SFM_TRY(run(c, labels_in, label, mirror<Opts>(*opts), tree_of, cap, (Stem*)stems, res));
  *out = mirror<sfmhip_trees_result>(res);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_trees_last_timing(sfmhip_cloud* c, double ms6[6], int32_t* sweeps) {
  if (!c || !ms6) return SFMHIP_ERR_ARG;
  const TrsState* s = sfmgrid::stage<TrsState>(c);
  for (int i = 0; i < 6; ++i) ms6[i] = s->ms[i];
  if (sweeps) *sweeps = s->sweeps;
  return SFMHIP_OK;
}
