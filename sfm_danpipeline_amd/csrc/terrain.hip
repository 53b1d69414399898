// terrain.hip -- the terrain model on gfx950 over the device-resident cloud of cloud.hip: ground points by a progressive
// morphological filter on a raster, the terrain raster from them, every point's height above it, the canopy raster and the
// normalised cloud.  The rules are DESIGN.md f-20's; the arithmetic is terrain.h's, which the CPU test stub compiles too, and
// every output is the same bytes as that build's.
//
//   ter_frame     (e, n, h) of every selected point as float32, NaN elsewhere; cloud_minmax gives the raster's bounds and the
//                 count of the selection (cloud_grid.h: integer atomics on ordered keys);
//   ter_cells     a point's cell id (the handle's stable cell sort then gives every cell's run in ascending input index) and
//                 rule 4's lowest-point raster by an integer atomicMin on the ordered key of h; ter_runs the runs' bounds;
//   the opening   per window four passes of one kernel pair and two transposes.  A pass takes the running extremum down the
//                 columns of a row-major raster, where a wave reads 256 contiguous bytes per row: ter_scan writes the prefix
//                 and the suffix extrema of the column's blocks of 2 k + 1 cells (van Herk / Gil-Werman: a thread per column
//                 and block, two walks), ter_combine takes out[y] = op(suffix[y - k], prefix[y + k]) with the window clipped at
//                 the raster's edge -- three comparisons a cell whatever k.  The passes along x run on the transposed raster:
//                 ter_transpose moves TILE x TILE tiles through LDS (rows padded by one word).  min passes commute, and so do
//                 max passes, so column min, transpose, column min, column max, transpose, column max is rule 6's opening; an
//                 empty cell is +inf in memory and -inf inside a max pass.  Every O_i stays in HBM;
//   ter_ground    rule 7 in cell order, one pass over the points; ter_cellsum rule 8, a wave per cell run, lane = slot, then the
//                 wave butterfly (lane 0 holds the fold by strides 32 .. 1);
//   ter_fill / ter_relax   rules 9 and 10, one launch per round from one buffer into the other; the count of cells each fill
//                 round took is read back once per batch of 16 rounds, and rounds after one that filled nothing change nothing;
//   ter_cellstats the counts by kind and the bounds of T; ter_hag rules 11 - 13 in one pass over the points, the canopy by an
//                 integer atomicMax on ordered keys; ter_chm turns the keys into floats.
// No spin, no hand-off between workgroups, no float atomic.  Launches are ordered by the stream alone.
#include "common.h"
#include "cloud_grid.h"
#include "terrain.h"
#include <algorithm>
#include <climits>
#include <cmath>

using namespace sfmterrain;
using sfmgrid::blocks;
using sfmgrid::mirror;

namespace {

constexpr int BATCH = 16;  // fill rounds between two reads of the counters

struct Totals {  // the counts and the ordered keys the cell and point passes reduce into
  unsigned n_ground, kind0, kind1, kind2, tmin, tmax, hagmax, pad;
};

struct DhTab {  // rule 5's thresholds as a kernel argument
  double v[MAX_WINDOWS];
};

struct TerState {  // on the cloud handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::TERRAIN;
  DevBufs B;
  bool ready = false, has_call = false;
  int* labels = nullptr;            // n
  float* enh = nullptr;             // 3 n
  int* is_ground = nullptr;         // n
  float* hag = nullptr;             // n
  float* norm = nullptr;            // 3 n: the normalised cloud
  unsigned char* gs = nullptr;      // n: rule 7 by sorted position
  Totals* tot = nullptr;            // 1
  unsigned* cnt = nullptr;          // BATCH
  sfmgrid::Grow<int> runs;          // 2 ncell: a cell's [start, end) in sorted order
  sfmgrid::Grow<unsigned> zkey;     // ncell: rule 4's keys, then rule 12's
  sfmgrid::Grow<float> ras;         // 5 ncell: the opening's rasters; afterwards T (two buffers) and chm
  sfmgrid::Grow<float> ostack;      // n_windows ncell: every O_i
  sfmgrid::Grow<unsigned char> kind;  // 2 ncell
  const float* T = nullptr;         // the last call's rasters (in ras / kind)
  const unsigned char* K = nullptr;
  const float* chm = nullptr;
  int ncell = 0;
  Dims d = {0.0f, 0.0f, 0, 0};      // the last call's raster and cell, for last_call()
  double c = 0;
  double ms[6] = {0, 0, 0, 0, 0, 0};
};

int ter_alloc(sfmhip_cloud* c, TerState* s) {
  if (s->ready) return SFMHIP_OK;
  const size_t n = (size_t)std::max(c->n, 1);
  SFM_TRY(s->B.alloc(&s->labels, n));
  SFM_TRY(s->B.alloc(&s->enh, 3 * n));
  SFM_TRY(s->B.alloc(&s->is_ground, n));
  SFM_TRY(s->B.alloc(&s->hag, n));
  SFM_TRY(s->B.alloc(&s->norm, 3 * n));
  SFM_TRY(s->B.alloc(&s->gs, n));
  SFM_TRY(s->B.alloc(&s->tot, 1));
  SFM_TRY(s->B.alloc(&s->cnt, (size_t)BATCH));
  s->ready = true;
  return SFMHIP_OK;
}

struct Selected {  // cloud_minmax's predicate over the frame coordinates: ter_frame wrote NaN outside the selection
  __device__ bool operator()(long long, const float* v) const { return v[2] == v[2]; }
};

__global__ __launch_bounds__(256) void ter_frame(const float* xyz, const int* labels, int label, int n, sfmdendro::Frame f, float* enh) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float q[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  float o[3];
  sfmdendro::frame_point(f, q, !labels || labels[i] == label, o);
  enh[3 * (size_t)i] = o[0], enh[3 * (size_t)i + 1] = o[1], enh[3 * (size_t)i + 2] = o[2];
}

__global__ __launch_bounds__(256) void ter_cells(const float* enh, int n, Dims d, double c, int ncell, int* keys, int* vals, unsigned* zkey) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float e = enh[3 * (size_t)i], nn = enh[3 * (size_t)i + 1], h = enh[3 * (size_t)i + 2];
  int key = ncell;
  if (h == h) {
    const int q = cell_of(e, nn, d, c);
    if (q >= 0 && q < ncell) {  // (always: the raster was sized by these points' own bounds)
      key = q;
      atomicMin(zkey + q, sfmcloud::ord_key(h));
    }
  }
  keys[i] = key;
  vals[i] = i;
}

__global__ __launch_bounds__(256) void ter_runs(const int* keys, int n_sel, int ncell, int* start, int* end) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sel) return;
  const int k = keys[i];
  if (k < 0 || k >= ncell) return;  // (never: the selected points sort first)
  if (i == 0 || keys[i - 1] != k) start[k] = i;
  if (i == n_sel - 1 || keys[i + 1] != k) end[k] = i + 1;
}

__global__ __launch_bounds__(256) void ter_z0(const unsigned* zkey, int ncell, float* Z) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ncell) return;
  const unsigned k = zkey[q];
  Z[q] = k == 0xFFFFFFFFu ? pinf() : sfmcloud::ord_val(k);
}

template <bool MAX>
__device__ __forceinline__ float ext(float a, float b) {
  return MAX ? (b > a ? b : a) : (b < a ? b : a);
}

// the prefix (G) and suffix (H) extrema of the blocks of w rows of every column of a W x Hh raster: a thread per column and
// block.  Empty cells are +inf in `in`; a max pass reads them as -inf.
template <bool MAX>
__global__ __launch_bounds__(256) void ter_scan(const float* __restrict__ in, int W, int Hh, int w, int nb, float* __restrict__ G,
                                                float* __restrict__ H) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= W * nb) return;
  const int x = t % W, b = t / W;
  const int y0 = b * w, y1 = min(y0 + w, Hh);
  float acc = MAX ? ninf() : pinf();
  for (int y = y0; y < y1; ++y) {
    float v = in[(size_t)y * W + x];
    if (MAX && v == pinf()) v = ninf();
    acc = ext<MAX>(acc, v);
    G[(size_t)y * W + x] = acc;
  }
  acc = MAX ? ninf() : pinf();
  for (int y = y1 - 1; y >= y0; --y) {
    float v = in[(size_t)y * W + x];
    if (MAX && v == pinf()) v = ninf();
    acc = ext<MAX>(acc, v);
    H[(size_t)y * W + x] = acc;
  }
}

// out[y] = the extremum over rows [y - k, y + k] clipped to the raster: the suffix of the block the window starts in and the
// prefix of the block it ends in; a clipped window that lies in one block starts at the block's first row or ends at its last
template <bool MAX>
__global__ __launch_bounds__(256) void ter_combine(const float* __restrict__ G, const float* __restrict__ H, int W, int Hh, int k, int w,
                                                   float* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= W * Hh) return;
  const int x = q % W, y = q / W;
  const int l = max(y - k, 0), r = min(y + k, Hh - 1);
  const float hl = H[(size_t)l * W + x], gr = G[(size_t)r * W + x];
  float v = l / w == r / w ? (l % w == 0 ? gr : hl) : ext<MAX>(hl, gr);
  if (MAX && v == ninf()) v = pinf();
  out[q] = v;
}

// out (Hh columns, W rows) = the transpose of in (W columns, Hh rows), TILE x TILE cells per workgroup through LDS
__global__ __launch_bounds__(256) void ter_transpose(const float* __restrict__ in, int W, int Hh, int gx, float* __restrict__ out) {
  __shared__ float tile[TILE][TILE + 1];
  const int bx = (blockIdx.x % gx) * TILE, by = (blockIdx.x / gx) * TILE;
  const int tx = threadIdx.x & (TILE - 1), ty = threadIdx.x / TILE;
  for (int j = ty; j < TILE; j += 256 / TILE) {
    const int x = bx + tx, y = by + j;
    if (x < W && y < Hh) tile[j][tx] = in[(size_t)y * W + x];
  }
  __syncthreads();
  for (int j = ty; j < TILE; j += 256 / TILE) {
    const int ox = by + tx, oy = bx + j;  // (the output's column is the input's row)
    if (ox < Hh && oy < W) out[(size_t)oy * Hh + ox] = tile[tx][j];
  }
}

// rule 7 at sorted position i (the selected points come first in sorted order)
__global__ __launch_bounds__(256) void ter_ground(const int* keys, const int* vals, int n_sel, int n, int ncell, const float* enh,
                                                  const float* ostack, int nw, DhTab dh, int* is_ground, unsigned char* gs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sel) return;
  const int q = keys[i], pt = vals[i];
  if (q < 0 || q >= ncell || pt < 0 || pt >= n) {  // (never)
    gs[i] = 0;
    return;
  }
  const float h = enh[3 * (size_t)pt + 2];
  bool g = true;
  for (int w = 0; w < nw; ++w) g = g && below_threshold(h, ostack[(size_t)w * ncell + q], dh.v[w]);
  gs[i] = g ? 1 : 0;
  is_ground[pt] = g ? 1 : 0;
}

// rule 8: a wave per cell, lane = slot
__global__ __launch_bounds__(256) void ter_cellsum(const int* start, const int* end, const int* vals, const unsigned char* gs, const float* enh,
                                                   int n, int ncell, float* T, unsigned char* kind, Totals* tot) {
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (q >= ncell) return;
  const int s = start[q], len = end[q] - s;
  double acc = 0.0;
  int m = 0;
  for (int j = lane; j < len; j += SLOTS) {
    const int pt = vals[s + j];
    if (!gs[s + j] || pt < 0 || pt >= n) continue;
    acc = acc + (double)enh[3 * (size_t)pt + 2];
    ++m;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    acc = acc + __shfl_xor(acc, off);
    m += __shfl_xor(m, off);
  }
  if (lane != 0) return;
  T[q] = m ? (float)(acc / (double)m) : sfmcloud::qnan();
  kind[q] = m ? K_GROUND : K_EMPTY;
  if (m) atomicAdd(&tot->n_ground, (unsigned)m);
}

__global__ __launch_bounds__(256) void ter_fill(const float* Tin, const unsigned char* kin, int De, int Dn, float* Tout, unsigned char* kout,
                                                unsigned* cnt) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  bool filled = false;
  if (q < De * Dn) {
    float v = Tin[q];
    unsigned char k = kin[q];
    if (k == K_EMPTY && fill_value(Tin, kin, q % De, q / De, De, Dn, v)) k = K_FILLED, filled = true;
    Tout[q] = v;
    kout[q] = k;
  }
  const unsigned m = (unsigned)__popcll(__ballot(filled));
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(cnt, m);
}

__global__ __launch_bounds__(256) void ter_relax(const float* Tin, const unsigned char* kind, int De, int Dn, float* Tout) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= De * Dn) return;
  Tout[q] = kind[q] == K_FILLED ? relax_value(Tin, kind, q % De, q / De, De, Dn) : Tin[q];
}

__global__ __launch_bounds__(256) void ter_cellstats(const float* T, const unsigned char* kind, int ncell, Totals* tot) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  const int k = q < ncell ? (int)kind[q] : -1;
  unsigned lo = 0xFFFFFFFFu, hi = 0u;
  if (k == K_GROUND || k == K_FILLED) lo = hi = sfmcloud::ord_key(T[q]);
  const unsigned k0 = (unsigned)__popcll(__ballot(k == K_EMPTY)), k1 = (unsigned)__popcll(__ballot(k == K_GROUND)),
                 k2 = (unsigned)__popcll(__ballot(k == K_FILLED));
  for (int off = 32; off >= 1; off >>= 1) {
    lo = min(lo, (unsigned)__shfl_xor(lo, off));
    hi = max(hi, (unsigned)__shfl_xor(hi, off));
  }
  if ((threadIdx.x & 63) != 0) return;
  if (k0) atomicAdd(&tot->kind0, k0);
  if (k1) atomicAdd(&tot->kind1, k1);
  if (k2) atomicAdd(&tot->kind2, k2);
  if (hi) {
    atomicMin(&tot->tmin, lo);
    atomicMax(&tot->tmax, hi);
  }
}

// rules 11 - 13 for point i
__global__ __launch_bounds__(256) void ter_hag(const float* enh, int n, Dims d, double c, int ncell, const float* T, const unsigned char* kind,
                                               float* hag, float* norm, unsigned* ckey, Totals* tot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned key = 0u;
  if (i < n) {
    const float e = enh[3 * (size_t)i], nn = enh[3 * (size_t)i + 1], h = enh[3 * (size_t)i + 2];
    float g = sfmcloud::qnan();
    int q = -1;
    if (h == h) {
      q = cell_of(e, nn, d, c);
      if (q >= 0 && q < ncell) g = height_above(e, nn, h, q, d, c, T, kind);  // (always in range)
    }
    const bool fin = g - g == 0.0f;
    hag[i] = g;
    norm[3 * (size_t)i] = fin ? e : sfmcloud::qnan();
    norm[3 * (size_t)i + 1] = fin ? nn : sfmcloud::qnan();
    norm[3 * (size_t)i + 2] = fin ? g : sfmcloud::qnan();
    if (fin && q >= 0 && q < ncell) {
      key = sfmcloud::ord_key(g);
      atomicMax(ckey + q, key);
    }
  }
  for (int off = 32; off >= 1; off >>= 1) key = max(key, (unsigned)__shfl_xor(key, off));
  if ((threadIdx.x & 63) == 0 && key) atomicMax(&tot->hagmax, key);
}

__global__ __launch_bounds__(256) void ter_chm(const unsigned* ckey, int ncell, float* chm) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= ncell) return;
  chm[q] = ckey[q] ? sfmcloud::ord_val(ckey[q]) : sfmcloud::qnan();
}

__global__ __launch_bounds__(256) void ter_blank(int n, int* is_ground, float* hag, float* norm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  is_ground[i] = 0;
  hag[i] = sfmcloud::qnan();
  norm[3 * (size_t)i] = norm[3 * (size_t)i + 1] = norm[3 * (size_t)i + 2] = sfmcloud::qnan();
}

#define TER_LAUNCH(kernel, grid, ...)                                \
  do {                                                               \
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, __VA_ARGS__); \
    SFM_HIP_TRY(hipGetLastError());                                  \
  } while (0)

// one pass of the opening down the columns of a W x Hh raster: in -> out through G and H
template <bool MAX>
int column_pass(hipStream_t st, const float* in, int W, int Hh, int k, float* G, float* H, float* out) {
  k = std::min(k, Hh - 1);
  const int w = 2 * k + 1, nb = (Hh + w - 1) / w;
  TER_LAUNCH(ter_scan<MAX>, dim3(blocks((long long)W * nb, 256)), in, W, Hh, w, nb, G, H);
  TER_LAUNCH(ter_combine<MAX>, dim3(blocks((long long)W * Hh, 256)), G, H, W, Hh, k, w, out);
  return SFMHIP_OK;
}

int transpose(hipStream_t st, const float* in, int W, int Hh, float* out) {
  const int gx = (W + TILE - 1) / TILE, gy = (Hh + TILE - 1) / TILE;
  TER_LAUNCH(ter_transpose, dim3((unsigned)(gx * gy)), in, W, Hh, gx, out);
  return SFMHIP_OK;
}

// rule 6: O = the opening of Z (De x Dn) by half-width k; A, B, G, H: scratch rasters
int opening(hipStream_t st, const float* Z, int De, int Dn, int k, float* A, float* B, float* G, float* H, float* O) {
  SFM_TRY(column_pass<false>(st, Z, De, Dn, k, G, H, A));
  SFM_TRY(transpose(st, A, De, Dn, B));
  SFM_TRY(column_pass<false>(st, B, Dn, De, k, G, H, A));
  SFM_TRY(column_pass<true>(st, A, Dn, De, k, G, H, B));
  SFM_TRY(transpose(st, B, Dn, De, A));
  SFM_TRY(column_pass<true>(st, A, De, Dn, k, G, H, O));
  return SFMHIP_OK;
}

int run(sfmhip_cloud* c, const int32_t* labels, int32_t label, const Opts& o, int32_t* is_ground, float* hag, Result& res) {
  Prep p;
  if (!prepare(o, p)) return SFMHIP_ERR_ARG;
  TerState* s = sfmgrid::stage<TerState>(c);
  for (double& m : s->ms) m = 0;
  s->has_call = false;
  s->ncell = 0;
  s->T = s->chm = nullptr, s->K = nullptr;
  s->d = Dims{0.0f, 0.0f, 0, 0}, s->c = p.c;
  empty_result(res, p, F_NONE_SELECTED);
  const int n = c->n;
  if (n <= 0) {
    s->has_call = true;
    return SFMHIP_OK;
  }
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  SFM_TRY(sfmgrid::ensure_ibuf(c));
  SFM_TRY(ter_alloc(c, s));
  const double t0 = sfm_now_ms();
  double t1 = t0, t2 = t0, t3 = t0, t4 = t0;
  auto stamp = [&](double t5) {
    s->ms[0] = t1 - t0, s->ms[1] = t2 - t1, s->ms[2] = t3 - t2, s->ms[3] = t4 - t3, s->ms[4] = t5 - t4, s->ms[5] = t5 - t0;
  };
  auto fetch = [&]() -> int {  // the per-point outputs to the host
    if (is_ground) SFM_HIP_TRY(hipMemcpyAsync(is_ground, s->is_ground, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (hag) SFM_HIP_TRY(hipMemcpyAsync(hag, s->hag, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    return SFMHIP_OK;
  };
  const dim3 gn(blocks(n, 256));
  // rules 2, 3: the frame, the bounds of the selection
  if (labels) SFM_HIP_TRY(hipMemcpyAsync(s->labels, labels, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  TER_LAUNCH(ter_frame, gn, c->xyz, labels ? s->labels : nullptr, label, n, p.f, s->enh);
  TER_LAUNCH(ter_blank, gn, n, s->is_ground, s->hag, s->norm);
  unsigned mm[7];
  SFM_TRY(sfmgrid::minmax(c, s->enh, n, Selected(), mm));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  res.n_selected = (int32_t)mm[6];
  if (res.n_selected == 0) {
    SFM_TRY(fetch());
    t1 = t2 = t3 = t4 = sfm_now_ms();
    stamp(t1);
    s->has_call = true;
    return SFMHIP_OK;
  }
  res.flags = 0;
  const float lo[2] = {sfmcloud::ord_val(mm[0]), sfmcloud::ord_val(mm[1])}, hi[2] = {sfmcloud::ord_val(mm[3]), sfmcloud::ord_val(mm[4])};
  Dims d;
  if (!make_dims(p, lo, hi, d)) return SFMHIP_ERR_ARG;
  res.e_min = d.e_min, res.n_min = d.n_min, res.De = d.De, res.Dn = d.Dn;
  const int ncell = d.De * d.Dn, n_sel = res.n_selected;
  Windows w;
  make_windows(p, w);
  res.n_windows = w.n;
  if (w.n == 0) res.flags |= F_NO_WINDOW;
  SFM_TRY(s->runs.need(2 * (size_t)ncell));
  SFM_TRY(s->zkey.need((size_t)ncell));
  SFM_TRY(s->ras.need(5 * (size_t)ncell));
  SFM_TRY(s->kind.need(2 * (size_t)ncell));
  SFM_TRY(s->ostack.need((size_t)std::max(w.n, 1) * ncell));
  const dim3 gc(blocks(ncell, 256));
  // rule 4 and the cells' runs
  int *keys_in = c->ibuf[0], *vals_in = c->ibuf[1], *keys = c->ibuf[2], *vals = c->ibuf[3];
  int *start = s->runs.p, *end = start + ncell;
  SFM_HIP_TRY(hipMemsetAsync(s->zkey.p, 0xFF, sizeof(unsigned) * (size_t)ncell, st));
  SFM_HIP_TRY(hipMemsetAsync(start, 0, sizeof(int) * 2 * (size_t)ncell, st));
  TER_LAUNCH(ter_cells, gn, s->enh, n, d, p.c, ncell, keys_in, vals_in, s->zkey.p);
  SFM_TRY(sfmgrid::cell_sort(c, ncell, keys_in, keys, vals_in, vals, n));
  TER_LAUNCH(ter_runs, dim3(blocks(n_sel, 256)), keys, n_sel, ncell, start, end);
  float *R0 = s->ras.p, *R1 = R0 + ncell, *R2 = R1 + ncell, *R3 = R2 + ncell, *R4 = R3 + ncell;
  TER_LAUNCH(ter_z0, gc, s->zkey.p, ncell, R0);
  if (c->ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t1 = t2 = t3 = t4 = sfm_now_ms();
  // rules 5, 6: every O_i, kept
  DhTab dh;
  for (int i = 0; i < MAX_WINDOWS; ++i) dh.v[i] = i < w.n ? w.dh[i] : 0.0;
  for (int i = 0; i < w.n; ++i)
    SFM_TRY(opening(st, i == 0 ? R0 : s->ostack.p + (size_t)(i - 1) * ncell, d.De, d.Dn, w.k[i], R1, R2, R3, R4,
                    s->ostack.p + (size_t)i * ncell));
  if (c->ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t2 = t3 = t4 = sfm_now_ms();
  // rules 7, 8
  static const Totals tot0 = {0u, 0u, 0u, 0u, 0xFFFFFFFFu, 0u, 0u, 0u};
  SFM_HIP_TRY(hipMemcpyAsync(s->tot, &tot0, sizeof tot0, hipMemcpyHostToDevice, st));
  float* T[2] = {R0, R1};
  unsigned char* K[2] = {s->kind.p, s->kind.p + ncell};
  TER_LAUNCH(ter_ground, dim3(blocks(n_sel, 256)), keys, vals, n_sel, n, ncell, s->enh, s->ostack.p, w.n, dh, s->is_ground, s->gs);
  TER_LAUNCH(ter_cellsum, dim3(blocks(ncell, 4)), start, end, vals, s->gs, s->enh, n, ncell, T[0], K[0], s->tot);
  if (c->ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t3 = t4 = sfm_now_ms();
  // rule 9: rounds in batches; a round after one that filled nothing fills nothing
  int cur = 0, rounds = 0;
  for (bool open = true; open && rounds < p.fill_rounds;) {
    const int batch = std::min(BATCH, p.fill_rounds - rounds);
    unsigned cnt[BATCH];
    SFM_HIP_TRY(hipMemsetAsync(s->cnt, 0, sizeof cnt, st));
    for (int b = 0; b < batch; ++b, cur ^= 1) TER_LAUNCH(ter_fill, gc, T[cur], K[cur], d.De, d.Dn, T[cur ^ 1], K[cur ^ 1], s->cnt + b);
    SFM_HIP_TRY(hipMemcpyAsync(cnt, s->cnt, sizeof cnt, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < batch && open; ++b) {
      ++rounds;
      open = cnt[b] != 0;
    }
  }
  res.fill_rounds = rounds;
  // rule 10
  const unsigned char* kinds = K[cur];  // (the kinds are final; T goes on from one buffer into the other)
  for (int k = 0; k < p.relax_sweeps; ++k, cur ^= 1) TER_LAUNCH(ter_relax, gc, T[cur], kinds, d.De, d.Dn, T[cur ^ 1]);
  TER_LAUNCH(ter_cellstats, gc, T[cur], kinds, ncell, s->tot);
  if (c->ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t4 = sfm_now_ms();
  // rules 11 - 13
  SFM_HIP_TRY(hipMemsetAsync(s->zkey.p, 0, sizeof(unsigned) * (size_t)ncell, st));
  TER_LAUNCH(ter_hag, gn, s->enh, n, d, p.c, ncell, T[cur], kinds, s->hag, s->norm, s->zkey.p, s->tot);
  TER_LAUNCH(ter_chm, gc, s->zkey.p, ncell, R2);
  Totals tot;
  SFM_HIP_TRY(hipMemcpyAsync(&tot, s->tot, sizeof tot, hipMemcpyDeviceToHost, st));
  SFM_TRY(fetch());
  res.n_ground = (int32_t)tot.n_ground;
  res.n_kind0 = (int32_t)tot.kind0, res.n_kind1 = (int32_t)tot.kind1, res.n_kind2 = (int32_t)tot.kind2;
  if (tot.kind0) res.flags |= F_UNFILLED;
  if (tot.tmax) res.t_min = sfmcloud::ord_val(tot.tmin), res.t_max = sfmcloud::ord_val(tot.tmax);
  if (tot.hagmax) res.hag_max = sfmcloud::ord_val(tot.hagmax);
  s->T = T[cur], s->K = kinds, s->chm = R2;
  s->ncell = ncell;
  s->d = d;
  s->has_call = true;
  stamp(sfm_now_ms());
  return SFMHIP_OK;
}

}  // namespace

// (not of the C ABI: crowns.hip reads the last call's rasters and per-point arrays where they lie)
bool sfmterrain::last_call(sfmhip_cloud* c, LastCall& out) {
  const TerState* s = sfmgrid::stage<TerState>(c);
  if (!s->has_call) return false;
  out.chm = s->chm, out.enh = s->enh, out.hag = s->hag;
  out.d = s->d, out.c = s->c, out.n = c->n;
  return true;
}

extern "C" void sfmhip_terrain_default_opts(sfmhip_terrain_opts* o) {
  if (!o) return;
  *o = mirror<sfmhip_terrain_opts>(default_opts());
}

extern "C" int sfmhip_terrain_opts_from_ground(const sfmhip_ground_result* g, sfmhip_terrain_opts* io) {
  if (!g || !io) return SFMHIP_ERR_ARG;
  Opts t = mirror<Opts>(*io);
  if (!opts_from_ground(mirror<sfmground::Result>(*g), t)) return SFMHIP_ERR_ARG;
  *io = mirror<sfmhip_terrain_opts>(t);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_terrain(sfmhip_cloud* c, const int32_t* labels, int32_t label, const sfmhip_terrain_opts* opts,
                                    int32_t* is_ground, float* hag, sfmhip_terrain_result* out) {
  if (!c || !opts || !out) return SFMHIP_ERR_ARG;
  Result res;
  SFM_TRY(run(c, labels, label, mirror<Opts>(*opts), is_ground, hag, res));
  *out = mirror<sfmhip_terrain_result>(res);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_terrain_raster(sfmhip_cloud* c, float* dtm, uint8_t* kind, float* chm) {
  if (!c) return SFMHIP_ERR_ARG;
  const TerState* s = sfmgrid::stage<TerState>(c);
  if (!s->has_call) return SFMHIP_ERR_ARG;
  if (s->ncell == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  if (dtm) SFM_HIP_TRY(hipMemcpyAsync(dtm, s->T, sizeof(float) * (size_t)s->ncell, hipMemcpyDeviceToHost, st));
  if (kind) SFM_HIP_TRY(hipMemcpyAsync(kind, s->K, (size_t)s->ncell, hipMemcpyDeviceToHost, st));
  if (chm) SFM_HIP_TRY(hipMemcpyAsync(chm, s->chm, sizeof(float) * (size_t)s->ncell, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_terrain_normalize(sfmhip_cloud* c, sfmhip_cloud** out) {
  if (!c || !out) return SFMHIP_ERR_ARG;
  *out = nullptr;
  const TerState* s = sfmgrid::stage<TerState>(c);
  if (!s->has_call) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  float* d = nullptr;
  SFM_TRY(sfm_dev_alloc(&d, (size_t)3 * std::max(c->n, 1)));
  if (c->n > 0) {
    hipError_t e = hipMemcpyAsync(d, s->norm, sizeof(float) * 3 * (size_t)c->n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      g_sfmhip_last_hip_error = (int)e;
      hipFree(d);
      return SFMHIP_ERR_HIP;
    }
  }
  return sfmgrid::adopt_device(c->ctx, d, c->n, out);
}

extern "C" int sfmhip_cloud_terrain_last_timing(sfmhip_cloud* c, double ms6[6]) {
  if (!c || !ms6) return SFMHIP_ERR_ARG;
  const TerState* s = sfmgrid::stage<TerState>(c);
  for (int i = 0; i < 6; ++i) ms6[i] = s->ms[i];
  return SFMHIP_OK;
}
