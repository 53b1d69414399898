// dendro.hip -- dendrometry on gfx950 over the device-resident cloud of cloud.hip: tree height, DBH, the stem taper
// profile, crown base, live crown and crown spread (the blanks of the reference's Dendrometry::estimate,
// src/DendrometryE.cpp:3-29).  The rules are DESIGN.md f-11's; the arithmetic is dendro.h's, which the CPU test stub
// compiles too, and every output is the same bits as that build's.
//
//   dnd_frame    (e, n, h) of every point as float32, NaN where the point is not selected (rules 2, 3);
//   cloud_minmax the ground and the top (cloud_grid.h: integer atomics on ordered keys);
//   dnd_keys     the slice of every point + the slice histogram (LDS, then integer atomics); the handle's scan turns the
//                histogram into slice offsets, its stable cell sort orders the points by (slice, input index);
//   dnd_gather   the (e, n) pairs in that order;
//   dnd_ransac   a workgroup per (16 hypotheses, slice): the slice's pairs go through LDS in chunks, each wave scores its
//                own 4 hypotheses with the lanes strided over the chunk, counts by ballot + popcount, and writes one 64-bit
//                atomicMax per hypothesis (count, lowest iteration, sector mask: rule 5's key);
//   dnd_refit    a workgroup per stem slice: Kasa, 10 Gauss-Newton steps and the residual, each a pass of fixed-order sums;
//   dnd_extent   a workgroup per slice: the radial histogram in LDS, its quantile (rule 8);
//   cloud_minmax the spread over the points at or above the crown base (rule 10).
// The host reads the S-row slice table twice (after the refit for the DBH axis, after the extents for the crown base) and
// two 7-word min / max records; nothing sized by the cloud comes back.  Launches are ordered by the stream alone.
#include "common.h"
#include "cloud_grid.h"
#include "dendro.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmdendro;
using sfmgrid::blocks;
using sfmgrid::mirror;  // (the options in, the defaults and the result out: size-checked)

static_assert(sizeof(sfmhip_dendro_slice) == sizeof(Slice), "sfmhip_dendro_slice mirrors sfmdendro::Slice");

namespace {

constexpr int RW = 4;            // waves of a dnd_ransac workgroup
constexpr int HPW = 4;           // hypotheses a wave scores at once
constexpr int HPB = RW * HPW;    // hypotheses of a workgroup
constexpr int STAGE = 1024;      // (e, n) pairs of one LDS chunk

struct DndState {  // on the cloud handle, freed with it; the cloud's size never changes, so the blocks are made once
  static constexpr sfmgrid::Stage slot = sfmgrid::DENDRO;  // (its slot on the handle: stage<DndState>(cloud))
  DevBufs B;
  bool ready = false;
  float* frame = nullptr;               // 3 n
  int* labels = nullptr;                // n
  P2* pts = nullptr;                    // n, by (slice, input index)
  int* cnt = nullptr;                   // MAX_SLICES + 1 (the last: points in no slice)
  int* start = nullptr;                 // MAX_SLICES + 1
  unsigned long long* keys = nullptr;   // MAX_SLICES winners
  Slice* table = nullptr;               // MAX_SLICES rows
  double ms[6] = {0, 0, 0, 0, 0, 0};
};

int dnd_alloc(sfmhip_cloud* c, DndState* s) {
  if (s->ready) return SFMHIP_OK;
  const size_t n = (size_t)std::max(c->n, 1);
  SFM_TRY(s->B.alloc(&s->frame, 3 * n));
  SFM_TRY(s->B.alloc(&s->labels, n));
  SFM_TRY(s->B.alloc(&s->pts, n));
  SFM_TRY(s->B.alloc(&s->cnt, (size_t)MAX_SLICES + 1));
  SFM_TRY(s->B.alloc(&s->start, (size_t)MAX_SLICES + 1));
  SFM_TRY(s->B.alloc(&s->keys, (size_t)MAX_SLICES));
  SFM_TRY(s->B.alloc(&s->table, (size_t)MAX_SLICES));
  s->ready = true;
  return SFMHIP_OK;
}

struct Selected {  // cloud_minmax's predicate: the selection (rule 2)
  __device__ bool operator()(long long, const float* v) const { return v[2] == v[2]; }
};
struct AtOrAbove {  // ... and the points of rule 10
  double hb;
  __device__ bool operator()(long long, const float* v) const { return (double)v[2] >= hb; }
};

__global__ __launch_bounds__(256) void dnd_frame(const float* xyz, const int* labels, int label, int n, Frame f, float* frame) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  float o[3];
  frame_point(f, p, !labels || labels[i] == label, o);
  frame[3 * (size_t)i] = o[0];
  frame[3 * (size_t)i + 1] = o[1];
  frame[3 * (size_t)i + 2] = o[2];
}

// keys[i] = the slice of point i (S: in none), vals[i] = i, cnt[k] += the points of slice k
__global__ __launch_bounds__(256) void dnd_keys(const float* frame, int n, double h0, double t, int S, int* keys, int* vals, int* cnt) {
  __shared__ int hist[MAX_SLICES + 1];
  for (int b = threadIdx.x; b <= S; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    int k = slice_of(frame[3 * (size_t)i + 2], h0, t, S);
    if (k < 0) k = S;
    keys[i] = k;
    vals[i] = (int)i;
    atomicAdd(&hist[k], 1);
  }
  __syncthreads();
  for (int b = threadIdx.x; b <= S; b += blockDim.x)
    if (hist[b]) atomicAdd(cnt + b, hist[b]);
}

__global__ __launch_bounds__(256) void dnd_gather(const float* frame, const int* vals, const int* n_in, int n, P2* pts) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n || s >= *n_in) return;
  const size_t j = (size_t)vals[s];
  P2 p;
  p.x = frame[3 * j];
  p.y = frame[3 * j + 1];
  pts[s] = p;
}

struct RansacArgs {
  double r_min, r_max, tol;
  int iters, min_slice_pts;
  uint32_t seed;
};

__global__ __launch_bounds__(64 * RW) void dnd_ransac(const P2* __restrict__ pts, const int* __restrict__ start,
                                                     const int* __restrict__ cnt, RansacArgs a, unsigned long long* keys) {
  __shared__ P2 tile[STAGE];
  const int k = blockIdx.y;
  const int nk = cnt[k];
  if (nk < a.min_slice_pts) return;  // (uniform over the workgroup)
  const P2* sp = pts + start[k];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * HPB + wave * HPW;
  Circle c[HPW];
  int count[HPW];
  unsigned mask[HPW];
#pragma unroll
  for (int h = 0; h < HPW; ++h) {
    count[h] = 0;
    mask[h] = 0;
    if (j0 + h < a.iters) {
      c[h] = hypothesis(sp, nk, a.seed, k, j0 + h, a.r_min, a.r_max);
    } else {
      c[h].cx = c[h].cy = c[h].r = 0.0;
      c[h].ok = 0;
    }
  }
  for (int base = 0; base < nk; base += STAGE) {
    const int m = min(STAGE, nk - base);
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += 64 * RW) tile[i] = sp[base + i];
    __syncthreads();
    for (int i0 = 0; i0 < m; i0 += 64) {
      const bool live = i0 + lane < m;
      const P2 p = tile[live ? i0 + lane : 0];
#pragma unroll
      for (int h = 0; h < HPW; ++h) {
        const double dx = (double)p.x - c[h].cx, dy = (double)p.y - c[h].cy;
        const bool in = live && c[h].ok && is_inlier(dx, dy, c[h].r, a.tol);
        count[h] += (int)__popcll(__ballot(in));
        if (in) mask[h] |= 1u << sector_of(dx, dy);
      }
    }
  }
#pragma unroll
  for (int h = 0; h < HPW; ++h) {
    unsigned mk = mask[h];
    for (int off = 32; off >= 1; off >>= 1) mk |= (unsigned)__shfl_xor((int)mk, off);
    if (lane == 0 && count[h] > 0) atomicMax(keys + k, winner_key(count[h], j0 + h, mk));
  }
}

struct RefitArgs {
  double r_min, r_max, tol;
  int min_inliers, min_sectors, min_slice_pts;
  uint32_t seed;
};

__global__ __launch_bounds__(CHUNK) void dnd_refit(const P2* __restrict__ pts, const int* __restrict__ start, const int* __restrict__ cnt,
                                                   const unsigned long long* __restrict__ keys, RefitArgs a, Slice* table) {
  __shared__ double sh[8][4];
  const int k = blockIdx.x;
  const int nk = cnt[k];
  const unsigned long long key = nk >= a.min_slice_pts ? keys[k] : 0ull;
  const bool stem = is_stem(key, a.min_inliers, a.min_sectors);
  Slice s;
  s.count = nk;
  s.stem = stem ? 1 : 0;
  s.inliers = key != 0ull ? key_count(key) : 0;
  s.mask = key != 0ull ? key_mask(key) : 0;
  s.ce = s.cn = s.radius = s.rms = s.extent = dnan();
  if (!stem) {  // (uniform over the workgroup)
    if (threadIdx.x == 0) table[k] = s;
    return;
  }
  const P2* sp = pts + start[k];
  const Circle c = hypothesis(sp, nk, a.seed, k, key_iter(key), a.r_min, a.r_max);
  const double N = (double)s.inliers;
  double fa = 0.0, fb = 0.0, fr = c.r;
  for (int pass = 0; pass <= GN_STEPS + 1; ++pass) {
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, term[8];
    const int nq = pass <= GN_STEPS ? 8 : 1;
    for (int i = threadIdx.x; i < nk; i += CHUNK) {
      const P2 p = sp[i];
      const double dx = (double)p.x - c.cx, dy = (double)p.y - c.cy;
      if (!is_inlier(dx, dy, c.r, a.tol)) continue;
      if (pass == 0)
        kasa_terms(dx, dy, term);
      else if (pass <= GN_STEPS)
        gn_terms(dx, dy, fa, fb, fr, term);
      else
        term[0] = res2_term(dx, dy, fa, fb, fr);
      for (int q = 0; q < nq; ++q) acc[q] = acc[q] + term[q];
    }
    sfmsum::block_tree<8>(acc, sh, nq);
    if (pass == 0)
      kasa_solve(acc, N, fa, fb, fr);
    else if (pass <= GN_STEPS)
      gn_solve(acc, N, fa, fb, fr);
    else
      s.rms = sqrt(acc[0] / N);
  }
  s.ce = c.cx + fa;
  s.cn = c.cy + fb;
  s.radius = fr;
  if (threadIdx.x == 0) table[k] = s;
}

__global__ __launch_bounds__(256) void dnd_extent(const P2* __restrict__ pts, const int* __restrict__ start, const int* __restrict__ cnt,
                                                  double ce, double cn, double bin, double q, Slice* table) {
  __shared__ int hist[BINS];
  const int k = blockIdx.x;
  const int nk = cnt[k];
  if (nk == 0) return;
  for (int b = threadIdx.x; b < BINS; b += blockDim.x) hist[b] = 0;
  __syncthreads();
  const P2* sp = pts + start[k];
  for (int i = threadIdx.x; i < nk; i += blockDim.x) {
    const P2 p = sp[i];
    atomicAdd(&hist[extent_bin_of((double)p.x - ce, (double)p.y - cn, bin)], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int need = extent_need(q, nk);
    int cum = 0;
    for (int b = 0; b < BINS; ++b) {
      cum += hist[b];
      if (cum >= need) {
        table[k].extent = (double)(b + 1) * bin;
        break;
      }
    }
  }
}

// the whole call; `slices` gets the S rows (cloud units)
int run(sfmhip_cloud* c, const int32_t* labels, int32_t label, const Opts& o, Result& res, std::vector<Slice>& slices) {
  Frame f;
  if (!make_frame(o, f)) return SFMHIP_ERR_ARG;
  slices.clear();
  empty_result(res);
  DndState* s = sfmgrid::stage<DndState>(c);
  for (double& m : s->ms) m = 0;
  if (c->n <= 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  const bool timing = c->ctx->timing;
  const int n = c->n;
  SFM_TRY(sfmgrid::ensure_ibuf(c));
  SFM_TRY(dnd_alloc(c, s));
  const double t0 = sfm_now_ms();
  // rules 2, 3: the frame, the ground and the top
  if (labels) SFM_HIP_TRY(hipMemcpyAsync(s->labels, labels, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(dnd_frame, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, labels ? s->labels : nullptr, label, n, f, s->frame);
  SFM_HIP_TRY(hipGetLastError());
  unsigned mm[7];
  SFM_TRY(sfmgrid::minmax(c, s->frame, n, Selected(), mm));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t1 = sfm_now_ms();
  s->ms[0] = t1 - t0;
  s->ms[5] = t1 - t0;
  const int n_sel = (int)mm[6];
  if (!n_sel) return SFMHIP_OK;
  const float hmax = sfmcloud::ord_val(mm[5]);
  const double h0 = o.ground != o.ground ? (double)sfmcloud::ord_val(mm[2]) : o.ground / o.scale;
  const int S = slice_count(hmax, h0, f.t);
  if (!S) return SFMHIP_OK;
  // rule 4: slices in (slice, input index) order
  int *keys_in = c->ibuf[0], *vals_in = c->ibuf[1], *keys_out = c->ibuf[2], *vals_out = c->ibuf[3];
  SFM_HIP_TRY(hipMemsetAsync(s->cnt, 0, sizeof(int) * ((size_t)S + 1), st));
  hipLaunchKernelGGL(dnd_keys, dim3(std::min(blocks(n, 256), 1024u)), dim3(256), 0, st, s->frame, n, h0, f.t, S, keys_in, vals_in, s->cnt);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(sfmgrid::scan(c, s->cnt, s->start, (size_t)S + 1, nullptr));
  SFM_TRY(sfmgrid::cell_sort(c, S, keys_in, keys_out, vals_in, vals_out, n));
  hipLaunchKernelGGL(dnd_gather, dim3(blocks(n, 256)), dim3(256), 0, st, s->frame, vals_out, s->start + S, n, s->pts);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t2 = sfm_now_ms();
  // rule 5
  SFM_HIP_TRY(hipMemsetAsync(s->keys, 0, sizeof(unsigned long long) * (size_t)S, st));
  RansacArgs ra;
  ra.r_min = f.r_min, ra.r_max = f.r_max, ra.tol = f.tol, ra.iters = o.ransac_iters, ra.min_slice_pts = o.min_slice_pts, ra.seed = o.seed;
  hipLaunchKernelGGL(dnd_ransac, dim3(blocks(o.ransac_iters, HPB), S), dim3(64 * RW), 0, st, s->pts, s->start, s->cnt, ra, s->keys);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t3 = sfm_now_ms();
  // rule 6, then the table for rule 7
  RefitArgs fa;
  fa.r_min = f.r_min, fa.r_max = f.r_max, fa.tol = f.tol, fa.min_inliers = o.min_inliers, fa.min_sectors = o.min_sectors;
  fa.min_slice_pts = o.min_slice_pts, fa.seed = o.seed;
  hipLaunchKernelGGL(dnd_refit, dim3(S), dim3(CHUNK), 0, st, s->pts, s->start, s->cnt, s->keys, fa, s->table);
  SFM_HIP_TRY(hipGetLastError());
  slices.resize((size_t)S);
  SFM_HIP_TRY(hipMemcpyAsync(slices.data(), s->table, sizeof(Slice) * (size_t)S, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t4 = sfm_now_ms();
  double r_dbh, ce, cn;
  const int dflags = dbh_from_slices(slices.data(), S, f, r_dbh, ce, cn);
  // rules 8 - 10
  if (!(dflags & F_DBH_NONE)) {
    hipLaunchKernelGGL(dnd_extent, dim3(S), dim3(256), 0, st, s->pts, s->start, s->cnt, ce, cn, f.bin, o.extent_q, s->table);
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(slices.data(), s->table, sizeof(Slice) * (size_t)S, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
  }
  const int cb = crown_base(slices.data(), S, o, f, r_dbh);
  float mn[2] = {0, 0}, mx[2] = {0, 0};
  if (cb >= 0) {
    AtOrAbove ok;
    ok.hb = h0 + (double)cb * f.t;
    SFM_TRY(sfmgrid::minmax(c, s->frame, n, ok, mm));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    for (int a = 0; a < 2; ++a) {
      mn[a] = sfmcloud::ord_val(mm[a]);
      mx[a] = sfmcloud::ord_val(mm[3 + a]);
    }
  }
  finish(o, f, h0, hmax, n_sel, S, dflags, r_dbh, ce, cn, cb, mn, mx, res);
  const double t5 = sfm_now_ms();
  s->ms[1] = t2 - t1;
  s->ms[2] = t3 - t2;
  s->ms[3] = t4 - t3;
  s->ms[4] = t5 - t4;
  s->ms[5] = t5 - t0;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_dendro_default_opts(sfmhip_dendro_opts* o) {
  if (!o) return;
  *o = mirror<sfmhip_dendro_opts>(default_opts());
}

extern "C" int sfmhip_cloud_dendrometry(sfmhip_cloud* c, const int32_t* labels, int32_t label, const sfmhip_dendro_opts* opts,
                                        sfmhip_dendro_result* out) {
  if (!c || !opts || !out) return SFMHIP_ERR_ARG;
  Result res;
  std::vector<Slice> slices;
  SFM_TRY(run(c, labels, label, mirror<Opts>(*opts), res, slices));
  *out = mirror<sfmhip_dendro_result>(res);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_dendro_profile(sfmhip_cloud* c, const int32_t* labels, int32_t label, const sfmhip_dendro_opts* opts,
                                           int cap, sfmhip_dendro_slice* slices, int32_t* n_slices, sfmhip_dendro_result* out) {
  if (!c || !opts || !n_slices || cap < 0 || (cap > 0 && !slices)) return SFMHIP_ERR_ARG;
  Result res;
  std::vector<Slice> rows;
  SFM_TRY(run(c, labels, label, mirror<Opts>(*opts), res, rows));
  *n_slices = (int32_t)rows.size();
  if (out) *out = mirror<sfmhip_dendro_result>(res);
  const size_t m = std::min(rows.size(), (size_t)cap);
  if (m) memcpy(slices, rows.data(), sizeof(Slice) * m);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_dendro_last_timing(sfmhip_cloud* c, double ms6[6]) {
  if (!c || !ms6) return SFMHIP_ERR_ARG;
  const DndState* s = sfmgrid::stage<DndState>(c);
  for (int i = 0; i < 6; ++i) ms6[i] = s->ms[i];
  return SFMHIP_OK;
}
