// segment.hip -- the colour region growing after map3D (reference src/Segmentation.cpp:3-66: pcl::RegionGrowingRGB over
// the indices of a PassThrough) and Dendrometry::estimate's bounds (src/DendrometryE.cpp) on gfx950, on the
// device-resident cloud of cloud.hip.  The rules are DESIGN.md f-8's; the arithmetic is segment.h's.
//
// The indexed points are gathered into an array of their own, in list order (ascending indices), so everything below
// works on list positions: position order is index order.
// seg_knn: one wave per point, in cell order, over a grid of the indexed points.  The wave keeps the sorted (d2, index)
// list of 128 slots two per lane (lane l: slots 2l, 2l + 1); candidates are tested a lane each, and every candidate
// that beats the k-th entry is inserted by one shift (a lane-to-lane move of the odd slots).  The ring search and its
// stopping rule restate cloud.hip's cloud_knn line for line (the nearest face of the searched block against the k-th d2);
// a change to either is a change to both.
// seg_grow_round: min-label propagation over the directed graph u -> v (v among u's first 30 entries, colour
// difference to u within the point threshold), atomicMin in place plus pointer jumping, until a round changes nothing;
// the segment of v is the smallest u that reaches it, segment numbers are the ranks of those minima (f-8, rule 4).
// Segment statistics: integer counts and channel sums by atomicAdd (exact, order-free); the segment-pair minima by
// emitting (a, b, d2) for every neighbour entry that crosses segments, rocPRIM's radix sort and reduce_by_key(min);
// a second stable sort by (a, d2) leaves every segment's neighbours ascending by (d2, segment), of which the first
// 100 are stored in reverse.  Rules 8-10 run on the host from the downloaded tables (segment.h).
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include "segment.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_reduce_by_key.hpp>
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmgrid;

namespace {

constexpr int WAVES = 4;  // points (waves) per seg_knn workgroup

struct SegState {  // on the cloud handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::SEGMENT;  // (its slot on the handle: stage<SegState>(cloud))
  Grid g;                             // the grid of the indexed points of the call in progress (releases itself)
  double ms[5] = {0, 0, 0, 0, 0};     // subset k-NN, growth, segment statistics, host region step, whole call
};

__global__ void seg_gather(const float* xyz, const int* ind, int m, float* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const size_t j = (size_t)ind[r];
  out[3 * (size_t)r] = xyz[3 * j];
  out[3 * (size_t)r + 1] = xyz[3 * j + 1];
  out[3 * (size_t)r + 2] = xyz[3 * j + 2];
}

__global__ __launch_bounds__(64 * WAVES) void seg_knn(GridDev g, double abs_eps, int k, int* out_idx, float* out_d2) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * WAVES + (threadIdx.x >> 6);
  if (i >= g.n_valid) return;  // (uniform in the wave; no barrier below)
  const float4 p = g.pts[i];
  const int orig = __float_as_int(p.w);
  const int key = g.keys[i];
  const int c[3] = {key % g.D[0], (key / g.D[0]) % g.D[1], key / (g.D[0] * g.D[1])};
  const float inf = sfmcloud::bits_f(0x7F800000u);
  float da = inf, db = inf;  // slots 2 lane and 2 lane + 1 of the sorted list
  int ia = INT_MAX, ib = INT_MAX;
  float kd = inf;  // slot k - 1
  int ki = INT_MAX;
  const int klane = (k - 1) >> 1;
  const bool kodd = ((k - 1) & 1) != 0;
  auto scan_row = [&](int row, int xa, int xb) {
    int s, e;
    row_span(g, row, xa, xb, &s, &e);
    for (int b = s; b < e; b += 64) {
      const int j = b + lane;
      float cd = inf;
      int ci = INT_MAX;
      if (j < e) {
        const float4 q = g.pts[j];
        cd = sfmcloud::dist2(p.x, p.y, p.z, q.x, q.y, q.z);
        ci = __float_as_int(q.w);
      }
      unsigned long long todo = __ballot(j < e && sfmcloud::knn_less(cd, ci, kd, ki));
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float xd = __shfl(cd, src);
        const int xi = __shfl(ci, src);
        if (!sfmcloud::knn_less(xd, xi, kd, ki)) continue;  // (the k-th entry moved since the ballot)
        const bool less_a = sfmcloud::knn_less(da, ia, xd, xi), less_b = sfmcloud::knn_less(db, ib, xd, xi);
        const float pd = __shfl_up(db, 1);  // slot 2 lane - 1
        const int pi = __shfl_up(ib, 1);
        const bool prev_less = lane == 0 || sfmcloud::knn_less(pd, pi, xd, xi);
        const float nda = less_a ? da : (prev_less ? xd : pd);
        const int nia = less_a ? ia : (prev_less ? xi : pi);
        const float ndb = less_b ? db : (less_a ? xd : da);
        const int nib = less_b ? ib : (less_a ? xi : ia);
        da = nda;
        ia = nia;
        db = ndb;
        ib = nib;
        kd = __shfl(kodd ? db : da, klane);
        ki = __shfl(kodd ? ib : ia, klane);
      }
    }
  };
  for (int R = 0;; ++R) {
    for (int z = max(c[2] - R, 0); z <= min(c[2] + R, g.D[2] - 1); ++z)
      for (int y = max(c[1] - R, 0); y <= min(c[1] + R, g.D[1] - 1); ++y) {
        const int row = (z * g.D[1] + y) * g.D[0];
        if (abs(z - c[2]) == R || abs(y - c[1]) == R) {
          scan_row(row, max(c[0] - R, 0), min(c[0] + R, g.D[0] - 1));
        } else {
          if (c[0] - R >= 0) scan_row(row, c[0] - R, c[0] - R);
          if (c[0] + R <= g.D[0] - 1) scan_row(row, c[0] + R, c[0] + R);
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
  const size_t base = (size_t)orig * k;
  if (2 * lane < k) {
    out_idx[base + 2 * lane] = 2 * lane < kk ? ia : -1;
    out_d2[base + 2 * lane] = 2 * lane < kk ? da : inf;
  }
  if (2 * lane + 1 < k) {
    out_idx[base + 2 * lane + 1] = 2 * lane + 1 < kk ? ib : -1;
    out_d2[base + 2 * lane + 1] = 2 * lane + 1 < kk ? db : inf;
  }
}

// a point with a list (a finite point: its own entry is there) starts as its own label; the others have none
__global__ void seg_grow_init(const int* knn_idx, int k, int m, int* lab) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  lab[u] = knn_idx[(size_t)u * k] >= 0 ? u : -1;
}

// lab[v] is always a point that reaches v; a round lowers it to lab[lab[..]] (reaching is transitive) and hands it to
// the points v reaches directly.  A round that lowers nothing leaves lab[v] <= lab[u] on every edge: the fixpoint.
__global__ void seg_grow_round(const int* knn_idx, int k, int nn, const uint32_t* rgb, float p2p2, int m, int* lab, int* changed) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  int lu = lab[u];
  if (lu < 0) return;
  bool ch = false;
  for (int r = lab[lu]; r < lu; r = lab[lu]) lu = r;  // (strictly decreasing: ends)
  if (atomicMin(&lab[u], lu) > lu) ch = true;
  const uint32_t cu = rgb[u];
  const int* row = knn_idx + (size_t)u * k;
  for (int s = 0; s < nn; ++s) {
    const int v = row[s];
    if (v < 0) break;
    if (v == u || !sfmseg::point_joins(cu, rgb[v], p2p2)) continue;
    if (atomicMin(&lab[v], lu) > lu) ch = true;
  }
  if (ch) *changed = 1;
}

__global__ void seg_root_flags(const int* lab, int m, int* flags) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  flags[u] = lab[u] == u ? 1 : 0;
}

// the segment of every point, and the segments' counts and channel sums
__global__ void seg_assign(const int* lab, const int* off, const uint32_t* rgb, int m, int* seg, unsigned* acc /* 4 per segment */) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  const int l = lab[u];
  const int s = l >= 0 ? off[l] : -1;
  seg[u] = s;
  if (s < 0) return;
  const uint32_t c = rgb[u];
  atomicAdd(acc + 4 * (size_t)s, 1u);
  atomicAdd(acc + 4 * (size_t)s + 1, (c >> 16) & 255u);
  atomicAdd(acc + 4 * (size_t)s + 2, (c >> 8) & 255u);
  atomicAdd(acc + 4 * (size_t)s + 3, c & 255u);
}

__global__ void seg_colours(const unsigned* acc, int n_seg, int* count, unsigned* colour) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  const unsigned n = acc[4 * (size_t)s];
  count[s] = (int)n;
  for (int ch = 0; ch < 3; ++ch) colour[3 * (size_t)s + ch] = sfmseg::seg_channel(acc[4 * (size_t)s + 1 + ch], n);
}

// mode 0: the number of u's entries that lie in another segment; mode 1: emit them at off[u]
__global__ void seg_cross(const int* knn_idx, const float* knn_d2, int k, const int* seg, int m, int n_seg, int mode, int* cnt,
                          const int* off, unsigned long long* keys, float* vals) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= m) return;
  const int a = seg[u];
  int n = 0;
  if (a >= 0) {
    const int* row = knn_idx + (size_t)u * k;
    const int o = mode ? off[u] : 0;
    for (int s = 0; s < k; ++s) {
      const int v = row[s];
      if (v < 0) break;
      const int b = seg[v];
      if (b == a) continue;
      if (mode) {
        keys[o + n] = (unsigned long long)a * (unsigned)n_seg + (unsigned)b;
        vals[o + n] = knn_d2[(size_t)u * k + s];
      }
      ++n;
    }
  }
  if (!mode) cnt[u] = n;
}

// reduced pairs (a n_seg + b, d2) -> keys (a << 32 | d2's bits: d2 >= 0, so its bits order as its value), values b
__global__ void seg_pair_keys(const unsigned long long* pair, const float* d2, int np, int n_seg, unsigned long long* keys, int* b_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= np) return;
  const unsigned long long a = pair[e] / (unsigned)n_seg;
  b_out[e] = (int)(pair[e] - a * (unsigned)n_seg);
  keys[e] = (a << 32) | (unsigned long long)(unsigned)__float_as_int(d2[e]);
}

__global__ void seg_pair_ranges(const unsigned long long* keys, int np, int* start, int* end) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= np) return;
  const int a = (int)(keys[e] >> 32);
  if (e == 0 || (int)(keys[e - 1] >> 32) != a) start[a] = e;
  if (e == np - 1 || (int)(keys[e + 1] >> 32) != a) end[a] = e + 1;
}

__global__ void seg_nbr_counts(const int* start, const int* end, int n_seg, int keep, int* cnt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_seg) return;
  cnt[s] = min(end[s] - start[s], keep);
}

// the first cnt[a] entries of a's ascending run, stored in reverse: descending (d2, segment), the heap's pop order
__global__ void seg_nbr_write(const unsigned long long* keys, const int* b, int np, const int* start, const int* cnt, const int* off,
                              int* nbr_seg, float* nbr_d2) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= np) return;
  const int a = (int)(keys[e] >> 32);
  const int pos = e - start[a];
  if (pos >= cnt[a]) return;
  const int o = off[a] + cnt[a] - 1 - pos;
  nbr_seg[o] = b[e];
  nbr_d2[o] = __int_as_float((int)(unsigned)(keys[e] & 0xFFFFFFFFull));
}

// the index list: strictly ascending indices of the cloud (what PassThrough writes)
bool indices_valid(const sfmhip_cloud* c, const int32_t* ind, int m) {
  if (!ind || m < 1 || m > c->n) return false;
  for (int r = 0; r < m; ++r)
    if (ind[r] < 0 || ind[r] >= c->n || (r > 0 && ind[r] <= ind[r - 1])) return false;
  return true;
}

// the device part of one call: everything that stays on the device between the stages
struct Work {
  int m = 0, k = 0, n_valid = 0;
  int* ind = nullptr;      // m: the index list
  float* xyz = nullptr;    // 3 m: the indexed points, list order
  uint32_t* rgb = nullptr; // m
  int* knn_idx = nullptr;  // m k, list positions, -1 padded
  float* knn_d2 = nullptr;
  int* lab = nullptr;      // m: the smallest position that reaches the point
  int* seg = nullptr;      // m
  int n_seg = 0, rounds = 0;
};

int subset_knn(sfmhip_cloud* c, SegState* s, DevBufs& B, const int32_t* indices, int m, int k, Work& w) {
  hipStream_t st = c->ctx->stream;
  if ((unsigned long long)m * (unsigned)k > (unsigned long long)INT_MAX) return SFMHIP_ERR_UNSUPPORTED;
  w.m = m;
  w.k = k;
  SFM_TRY(B.alloc(&w.ind, (size_t)m));
  SFM_TRY(B.alloc(&w.xyz, (size_t)3 * m));
  SFM_TRY(B.alloc(&w.knn_idx, (size_t)m * k));
  SFM_TRY(B.alloc(&w.knn_d2, (size_t)m * k));
  SFM_HIP_TRY(hipMemcpyAsync(w.ind, indices, sizeof(int) * (size_t)m, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(seg_gather, dim3(blocks(m, 256)), dim3(256), 0, st, c->xyz, w.ind, m, w.xyz);
  SFM_HIP_TRY(hipGetLastError());
  GridSrc src;
  src.xyz = w.xyz;
  src.n = m;
  unsigned mm[7];
  SFM_TRY(minmax(c, w.xyz, m, FinitePoint(), mm));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  src.n_valid = (int)mm[6];
  for (int a = 0; a < 3; ++a) {
    src.lo[a] = src.n_valid ? (double)sfmcloud::ord_val(mm[a]) : 0.0;
    src.hi[a] = src.n_valid ? (double)sfmcloud::ord_val(mm[3 + a]) : 0.0;
  }
  w.n_valid = src.n_valid;
  SFM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)w.knn_idx, -1, (size_t)m * k, st));  // points with no list: -1 / +inf
  SFM_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)w.knn_d2, (int)0x7F800000, (size_t)m * k, st));
  if (src.n_valid > 0) {
    SFM_TRY(density_grid(c, src, s->g, std::min(48.0, std::max(16.0, k / 3.0))));
    double mag = 0;
    for (int a = 0; a < 3; ++a) mag = std::max(mag, std::fabs(src.lo[a]) + std::fabs(src.hi[a]));
    const double abs_eps = (mag + s->g.cell) * 1e-12;  // (the double rounding of a cell coordinate, with room to spare)
    hipLaunchKernelGGL(seg_knn, dim3(blocks(src.n_valid, WAVES)), dim3(64 * WAVES), 0, st, s->g.dev(src.n_valid), abs_eps, k,
                       w.knn_idx, w.knn_d2);
    SFM_HIP_TRY(hipGetLastError());
  }
  SFM_HIP_TRY(hipStreamSynchronize(st));
  s->g.release();
  return SFMHIP_OK;
}

int grow(sfmhip_cloud* c, DevBufs& B, const uint32_t* rgb_all, const int32_t* indices, const sfmseg::Opts& o, Work& w) {
  hipStream_t st = c->ctx->stream;
  const int m = w.m;
  std::vector<uint32_t> rgb((size_t)m);
  for (int r = 0; r < m; ++r) rgb[r] = rgb_all[indices[r]] & 0x00FFFFFFu;
  SFM_TRY(B.alloc(&w.rgb, (size_t)m));
  SFM_TRY(B.alloc(&w.lab, (size_t)m));
  SFM_TRY(B.alloc(&w.seg, (size_t)m));
  int* changed = nullptr;
  SFM_TRY(B.alloc(&changed, 1));
  SFM_HIP_TRY(hipMemcpyAsync(w.rgb, rgb.data(), sizeof(uint32_t) * (size_t)m, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(seg_grow_init, dim3(blocks(m, 256)), dim3(256), 0, st, w.knn_idx, w.k, m, w.lab);
  SFM_HIP_TRY(hipGetLastError());
  const int nn = std::min(o.neighbour_number, w.k);
  const float p2p2 = sfmseg::squared(o.point_color_threshold);
  w.rounds = 0;
  for (;;) {
    if (w.rounds > m) return SFMHIP_ERR_STATE;  // (a label falls at most m times: cannot happen)
    int ch = 0;
    SFM_HIP_TRY(hipMemsetAsync(changed, 0, sizeof(int), st));
    hipLaunchKernelGGL(seg_grow_round, dim3(blocks(m, 256)), dim3(256), 0, st, w.knn_idx, w.k, nn, w.rgb, p2p2, m, w.lab, changed);
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(&ch, changed, sizeof(int), hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    ++w.rounds;
    if (!ch) break;
  }
  return SFMHIP_OK;
}

// segment numbers (the ranks of the roots), counts, colours; the tables stay on the device in `d_*`, sized by n_seg
struct DevTables {
  unsigned* acc = nullptr;
  int* count = nullptr;
  unsigned* colour = nullptr;
};

int number_segments(sfmhip_cloud* c, DevBufs& B, Work& w, DevTables& d) {
  hipStream_t st = c->ctx->stream;
  const int m = w.m;
  int *flags = nullptr, *off = nullptr;
  SFM_TRY(B.alloc(&flags, (size_t)m));
  SFM_TRY(B.alloc(&off, (size_t)m));
  hipLaunchKernelGGL(seg_root_flags, dim3(blocks(m, 256)), dim3(256), 0, st, w.lab, m, flags);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(scan(c, flags, off, (size_t)m, &w.n_seg));  // (m >= 1: indices_valid)
  if (w.n_seg < 0 || w.n_seg > m) return SFMHIP_ERR_STATE;
  const size_t ns = (size_t)std::max(w.n_seg, 1);  // (a list with no finite point has no segment: the tables keep one unused row)
  SFM_TRY(B.alloc(&d.acc, 4 * ns));
  SFM_TRY(B.alloc(&d.count, ns));
  SFM_TRY(B.alloc(&d.colour, 3 * ns));
  SFM_HIP_TRY(hipMemsetAsync(d.acc, 0, sizeof(unsigned) * 4 * ns, st));
  hipLaunchKernelGGL(seg_assign, dim3(blocks(m, 256)), dim3(256), 0, st, w.lab, off, w.rgb, m, w.seg, d.acc);
  SFM_HIP_TRY(hipGetLastError());
  if (w.n_seg > 0) hipLaunchKernelGGL(seg_colours, dim3(blocks(w.n_seg, 256)), dim3(256), 0, st, d.acc, w.n_seg, d.count, d.colour);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

int segment_tables(sfmhip_cloud* c, DevBufs& B, const sfmseg::Opts& o, Work& w, const DevTables& d, sfmseg::SegTables& t) {
  hipStream_t st = c->ctx->stream;
  const int m = w.m, S = w.n_seg;
  t.n_seg = S;
  t.count.assign((size_t)S, 0);
  t.colour.assign((size_t)3 * S, 0);
  t.nbr_off.assign((size_t)S + 1, 0);
  t.nbr_seg.clear();
  t.nbr_d2.clear();
  if (S == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipMemcpyAsync(t.count.data(), d.count, sizeof(int) * (size_t)S, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(t.colour.data(), d.colour, sizeof(unsigned) * 3 * (size_t)S, hipMemcpyDeviceToHost, st));
  int *cnt = nullptr, *off = nullptr;
  SFM_TRY(B.alloc(&cnt, (size_t)m));
  SFM_TRY(B.alloc(&off, (size_t)m));
  hipLaunchKernelGGL(seg_cross, dim3(blocks(m, 256)), dim3(256), 0, st, w.knn_idx, w.knn_d2, w.k, w.seg, m, S, 0, cnt, nullptr, nullptr,
                     nullptr);
  SFM_HIP_TRY(hipGetLastError());
  int ne = 0;
  SFM_TRY(scan(c, cnt, off, (size_t)m, &ne));
  if (ne < 0) return SFMHIP_ERR_STATE;
  if (ne == 0) return SFMHIP_OK;
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  float *v0 = nullptr, *v1 = nullptr;
  SFM_TRY(B.alloc(&k0, (size_t)ne));
  SFM_TRY(B.alloc(&k1, (size_t)ne));
  SFM_TRY(B.alloc(&v0, (size_t)ne));
  SFM_TRY(B.alloc(&v1, (size_t)ne));
  hipLaunchKernelGGL(seg_cross, dim3(blocks(m, 256)), dim3(256), 0, st, w.knn_idx, w.knn_d2, w.k, w.seg, m, S, 1, cnt, off, k0, v0);
  SFM_HIP_TRY(hipGetLastError());
  unsigned sbits = 1;
  while (sbits < 32 && (1ull << sbits) < (unsigned long long)S) ++sbits;
  size_t need = 0;
  SFM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, k0, k1, v0, v1, (size_t)ne, 0u, std::min(64u, 2 * sbits + 1), st));
  SFM_TRY(grow_tmp(c, need));
  need = c->tmp.cap;
  SFM_HIP_TRY(rocprim::radix_sort_pairs(c->tmp.p, need, k0, k1, v0, v1, (size_t)ne, 0u, std::min(64u, 2 * sbits + 1), st));
  // the minimum d2 of every (a, b): the unique keys into k0, the minima into v0, their number into cnt[0]
  need = 0;
  SFM_HIP_TRY(rocprim::reduce_by_key(nullptr, need, k1, v1, (size_t)ne, k0, v0, cnt, rocprim::minimum<float>(),
                                     rocprim::equal_to<unsigned long long>(), st));
  SFM_TRY(grow_tmp(c, need));
  need = c->tmp.cap;
  SFM_HIP_TRY(rocprim::reduce_by_key(c->tmp.p, need, k1, v1, (size_t)ne, k0, v0, cnt, rocprim::minimum<float>(),
                                     rocprim::equal_to<unsigned long long>(), st));
  int np = 0;
  SFM_HIP_TRY(hipMemcpyAsync(&np, cnt, sizeof(int), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (np < 1 || np > ne) return SFMHIP_ERR_STATE;
  // every segment's neighbours ascending by (d2, segment): a stable sort by (a, d2) of pairs that are ascending in b
  int *b0 = nullptr, *b1 = nullptr;
  SFM_TRY(B.alloc(&b0, (size_t)np));
  SFM_TRY(B.alloc(&b1, (size_t)np));
  hipLaunchKernelGGL(seg_pair_keys, dim3(blocks(np, 256)), dim3(256), 0, st, k0, v0, np, S, k1, b0);
  SFM_HIP_TRY(hipGetLastError());
  need = 0;
  SFM_HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, k1, k0, b0, b1, (size_t)np, 0u, 32u + sbits, st));
  SFM_TRY(grow_tmp(c, need));
  need = c->tmp.cap;
  SFM_HIP_TRY(rocprim::radix_sort_pairs(c->tmp.p, need, k1, k0, b0, b1, (size_t)np, 0u, 32u + sbits, st));
  int *start = nullptr, *end = nullptr, *ncnt = nullptr, *noff = nullptr, *nseg = nullptr;
  float* nd2 = nullptr;
  SFM_TRY(B.alloc(&start, (size_t)S));
  SFM_TRY(B.alloc(&end, (size_t)S));
  SFM_TRY(B.alloc(&ncnt, (size_t)S));
  SFM_TRY(B.alloc(&noff, (size_t)S));
  SFM_HIP_TRY(hipMemsetAsync(start, 0, sizeof(int) * (size_t)S, st));
  SFM_HIP_TRY(hipMemsetAsync(end, 0, sizeof(int) * (size_t)S, st));
  hipLaunchKernelGGL(seg_pair_ranges, dim3(blocks(np, 256)), dim3(256), 0, st, k0, np, start, end);
  hipLaunchKernelGGL(seg_nbr_counts, dim3(blocks(S, 256)), dim3(256), 0, st, start, end, S, o.region_neighbour_number, ncnt);
  SFM_HIP_TRY(hipGetLastError());
  int total = 0;
  SFM_TRY(scan(c, ncnt, noff, (size_t)S, &total));  // (S >= 1: the early return above)
  if (total < 1 || total > np) return SFMHIP_ERR_STATE;
  SFM_TRY(B.alloc(&nseg, (size_t)total));
  SFM_TRY(B.alloc(&nd2, (size_t)total));
  hipLaunchKernelGGL(seg_nbr_write, dim3(blocks(np, 256)), dim3(256), 0, st, k0, b1, np, start, ncnt, noff, nseg, nd2);
  SFM_HIP_TRY(hipGetLastError());
  t.nbr_seg.resize((size_t)total);
  t.nbr_d2.resize((size_t)total);
  SFM_HIP_TRY(hipMemcpyAsync(t.nbr_off.data(), noff, sizeof(int) * (size_t)S, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(t.nbr_seg.data(), nseg, sizeof(int) * (size_t)total, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(t.nbr_d2.data(), nd2, sizeof(float) * (size_t)total, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  t.nbr_off[(size_t)S] = total;
  return SFMHIP_OK;
}

sfmseg::Opts to_opts(const sfmhip_segment_opts* o) {
  sfmseg::Opts r;
  r.region_neighbour_number = o->region_neighbour_number;
  r.neighbour_number = o->neighbour_number;
  r.min_cluster_size = o->min_cluster_size;
  r.max_cluster_size = o->max_cluster_size;
  r.distance_threshold = o->distance_threshold;
  r.point_color_threshold = o->point_color_threshold;
  r.region_color_threshold = o->region_color_threshold;
  return r;
}

}  // namespace

extern "C" void sfmhip_segment_default_opts(sfmhip_segment_opts* o) {
  if (!o) return;
  const sfmseg::Opts r = sfmseg::reference_opts();
  o->region_neighbour_number = r.region_neighbour_number;
  o->neighbour_number = r.neighbour_number;
  o->min_cluster_size = r.min_cluster_size;
  o->max_cluster_size = r.max_cluster_size;
  o->distance_threshold = r.distance_threshold;
  o->point_color_threshold = r.point_color_threshold;
  o->region_color_threshold = r.region_color_threshold;
}

extern "C" int sfmhip_cloud_minmax(sfmhip_cloud* c, float* mn, float* mx, double* height) {
  if (!c || !mn || !mx) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  unsigned mm[7];
  SFM_TRY(minmax(c, c->xyz, c->n, FinitePoint(), mm));
  SFM_HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  for (int a = 0; a < 3; ++a) {  // (pcl::getMinMax3D starts at FLT_MAX / -FLT_MAX: what a cloud with no finite point keeps)
    mn[a] = mm[6] ? sfmcloud::ord_val(mm[a]) : FLT_MAX;
    mx[a] = mm[6] ? sfmcloud::ord_val(mm[3 + a]) : -FLT_MAX;
  }
  if (height) *height = sfmseg::height(mn, mx);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_subset_knn(sfmhip_cloud* c, const int32_t* indices, int n_idx, int k, int32_t* idx, float* d2) {
  if (!c || k < 1 || k > sfmseg::KMAX || !idx || !d2 || !indices_valid(c, indices, n_idx)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  DevBufs B;
  Work w;
  SFM_TRY(subset_knn(c, stage<SegState>(c), B, indices, n_idx, k, w));
  const size_t e = (size_t)n_idx * k;
  hipStream_t st = c->ctx->stream;
  SFM_HIP_TRY(hipMemcpyAsync(idx, w.knn_idx, e * 4, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(d2, w.knn_d2, e * 4, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  for (size_t s = 0; s < e; ++s)
    if (idx[s] >= 0) idx[s] = indices[idx[s]];  // list positions -> cloud indices
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_segment_grow(sfmhip_cloud* c, const uint32_t* rgb, const int32_t* indices, int n_idx,
                                         const sfmhip_segment_opts* opts, int32_t* segment, int32_t* n_segments, int32_t* rounds) {
  if (!c || !rgb || !opts || !segment || !n_segments || !indices_valid(c, indices, n_idx)) return SFMHIP_ERR_ARG;
  const sfmseg::Opts o = to_opts(opts);
  if (!sfmseg::opts_valid(o)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  DevBufs B;
  Work w;
  DevTables d;
  SFM_TRY(subset_knn(c, stage<SegState>(c), B, indices, n_idx, o.region_neighbour_number, w));
  SFM_TRY(grow(c, B, rgb, indices, o, w));
  SFM_TRY(number_segments(c, B, w, d));
  std::vector<int> seg((size_t)n_idx);
  SFM_HIP_TRY(hipMemcpyAsync(seg.data(), w.seg, sizeof(int) * (size_t)n_idx, hipMemcpyDeviceToHost, c->ctx->stream));
  SFM_HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  for (int i = 0; i < c->n; ++i) segment[i] = -1;
  for (int r = 0; r < n_idx; ++r) segment[indices[r]] = seg[r];
  *n_segments = w.n_seg;
  if (rounds) *rounds = w.rounds;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_segment_rgb(sfmhip_cloud* c, const uint32_t* rgb, const int32_t* indices, int n_idx,
                                        const sfmhip_segment_opts* opts, int32_t* labels, int32_t* n_clusters,
                                        sfmhip_segment_stats* stats) {
  if (!c || !rgb || !opts || !labels || !n_clusters || !indices_valid(c, indices, n_idx)) return SFMHIP_ERR_ARG;
  const sfmseg::Opts o = to_opts(opts);
  if (!sfmseg::opts_valid(o)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  SegState* s = stage<SegState>(c);
  DevBufs B;
  Work w;
  DevTables d;
  sfmseg::SegTables t;
  const double t0 = sfm_now_ms();
  SFM_TRY(subset_knn(c, s, B, indices, n_idx, o.region_neighbour_number, w));
  const double t1 = sfm_now_ms();
  SFM_TRY(grow(c, B, rgb, indices, o, w));
  const double t2 = sfm_now_ms();
  SFM_TRY(number_segments(c, B, w, d));
  SFM_TRY(segment_tables(c, B, o, w, d, t));
  std::vector<int> seg((size_t)n_idx);
  SFM_HIP_TRY(hipMemcpyAsync(seg.data(), w.seg, sizeof(int) * (size_t)n_idx, hipMemcpyDeviceToHost, c->ctx->stream));
  SFM_HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  const double t3 = sfm_now_ms();
  std::vector<int> seg_region, point_cluster;
  int n_regions = 0, nc = 0;
  sfmseg::regions_from_tables(o, t, seg.data(), n_idx, seg_region, n_regions, point_cluster, nc);
  for (int i = 0; i < c->n; ++i) labels[i] = -1;
  for (int r = 0; r < n_idx; ++r) labels[indices[r]] = point_cluster[r];
  *n_clusters = nc;
  const double t4 = sfm_now_ms();
  s->ms[0] = t1 - t0;
  s->ms[1] = t2 - t1;
  s->ms[2] = t3 - t2;
  s->ms[3] = t4 - t3;
  s->ms[4] = t4 - t0;
  if (stats) {
    stats->n_idx = w.n_valid;
    stats->n_segments = w.n_seg;
    stats->n_regions = n_regions;
    stats->rounds = w.rounds;
  }
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_segment_last_timing(sfmhip_cloud* c, double* ms5) {
  if (!c || !ms5) return SFMHIP_ERR_ARG;
  const SegState* s = stage<SegState>(c);
  for (int i = 0; i < 5; ++i) ms5[i] = s->ms[i];
  return SFMHIP_OK;
}
