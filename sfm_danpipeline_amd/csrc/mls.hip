// mls.hip -- moving-least-squares smoothing of the device-resident cloud (sfmhip_cloud_mls) on gfx950: PCL
// 1.8.1's MovingLeastSquares with no upsampling and SIMPLE projection, by the rules M1-M7 of include/sfmhip.h.  The arithmetic
// is mls.h's, which the CPU test stub compiles too.
//
// mls_fit<O>: cloud_radius_count's shape on the handle's radius grid -- a workgroup of one wave per chunk of <= 64 points of
// one cell; the 9 row spans around the cell are staged through LDS in tiles of 64 points and every lane tests the tile against
// its own point -- because that walk meets a point's neighbours in ascending (cell key, input index), which is M2's order.
// Sweep A sums the 9 moments of the plane fit and the count in f64 registers; the eigen step, the projection and the local
// frame follow per lane; sweep B (orders 1 and 2 only: the kernel is a template on the order) walks the same spans again and
// sums the distinct moments of the weighted normal equations and their right-hand side; the Cholesky solve runs per lane with
// every index known at compile time.  A point's row goes to its input index; flags, the handle's scan and a gather bring the
// surviving rows together in input order (M7).  The stats are integer ballots and integer atomics.  No atomics on floats.
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include "mls.h"
#include <algorithm>
#include <vector>

using namespace sfmgrid;

namespace {

struct MlsState {  // on the cloud handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::MLS;
  Grow<float> xyz, n4, xyz_out, n4_out;  // rows by input index (3 n, 4 n); the gathered rows (3 m, 4 m)
  Grow<int> stats;
  double ms[3] = {0, 0, 0};  // grid, fit, compaction of the last call
};

enum { S_DROPPED, S_PLANE_ONLY, S_DEGENERATE, S_FIT_FAILED, S_MAX_NEIGHBOURS, S_WORDS };

// the walk of cloud_radius_count: f(q) for every point q of the 9 row spans around cell `cell`, in sorted order.  Every lane
// of the wave takes every step (the barriers are uniform); what a lane does with q is its own business.
template <class F>
__device__ __forceinline__ void sweep(const GridDev& g, int cell, float4* tile, int lane, F f) {
  const int cx = cell % g.D[0], cy = (cell / g.D[0]) % g.D[1], cz = cell / (g.D[0] * g.D[1]);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.D[0] - 1);
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
        for (int j = 0; j < m; ++j) f(tile[j]);
      }
    }
}

__device__ __forceinline__ int wave_count(bool x) { return __popcll(__ballot(x)); }

template <int O>
__global__ __launch_bounds__(CHUNK) void mls_fit(GridDev g, const int4* chunks, float r2, double gauss, float* xyz, float* n4,
                                                 int* flags, int* stats) {
  __shared__ float4 tile[CHUNK];
  const int4 ch = chunks[blockIdx.x];
  const int lane = threadIdx.x;
  const bool live = lane < ch.y;
  const float4 p = g.pts[ch.x + (live ? lane : 0)];
  // sweep A (M3): the plane's sums
  sfmmls::Accu acc;
  sfmmls::accu_zero(acc);
  int cnt = 0;
  sweep(g, ch.z, tile, lane, [&](const float4& q) {
    if (sfmcloud::in_radius(sfmcloud::dist2(p.x, p.y, p.z, q.x, q.y, q.z), r2)) {
      sfmmls::accu_add(acc, (double)q.x, (double)q.y, (double)q.z);
      ++cnt;
    }
  });
  const bool kept = live && cnt >= sfmmls::MIN_NEIGHBOURS;
  const double pd[3] = {(double)p.x, (double)p.y, (double)p.z};
  sfmmls::Plane pl = {};
  if (kept) sfmmls::plane_fit(acc, cnt, pd, pl);
  const bool degenerate = kept && pl.degenerate;
  bool plane_only = false, failed = false;
  double qo[3] = {pl.q[0], pl.q[1], pl.q[2]}, no[3] = {pl.n[0], pl.n[1], pl.n[2]};
  if (O > 0) {
    constexpr int NC = sfmmls::Fit<O>::NC;
    plane_only = kept && !degenerate && cnt < NC;
    const bool fit = kept && !degenerate && cnt >= NC;
    if (__any(fit)) {  // (the workgroup is one wave: uniform)
      // sweep B (M5): the normal equations in the local frame
      sfmmls::Fit<O> f;
      sfmmls::fit_zero(f);
      if (fit) sfmmls::frame(pl);
      sweep(g, ch.z, tile, lane, [&](const float4& q) {
        if (fit && sfmcloud::in_radius(sfmcloud::dist2(p.x, p.y, p.z, q.x, q.y, q.z), r2))
          sfmmls::fit_add<O>(f, pl, gauss, (double)q.x, (double)q.y, (double)q.z);
      });
      if (fit) {
        double c[NC];
        if (sfmmls::fit_solve<O>(f, c)) sfmmls::fit_apply<O>(pl, c, qo, no);
        else failed = true;
      }
    }
  }
  if (kept) {
    const size_t i = (size_t)__float_as_int(p.w);
    float o3[3], o4[4];
    if (degenerate) sfmmls::write_degenerate(pd, o3, o4);
    else sfmmls::write_row(qo, no, pl.curv, false, o3, o4);
    xyz[3 * i] = o3[0], xyz[3 * i + 1] = o3[1], xyz[3 * i + 2] = o3[2];
    *(float4*)(n4 + 4 * i) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    flags[i] = 1;
  }
  // the stats: counts by ballot, the largest neighbourhood by a shuffle tree, one integer atomic each per wave
  const int nd = wave_count(live && !kept), np = wave_count(plane_only), ng = wave_count(degenerate), nf = wave_count(failed);
  int mx = live ? cnt : 0;
  for (int off = 32; off >= 1; off >>= 1) mx = max(mx, __shfl_xor(mx, off));
  if (lane == 0) {
    if (nd) atomicAdd(stats + S_DROPPED, nd);
    if (np) atomicAdd(stats + S_PLANE_ONLY, np);
    if (ng) atomicAdd(stats + S_DEGENERATE, ng);
    if (nf) atomicAdd(stats + S_FIT_FAILED, nf);
    atomicMax(stats + S_MAX_NEIGHBOURS, mx);
  }
}

// row r of the output: the row of input point idx[r]
__global__ void mls_gather(const float* xyz, const float* n4, const int* idx, int m, float* out_xyz, float* out_n4) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const size_t i = (size_t)idx[r];
  out_xyz[3 * (size_t)r] = xyz[3 * i];
  out_xyz[3 * (size_t)r + 1] = xyz[3 * i + 1];
  out_xyz[3 * (size_t)r + 2] = xyz[3 * i + 2];
  *(float4*)(out_n4 + 4 * (size_t)r) = *(const float4*)(n4 + 4 * i);
}

template <int O>
void launch_fit(hipStream_t st, sfmhip_cloud* c, double radius, double gauss, MlsState* s) {
  hipLaunchKernelGGL(mls_fit<O>, dim3((unsigned)c->rg.n_chunks), dim3(CHUNK), 0, st, c->rg.dev(c->n_valid), c->rg.chunks,
                     sfmcloud::radius2(radius), gauss, s->xyz.p, s->n4.p, c->ibuf[0], s->stats.p);
}

}  // namespace

extern "C" int sfmhip_mls_default_opts(sfmhip_mls_opts* o) {
  if (!o) return SFMHIP_ERR_ARG;
  o->search_radius = 0.0;
  o->polynomial_order = 2;
  o->compute_normals = 1;
  o->sqr_gauss_param = 0.0;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_mls(sfmhip_cloud* c, const sfmhip_mls_opts* opts, float* out_xyz, float* out_normals4, int32_t* src_index,
                                int32_t* n_out, sfmhip_mls_stats* stats, sfmhip_cloud** out_cloud) {
  if (!c || !opts || !n_out) return SFMHIP_ERR_ARG;
  const double radius = opts->search_radius;
  if (!(radius > 0.0) || !sfmmls::finite_d(radius) || opts->polynomial_order < 0 || opts->polynomial_order > 2 ||
      !sfmmls::finite_d(opts->sqr_gauss_param))
    return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  const bool timing = c->ctx->timing;
  MlsState* s = stage<MlsState>(c);
  s->ms[0] = s->ms[1] = s->ms[2] = 0;
  const int n = c->n;
  int m = 0;
  int hs[S_WORDS] = {0, 0, 0, 0, 0};
  float* d_out = nullptr;
  if (c->n_valid > 0) {
    const double t0 = sfm_now_ms();
    SFM_TRY(radius_grid(c, radius));  // (waits for the build)
    const double t1 = sfm_now_ms();
    SFM_TRY(s->xyz.need((size_t)3 * n));
    SFM_TRY(s->n4.need((size_t)4 * n));
    SFM_TRY(s->stats.need(S_WORDS));
    SFM_HIP_TRY(hipMemsetAsync(c->ibuf[0], 0, sizeof(int) * (size_t)n, st));  // a non-finite or a dropped point's flag
    SFM_HIP_TRY(hipMemsetAsync(s->stats.p, 0, sizeof(int) * S_WORDS, st));
    if (c->rg.n_chunks > 0) {
      const double gauss = sfmmls::gauss_param(opts->sqr_gauss_param, radius);
      if (opts->polynomial_order == 0) launch_fit<0>(st, c, radius, gauss, s);
      else if (opts->polynomial_order == 1) launch_fit<1>(st, c, radius, gauss, s);
      else launch_fit<2>(st, c, radius, gauss, s);
    }
    SFM_HIP_TRY(hipGetLastError());
    if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
    const double t2 = sfm_now_ms();
    std::vector<int32_t> own;
    int32_t* idx = src_index;
    if (!idx) {
      own.resize((size_t)n);
      idx = own.data();
    }
    SFM_TRY(compact(c, idx, &m));  // (the kept indices stay in ibuf[2] on the device)
    SFM_TRY(s->n4_out.need((size_t)4 * std::max(m, 1)));
    if (out_cloud) {  // the new handle will own its points; without one the gathered points stay in the state's block
      SFM_TRY(sfm_dev_alloc(&d_out, (size_t)3 * std::max(m, 1)));
    } else {
      SFM_TRY(s->xyz_out.need((size_t)3 * std::max(m, 1)));
      d_out = s->xyz_out.p;
    }
    int rc = SFMHIP_OK;
    if (m > 0) {
      hipLaunchKernelGGL(mls_gather, dim3(blocks(m, 256)), dim3(256), 0, st, s->xyz.p, s->n4.p, c->ibuf[2], m, d_out, s->n4_out.p);
      if (hipGetLastError() != hipSuccess) rc = SFMHIP_ERR_HIP;
    }
    auto get = [&](void* dst, const void* src, size_t bytes) {
      if (rc == SFMHIP_OK && dst && bytes && hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) != hipSuccess) rc = SFMHIP_ERR_HIP;
    };
    get(out_xyz, d_out, sizeof(float) * 3 * (size_t)m);
    get(opts->compute_normals ? out_normals4 : nullptr, s->n4_out.p, sizeof(float) * 4 * (size_t)m);
    get(hs, s->stats.p, sizeof hs);
    if (rc == SFMHIP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SFMHIP_ERR_HIP;
    if (rc != SFMHIP_OK) {
      if (out_cloud) hipFree(d_out);
      return rc;
    }
    if (timing) {
      s->ms[0] = t1 - t0;
      s->ms[1] = t2 - t1;
      s->ms[2] = sfm_now_ms() - t2;
    }
  } else if (out_cloud) {
    SFM_TRY(sfm_dev_alloc(&d_out, (size_t)3));
  }
  *n_out = m;
  if (stats) {
    stats->n_out = m;
    stats->n_dropped = hs[S_DROPPED];
    stats->n_plane_only = hs[S_PLANE_ONLY];
    stats->n_degenerate = hs[S_DEGENERATE];
    stats->n_fit_failed = hs[S_FIT_FAILED];
    stats->max_neighbours = hs[S_MAX_NEIGHBOURS];
  }
  if (out_cloud) return adopt_device(c->ctx, d_out, m, out_cloud);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_mls_last_timing(sfmhip_cloud* c, double ms3[3]) {
  if (!c || !ms3) return SFMHIP_ERR_ARG;
  const MlsState* s = stage<MlsState>(c);
  for (int i = 0; i < 3; ++i) ms3[i] = s->ms[i];
  return SFMHIP_OK;
}
