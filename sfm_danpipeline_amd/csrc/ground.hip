// ground.hip -- the dominant ground plane of the device-resident cloud of cloud.hip on gfx950: RANSAC, refit, orientation,
// and the frame (up, north, ground) that dendro.hip measures in.  The rules are DESIGN.md f-12's; the arithmetic is
// ground.h's, which the CPU test stub compiles too, and every output is the same bits as that build's.
//
//   gnd_flag     1 where a point is selected (finite, its label); the handle's scan; gnd_emit the list in input order;
//   cloud_minmax the selection's float bounding box (cloud_grid.h: integer atomics on ordered keys) for the tolerance;
//   gnd_hyp      a thread per iteration: the three draws, (a, n), the tilt test; zeroes the iteration's counts;
//   gnd_score    a workgroup per (16 hypotheses, block of points): the block's points go through LDS in chunks, each wave
//                scores its own 4 hypotheses -- read through the constant address space, so they sit in SGPRs -- with
//                the lanes strided over the chunk, counts by ballot + popcount and adds three u32 counts per hypothesis
//                with integer atomics;
//   gnd_pick     one workgroup: orientation and admissibility of every hypothesis, the maximum of rule 6's key;
//   gnd_refit    one workgroup per round: centroid, covariance and the 3 x 3 Jacobi SVD, each sum in rule 7's fixed order;
//                once more with `last` for the final plane's counts and residual.
// The host waits twice: for the list's length and box, and for the final plane.  No float atomic feeds an output;
// launches are ordered by the stream alone.
#include "common.h"
#include "cloud_grid.h"
#include "ground.h"
#include <algorithm>
#include <cmath>

using namespace sfmground;
using sfmgrid::blocks;
using sfmgrid::mirror;  // (the options in, the defaults and the result out: size-checked)
using sfmsum::block_count;  // (block_sum.h: rule 7's fixed-order sums over the 256 threads of a workgroup)
using sfmsum::block_tree;

namespace {

constexpr int SW = 4;              // waves of a gnd_score workgroup
constexpr int HPW = 4;             // hypotheses a wave scores at once
constexpr int HPB = SW * HPW;      // hypotheses of a workgroup
constexpr int STAGE = 1024;        // points of one LDS chunk
constexpr int PPB = 8 * STAGE;     // points of a workgroup's block

struct Last {  // the final plane's counts and the fixed-order sum of s^2 over its inliers
  uint32_t inl, pos, neg, pad;
  double s2;
};

struct GndState {  // on the cloud handle, freed with it; the cloud's size never changes, so the blocks are made once
  static constexpr sfmgrid::Stage slot = sfmgrid::GROUND;  // (its slot on the handle: stage<GndState>(cloud))
  DevBufs B;
  bool ready = false;
  int* labels = nullptr;     // n
  P3* pts = nullptr;         // n: the selection list
  Hyp* hyp = nullptr;        // MAX_ITERS
  Counts* cnt = nullptr;     // MAX_ITERS
  Plane* plane = nullptr;    // 1
  Last* last = nullptr;      // 1
  sfmgrid::Grow<double> cams;  // 3 per camera centre
  double ms[4] = {0, 0, 0, 0};
};

int gnd_alloc(sfmhip_cloud* c, GndState* s, int n_cam) {
  if (!s->ready) {
    const size_t n = (size_t)std::max(c->n, 1);
    SFM_TRY(s->B.alloc(&s->labels, n));
    SFM_TRY(s->B.alloc(&s->pts, n));
    SFM_TRY(s->B.alloc(&s->hyp, (size_t)MAX_ITERS));
    SFM_TRY(s->B.alloc(&s->cnt, (size_t)MAX_ITERS));
    SFM_TRY(s->B.alloc(&s->plane, 1));
    SFM_TRY(s->B.alloc(&s->last, 1));
    s->ready = true;
  }
  if (n_cam) SFM_TRY(s->cams.need(3 * (size_t)n_cam));
  return SFMHIP_OK;
}

struct Selected {  // rule 1's predicate, for gnd_flag and cloud_minmax
  const int* labels;
  int label;
  __device__ bool operator()(long long i, const float* v) const {
    return sfmcloud::finite3(v[0], v[1], v[2]) && (!labels || labels[i] == label);
  }
};

__global__ __launch_bounds__(256) void gnd_flag(const float* xyz, int n, Selected ok, int* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float v[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  flag[i] = ok(i, v) ? 1 : 0;
}

__global__ __launch_bounds__(256) void gnd_emit(const float* xyz, int n, const int* flag, const int* at, P3* pts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i]) return;
  P3 p;
  p.x = xyz[3 * (size_t)i];
  p.y = xyz[3 * (size_t)i + 1];
  p.z = xyz[3 * (size_t)i + 2];
  pts[at[i]] = p;  // (at[i] < n: an exclusive scan of n flags)
}

struct HypArgs {
  double hint[3], cos_tilt;
  int has_hint, iters;
  uint32_t seed;
};

// hypotheses 0 .. gridDim.x * 64 - 1 (a multiple of HPB, at most MAX_ITERS): those at or past `iters` are written as skipped
__global__ __launch_bounds__(64) void gnd_hyp(const P3* __restrict__ pts, int n_sel, HypArgs a, Hyp* hyp, Counts* cnt) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  Hyp h;
  if (j < a.iters) {
    h = hypothesis(pts, n_sel, a.seed, j, a.hint, a.cos_tilt, a.has_hint);
  } else {
    for (int k = 0; k < 3; ++k) h.a[k] = h.n[k] = 0.0;
    h.ok = h.pad = 0;
  }
  hyp[j] = h;
  Counts z;
  z.inl = z.pos = z.neg = 0u;
  cnt[j] = z;
}

typedef const Hyp __attribute__((address_space(4))) ConstHyp;  // the constant address space: uniform reads become scalar loads

__global__ __launch_bounds__(64 * SW) void gnd_score(const P3* __restrict__ pts, int n_sel, const Hyp* __restrict__ hyp, double tol, Counts* cnt) {
  __shared__ P3 tile[STAGE];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int j0 = blockIdx.x * HPB + wave * HPW;
  ConstHyp* ch = (ConstHyp*)(hyp + j0);
  double a[HPW][3], n[HPW][3];
  int ok[HPW];
  uint32_t inl[HPW], pos[HPW], neg[HPW];
#pragma unroll
  for (int h = 0; h < HPW; ++h) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      a[h][k] = ch[h].a[k];
      n[h][k] = ch[h].n[k];
    }
    ok[h] = ch[h].ok;
    inl[h] = pos[h] = neg[h] = 0u;
  }
  const int p0 = blockIdx.y * PPB, p1 = min(n_sel, p0 + PPB);
  for (int base = p0; base < p1; base += STAGE) {
    const int m = min(STAGE, p1 - base);
    __syncthreads();
    for (int i = threadIdx.x; i < m; i += 64 * SW) tile[i] = pts[base + i];
    __syncthreads();
    for (int i0 = 0; i0 < m; i0 += 64) {
      const bool live = i0 + lane < m;
      const P3 p = tile[live ? i0 + lane : 0];
      const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
#pragma unroll
      for (int h = 0; h < HPW; ++h) {
        if (!ok[h]) continue;  // (uniform over the wave)
        const double s = signed_dist(a[h], n[h], x, y, z);
        inl[h] += (uint32_t)__popcll(__ballot(live && fabs(s) <= tol));
        pos[h] += (uint32_t)__popcll(__ballot(live && s > tol));
        neg[h] += (uint32_t)__popcll(__ballot(live && s < -tol));
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int h = 0; h < HPW; ++h) {
      if (!ok[h]) continue;
      if (inl[h]) atomicAdd(&cnt[j0 + h].inl, inl[h]);
      if (pos[h]) atomicAdd(&cnt[j0 + h].pos, pos[h]);
      if (neg[h]) atomicAdd(&cnt[j0 + h].neg, neg[h]);
    }
  }
}

__global__ __launch_bounds__(CHUNK) void gnd_pick(const Hyp* __restrict__ hyp, const Counts* __restrict__ cnt, int iters,
                                                  const double* __restrict__ cams, int n_cam, int min_inliers, long long cap, Plane* plane) {
  __shared__ unsigned long long sh[4];
  unsigned long long best = 0ull;
  int best_sign = 1;
  for (int j = threadIdx.x; j < iters; j += CHUNK) {
    int sign;
    const unsigned long long key = hyp_key(hyp[j], cnt[j], j, cams, n_cam, min_inliers, cap, sign);
    if (key > best) {
      best = key;
      best_sign = sign;
    }
  }
  unsigned long long top = best;
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(top, off);
    top = o > top ? o : top;
  }
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = top;
  __syncthreads();
  top = sh[0];
  for (int w = 1; w < 4; ++w) top = sh[w] > top ? sh[w] : top;
  if (top == 0ull) {
    if (threadIdx.x == 0) {
      Plane p;
      for (int k = 0; k < 3; ++k) p.a[k] = p.n[k] = 0.0;
      p.winner = -1;
      p.flags = F_NO_PLANE;
      *plane = p;
    }
    return;
  }
  if (best == top) {  // (one thread: the key holds j)
    const int j = key_iter(top);
    Plane p;
    plane_from(hyp[j], best_sign, j, p);
    *plane = p;
  }
}

// f(i, point) for the points i = threadIdx.x, threadIdx.x + 256, ... of the list in ascending i: rule 7's order.  The loads
// of RB points are issued together and consumed in order, so a thread waits for memory once per RB points, not once per point.
constexpr int RB = 8;
template <typename F>
__device__ __forceinline__ void for_own_points(const P3* __restrict__ pts, int n_sel, F f) {
  for (long long i0 = threadIdx.x; i0 < n_sel; i0 += CHUNK * RB) {
    P3 q[RB];
#pragma unroll
    for (int u = 0; u < RB; ++u) {
      const long long i = i0 + u * CHUNK;
      q[u] = pts[i < n_sel ? i : i0];
    }
#pragma unroll
    for (int u = 0; u < RB; ++u)
      if (i0 + u * CHUNK < n_sel) f(q[u]);
  }
}

// one round of rule 7 on *plane, or with `last` the counts and residual of the plane as it stands
__global__ __launch_bounds__(CHUNK) void gnd_refit(const P3* __restrict__ pts, int n_sel, double tol, Plane* plane, int is_last, Last* last) {
  __shared__ double sh[6][4];
  __shared__ uint32_t shc[4];
  __shared__ double work[21];
  Plane p = *plane;
  if (p.winner < 0) return;  // (uniform over the workgroup)
  uint32_t inl = 0, pos = 0, neg = 0;
  double s3[3] = {0.0, 0.0, 0.0};
  for_own_points(pts, n_sel, [&](const P3& q) {
    const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
    const double s = signed_dist(p.a, p.n, x, y, z);
    pos += s > tol ? 1u : 0u;
    neg += s < -tol ? 1u : 0u;
    if (!(fabs(s) <= tol)) return;
    ++inl;
    if (is_last) {
      s3[0] = s3[0] + s * s;
    } else {
      s3[0] = s3[0] + x;
      s3[1] = s3[1] + y;
      s3[2] = s3[2] + z;
    }
  });
  inl = block_count(inl, shc);
  if (is_last) {
    pos = block_count(pos, shc);
    neg = block_count(neg, shc);
    block_tree<1>(s3, sh);
    if (threadIdx.x == 0) {
      Last r;
      r.inl = inl, r.pos = pos, r.neg = neg, r.pad = 0u;
      r.s2 = s3[0];
      *last = r;
    }
    return;
  }
  if (inl < 3u) {
    if (threadIdx.x == 0) plane->flags = p.flags | F_REFIT_KEPT;
    return;
  }
  block_tree<3>(s3, sh);
  const double N = (double)inl;
  const double cen[3] = {s3[0] / N, s3[1] / N, s3[2] / N};
  double cs[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[6];
  for_own_points(pts, n_sel, [&](const P3& q) {
    const double x = (double)q.x, y = (double)q.y, z = (double)q.z;
    const double s = signed_dist(p.a, p.n, x, y, z);
    if (!(fabs(s) <= tol)) return;
    cov_terms(x - cen[0], y - cen[1], z - cen[2], t);
#pragma unroll
    for (int k = 0; k < 6; ++k) cs[k] = cs[k] + t[k];
  });
  block_tree<6>(cs, sh);
  if (threadIdx.x == 0) {
    if (!refit_plane(cen, cs, N, work, p)) p.flags |= F_REFIT_KEPT;
    *plane = p;
  }
}

int run(sfmhip_cloud* c, const int32_t* labels, int32_t label, const Opts& o, const double* cams, int n_cam, Result& res) {
  Prep pr;
  if (!prepare(o, pr) || n_cam < 0 || (n_cam > 0 && !cams)) return SFMHIP_ERR_ARG;
  GndState* s = sfmgrid::stage<GndState>(c);
  for (double& m : s->ms) m = 0;
  empty_result(res, 0, dnan(), F_FEW);
  if (c->n <= 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  const bool timing = c->ctx->timing;
  const int n = c->n;
  SFM_TRY(sfmgrid::ensure_ibuf(c));
  SFM_TRY(gnd_alloc(c, s, n_cam));
  const double t0 = sfm_now_ms();
  // rules 1, 2: the list, its length and its box
  if (labels) SFM_HIP_TRY(hipMemcpyAsync(s->labels, labels, sizeof(int) * (size_t)n, hipMemcpyHostToDevice, st));
  if (n_cam) SFM_HIP_TRY(hipMemcpyAsync(s->cams.p, cams, sizeof(double) * 3 * (size_t)n_cam, hipMemcpyHostToDevice, st));
  Selected sel;
  sel.labels = labels ? s->labels : nullptr;
  sel.label = label;
  int *flag = c->ibuf[2], *at = c->ibuf[3];
  hipLaunchKernelGGL(gnd_flag, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, n, sel, flag);
  SFM_HIP_TRY(hipGetLastError());
  unsigned mm[7];
  SFM_TRY(sfmgrid::minmax(c, c->xyz, n, sel, mm));
  int n_sel = 0;
  SFM_TRY(sfmgrid::scan(c, flag, at, (size_t)n, &n_sel));  // (waits for the stream: mm has arrived too)
  const double t1 = sfm_now_ms();
  s->ms[0] = s->ms[3] = t1 - t0;
  if (n_sel < 3) {
    empty_result(res, n_sel, dnan(), F_FEW);
    return SFMHIP_OK;
  }
  hipLaunchKernelGGL(gnd_emit, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, n, flag, at, s->pts);
  SFM_HIP_TRY(hipGetLastError());
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) lo[a] = sfmcloud::ord_val(mm[a]), hi[a] = sfmcloud::ord_val(mm[3 + a]);
  const double tol = tolerance(o, lo, hi);
  // rules 3, 4
  HypArgs ha;
  for (int a = 0; a < 3; ++a) ha.hint[a] = pr.hint[a];
  ha.cos_tilt = pr.cos_tilt, ha.has_hint = pr.has_hint, ha.iters = o.ransac_iters, ha.seed = o.seed;
  const unsigned groups = blocks(o.ransac_iters, HPB);  // <= MAX_ITERS / HPB
  hipLaunchKernelGGL(gnd_hyp, dim3(blocks((long long)groups * HPB, 64)), dim3(64), 0, st, s->pts, n_sel, ha, s->hyp, s->cnt);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t2 = sfm_now_ms();
  hipLaunchKernelGGL(gnd_score, dim3(groups, blocks(n_sel, PPB)), dim3(64 * SW), 0, st, s->pts, n_sel, s->hyp, tol, s->cnt);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t3 = sfm_now_ms();
  // rules 5 - 7
  hipLaunchKernelGGL(gnd_pick, dim3(1), dim3(CHUNK), 0, st, s->hyp, s->cnt, o.ransac_iters, s->cams.p, n_cam, o.min_inliers,
                     below_cap(o.below_max, n_sel), s->plane);
  SFM_HIP_TRY(hipGetLastError());
  for (int r = 0; r <= o.refit_rounds; ++r) {
    hipLaunchKernelGGL(gnd_refit, dim3(1), dim3(CHUNK), 0, st, s->pts, n_sel, tol, s->plane, r == o.refit_rounds ? 1 : 0, s->last);
    SFM_HIP_TRY(hipGetLastError());
  }
  Plane p;
  Last l;
  SFM_HIP_TRY(hipMemcpyAsync(&p, s->plane, sizeof p, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(&l, s->last, sizeof l, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  // rule 8
  if (p.winner < 0)
    empty_result(res, n_sel, tol, F_NO_PLANE);
  else
    finish(o, p, n_sel, tol, l.inl, l.pos, l.neg, l.inl ? std::sqrt(l.s2 / (double)l.inl) : dnan(), res);
  const double t4 = sfm_now_ms();
  s->ms[0] = t2 - t0;
  s->ms[1] = t3 - t2;
  s->ms[2] = t4 - t3;
  s->ms[3] = t4 - t0;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_ground_default_opts(sfmhip_ground_opts* o) {
  if (!o) return;
  *o = mirror<sfmhip_ground_opts>(default_opts());
}

extern "C" int sfmhip_cloud_ground_plane(sfmhip_cloud* c, const int32_t* labels, int32_t label, const sfmhip_ground_opts* opts,
                                         const double* cam_centres, int n_cam, sfmhip_ground_result* out) {
  if (!c || !opts || !out) return SFMHIP_ERR_ARG;
  Result res;
  SFM_TRY(run(c, labels, label, mirror<Opts>(*opts), cam_centres, n_cam, res));
  *out = mirror<sfmhip_ground_result>(res);
  return SFMHIP_OK;
}

extern "C" int sfmhip_dendro_opts_from_ground(const sfmhip_ground_result* g, sfmhip_dendro_opts* io) {
  if (!g || !io) return SFMHIP_ERR_ARG;
  sfmdendro::Opts d = mirror<sfmdendro::Opts>(*io);
  if (!opts_from_ground(mirror<Result>(*g), d)) return SFMHIP_ERR_ARG;
  *io = mirror<sfmhip_dendro_opts>(d);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_ground_last_timing(sfmhip_cloud* c, double ms4[4]) {
  if (!c || !ms4) return SFMHIP_ERR_ARG;
  const GndState* s = sfmgrid::stage<GndState>(c);
  for (int i = 0; i < 4; ++i) ms4[i] = s->ms[i];
  return SFMHIP_OK;
}
