// pnp.hip -- findCameraPosePNP's cv::solvePnPRansac(..., CV_EPNP) (reference src/Sfm.cpp:1137-1210) on gfx950, batched over
// views and over RANSAC iterations the way score.hip batches findEssentialMat: the host draws the sample tables, the
// device solves every (view, iteration) sample of a chunk and counts its model's inliers, and the host replays
// ptsetreg.cpp's update rule over the counts (ransac_host.h: ransac_replay, shared with score.hip and the CPU test stubs; pnp.h states how PnP calls it).
//
// Kernels.  pnp_solve: one thread per (view, iteration): five float correspondences -> undistortPoints -> EPnP -> Rodrigues;
// the 714 doubles a solve works on (the 12 x 12 system, its V^T, the 6 x 10 matrix, the small solves) live in a global
// work buffer interleaved over the 64 lanes of a wave, so a wave's accesses coalesce and nothing of it is a private array.
// pnp_count: one workgroup per (view, iteration): the points are read once as float, the count is integer (wave sums, one
// LDS atomicAdd per wave).  pnp_keep_best: the model that raised a view's best count stays on the device.  pnp_mask: one
// workgroup per view: the best model's mask and, by ballot / popcount prefix sums, the ordered list of its inliers.
// pnp_prepare: the float points back to f64 and undistortPoints in f64 (the refit's inputs).  pnp_epnp_group: EPnP on a
// point set of any size by one workgroup: every sum over the points is pnp.h's fixed-order tree (wave shuffles, then the
// four wave sums from LDS; no floating-point atomics), the serial stages run on thread 0 with the work area in LDS.
// The arithmetic is pnp.h's, which the CPU test stub compiles too.
#include "common.h"
#include "pnp.h"
#include <algorithm>
#include <vector>

namespace {

using namespace sfmpnp;

struct PnpParams {
  double K[9], dist[5];
};

// thread (job, iteration of the chunk): the sample's model (rvec, tvec) and ok = models | flags << 8
__global__ __launch_bounds__(64) void pnp_solve(const Job* __restrict__ jobs, int n_jobs, int chunk, const int* __restrict__ samples,
                                                const float* __restrict__ xyz, const float* __restrict__ xy, PnpParams p,
                                                double* __restrict__ work, double* __restrict__ models, int* __restrict__ ok) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_jobs * chunk) return;
  const int j = t / chunk, it = t - j * chunk;
  const Job jb = jobs[j];
  const int* s = samples + ((size_t)jb.samp + it) * 5;
  float P3[5][3], P2[5][2];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const size_t m = (size_t)jb.off + s[k];
    P3[k][0] = xyz[3 * m];
    P3[k][1] = xyz[3 * m + 1];
    P3[k][2] = xyz[3 * m + 2];
    P2[k][0] = xy[2 * m];
    P2[k][1] = xy[2 * m + 1];
  }
  double model[6];
  const Mem<64> w{work + (size_t)(t >> 6) * (64 * (size_t)WORK_DOUBLES) + (t & 63)};
  ok[t] = solve_sample<64>(P3, P2, p.K, p.dist, w, model);
#pragma unroll
  for (int k = 0; k < 6; ++k) models[(size_t)t * 6 + k] = model[k];
}

// workgroup (job, iteration): the inlier count of the sample's model
__global__ __launch_bounds__(256) void pnp_count(const Job* __restrict__ jobs, int chunk, const float* __restrict__ xyz,
                                                 const float* __restrict__ xy, PnpParams p, const float* __restrict__ thr2,
                                                 const double* __restrict__ models, const int* __restrict__ ok,
                                                 int* __restrict__ counts) {
  __shared__ double sP[12];
  __shared__ int s_cnt;
  const int slot = blockIdx.x;
  const Job jb = jobs[slot / chunk];
  const bool has = (ok[slot] & 0xff) != 0;  // (uniform over the workgroup)
  if (threadIdx.x == 0) {
    s_cnt = 0;
    double P[12];
    pose_matrix(models + (size_t)slot * 6, models + (size_t)slot * 6 + 3, P);
    for (int k = 0; k < 12; ++k) sP[k] = P[k];
  }
  __syncthreads();
  if (has) {
    double P[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = sP[k];
    const float t = thr2[jb.view];
    int c = 0;
    for (int i = threadIdx.x; i < jb.count; i += 256) {
      const size_t m = (size_t)jb.off + i;
      c += reproj_err2(P, p.K, p.dist, xyz[3 * m], xyz[3 * m + 1], xyz[3 * m + 2], xy[2 * m], xy[2 * m + 1]) <= t ? 1 : 0;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&s_cnt, c);
  }
  __syncthreads();
  if (threadIdx.x == 0) counts[slot] = s_cnt;
}

struct KeepBatch {
  enum { N = 64 };
  int n;
  Keep k[N];
};
__global__ void pnp_keep_best(KeepBatch keeps, const double* __restrict__ models, double* __restrict__ best) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * keeps.n) return;
  const Keep k = keeps.k[i / 6];
  best[(size_t)k.view * 6 + i % 6] = models[(size_t)k.slot * 6 + i % 6];
}

// workgroup per view: the best model's mask, the ordered list of its inliers and their number.  has: 0 no model (mask 0),
// 1 a RANSAC model, 2 exactly five correspondences (every one an inlier)
__global__ __launch_bounds__(256) void pnp_mask(const int* __restrict__ offsets, const float* __restrict__ xyz,
                                                const float* __restrict__ xy, PnpParams p, const float* __restrict__ thr2,
                                                const double* __restrict__ best, const unsigned char* __restrict__ has,
                                                unsigned char* __restrict__ mask, int* __restrict__ inl, int* __restrict__ n_inl) {
  __shared__ double sP[12];
  __shared__ int s_w[4], s_base;
  const int v = blockIdx.x;
  const int o = offsets[v], n = offsets[v + 1] - o;
  const int h = has[v];
  if (threadIdx.x == 0) {
    s_base = 0;
    double P[12];
    pose_matrix(best + (size_t)v * 6, best + (size_t)v * 6 + 3, P);
    for (int k = 0; k < 12; ++k) sP[k] = P[k];
  }
  __syncthreads();
  double P[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) P[k] = sP[k];
  const float t = thr2[v];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int base = 0; base < n; base += 256) {  // (uniform trip count)
    const int i = base + (int)threadIdx.x;
    bool in = false;
    if (i < n) {
      const size_t m = (size_t)o + i;
      in = h == 2 || (h == 1 && reproj_err2(P, p.K, p.dist, xyz[3 * m], xyz[3 * m + 1], xyz[3 * m + 2], xy[2 * m], xy[2 * m + 1]) <= t);
      mask[m] = in ? 1 : 0;
    }
    const unsigned long long b = __ballot(in);
    const int rank = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) s_w[wv] = __popcll(b);
    __syncthreads();
    int pre = s_base;
    for (int k = 0; k < wv; ++k) pre += s_w[k];
    if (in) inl[(size_t)o + pre + rank] = i;
    __syncthreads();
    if (threadIdx.x == 0) s_base += s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) n_inl[v] = s_base;
}

// the refit's inputs: the float points as f64, cv::undistortPoints of the float pixels in f64
__global__ void pnp_prepare(const float* __restrict__ xyz, const float* __restrict__ xy, long long n, PnpParams p,
                            double* __restrict__ pw, double* __restrict__ uv) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  pw[3 * i] = (double)xyz[3 * i];
  pw[3 * i + 1] = (double)xyz[3 * i + 1];
  pw[3 * i + 2] = (double)xyz[3 * i + 2];
  double x, y;
  sfmcam::undistort_point(p.K, p.dist, (double)xy[2 * i], (double)xy[2 * i + 1], x, y);
  uv[2 * i] = x;
  uv[2 * i + 1] = y;
}

struct GroupPoints {
  int n;
  const double* pw;
  const double* uv;
  const int* idx;  // nullable
  __device__ void get(int i, double* p, double* q) const {
    const size_t k = idx ? (size_t)idx[i] : (size_t)i;
    p[0] = pw[3 * k];
    p[1] = pw[3 * k + 1];
    p[2] = pw[3 * k + 2];
    q[0] = uv[2 * k];
    q[1] = uv[2 * k + 1];
  }
};

// the fixed-order sum of pnp.h by a workgroup of 256: lane = slot, wave = group
template <int K, class F>
__device__ __forceinline__ void group_sum(int n, F f, double* part, Mem<1> w) {
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += SLOTS) {
    double t[K];
    f(i, t);
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] += t[k];
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    acc[k] = v;
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) part[(threadIdx.x >> 6) * K + k] = acc[k];
  }
  __syncthreads();
  if ((int)threadIdx.x < K) w[W_ACC + threadIdx.x] = (part[threadIdx.x] + part[K + threadIdx.x]) + (part[2 * K + threadIdx.x] + part[3 * K + threadIdx.x]);
  __syncthreads();
}

// workgroup per problem: EPnP on points [off[g], off[g] + cnt) of pw / uv (cnt = n_sel[g] points through the index list
// when idx is given, else the whole range); run[g] == 0 (nullable) skips the problem (outputs zero)
__global__ __launch_bounds__(256) void pnp_epnp_group(const int* __restrict__ offsets, const int* __restrict__ n_sel,
                                                      const int* __restrict__ idx, const double* __restrict__ pw,
                                                      const double* __restrict__ uv, const unsigned char* __restrict__ run,
                                                      double* __restrict__ R_out, double* __restrict__ t_out,
                                                      double* __restrict__ rvec_out, int* __restrict__ flags) {
  __shared__ double sw[WORK_DOUBLES];
  __shared__ double part[4 * 78];
  __shared__ int s_fl;
  const int g = blockIdx.x;
  const int o = offsets[g];
  const int n = n_sel ? n_sel[g] : offsets[g + 1] - o;
  const bool live = (!run || run[g] == 1) && n >= MODEL_POINTS;  // (uniform)
  if (!live) {
    if (threadIdx.x < 9 && R_out) R_out[(size_t)g * 9 + threadIdx.x] = 0;
    if (threadIdx.x < 3) {
      t_out[(size_t)g * 3 + threadIdx.x] = 0;
      if (rvec_out) rvec_out[(size_t)g * 3 + threadIdx.x] = 0;
    }
    return;
  }
  const Mem<1> w{sw};
  GroupPoints pts{n, pw + 3 * (size_t)o, uv + 2 * (size_t)o, idx ? idx + o : nullptr};
  const bool lead = threadIdx.x == 0;
  group_sum<3>(n, [&](int i, double* out) {
    double p[3], q[2];
    pts.get(i, p, q);
    out[0] = p[0];
    out[1] = p[1];
    out[2] = p[2];
  }, part, w);
  double c0[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) c0[j] = w[W_ACC + j] / (double)n;
  __syncthreads();
  group_sum<6>(n, [&](int i, double* out) {
    double p[3], q[2];
    pts.get(i, p, q);
    const double d0 = p[0] - c0[0], d1 = p[1] - c0[1], d2 = p[2] - c0[2];
    out[0] = d0 * d0;
    out[1] = d0 * d1;
    out[2] = d0 * d2;
    out[3] = d1 * d1;
    out[4] = d1 * d2;
    out[5] = d2 * d2;
  }, part, w);
  if (lead) {
    double cov[6];
    for (int j = 0; j < 6; ++j) cov[j] = w[W_ACC + j];
    s_fl = stage_control<1>(n, c0, cov, w);
  }
  __syncthreads();
  if (s_fl & FLAG_RANK_DEFICIENT) {  // (uniform) not solved: zero outputs, the flag
    if (threadIdx.x < 9 && R_out) R_out[(size_t)g * 9 + threadIdx.x] = 0;
    if (threadIdx.x < 3) {
      t_out[(size_t)g * 3 + threadIdx.x] = 0;
      if (rvec_out) rvec_out[(size_t)g * 3 + threadIdx.x] = 0;
    }
    if (lead) atomicOr(flags, s_fl);
    return;
  }
  double cws[12], ci[9];
#pragma unroll
  for (int k = 0; k < 12; ++k) cws[k] = w[W_CWS + k];
#pragma unroll
  for (int k = 0; k < 9; ++k) ci[k] = w[W_CI + k];
  group_sum<78>(n, [&](int i, double* out) {
    double p[3], q[2], a[4];
    pts.get(i, p, q);
    alphas_of(cws, ci, p, a);
    mtm_terms(a, q[0], q[1], out);
  }, part, w);
  if (lead) {
    int k = 0;
    for (int r = 0; r < 12; ++r)
      for (int c = r; c < 12; ++c, ++k) {
        const double v = w[W_ACC + k];
        w[W_AT + 12 * r + c] = v;
        w[W_AT + 12 * c + r] = v;
      }
    s_fl |= stage_betas<1>(w);
  }
  __syncthreads();
  double p_first[3], q_first[2];
  pts.get(0, p_first, q_first);
  for (int N = 0; N < 3; ++N) {
    if (lead) stage_ccs<1>(w, N, p_first);
    __syncthreads();
    double ccs[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) ccs[k] = w[W_CCS + k];
    group_sum<6>(n, [&](int i, double* out) {
      double p[3], q[2], a[4], pc[3];
      pts.get(i, p, q);
      alphas_of(cws, ci, p, a);
      pc_of(a, ccs, pc);
      out[0] = pc[0];
      out[1] = pc[1];
      out[2] = pc[2];
      out[3] = p[0];
      out[4] = p[1];
      out[5] = p[2];
    }, part, w);
    double pc0[3], pw0[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      pc0[j] = w[W_ACC + j] / (double)n;
      pw0[j] = w[W_ACC + 3 + j] / (double)n;
    }
    __syncthreads();
    if (lead)
      for (int j = 0; j < 3; ++j) {
        w[W_PCW + j] = pc0[j];
        w[W_PCW + 3 + j] = pw0[j];
      }
    group_sum<9>(n, [&](int i, double* out) {
      double p[3], q[2], a[4], pc[3];
      pts.get(i, p, q);
      alphas_of(cws, ci, p, a);
      pc_of(a, ccs, pc);
#pragma unroll
      for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int k = 0; k < 3; ++k) out[3 * j + k] = (pc[j] - pc0[j]) * (p[k] - pw0[k]);
    }, part, w);
    if (lead) {
      double abt[9];
      for (int k = 0; k < 9; ++k) abt[k] = w[W_ACC + k];
      s_fl |= stage_rt<1>(w, N, abt);
    }
    __syncthreads();
    double Rn[9], tn[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) Rn[k] = w[W_RT + 12 * N + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) tn[k] = w[W_RT + 12 * N + 9 + k];
    group_sum<1>(n, [&](int i, double* out) {
      double p[3], q[2];
      pts.get(i, p, q);
      out[0] = reproj_term(Rn, tn, p, q[0], q[1]);
    }, part, w);
    if (lead) w[W_ERR + N] = w[W_ACC] / (double)n;
    __syncthreads();
  }
  if (lead) {
    const int N = stage_choose<1>(w);
    double R[9], rv[3];
    for (int k = 0; k < 9; ++k) R[k] = w[W_RT + 12 * N + k];
    if (R_out)
      for (int k = 0; k < 9; ++k) R_out[(size_t)g * 9 + k] = R[k];
    for (int k = 0; k < 3; ++k) t_out[(size_t)g * 3 + k] = w[W_RT + 12 * N + 9 + k];
    if (rvec_out) {
      s_fl |= rodrigues_to_vector(R, rv);
      for (int k = 0; k < 3; ++k) rvec_out[(size_t)g * 3 + k] = rv[k];
    }
    if (s_fl) atomicOr(flags, s_fl);
  }
}

// the device side of ransac_replay
struct DeviceBackend {
  hipStream_t st;
  DevBufs& bufs;
  PnpParams p;
  const float *d_xyz, *d_xy, *d_thr2;
  double* d_best;
  Job* d_jobs = nullptr;
  int *d_samples = nullptr, *d_ok = nullptr, *d_counts = nullptr;
  double *d_models = nullptr, *d_work = nullptr;
  size_t cap_jobs = 0, cap_slots = 0, cap_samples = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // timing (nullable): around the solver and the scoring kernel
  float ms_solve = 0, ms_count = 0;

  int run_chunk(const std::vector<Job>& jobs, int chunk, const std::vector<int>& samples, std::vector<int>& ok, std::vector<int>& counts) {
    const size_t nj = jobs.size(), slots = nj * (size_t)chunk;
    if (nj > cap_jobs) {
      SFM_TRY(bufs.alloc(&d_jobs, nj));
      cap_jobs = nj;
    }
    if (slots > cap_slots) {
      SFM_TRY(bufs.alloc(&d_ok, slots));
      SFM_TRY(bufs.alloc(&d_counts, slots));
      SFM_TRY(bufs.alloc(&d_models, slots * 6));
      SFM_TRY(bufs.alloc(&d_work, (slots + 63) / 64 * 64 * (size_t)WORK_DOUBLES));
      cap_slots = slots;
    }
    if (samples.size() > cap_samples) {
      SFM_TRY(bufs.alloc(&d_samples, samples.size()));
      cap_samples = samples.size();
    }
    SFM_HIP_TRY(hipMemcpyAsync(d_jobs, jobs.data(), sizeof(Job) * nj, hipMemcpyHostToDevice, st));
    SFM_HIP_TRY(hipMemcpyAsync(d_samples, samples.data(), sizeof(int) * samples.size(), hipMemcpyHostToDevice, st));
    if (ev[0]) SFM_HIP_TRY(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(pnp_solve, dim3((unsigned)((slots + 63) / 64)), dim3(64), 0, st, (const Job*)d_jobs, (int)nj, chunk,
                       (const int*)d_samples, d_xyz, d_xy, p, d_work, d_models, d_ok);
    if (ev[0]) SFM_HIP_TRY(hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(pnp_count, dim3((unsigned)slots), dim3(256), 0, st, (const Job*)d_jobs, chunk, d_xyz, d_xy, p, d_thr2,
                       (const double*)d_models, (const int*)d_ok, d_counts);
    if (ev[0]) SFM_HIP_TRY(hipEventRecord(ev[2], st));
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(ok.data(), d_ok, sizeof(int) * slots, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * slots, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    if (ev[0]) {
      float a = 0, b = 0;
      SFM_HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
      SFM_HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
      ms_solve += a;
      ms_count += b;
    }
    return SFMHIP_OK;
  }
  int keep_best(const std::vector<Keep>& keeps) {  // (before the next chunk's solve overwrites the models; same stream)
    // (the list is passed by value in the launch's argument buffer in batches of 64: no copy whose source must outlive it,
    // no synchronisation; the next chunk's download synchronises the stream anyway)
    for (size_t first = 0; first < keeps.size(); first += KeepBatch::N) {
      KeepBatch kb;
      kb.n = (int)std::min<size_t>(KeepBatch::N, keeps.size() - first);
      for (int i = 0; i < kb.n; ++i) kb.k[i] = keeps[first + i];
      hipLaunchKernelGGL(pnp_keep_best, dim3((unsigned)((6 * kb.n + 255) / 256)), dim3(256), 0, st, kb, (const double*)d_models, d_best);
    }
    SFM_HIP_TRY(hipGetLastError());
    return SFMHIP_OK;
  }
};

bool offsets_ok(int n, const int32_t* offsets) {
  if (offsets[0] != 0) return false;
  for (int p = 0; p < n; ++p)
    if (offsets[p + 1] < offsets[p]) return false;
  return true;
}

}  // namespace

extern "C" int sfmhip_pnp_ransac(sfmhip_ctx* ctx, int n_views, const int32_t* offsets, const double* xyz, const double* xy,
                                 const double K[9], const double dist[5], const double* thresholds, double confidence,
                                 int max_iters, int32_t* status, double* rvec, double* tvec, double* rvec_ransac,
                                 double* tvec_ransac, double* rvec_refit, double* tvec_refit, int32_t* inliers, uint8_t* mask,
                                 int32_t* iterations) {
  if (!ctx || n_views < 0 || !offsets || !K || !dist || !thresholds || !status || !rvec || !tvec || !inliers || max_iters < 0)
    return SFMHIP_ERR_ARG;
  if (n_views == 0) return SFMHIP_OK;
  if (!offsets_ok(n_views, offsets)) return SFMHIP_ERR_ARG;
  const size_t total = (size_t)offsets[n_views];
  if (total > 0 && (!xyz || !xy)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ctx->pnp_flags = 0;
  ctx->pnp_ms[0] = ctx->pnp_ms[1] = ctx->pnp_ms[2] = 0;
  // solvePnPRansac converts the points to float before anything else
  std::vector<float> fxyz(3 * total + 1), fxy(2 * total + 1), thr2((size_t)n_views);
  for (size_t i = 0; i < 3 * total; ++i) fxyz[i] = (float)xyz[i];
  for (size_t i = 0; i < 2 * total; ++i) fxy[i] = (float)xy[i];
  for (int v = 0; v < n_views; ++v) thr2[v] = (float)(thresholds[v] * thresholds[v]);
  DevBufs bufs;
  float *d_xyz = nullptr, *d_xy = nullptr, *d_thr2 = nullptr;
  double *d_best = nullptr, *d_pw = nullptr, *d_uv = nullptr, *d_refit_t = nullptr, *d_refit_r = nullptr;
  int *d_off = nullptr, *d_inl = nullptr, *d_ninl = nullptr, *d_flags = nullptr;
  unsigned char *d_has = nullptr, *d_mask = nullptr;
  SFM_TRY(bufs.alloc(&d_xyz, 3 * total + 1));
  SFM_TRY(bufs.alloc(&d_xy, 2 * total + 1));
  SFM_TRY(bufs.alloc(&d_thr2, (size_t)n_views));
  SFM_TRY(bufs.alloc(&d_best, 6 * (size_t)n_views));
  SFM_TRY(bufs.alloc(&d_off, (size_t)n_views + 1));
  SFM_HIP_TRY(hipMemcpyAsync(d_xyz, fxyz.data(), sizeof(float) * (3 * total + 1), hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_xy, fxy.data(), sizeof(float) * (2 * total + 1), hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_thr2, thr2.data(), sizeof(float) * n_views, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_off, offsets, sizeof(int) * ((size_t)n_views + 1), hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(d_best, 0, sizeof(double) * 6 * n_views, st));
  DeviceBackend be{st, bufs};
  for (int k = 0; k < 9; ++k) be.p.K[k] = K[k];
  for (int k = 0; k < 5; ++k) be.p.dist[k] = dist[k];
  be.d_xyz = d_xyz;
  be.d_xy = d_xy;
  be.d_thr2 = d_thr2;
  be.d_best = d_best;
  struct Events {
    hipEvent_t e[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) hipEventDestroy(x);
    }
  } evs;
  if (ctx->timing) {
    for (hipEvent_t& x : evs.e) SFM_HIP_TRY(hipEventCreate(&x));
    for (int k = 0; k < 3; ++k) be.ev[k] = evs.e[k];
  }
  std::vector<ViewState> vs;
  int flags_any = 0;
  SFM_TRY(ransac_replay(be, n_views, offsets, confidence, max_iters, vs, flags_any));
  // the best model's mask and inlier list, then the refit on the inliers
  std::vector<unsigned char> has((size_t)n_views);
  for (int v = 0; v < n_views; ++v) has[v] = sfmransac::has_code(vs[v].status, vs[v].count, MODEL_POINTS);
  SFM_TRY(bufs.alloc(&d_has, (size_t)n_views));
  SFM_TRY(bufs.alloc(&d_mask, total + 1));
  SFM_TRY(bufs.alloc(&d_inl, total + 1));
  SFM_TRY(bufs.alloc(&d_ninl, (size_t)n_views));
  SFM_TRY(bufs.alloc(&d_flags, 1));
  SFM_TRY(bufs.alloc(&d_pw, 3 * total + 1));
  SFM_TRY(bufs.alloc(&d_uv, 2 * total + 1));
  SFM_TRY(bufs.alloc(&d_refit_r, 3 * (size_t)n_views));
  SFM_TRY(bufs.alloc(&d_refit_t, 3 * (size_t)n_views));
  SFM_HIP_TRY(hipMemcpyAsync(d_has, has.data(), n_views, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int), st));
  hipLaunchKernelGGL(pnp_mask, dim3(n_views), dim3(256), 0, st, (const int*)d_off, (const float*)d_xyz, (const float*)d_xy, be.p,
                     (const float*)d_thr2, (const double*)d_best, (const unsigned char*)d_has, d_mask, d_inl, d_ninl);
  if (total > 0)
    hipLaunchKernelGGL(pnp_prepare, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float*)d_xyz, (const float*)d_xy,
                       (long long)total, be.p, d_pw, d_uv);
  if (ctx->timing) SFM_HIP_TRY(hipEventRecord(evs.e[3], st));
  // run[v] == 1 only: a view of exactly five correspondences (has 2) is refitted too -- its five points are its inliers
  std::vector<unsigned char> run((size_t)n_views);
  for (int v = 0; v < n_views; ++v) run[v] = has[v] ? 1 : 0;
  unsigned char* d_run = nullptr;
  SFM_TRY(bufs.alloc(&d_run, (size_t)n_views));
  SFM_HIP_TRY(hipMemcpyAsync(d_run, run.data(), n_views, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pnp_epnp_group, dim3(n_views), dim3(256), 0, st, (const int*)d_off, (const int*)d_ninl, (const int*)d_inl,
                     (const double*)d_pw, (const double*)d_uv, (const unsigned char*)d_run, (double*)nullptr, d_refit_t, d_refit_r,
                     d_flags);
  if (ctx->timing) SFM_HIP_TRY(hipEventRecord(evs.e[4], st));
  SFM_HIP_TRY(hipGetLastError());
  std::vector<double> best(6 * (size_t)n_views), rr(3 * (size_t)n_views), rt(3 * (size_t)n_views);
  int refit_flags = 0;
  SFM_HIP_TRY(hipMemcpyAsync(best.data(), d_best, sizeof(double) * best.size(), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(rr.data(), d_refit_r, sizeof(double) * rr.size(), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(rt.data(), d_refit_t, sizeof(double) * rt.size(), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(&refit_flags, d_flags, sizeof(int), hipMemcpyDeviceToHost, st));
  if (mask && total) SFM_HIP_TRY(hipMemcpyAsync(mask, d_mask, total, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (ctx->timing) {
    float ms = 0;
    SFM_HIP_TRY(hipEventElapsedTime(&ms, evs.e[3], evs.e[4]));
    ctx->pnp_ms[0] = be.ms_solve;
    ctx->pnp_ms[1] = be.ms_count;
    ctx->pnp_ms[2] = ms;
  }
  for (int v = 0; v < n_views; ++v) {
    status[v] = vs[v].status;
    inliers[v] = vs[v].best;
    if (iterations) iterations[v] = vs[v].iter;
    for (int k = 0; k < 3; ++k) {
      // which pose 3.4.1 hands back: the RANSAC model (the refit decides success only)
      rvec[3 * v + k] = best[6 * (size_t)v + k];
      tvec[3 * v + k] = best[6 * (size_t)v + 3 + k];
      if (rvec_ransac) rvec_ransac[3 * v + k] = best[6 * (size_t)v + k];
      if (tvec_ransac) tvec_ransac[3 * v + k] = best[6 * (size_t)v + 3 + k];
      if (rvec_refit) rvec_refit[3 * v + k] = rr[3 * (size_t)v + k];
      if (tvec_refit) tvec_refit[3 * v + k] = rt[3 * (size_t)v + k];
    }
  }
  ctx->pnp_flags = flags_any | refit_flags;
  return SFMHIP_OK;
}

extern "C" int sfmhip_pnp_epnp(sfmhip_ctx* ctx, int n_problems, const int32_t* offsets, const double* xyz,
                               const double* xy_normalised, double* R, double* t) {
  if (!ctx || n_problems < 0 || !offsets || !R || !t) return SFMHIP_ERR_ARG;
  if (n_problems == 0) return SFMHIP_OK;
  if (!offsets_ok(n_problems, offsets) || !xyz || !xy_normalised) return SFMHIP_ERR_ARG;
  for (int p = 0; p < n_problems; ++p)
    if (offsets[p + 1] - offsets[p] < MODEL_POINTS) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ctx->pnp_flags = 0;
  const size_t total = (size_t)offsets[n_problems];
  DevBufs bufs;
  double *d_pw = nullptr, *d_uv = nullptr, *d_R = nullptr, *d_t = nullptr;
  int *d_off = nullptr, *d_flags = nullptr;
  SFM_TRY(bufs.alloc(&d_pw, 3 * total));
  SFM_TRY(bufs.alloc(&d_uv, 2 * total));
  SFM_TRY(bufs.alloc(&d_R, 9 * (size_t)n_problems));
  SFM_TRY(bufs.alloc(&d_t, 3 * (size_t)n_problems));
  SFM_TRY(bufs.alloc(&d_off, (size_t)n_problems + 1));
  SFM_TRY(bufs.alloc(&d_flags, 1));
  SFM_HIP_TRY(hipMemcpyAsync(d_pw, xyz, sizeof(double) * 3 * total, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_uv, xy_normalised, sizeof(double) * 2 * total, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_off, offsets, sizeof(int) * ((size_t)n_problems + 1), hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(d_flags, 0, sizeof(int), st));
  hipLaunchKernelGGL(pnp_epnp_group, dim3(n_problems), dim3(256), 0, st, (const int*)d_off, (const int*)nullptr, (const int*)nullptr,
                     (const double*)d_pw, (const double*)d_uv, (const unsigned char*)nullptr, d_R, d_t, (double*)nullptr, d_flags);
  SFM_HIP_TRY(hipGetLastError());
  int flags = 0;
  SFM_HIP_TRY(hipMemcpyAsync(R, d_R, sizeof(double) * 9 * n_problems, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(t, d_t, sizeof(double) * 3 * n_problems, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(&flags, d_flags, sizeof(int), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  ctx->pnp_flags = flags;
  return SFMHIP_OK;
}

extern "C" int sfmhip_pnp_last_flags(sfmhip_ctx* ctx) { return ctx ? ctx->pnp_flags : 0; }

extern "C" int sfmhip_pnp_last_timing(sfmhip_ctx* ctx, double* ms3) {
  if (!ctx || !ms3) return SFMHIP_ERR_ARG;
  for (int k = 0; k < 3; ++k) ms3[k] = ctx->pnp_ms[k];
  return SFMHIP_OK;
}
