// cloud_filter.hip -- PCL 1.8.1's VoxelGrid and StatisticalOutlierRemoval on the device-resident cloud (sfmhip_cloud), and
// the calls that keep a filter's result on the device: sfmhip_cloud_select, the voxel grid's out_cloud, sfmhip_cloud_download.
// The rules are cloud_filter.h's (V1-V7, S1-S5), which the CPU test stub compiles too.
//
// Voxel grid: vg_keys (V3) -> the handle's cell_sort over the bits div[0] div[1] div[2] needs (stable: a run of equal keys
// is in ascending input index) -> run heads by flag + scan -> vg_reduce.  vg_reduce gives every run to a lane; a lane sums
// a run of at most one block (64 points) itself, and the runs of a wave's 64 that are longer are then taken one after the
// other by the whole wave: lane l sums blocks l, l + 64, ... sequentially (block_sum) and the block sums are folded in
// ascending order by walking the lanes (fold_block), which is V5's order whatever the launch looks like.  The colours
// and the normals ride the same pass.
// Neighbour means: sor_mean_dist, one wave per query point.  Lane j holds slot j of the sorted list of the mean_k + 1
// smallest d2 seen so far (the index is not kept: S1, ties give equal terms).  Candidates come 64 at a time, coalesced,
// from the k-NN grid's row spans; a ballot screens them against the current k-th d2 and the survivors are merged by rank:
// a list entry moves up by the number of survivors below it, a survivor goes to (entries <= it) + (survivors before it),
// and one LDS round trip of 64 floats applies the permutation.  Ring expansion and the stop rule are cloud_knn's.  S2's
// sum walks the lanes in order.  S3's partials take a lane per block of 256 points; the host adds them in order.
// No atomics on floats, no spins, no hand-offs between workgroups.
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include "cloud_filter.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmgrid;
using sfmfilter::VoxelPlan;

namespace {

constexpr int RED_BLOCK = 256;  // runs per vg_reduce workgroup (4 waves)

struct FltState {  // on the cloud handle, freed with it: run tables, attributes, mean distances
  static constexpr sfmgrid::Stage slot = sfmgrid::FILTER;  // (its slot on the handle: stage<FltState>(cloud))
  Grow<int> run_start, emit, row, voxel_of, sel;
  Grow<uint32_t> rgb_in, rgb_out;
  Grow<float> nrm_in, nrm_out, md;
  Grow<double> part;
  double ms[4] = {0, 0, 0, 0};  // key + sort, voxel reduce (last voxel grid); neighbour means, threshold + compaction (last outlier call)
};

// ---- voxel grid

__global__ void vg_keys(const float* xyz, int n, VoxelPlan p, int invalid, int* keys, int* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  keys[i] = sfmcloud::finite3(x, y, z) ? sfmfilter::voxel_key(p, x, y, z) : invalid;
  vals[i] = i;
}

__global__ void vg_heads(const int* skeys, int n_valid, int* head) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_valid) return;
  head[i] = (i == 0 || skeys[i - 1] != skeys[i]) ? 1 : 0;
}

__global__ void vg_run_starts(const int* head, const int* before, int n_valid, int* run_start) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_valid) return;
  if (head[i]) run_start[before[i]] = i;
}

__device__ __forceinline__ int run_count(const int* run_start, int r, int n_runs, int n_valid) {
  return (r + 1 < n_runs ? run_start[r + 1] : n_valid) - run_start[r];
}

__global__ void vg_emit_flags(const int* run_start, int n_runs, int n_valid, int min_points, int* emit) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_runs) return;
  emit[r] = run_count(run_start, r, n_runs, n_valid) >= min_points ? 1 : 0;
}

template <int C>
struct RunReader {  // V5's get(j, v): point j of the run that starts at `s` in sorted order
  const float* xyz;
  const float* nrm;
  const int* svals;
  int s;
  __device__ void operator()(int j, float* v) const {
    const size_t i = (size_t)svals[s + j];
    v[0] = xyz[3 * i], v[1] = xyz[3 * i + 1], v[2] = xyz[3 * i + 2];
    if (C == 6) v[3] = nrm[3 * i], v[4] = nrm[3 * i + 1], v[5] = nrm[3 * i + 2];
  }
};

template <int C>
__device__ __forceinline__ void vg_write(int row, int cnt, const float (&t)[C], const uint64_t (&cs)[3], bool has_rgb, float* out_xyz,
                                         uint32_t* out_rgb, float* out_nrm) {
  for (int a = 0; a < 3; ++a) out_xyz[3 * (size_t)row + a] = sfmfilter::centroid(t[a], cnt);
  if (has_rgb) out_rgb[row] = sfmfilter::rgb_mean(cs, cnt);
  if (C == 6) {
    const float s[3] = {t[3], t[4], t[5]};
    float o[3];
    sfmfilter::normal_mean(s, o);
    for (int a = 0; a < 3; ++a) out_nrm[3 * (size_t)row + a] = o[a];
  }
}

// one lane per run; the long runs of a wave's 64 are then summed by the whole wave, one after the other.  No early
// return: every lane of a wave reaches the ballot.
template <int C>
__global__ __launch_bounds__(RED_BLOCK) void vg_reduce(const float* xyz, const int* svals, const int* run_start, const int* emit,
                                                      const int* row, int n_runs, int n_valid, const uint32_t* rgb, const float* nrm,
                                                      float* out_xyz, uint32_t* out_rgb, float* out_nrm) {
  const int r = blockIdx.x * RED_BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int s = 0, cnt = 0, orow = 0;
  bool live = false;
  if (r < n_runs) {
    s = run_start[r];
    cnt = run_count(run_start, r, n_runs, n_valid);
    live = emit[r] != 0;
    orow = row[r];
  }
  if (live && cnt <= sfmfilter::BLOCK) {
    float t[C];
    sfmfilter::run_sum<C>(cnt, RunReader<C>{xyz, nrm, svals, s}, t);
    uint64_t cs[3] = {0, 0, 0};
    if (rgb)
      for (int j = 0; j < cnt; ++j) sfmfilter::rgb_add(cs, rgb[svals[s + j]]);
    vg_write<C>(orow, cnt, t, cs, rgb != nullptr, out_xyz, out_rgb, out_nrm);
  }
  unsigned long long todo = __ballot(live && cnt > sfmfilter::BLOCK);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    const int ws = __shfl(s, src), wcnt = __shfl(cnt, src), wrow = __shfl(orow, src);
    const int nb = (wcnt + sfmfilter::BLOCK - 1) / sfmfilter::BLOCK;
    const RunReader<C> get{xyz, nrm, svals, ws};
    float t[C];
    for (int c = 0; c < C; ++c) t[c] = 0.0f;
    uint64_t cs[3] = {0, 0, 0};
    for (int b0 = 0; b0 < nb; b0 += 64) {
      const int b = b0 + lane;
      float sb[C];
      for (int c = 0; c < C; ++c) sb[c] = 0.0f;
      if (b < nb) {
        const int j0 = b * sfmfilter::BLOCK, j1 = min(j0 + sfmfilter::BLOCK, wcnt);
        sfmfilter::block_sum<C>(j0, j1, get, sb);
        if (rgb)
          for (int j = j0; j < j1; ++j) sfmfilter::rgb_add(cs, rgb[svals[ws + j]]);
      }
      const int m = min(64, nb - b0);
      for (int l = 0; l < m; ++l) {  // the block sums in ascending order: the same chain in every lane
        float sl[C];
        for (int c = 0; c < C; ++c) sl[c] = __shfl(sb[c], l);
        sfmfilter::fold_block<C>(t, sl);
      }
    }
    for (int off = 32; off >= 1; off >>= 1)
      for (int a = 0; a < 3; ++a) cs[a] += (uint64_t)__shfl_xor((unsigned long long)cs[a], off);  // (integers: any order)
    if (lane == 0) vg_write<C>(wrow, wcnt, t, cs, rgb != nullptr, out_xyz, out_rgb, out_nrm);
  }
}

__global__ void vg_voxel_of(const int* svals, const int* head, const int* before, const int* emit, const int* row, int n, int n_valid,
                            int* voxel_of) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int v = -1;
  if (i < n_valid) {
    const int r = before[i] + head[i] - 1;
    if (emit[r]) v = row[r];
  }
  voxel_of[svals[i]] = v;
}

__global__ void flt_gather(const float* xyz, const int* ind, int m, float* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= m) return;
  const size_t j = (size_t)ind[r];
  out[3 * (size_t)r] = xyz[3 * j];
  out[3 * (size_t)r + 1] = xyz[3 * j + 1];
  out[3 * (size_t)r + 2] = xyz[3 * j + 2];
}

// ---- statistical outlier removal

// a workgroup is one wave and one query point (sorted position blockIdx.x): control flow is uniform
__global__ __launch_bounds__(64) void sor_mean_dist(GridDev g, double abs_eps, int mean_k, float* md) {
  __shared__ float slot[64];
  const int lane = threadIdx.x;
  const int i = blockIdx.x;
  const float4 p = g.pts[i];
  const int key = g.keys[i];
  const int c[3] = {key % g.D[0], (key / g.D[0]) % g.D[1], key / (g.D[0] * g.D[1])};
  const float inf = sfmcloud::bits_f(0x7F800000u);
  const int K = mean_k + 1;
  float L = inf;    // slot `lane` of the ascending list
  float kth = inf;  // slot K - 1
  auto scan_row = [&](int row, int xa, int xb) {
    int s, e;
    row_span(g, row, xa, xb, &s, &e);
    for (int b = s; b < e; b += 64) {
      const int j = b + lane;
      float d = inf;
      if (j < e) {
        const float4 q = g.pts[j];
        d = sfmcloud::dist2(p.x, p.y, p.z, q.x, q.y, q.z);
      }
      const bool surv = d < kth;  // (a candidate equal to the k-th would leave the list's values as they are)
      unsigned long long todo = __ballot(surv);
      if (!todo) continue;
      int up = 0, rank = 0, below = 0;
      while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const float ds = __shfl(d, src);
        up += ds < L ? 1 : 0;                                           // list entry: survivors below it
        const int nle = __popcll(__ballot(L <= ds));                    // entries that stay in front of survivor src
        rank += (ds < d || (ds == d && src < lane)) ? 1 : 0;            // survivor: survivors before it
        below = lane == src ? nle : below;
      }
      __syncthreads();
      if (lane + up < 64) slot[lane + up] = L;
      if (surv && below + rank < 64) slot[below + rank] = d;
      __syncthreads();
      L = slot[lane];
      kth = slot[K - 1];
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
    if (kth < inf) {           // K entries: stop once every unsearched point is strictly farther than the k-th
      const double bs = b * (1.0 - 1.0 / 65536.0) - abs_eps;
      if (bs > 0.0 && bs * bs > (double)kth) break;
    }
  }
  const double term = sfmfilter::dist_term(L);
  double sum = 0.0;
  for (int k = 1; k <= mean_k; ++k) sum += __shfl(term, k);  // S2: slots 1..mean_k in order
  if (lane == 0) md[__float_as_int(p.w)] = sfmfilter::mean_dist(sum, mean_k);
}

__global__ void sor_partials(const float* md, int n, long long n_part, double* part) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_part) return;
  const long long i0 = b * sfmfilter::SUM_BLOCK;
  double sum, sq;
  sfmfilter::stat_partial(md, i0, i0 + sfmfilter::SUM_BLOCK < n ? i0 + sfmfilter::SUM_BLOCK : (long long)n, sum, sq);
  part[2 * b] = sum;
  part[2 * b + 1] = sq;
}

__global__ void sor_flags(const float* xyz, const float* md, int n, double thr, int negative, int* flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool fin = sfmcloud::finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
  flags[i] = fin && sfmfilter::stat_keep(md[i], thr, negative != 0) ? 1 : 0;
}

template <typename T>
int upload(hipStream_t st, T* dst, const T* src, size_t n) {
  SFM_HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, st));
  return SFMHIP_OK;
}
template <typename T>
int download(hipStream_t st, T* dst, const T* src, size_t n) {
  if (n) SFM_HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, st));
  return SFMHIP_OK;
}

template <int C>
void launch_reduce(hipStream_t st, const sfmhip_cloud* c, const FltState* s, int n_runs, const uint32_t* rgb, const float* nrm,
                   float* out_xyz) {
  hipLaunchKernelGGL(vg_reduce<C>, dim3(blocks(n_runs, RED_BLOCK)), dim3(RED_BLOCK), 0, st, c->xyz, c->ibuf[3], s->run_start.p, s->emit.p,
                     s->row.p, n_runs, c->n_valid, rgb, nrm, out_xyz, s->rgb_out.p, s->nrm_out.p);
}

}  // namespace

extern "C" int sfmhip_cloud_voxel_grid(sfmhip_cloud* c, const float leaf[3], int min_points, const uint32_t* rgb, const float* normals,
                                       float* out_xyz, uint32_t* out_rgb, float* out_normals, int32_t* voxel_of, int32_t* n_out,
                                       sfmhip_cloud** out_cloud) {
  if (!c || !leaf || !n_out || min_points < 0) return SFMHIP_ERR_ARG;
  float mn[3], mx[3];
  for (int a = 0; a < 3; ++a) mn[a] = (float)c->lo[a], mx[a] = (float)c->hi[a];  // (the box is of floats: exact)
  VoxelPlan plan;
  const int pr = sfmfilter::voxel_plan(leaf, mn, mx, plan);
  if (pr == sfmfilter::PLAN_ARG) return SFMHIP_ERR_ARG;
  if (pr == sfmfilter::PLAN_UNSUPPORTED) return SFMHIP_ERR_UNSUPPORTED;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  const bool timing = c->ctx->timing;
  FltState* s = stage<FltState>(c);
  s->ms[0] = s->ms[1] = 0;
  const int n = c->n, nv = c->n_valid;
  int n_runs = 0, m = 0;
  float* d_out = nullptr;
  if (nv > 0) {
    SFM_TRY(ensure_ibuf(c));
    SFM_TRY(s->run_start.need(n));
    SFM_TRY(s->emit.need(n));
    SFM_TRY(s->row.need(n));
    if (rgb) {
      SFM_TRY(s->rgb_in.need(n));
      SFM_TRY(s->rgb_out.need(n));
      SFM_TRY(upload(st, s->rgb_in.p, rgb, (size_t)n));
    }
    if (normals) {
      SFM_TRY(s->nrm_in.need((size_t)3 * n));
      SFM_TRY(s->nrm_out.need((size_t)3 * n));
      SFM_TRY(upload(st, s->nrm_in.p, normals, (size_t)3 * n));
    }
    const double t0 = sfm_now_ms();
    int *kin = c->ibuf[0], *vin = c->ibuf[1], *skeys = c->ibuf[2], *svals = c->ibuf[3];
    hipLaunchKernelGGL(vg_keys, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, n, plan, (int)plan.ncell, kin, vin);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(cell_sort(c, plan.ncell, kin, skeys, vin, svals, n));
    if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
    const double t1 = sfm_now_ms();
    int *head = c->ibuf[0], *before = c->ibuf[1];
    hipLaunchKernelGGL(vg_heads, dim3(blocks(nv, 256)), dim3(256), 0, st, skeys, nv, head);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(scan(c, head, before, (size_t)nv, &n_runs));
    if (n_runs < 1 || n_runs > nv) return SFMHIP_ERR_STATE;
    hipLaunchKernelGGL(vg_run_starts, dim3(blocks(nv, 256)), dim3(256), 0, st, head, before, nv, s->run_start.p);
    SFM_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(vg_emit_flags, dim3(blocks(n_runs, 256)), dim3(256), 0, st, s->run_start.p, n_runs, nv, min_points, s->emit.p);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(scan(c, s->emit.p, s->row.p, (size_t)n_runs, &m));
    if (m < 0 || m > n_runs) return SFMHIP_ERR_STATE;
    SFM_TRY(sfm_dev_alloc(&d_out, (size_t)3 * std::max(m, 1)));
    if (normals)
      launch_reduce<6>(st, c, s, n_runs, rgb ? s->rgb_in.p : nullptr, s->nrm_in.p, d_out);
    else
      launch_reduce<3>(st, c, s, n_runs, rgb ? s->rgb_in.p : nullptr, nullptr, d_out);
    int rc = hipGetLastError() == hipSuccess ? SFMHIP_OK : SFMHIP_ERR_HIP;
    if (rc == SFMHIP_OK && voxel_of) {
      rc = s->voxel_of.need(n);
      if (rc == SFMHIP_OK) {
        hipLaunchKernelGGL(vg_voxel_of, dim3(blocks(n, 256)), dim3(256), 0, st, svals, head, before, s->emit.p, s->row.p, n, nv,
                           s->voxel_of.p);
        rc = hipGetLastError() == hipSuccess ? SFMHIP_OK : SFMHIP_ERR_HIP;
      }
    }
    if (rc == SFMHIP_OK && out_xyz) rc = download(st, out_xyz, d_out, (size_t)3 * m);
    if (rc == SFMHIP_OK && out_rgb && rgb) rc = download(st, out_rgb, s->rgb_out.p, (size_t)m);
    if (rc == SFMHIP_OK && out_normals && normals) rc = download(st, out_normals, s->nrm_out.p, (size_t)3 * m);
    if (rc == SFMHIP_OK && voxel_of) rc = download(st, voxel_of, s->voxel_of.p, (size_t)n);
    if (rc == SFMHIP_OK && hipStreamSynchronize(st) != hipSuccess) rc = SFMHIP_ERR_HIP;
    if (rc != SFMHIP_OK) {
      hipFree(d_out);
      return rc;
    }
    if (timing) {
      s->ms[0] = t1 - t0;
      s->ms[1] = sfm_now_ms() - t1;
    }
  } else {
    for (int i = 0; voxel_of && i < n; ++i) voxel_of[i] = -1;
    if (out_cloud) SFM_TRY(sfm_dev_alloc(&d_out, (size_t)3));
  }
  *n_out = m;
  if (out_cloud) return adopt_device(c->ctx, d_out, m, out_cloud);
  hipFree(d_out);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_statistical_outlier(sfmhip_cloud* c, int mean_k, double std_mul, int negative, int32_t* idx_out,
                                                int32_t* n_out, float* mean_dist, double* threshold) {
  if (!c || mean_k < 1 || mean_k > sfmfilter::MEAN_K_MAX || !(std_mul - std_mul == 0.0) || !n_out || (c->n > 0 && !idx_out))
    return SFMHIP_ERR_ARG;
  const int n = c->n, nv = c->n_valid;
  if (nv > 0 && nv <= mean_k) return SFMHIP_ERR_ARG;  // S5
  FltState* s = stage<FltState>(c);
  s->ms[2] = s->ms[3] = 0;
  *n_out = 0;
  if (threshold) *threshold = 0.0;
  if (nv == 0) {
    for (int i = 0; mean_dist && i < n; ++i) mean_dist[i] = 0.0f;
    return SFMHIP_OK;
  }
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  const bool timing = c->ctx->timing;
  SFM_TRY(ensure_ibuf(c));
  SFM_TRY(knn_grid(c));
  const long long n_part = (n + (long long)sfmfilter::SUM_BLOCK - 1) / sfmfilter::SUM_BLOCK;
  SFM_TRY(s->md.need(n));
  SFM_TRY(s->part.need((size_t)2 * n_part));
  const double t0 = sfm_now_ms();
  SFM_HIP_TRY(hipMemsetAsync(s->md.p, 0, sizeof(float) * (size_t)n, st));  // S2: a non-finite point's 0
  hipLaunchKernelGGL(sor_mean_dist, dim3((unsigned)nv), dim3(64), 0, st, c->kg.dev(nv), knn_abs_eps(c), mean_k, s->md.p);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t1 = sfm_now_ms();
  hipLaunchKernelGGL(sor_partials, dim3(blocks(n_part, 64)), dim3(64), 0, st, s->md.p, n, n_part, s->part.p);
  SFM_HIP_TRY(hipGetLastError());
  std::vector<double> part((size_t)2 * n_part);
  SFM_TRY(download(st, part.data(), s->part.p, part.size()));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  const double thr = sfmfilter::threshold(part.data(), n_part, nv, std_mul);
  hipLaunchKernelGGL(sor_flags, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, s->md.p, n, thr, negative, c->ibuf[0]);
  SFM_HIP_TRY(hipGetLastError());
  if (mean_dist) SFM_TRY(download(st, mean_dist, s->md.p, (size_t)n));
  SFM_TRY(compact(c, idx_out, n_out));
  if (threshold) *threshold = thr;
  if (timing) {
    s->ms[2] = t1 - t0;
    s->ms[3] = sfm_now_ms() - t1;
  }
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_select(sfmhip_cloud* c, const int32_t* indices, int n_idx, sfmhip_cloud** out) {
  if (!c || !out || n_idx < 0 || (n_idx > 0 && !indices)) return SFMHIP_ERR_ARG;
  for (int r = 0; r < n_idx; ++r)
    if (indices[r] < 0 || indices[r] >= c->n) return SFMHIP_ERR_ARG;
  *out = nullptr;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  FltState* s = stage<FltState>(c);
  float* d = nullptr;
  SFM_TRY(sfm_dev_alloc(&d, (size_t)3 * std::max(n_idx, 1)));
  if (n_idx > 0) {
    int rc = s->sel.need(n_idx);
    if (rc == SFMHIP_OK) rc = upload(st, s->sel.p, (const int*)indices, (size_t)n_idx);
    if (rc == SFMHIP_OK) {
      hipLaunchKernelGGL(flt_gather, dim3(blocks(n_idx, 256)), dim3(256), 0, st, c->xyz, s->sel.p, n_idx, d);
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) rc = SFMHIP_ERR_HIP;
    }
    if (rc != SFMHIP_OK) {
      hipFree(d);
      return rc;
    }
  }
  return adopt_device(c->ctx, d, n_idx, out);
}

extern "C" int sfmhip_cloud_size(const sfmhip_cloud* c, int32_t* n, int32_t* n_valid) {
  if (!c) return SFMHIP_ERR_ARG;
  if (n) *n = c->n;
  if (n_valid) *n_valid = c->n_valid;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_download(sfmhip_cloud* c, float* xyz) {
  if (!c || (c->n > 0 && !xyz)) return SFMHIP_ERR_ARG;
  if (c->n == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  SFM_TRY(download(c->ctx->stream, xyz, (const float*)c->xyz, (size_t)3 * c->n));
  SFM_HIP_TRY(hipStreamSynchronize(c->ctx->stream));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_filter_last_timing(sfmhip_cloud* c, double ms4[4]) {
  if (!c || !ms4) return SFMHIP_ERR_ARG;
  const FltState* s = stage<FltState>(c);
  for (int i = 0; i < 4; ++i) ms4[i] = s->ms[i];
  return SFMHIP_OK;
}
