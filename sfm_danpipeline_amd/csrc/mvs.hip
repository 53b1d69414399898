// mvs.hip -- dense multi-view stereo on the GPU (map3D step 7): the image pyramid, the plane-sweep kernel
// (one workgroup per 16x16 reference tile, warped 12-bit samples and separable integer box sums in LDS, the winner and its
// neighbours in registers: no cost volume in HBM), and the fusion (flag, scan, emit).  The arithmetic is mvs.h's.
#include "common.h"
#include "cloud_grid.h"
#include "mvs.h"
#include "undistort.h"
#include <string.h>

using namespace sfmmvs;
using sfmgrid::blocks;

struct sfmhip_mvs {
  sfmhip_ctx* ctx = nullptr;
  int n = 0, rows = 0, cols = 0;
  Cam K{};
  std::vector<double> poses;
  DevBufs own;
  uint8_t* gray = nullptr;  // n x rows x cols, the working level
  uint8_t* bgr = nullptr;   // n x rows x cols x 3, or null
  float* depth = nullptr;   // n x rows x cols, 0 = no depth
  uint8_t* valid = nullptr; // rows x cols: the level mask of a handle created with distortion (f-14 rule 6), else null
  double* d_poses = nullptr;
  double* d_H = nullptr;    // MAX_PLANES x MAX_SRC x 9: one view's table (sfmhip_mvs_depthmap)
  double* run_H = nullptr;  // n tables of n_planes x MAX_SRC x 9 (sfmhip_mvs_run: one upload for all views)
  size_t run_H_n = 0;
  int32_t* idx = nullptr;   // one view's winner indices and scores
  float* score = nullptr;
  int *flag = nullptr, *offs = nullptr;  // fusion: n x rows x cols
  void* scan_tmp = nullptr;
  size_t scan_bytes = 0;
  std::vector<float> xyz, nrm;
  std::vector<uint32_t> rgb;
  double ms[4] = {0, 0, 0, 0};
};

namespace {

// rule 1: one level of the pyramid for all views (ch interleaved channels)
__global__ void mvs_halve(const uint8_t* __restrict__ in, int n, int rows, int cols, int ch, uint8_t* __restrict__ out) {
  const int r2 = rows >> 1, c2 = cols >> 1;
  const size_t total = (size_t)n * r2 * c2 * ch;
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % ch);
  const int x = (int)((i / ch) % c2), y = (int)((i / ((size_t)ch * c2)) % r2), v = (int)(i / ((size_t)ch * c2 * r2));
  const uint8_t* p = in + (((size_t)v * rows + 2 * y) * cols + 2 * x) * ch + c;
  out[i] = box4(p[0], p[ch], p[(size_t)cols * ch], p[(size_t)cols * ch + ch]);
}

typedef const double __attribute__((address_space(4))) * ConstF64;

struct SweepArgs {
  const uint8_t* gray;
  const double* H;  // [k][s][9], read through wave-uniform addresses
  int rows, cols, ref, n_src, src[MAX_SRC];
  int D, w, n_best;
  double inv_far, step, ncc_min, var_min;
  int32_t* idx;
  float *depth, *score;
};

__global__ __launch_bounds__(TILE* TILE) void mvs_sweep(const SweepArgs A) {
  __shared__ uint16_t s_r[TILE_MAX * TILE_MAX], s_q[TILE_MAX * TILE_MAX];
  __shared__ uint32_t s_a[TILE_MAX * TILE], s_b[TILE_MAX * TILE], s_c[TILE_MAX * TILE];
  __shared__ uint16_t s_bad[TILE_MAX * TILE];
  const int w = A.w, T = TILE + 2 * w, W2 = 2 * w + 1, N = W2 * W2, rows = A.rows, cols = A.cols;
  const int tid = threadIdx.x, lx = tid % TILE, ly = tid / TILE;
  const int ox = blockIdx.x * TILE - w, oy = blockIdx.y * TILE - w;  // image coordinates of tile element (0, 0)
  const int px = ox + w + lx, py = oy + w + ly;
  const bool inside = px < cols && py < rows;
  const size_t npx = (size_t)rows * cols;
  const uint8_t* I = A.gray + npx * A.ref;

  // the reference tile with its apron, then its box sums
  for (int e = tid; e < T * T; e += TILE * TILE) {
    const int x = ox + e % T, y = oy + e / T;
    s_r[e] = (x >= 0 && y >= 0 && x < cols && y < rows) ? (uint16_t)(16 * I[(size_t)y * cols + x]) : (uint16_t)INVALID;
  }
  __syncthreads();
  for (int e = tid; e < T * TILE; e += TILE * TILE) {
    const int j = e / TILE, c = e % TILE;
    uint32_t a = 0, b = 0, bad = 0;
    for (int i = 0; i < W2; ++i) {
      const uint32_t r = s_r[j * T + c + i];
      if (r == (uint32_t)INVALID) ++bad;
      else a += r, b += r * r;
    }
    s_a[e] = a, s_b[e] = b, s_bad[e] = (uint16_t)bad;
  }
  __syncthreads();
  uint32_t sr = 0;
  int64_t vr = 0;
  bool rok;
  {
    uint32_t b = 0, bad = 0;
    for (int j = 0; j < W2; ++j) {
      const int e = (ly + j) * TILE + lx;
      sr += s_a[e], b += s_b[e], bad += s_bad[e];
    }
    vr = var_term(N, sr, b);
    rok = inside && bad == 0 && vr > 0 && (double)vr >= A.var_min;
  }
  Winner win;
  win.clear();
  if (__syncthreads_or(rok)) {  // (also orders the reads above before the sums are overwritten)
    for (int k = 0; k < A.D; ++k) {
      Top top;
      top.clear();
      for (int s = 0; s < A.n_src; ++s) {
        const uint8_t* J = A.gray + npx * A.src[s];
        // the homography through the constant address space: a wave-uniform address there is a scalar load, the nine
        // doubles live in SGPRs
        const ConstF64 hc = (ConstF64)(uintptr_t)(A.H + ((size_t)k * A.n_src + s) * 9);
        double h[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = hc[i];
        for (int e = tid; e < T * T; e += TILE * TILE) {
          const int x = ox + e % T, y = oy + e / T;
          int v = -1;
          if (x >= 0 && y >= 0 && x < cols && y < rows) v = warp_sample(J, rows, cols, h, x, y);
          s_q[e] = (uint16_t)(v < 0 ? INVALID : v);
        }
        __syncthreads();
        for (int e = tid; e < T * TILE; e += TILE * TILE) {
          const int j = e / TILE, c = e % TILE;
          uint32_t a = 0, b = 0, cc = 0, bad = 0;
          for (int i = 0; i < W2; ++i) {
            const uint32_t v = s_q[j * T + c + i], r = s_r[j * T + c + i];
            if (v == (uint32_t)INVALID || r == (uint32_t)INVALID) ++bad;
            else a += v, b += v * v, cc += r * v;
          }
          s_a[e] = a, s_b[e] = b, s_c[e] = cc, s_bad[e] = (uint16_t)bad;
        }
        __syncthreads();
        if (rok) {
          uint32_t a = 0, b = 0, cc = 0, bad = 0;
          for (int j = 0; j < W2; ++j) {
            const int e = (ly + j) * TILE + lx;
            a += s_a[e], b += s_b[e], cc += s_c[e], bad += s_bad[e];
          }
          double v;
          if (bad == 0 && ncc(N, sr, vr, a, b, cc, &v)) top.add(v);
        }
        // (the next round's samples go to s_q, which nobody reads now; its sums are written after the barrier behind them)
      }
      double sc = 0.0;
      const bool ok = rok && top.score(A.n_best, &sc);
      win.step(k, ok, sc);
    }
  }
  if (inside) {
    int32_t bi;
    float d, sc;
    win.finish(A.D, A.inv_far, A.step, A.ncc_min, &bi, &d, &sc);
    const size_t g = (size_t)py * cols + px;
    A.idx[g] = bi, A.depth[g] = d, A.score[g] = sc;
  }
}

struct FuseArgs {
  int n, rows, cols, min_views;
  Cam K;
  double eps;
  const double* poses;
  const float* depth;
  const uint8_t *gray, *bgr;
};

__global__ void mvs_fuse_flag(const FuseArgs A, int* __restrict__ flag) {
  const size_t npx = (size_t)A.rows * A.cols, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npx * A.n) return;
  const int r = (int)(i / npx), y = (int)((i % npx) / A.cols), x = (int)(i % A.cols);
  float p[3], q[3];
  flag[i] = fuse_pixel(r, x, y, A.n, A.rows, A.cols, A.K, A.poses, A.depth, A.eps, A.min_views, p, q) ? 1 : 0;
}

__global__ void mvs_fuse_emit(const FuseArgs A, const int* __restrict__ flag, const int* __restrict__ offs, float* __restrict__ xyz,
                              float* __restrict__ nrm, uint32_t* __restrict__ rgb) {
  const size_t npx = (size_t)A.rows * A.cols, i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= npx * A.n || !flag[i]) return;
  const int r = (int)(i / npx), y = (int)((i % npx) / A.cols), x = (int)(i % A.cols);
  float p[3], q[3];
  if (!fuse_pixel(r, x, y, A.n, A.rows, A.cols, A.K, A.poses, A.depth, A.eps, A.min_views, p, q)) return;
  const size_t o = (size_t)offs[i];
  for (int a = 0; a < 3; ++a) xyz[3 * o + a] = p[a], nrm[3 * o + a] = q[a];
  rgb[o] = pack_rgb(A.gray, A.bgr, i);
}

Opts to_opts(const sfmhip_mvs_opts* o) {
  return Opts{o->n_planes, o->window, o->n_src, o->n_best, o->min_views, o->ncc_min, o->eps, o->var_min};
}

// one depth map into the handle (no synchronisation)
// one view's sweep from a homography table that is already on the device (or on its way there, on the same stream)
int sweep(sfmhip_mvs* h, int ref, int n_src, const int32_t* src, double dmin, double dmax, const Opts& o, const double* d_H) {
  hipStream_t st = h->ctx->stream;
  SweepArgs A;
  plane_range(dmin, dmax, o.n_planes, &A.inv_far, &A.step);
  A.gray = h->gray, A.H = d_H, A.rows = h->rows, A.cols = h->cols, A.ref = ref, A.n_src = n_src;
  for (int s = 0; s < MAX_SRC; ++s) A.src[s] = s < n_src ? src[s] : 0;
  A.D = o.n_planes, A.w = o.window, A.n_best = o.n_best, A.ncc_min = o.ncc_min, A.var_min = o.var_min;
  A.idx = h->idx, A.score = h->score, A.depth = h->depth + (size_t)h->rows * h->cols * ref;
  hipLaunchKernelGGL(mvs_sweep, dim3(blocks(h->cols, TILE), blocks(h->rows, TILE)), dim3(TILE * TILE), 0, st, A);
  SFM_HIP_TRY(hipGetLastError());
  if (h->valid) SFM_TRY(sfm_undistort_seam(st, h->rows, h->cols, o.window, h->valid, A.idx, A.depth, A.score));  // f-14 rule 7
  return SFMHIP_OK;
}

int fuse(sfmhip_mvs* h, const Opts& o, int32_t* n_points) {
  hipStream_t st = h->ctx->stream;
  const size_t total = (size_t)h->n * h->rows * h->cols;
  FuseArgs A{h->n, h->rows, h->cols, o.min_views, h->K, o.eps, h->d_poses, h->depth, h->gray, h->bgr};
  hipLaunchKernelGGL(mvs_fuse_flag, dim3(blocks((long long)total, 256)), dim3(256), 0, st, A, h->flag);
  SFM_HIP_TRY(hipGetLastError());
  size_t need = 0;
  SFM_TRY(sfm_scan_bytes(total, st, &need));
  if (need > h->scan_bytes) {
    unsigned char* t = nullptr;
    SFM_TRY(h->own.alloc(&t, need));
    h->scan_tmp = t, h->scan_bytes = need;
  }
  long long kept = 0;
  SFM_TRY(sfm_exclusive_scan(h->scan_tmp, need, h->flag, h->offs, total, st, &kept));  // (total >= 2: sfmhip_mvs_create)
  const size_t m = (size_t)kept;
  h->xyz.assign(3 * m, 0.0f), h->nrm.assign(3 * m, 0.0f), h->rgb.assign(m, 0u);
  if (m) {
    DevBufs B;
    float *xyz = nullptr, *nrm = nullptr;
    uint32_t* rgb = nullptr;
    SFM_TRY(B.alloc(&xyz, 3 * m));
    SFM_TRY(B.alloc(&nrm, 3 * m));
    SFM_TRY(B.alloc(&rgb, m));
    hipLaunchKernelGGL(mvs_fuse_emit, dim3(blocks((long long)total, 256)), dim3(256), 0, st, A, h->flag, h->offs, xyz, nrm, rgb);
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(h->xyz.data(), xyz, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(h->nrm.data(), nrm, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipMemcpyAsync(h->rgb.data(), rgb, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
  }
  if (n_points) *n_points = (int32_t)m;
  return SFMHIP_OK;
}

// dist5 (with K9, the level-0 camera matrix): null for pinhole views; else every level-0 picture goes through f-14's map first
int create(sfmhip_mvs* h, int n_views, int rows, int cols, const uint8_t* const* gray, const uint8_t* const* bgr, int level,
           const double* K9, const double* dist5) {
  hipStream_t st = h->ctx->stream;
  const size_t px0 = (size_t)rows * cols, px = (size_t)h->rows * h->cols, total = px * n_views;
  SFM_TRY(h->own.alloc(&h->gray, total));
  if (bgr) SFM_TRY(h->own.alloc(&h->bgr, 3 * total));
  SFM_TRY(h->own.alloc(&h->depth, total));
  SFM_TRY(h->own.alloc(&h->d_poses, 12 * (size_t)n_views));
  SFM_TRY(h->own.alloc(&h->d_H, (size_t)MAX_PLANES * MAX_SRC * 9));
  SFM_TRY(h->own.alloc(&h->idx, px));
  SFM_TRY(h->own.alloc(&h->score, px));
  SFM_TRY(h->own.alloc(&h->flag, total));
  SFM_TRY(h->own.alloc(&h->offs, total));
  SFM_HIP_TRY(hipMemsetAsync(h->depth, 0, sizeof(float) * total, st));
  SFM_HIP_TRY(hipMemcpyAsync(h->d_poses, h->poses.data(), sizeof(double) * 12 * n_views, hipMemcpyHostToDevice, st));
  DevBufs U;  // the map of the call and its level-0 mask (the loop below ends on a stream synchronisation)
  sfmund::Packed* map = nullptr;
  if (dist5) {
    uint8_t* valid0 = nullptr;
    SFM_TRY(U.alloc(&map, sfm_undistort_map_entries(rows, cols)));
    SFM_TRY(U.alloc(&valid0, px0));
    SFM_TRY(h->own.alloc(&h->valid, px));
    SFM_TRY(sfm_undistort_map(st, rows, cols, K9, dist5, map, valid0));
    SFM_TRY(sfm_undistort_level_mask(st, rows, cols, level, valid0, h->valid));
  }
  for (int ch = 1; ch <= (bgr ? 3 : 1); ch += 2) {
    uint8_t* dst = ch == 1 ? h->gray : h->bgr;
    DevBufs B;  // the levels above the working one
    uint8_t *a = dst, *b = nullptr, *raw = nullptr;
    if (level > 0) {
      SFM_TRY(B.alloc(&a, px0 * n_views * ch));
      SFM_TRY(B.alloc(&b, (px0 >> 2) * n_views * ch + 1));
    }
    if (dist5) SFM_TRY(B.alloc(&raw, px0 * n_views * ch));
    uint8_t* up = dist5 ? raw : a;
    for (int v = 0; v < n_views; ++v)
      SFM_HIP_TRY(hipMemcpyAsync(up + px0 * v * ch, ch == 1 ? gray[v] : bgr[v], px0 * ch, hipMemcpyHostToDevice, st));
    if (dist5) SFM_TRY(sfm_undistort_apply(st, n_views, rows, cols, ch, raw, a, map));  // all views of this buffer in one launch
    int r = rows, c = cols;
    for (int l = 0; l < level; ++l, r >>= 1, c >>= 1) {
      uint8_t* out = l == level - 1 ? dst : b;
      const size_t m = (size_t)n_views * (r >> 1) * (c >> 1) * ch;
      hipLaunchKernelGGL(mvs_halve, dim3(blocks((long long)m, 256)), dim3(256), 0, st, a, n_views, r, c, ch, out);
      SFM_HIP_TRY(hipGetLastError());
      b = a, a = out;
    }
    SFM_HIP_TRY(hipStreamSynchronize(st));  // before B goes
  }
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_mvs_default_opts(sfmhip_mvs_opts* o) {
  if (!o) return;
  const Opts r = default_opts();
  o->n_planes = r.n_planes, o->window = r.window, o->n_src = r.n_src, o->n_best = r.n_best, o->min_views = r.min_views, o->pad = 0;
  o->ncc_min = r.ncc_min, o->eps = r.eps, o->var_min = r.var_min;
}

static int make_handle(sfmhip_ctx* ctx, int n_views, int rows, int cols, const uint8_t* const* gray, const uint8_t* const* bgr,
                       const double* K9, const double* dist5, const double* poses12, int level, sfmhip_mvs** out) {
  if (!ctx || !out || n_views < 2 || rows < 1 || cols < 1 || !gray || !K9 || !poses12 || level < 0 || level > 8) return SFMHIP_ERR_ARG;
  *out = nullptr;
  if ((rows >> level) < 1 || (cols >> level) < 1 || (double)n_views * rows * cols * 3.0 >= 2147483648.0) return SFMHIP_ERR_ARG;
  for (int v = 0; v < n_views; ++v)
    if (!gray[v] || (bgr && !bgr[v])) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  sfmhip_mvs* h = new sfmhip_mvs();
  h->ctx = ctx, h->n = n_views, h->rows = rows >> level, h->cols = cols >> level;
  h->K = Cam{K9[0], K9[4], K9[2], K9[5]};
  for (int l = 0; l < level; ++l) h->K = halve_cam(h->K);
  h->poses.assign(poses12, poses12 + 12 * (size_t)n_views);
  const int rc = create(h, n_views, rows, cols, gray, bgr, level, K9, dist5);
  if (rc != SFMHIP_OK) {
    delete h;
    return rc;
  }
  *out = h;
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_create(sfmhip_ctx* ctx, int n_views, int rows, int cols, const uint8_t* const* gray, const uint8_t* const* bgr,
                                 const double* K9, const double* poses12, int level, sfmhip_mvs** out) {
  return make_handle(ctx, n_views, rows, cols, gray, bgr, K9, nullptr, poses12, level, out);
}

extern "C" int sfmhip_mvs_create_distorted(sfmhip_ctx* ctx, int n_views, int rows, int cols, const uint8_t* const* gray,
                                           const uint8_t* const* bgr, const double* K9, const double* dist5, const double* poses12,
                                           int level, sfmhip_mvs** out) {
  if (out) *out = nullptr;
  if (!sfmund::model_ok(K9, dist5)) return SFMHIP_ERR_ARG;
  return make_handle(ctx, n_views, rows, cols, gray, bgr, K9, dist5, poses12, level, out);
}

extern "C" int sfmhip_mvs_valid(sfmhip_mvs* h, uint8_t* valid) {
  if (!h || !valid) return SFMHIP_ERR_ARG;
  const size_t px = (size_t)h->rows * h->cols;
  if (!h->valid) {
    memset(valid, 1, px);
    return SFMHIP_OK;
  }
  SFM_HIP_TRY(hipSetDevice(h->ctx->device));
  SFM_HIP_TRY(hipMemcpyAsync(valid, h->valid, px, hipMemcpyDeviceToHost, h->ctx->stream));
  SFM_HIP_TRY(hipStreamSynchronize(h->ctx->stream));
  return SFMHIP_OK;
}

extern "C" void sfmhip_mvs_destroy(sfmhip_mvs* h) {
  if (!h) return;
  hipSetDevice(h->ctx->device);
  hipStreamSynchronize(h->ctx->stream);
  delete h;
}

extern "C" int sfmhip_mvs_level(sfmhip_mvs* h, int32_t* rows, int32_t* cols, double* K9, int view, uint8_t* gray, uint8_t* bgr) {
  if (!h || (view >= h->n) || (bgr && !h->bgr)) return SFMHIP_ERR_ARG;
  if (rows) *rows = h->rows;
  if (cols) *cols = h->cols;
  if (K9) {
    const double k[9] = {h->K.fx, 0, h->K.cx, 0, h->K.fy, h->K.cy, 0, 0, 1};
    memcpy(K9, k, sizeof k);
  }
  if (view >= 0 && (gray || bgr)) {
    SFM_HIP_TRY(hipSetDevice(h->ctx->device));
    const size_t px = (size_t)h->rows * h->cols;
    if (gray) SFM_HIP_TRY(hipMemcpyAsync(gray, h->gray + px * view, px, hipMemcpyDeviceToHost, h->ctx->stream));
    if (bgr) SFM_HIP_TRY(hipMemcpyAsync(bgr, h->bgr + 3 * px * view, 3 * px, hipMemcpyDeviceToHost, h->ctx->stream));
    SFM_HIP_TRY(hipStreamSynchronize(h->ctx->stream));
  }
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_depthmap(sfmhip_mvs* h, int ref, int n_src, const int32_t* src, double dmin, double dmax,
                                   const sfmhip_mvs_opts* opts, int32_t* idx, float* depth, float* score) {
  if (!h || !opts || !depthmap_args_ok(h->n, ref, n_src, src, dmin, dmax, to_opts(opts))) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(h->ctx->device));
  hipStream_t st = h->ctx->stream;
  {
    const Opts o = to_opts(opts);
    double inv_far, step;
    plane_range(dmin, dmax, o.n_planes, &inv_far, &step);
    std::vector<double> H;
    make_homographies(h->K, h->poses.data(), ref, n_src, src, o.n_planes, inv_far, step, H);
    // (a pageable source: the copy waits for the stream and has left H when the call returns)
    SFM_HIP_TRY(hipMemcpyAsync(h->d_H, H.data(), sizeof(double) * H.size(), hipMemcpyHostToDevice, st));
    SFM_TRY(sweep(h, ref, n_src, src, dmin, dmax, o, h->d_H));
  }
  const size_t px = (size_t)h->rows * h->cols;
  if (idx) SFM_HIP_TRY(hipMemcpyAsync(idx, h->idx, sizeof(int32_t) * px, hipMemcpyDeviceToHost, st));
  if (depth) SFM_HIP_TRY(hipMemcpyAsync(depth, h->depth + px * ref, sizeof(float) * px, hipMemcpyDeviceToHost, st));
  if (score) SFM_HIP_TRY(hipMemcpyAsync(score, h->score, sizeof(float) * px, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_set_depthmap(sfmhip_mvs* h, int view, const float* depth) {
  if (!h || view < 0 || view >= h->n || !depth) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(h->ctx->device));
  const size_t px = (size_t)h->rows * h->cols;
  SFM_HIP_TRY(hipMemcpyAsync(h->depth + px * view, depth, sizeof(float) * px, hipMemcpyHostToDevice, h->ctx->stream));
  SFM_HIP_TRY(hipStreamSynchronize(h->ctx->stream));
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_fuse(sfmhip_mvs* h, const sfmhip_mvs_opts* opts, int32_t* n_points) {
  if (!h || !opts || !opts_valid(to_opts(opts))) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(h->ctx->device));
  const double t0 = sfm_now_ms();
  SFM_TRY(fuse(h, to_opts(opts), n_points));
  h->ms[0] = 0.0, h->ms[1] = h->ms[2] = sfm_now_ms() - t0;
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_run(sfmhip_mvs* h, const double* dmin, const double* dmax, const sfmhip_mvs_opts* opts, int32_t* n_points) {
  if (!h || !opts || !dmin || !dmax || !opts_valid(to_opts(opts))) return SFMHIP_ERR_ARG;
  for (int v = 0; v < h->n; ++v)
    if (!(dmin[v] > 0.0) || !(dmin[v] < dmax[v]) || !(dmax[v] < INFINITY)) return SFMHIP_ERR_ARG;
  const Opts o = to_opts(opts);
  SFM_HIP_TRY(hipSetDevice(h->ctx->device));
  const double t0 = sfm_now_ms();
  // every view's sources and homographies first, ONE upload, then the sweeps back to back: a copy per view from pageable
  // memory would wait on the host for the view before it
  const size_t per = (size_t)o.n_planes * MAX_SRC * 9;
  std::vector<double> all(per * h->n), H;
  std::vector<int32_t> src((size_t)MAX_SRC * h->n);
  std::vector<int> ns((size_t)h->n);
  for (int v = 0; v < h->n; ++v) {
    double inv_far, step;
    plane_range(dmin[v], dmax[v], o.n_planes, &inv_far, &step);
    ns[v] = choose_sources(h->poses.data(), h->n, v, o.n_src, &src[(size_t)MAX_SRC * v]);
    make_homographies(h->K, h->poses.data(), v, ns[v], &src[(size_t)MAX_SRC * v], o.n_planes, inv_far, step, H);
    memcpy(&all[per * v], H.data(), sizeof(double) * H.size());
  }
  if (h->run_H_n < all.size()) {
    SFM_TRY(h->own.alloc(&h->run_H, all.size()));  // (grow-only; an outgrown block goes with the handle)
    h->run_H_n = all.size();
  }
  SFM_HIP_TRY(hipMemcpyAsync(h->run_H, all.data(), sizeof(double) * all.size(), hipMemcpyHostToDevice, h->ctx->stream));
  for (int v = 0; v < h->n; ++v)
    SFM_TRY(sweep(h, v, ns[v], &src[(size_t)MAX_SRC * v], dmin[v], dmax[v], o, h->run_H + per * v));
  double t1 = t0;
  if (h->ctx->timing) {  // (the stage split costs one stream bubble)
    SFM_HIP_TRY(hipStreamSynchronize(h->ctx->stream));
    t1 = sfm_now_ms();
  }
  SFM_TRY(fuse(h, o, n_points));
  const double t2 = sfm_now_ms();
  h->ms[0] = t1 - t0, h->ms[1] = t2 - t1, h->ms[2] = t2 - t0;
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_download(const sfmhip_mvs* h, float* xyz, float* normals, uint32_t* rgb) {
  if (!h) return SFMHIP_ERR_ARG;
  if (xyz && !h->xyz.empty()) memcpy(xyz, h->xyz.data(), h->xyz.size() * sizeof(float));
  if (normals && !h->nrm.empty()) memcpy(normals, h->nrm.data(), h->nrm.size() * sizeof(float));
  if (rgb && !h->rgb.empty()) memcpy(rgb, h->rgb.data(), h->rgb.size() * sizeof(uint32_t));
  return SFMHIP_OK;
}

extern "C" int sfmhip_mvs_last_timing(const sfmhip_mvs* h, double* ms3) {
  if (!h || !ms3) return SFMHIP_ERR_ARG;
  for (int i = 0; i < 3; ++i) ms3[i] = h->ms[i];
  return SFMHIP_OK;
}
