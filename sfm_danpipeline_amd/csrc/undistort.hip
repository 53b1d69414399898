// undistort.hip -- the lens-distortion resampling in front of the dense stereo on the GPU: one launch builds
// the packed map of a call (it depends on K, the coefficients and the size only), one launch gathers every view and channel
// through it, and two small kernels give the stereo its masks (the level mask, and "no depth at the seam").  The arithmetic
// is undistort.h's.
#include "common.h"
#include "undistort.h"

using namespace sfmund;

namespace {

constexpr int BLOCK = 256;
constexpr int QUAD = 4;  // destination pixels per thread of the gather

unsigned grid_for(size_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

struct Model {
  double K[9], dist[5];
};

// rules 1-3: one thread per destination pixel
__global__ __launch_bounds__(BLOCK) void und_map(const Model M, int rows, int cols, Packed* __restrict__ map, uint8_t* __restrict__ valid) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (size_t)rows * cols) return;
  double u, v;
  distort_pixel(M.K, M.dist, (int)(i % cols), (int)(i / cols), &u, &v);
  const Tap t = quantise(u, v, rows, cols);
  map[i] = pack(t, cols);
  valid[i] = (uint8_t)t.valid;
}

// rule 4: one thread per QUAD consecutive destination pixels; their map entries are read once (two 16-byte loads) and reused
// for every view and channel.  With px a multiple of 4 every view starts on a word and the QUAD * CH bytes leave as words.
template <int CH>
__global__ __launch_bounds__(BLOCK) void und_gather(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const Packed* __restrict__ map,
                                                    int n, int cols, size_t px) {
  const size_t i0 = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * QUAD;
  if (i0 >= px) return;
  Packed m[QUAD];  // (the map is padded to a multiple of QUAD entries: the tail's surplus is loaded and never used)
  const uint4* mp = (const uint4*)(map + i0);
  const uint4 lo = mp[0], hi = mp[1];
  m[0] = Packed{lo.x, lo.y}, m[1] = Packed{lo.z, lo.w}, m[2] = Packed{hi.x, hi.y}, m[3] = Packed{hi.z, hi.w};
  const bool words = (px % QUAD) == 0;  // (then i0 + QUAD <= px as well)
  for (int v = 0; v < n; ++v) {
    const uint8_t* in = src + (size_t)v * px * CH;
    uint8_t* out = dst + ((size_t)v * px + i0) * CH;
    uint8_t b[QUAD * CH];
#pragma unroll
    for (int k = 0; k < QUAD; ++k)
#pragma unroll
      for (int c = 0; c < CH; ++c) b[k * CH + c] = i0 + k < px ? blend(in, cols, CH, c, m[k]) : (uint8_t)0;
    if (words) {
#pragma unroll
      for (int q = 0; q < CH; ++q)
        ((uint32_t*)out)[q] = (uint32_t)b[4 * q] | ((uint32_t)b[4 * q + 1] << 8) | ((uint32_t)b[4 * q + 2] << 16) | ((uint32_t)b[4 * q + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < QUAD; ++k)
        if (i0 + k < px)
#pragma unroll
          for (int c = 0; c < CH; ++c) out[k * CH + c] = b[k * CH + c];
    }
  }
}

// rule 6: one thread per pixel of the level
__global__ __launch_bounds__(BLOCK) void und_level_mask(const uint8_t* __restrict__ valid0, int cols0, int level, int r, int c,
                                                        uint8_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (size_t)r * c) return;
  out[i] = level_valid(valid0, cols0, level, (int)(i % c), (int)(i / c));
}

// rule 7: one thread per pixel of the depth map
__global__ __launch_bounds__(BLOCK) void und_seam(const uint8_t* __restrict__ valid, int rows, int cols, int window, int32_t* __restrict__ idx,
                                                  float* __restrict__ depth, float* __restrict__ score) {
  const size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= (size_t)rows * cols) return;
  if (!touches_invalid(valid, rows, cols, window, (int)(i % cols), (int)(i / cols))) return;
  idx[i] = -1, depth[i] = 0.0f, score[i] = 0.0f;
}

}  // namespace

size_t sfm_undistort_map_entries(int rows, int cols) { return ((size_t)rows * cols + QUAD - 1) / QUAD * QUAD; }

int sfm_undistort_map(hipStream_t st, int rows, int cols, const double* K9, const double* dist5, Packed* map, uint8_t* valid) {
  Model M;
  memcpy(M.K, K9, sizeof M.K);
  memcpy(M.dist, dist5, sizeof M.dist);
  hipLaunchKernelGGL(und_map, dim3(grid_for((size_t)rows * cols)), dim3(BLOCK), 0, st, M, rows, cols, map, valid);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

int sfm_undistort_apply(hipStream_t st, int n, int rows, int cols, int ch, const uint8_t* src, uint8_t* dst, const Packed* map) {
  const size_t px = (size_t)rows * cols;
  const dim3 grid(grid_for((px + QUAD - 1) / QUAD)), block(BLOCK);
  if (ch == 1) hipLaunchKernelGGL(und_gather<1>, grid, block, 0, st, src, dst, map, n, cols, px);
  else if (ch == 3) hipLaunchKernelGGL(und_gather<3>, grid, block, 0, st, src, dst, map, n, cols, px);
  else return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

int sfm_undistort_level_mask(hipStream_t st, int rows, int cols, int level, const uint8_t* valid0, uint8_t* out) {
  const int r = rows >> level, c = cols >> level;
  hipLaunchKernelGGL(und_level_mask, dim3(grid_for((size_t)r * c)), dim3(BLOCK), 0, st, valid0, cols, level, r, c, out);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

int sfm_undistort_seam(hipStream_t st, int rows, int cols, int window, const uint8_t* valid, int32_t* idx, float* depth, float* score) {
  hipLaunchKernelGGL(und_seam, dim3(grid_for((size_t)rows * cols)), dim3(BLOCK), 0, st, valid, rows, cols, window, idx, depth, score);
  SFM_HIP_TRY(hipGetLastError());
  return SFMHIP_OK;
}

extern "C" int sfmhip_image_undistort(sfmhip_ctx* ctx, int n_images, int rows, int cols, int channels, const uint8_t* const* src,
                                      const double* K9, const double* dist5, uint8_t* const* dst, uint8_t* valid) {
  if (!ctx || n_images < 1 || rows < 1 || cols < 1 || (channels != 1 && channels != 3) || !src || !dst || !model_ok(K9, dist5))
    return SFMHIP_ERR_ARG;
  if ((double)n_images * rows * cols * channels >= 2147483648.0) return SFMHIP_ERR_ARG;
  for (int i = 0; i < n_images; ++i)
    if (!src[i] || !dst[i]) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  ctx->undistort_ms[0] = ctx->undistort_ms[1] = 0;
  const size_t px = (size_t)rows * cols, bytes = px * channels;
  DevBufs B;
  uint8_t *in = nullptr, *out = nullptr, *d_valid = nullptr;
  Packed* map = nullptr;
  SFM_TRY(B.alloc(&in, bytes * n_images));
  SFM_TRY(B.alloc(&out, bytes * n_images));
  SFM_TRY(B.alloc(&d_valid, px));
  SFM_TRY(B.alloc(&map, sfm_undistort_map_entries(rows, cols)));
  struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events() {
      for (hipEvent_t x : e)
        if (x) hipEventDestroy(x);
    }
  } evs;
  if (ctx->timing)
    for (hipEvent_t& x : evs.e) SFM_HIP_TRY(hipEventCreate(&x));
  for (int i = 0; i < n_images; ++i) SFM_HIP_TRY(hipMemcpyAsync(in + bytes * i, src[i], bytes, hipMemcpyHostToDevice, st));
  if (ctx->timing) SFM_HIP_TRY(hipEventRecord(evs.e[0], st));
  SFM_TRY(sfm_undistort_map(st, rows, cols, K9, dist5, map, d_valid));
  if (ctx->timing) SFM_HIP_TRY(hipEventRecord(evs.e[1], st));
  SFM_TRY(sfm_undistort_apply(st, n_images, rows, cols, channels, in, out, map));
  if (ctx->timing) SFM_HIP_TRY(hipEventRecord(evs.e[2], st));
  for (int i = 0; i < n_images; ++i) SFM_HIP_TRY(hipMemcpyAsync(dst[i], out + bytes * i, bytes, hipMemcpyDeviceToHost, st));
  if (valid) SFM_HIP_TRY(hipMemcpyAsync(valid, d_valid, px, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (ctx->timing) {
    float a = 0, b = 0;
    SFM_HIP_TRY(hipEventElapsedTime(&a, evs.e[0], evs.e[1]));
    SFM_HIP_TRY(hipEventElapsedTime(&b, evs.e[1], evs.e[2]));
    ctx->undistort_ms[0] = a, ctx->undistort_ms[1] = b;
  }
  return SFMHIP_OK;
}

extern "C" int sfmhip_image_undistort_last_timing(sfmhip_ctx* ctx, double* ms2) {
  if (!ctx || !ms2) return SFMHIP_ERR_ARG;
  ms2[0] = ctx->undistort_ms[0], ms2[1] = ctx->undistort_ms[1];
  return SFMHIP_OK;
}
