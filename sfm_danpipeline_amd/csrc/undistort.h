// undistort.h -- the lens-distortion resampling in front of the dense stereo: for every pixel of the
// undistorted picture (camera matrix K, unchanged) where it lies in the distorted one, quantised to 1/32 pixel, and the
// integer bilinear blend that fetches it; then the validity masks the stereo needs.  Shared by the HIP kernels
// (undistort.hip) and by a g++ build (tests/stub/undistort_capi.cpp); compiled without floating-point contraction on both
// sides.  The map is f64 in one written-out order (camera.h's forward model), everything after it is integer, so the device
// equals the host build bit for bit.  There is no library to pin parity against: the rule list is the contract.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "camera.h"

#if defined(__HIPCC__)
#define UND_HD __host__ __device__ __forceinline__
#else
#define UND_HD inline
#endif

namespace sfmund {

// rules 2-3: the four taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1) with weights out of 32
struct Tap {
  int32_t ix, iy, wx, wy, valid;
};

// the map as the kernels keep it: the byte-pixel offset of tap (ix, iy) and wx | wy << 8 | valid << 16 (both 0 when invalid).
// A valid entry has 0 <= ix < cols and 0 <= iy < rows: tap (ix, iy) always carries weight (wx, wy <= 31).
struct Packed {
  uint32_t off, w;
};

// rule 1: where destination pixel (x, y) lies in the distorted picture.  project_point under P = [I | 0] on (xn, yn, 1) is
// the forward model alone: its products with 1 and sums with 0 are exact.
UND_HD void distort_pixel(const double* K9, const double* dist5, int x, int y, double* u, double* v) {
  const double P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  const double X[3] = {((double)x - K9[2]) / K9[0], ((double)y - K9[5]) / K9[4], 1.0};
  sfmcam::project_point(P, K9, dist5, X, *u, *v);
}

// rules 2-3.  Outside [-1, cols) x [-1, rows) no carry can bring tap (ix, iy) inside, and a NaN fails the comparison: both
// are invalid before anything is converted to an integer.
UND_HD Tap quantise(double u, double v, int rows, int cols) {
  Tap t{0, 0, 0, 0, 0};
  if (!(u >= -1.0 && v >= -1.0 && u < (double)cols && v < (double)rows)) return t;
  const double fu = floor(u), fv = floor(v);
  t.ix = (int32_t)fu, t.iy = (int32_t)fv;
  t.wx = (int32_t)floor((u - fu) * 32.0 + 0.5), t.wy = (int32_t)floor((v - fv) * 32.0 + 0.5);
  if (t.wx == 32) t.wx = 0, ++t.ix;
  if (t.wy == 32) t.wy = 0, ++t.iy;
  // after the carry: a tap is needed iff its weight is not zero
  t.valid = t.ix >= 0 && t.iy >= 0 && t.ix + (t.wx ? 1 : 0) < cols && t.iy + (t.wy ? 1 : 0) < rows;
  return t;
}

UND_HD Packed pack(const Tap& t, int cols) {
  if (!t.valid) return Packed{0u, 0u};
  return Packed{(uint32_t)t.iy * (uint32_t)cols + (uint32_t)t.ix, (uint32_t)t.wx | ((uint32_t)t.wy << 8) | (1u << 16)};
}

// rule 4 for channel c of an image with ch interleaved channels; a tap of weight zero is not read
UND_HD uint8_t blend(const uint8_t* img, int cols, int ch, int c, const Packed m) {
  if (!(m.w >> 16)) return 0;
  const int wx = (int)(m.w & 0xFF), wy = (int)((m.w >> 8) & 0xFF);
  const uint8_t* p = img + (size_t)m.off * ch + c;
  const size_t row = (size_t)cols * ch;
  const int a = p[0], b = wx ? p[ch] : 0, cc = wy ? p[row] : 0, d = (wx && wy) ? p[row + ch] : 0;
  return (uint8_t)(((a * (32 - wx) + b * wx) * (32 - wy) + (cc * (32 - wx) + d * wx) * wy + 512) >> 10);
}

// rule 6: level-L pixel (x, y) over the level-0 mask
UND_HD uint8_t level_valid(const uint8_t* valid0, int cols0, int level, int x, int y) {
  const int s = 1 << level;
  for (int dy = 0; dy < s; ++dy)
    for (int dx = 0; dx < s; ++dx)
      if (!valid0[(size_t)(y * s + dy) * cols0 + (x * s + dx)]) return 0;
  return 1;
}

// rule 7: does the (2 window + 1)^2 window of (x, y) touch an invalid pixel of the mask?  (Positions off the image are not
// pixels; a reference pixel that close to the border has no depth by f-10's rule 4.)
UND_HD bool touches_invalid(const uint8_t* valid, int rows, int cols, int window, int x, int y) {
  const int y0 = y - window < 0 ? 0 : y - window, y1 = y + window >= rows ? rows - 1 : y + window;
  const int x0 = x - window < 0 ? 0 : x - window, x1 = x + window >= cols ? cols - 1 : x + window;
  for (int yy = y0; yy <= y1; ++yy)
    for (int xx = x0; xx <= x1; ++xx)
      if (!valid[(size_t)yy * cols + xx]) return true;
  return false;
}

// what the entry points refuse (SFMHIP_ERR_ARG): a focal length of 0 or a non-finite number
inline bool model_ok(const double* K9, const double* dist5) {
  if (!K9 || !dist5) return false;
  for (int i : {0, 2, 4, 5})
    if (!isfinite(K9[i])) return false;
  if (K9[0] == 0.0 || K9[4] == 0.0) return false;
  for (int i = 0; i < 5; ++i)
    if (!isfinite(dist5[i])) return false;
  return true;
}

// ------------------------------------------------------------------------------------------------ host only
#ifndef __HIPCC__
namespace host {

inline void make_map(int rows, int cols, const double* K9, const double* dist5, std::vector<Packed>& map, uint8_t* valid) {
  map.resize((size_t)rows * cols);
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      double u, v;
      distort_pixel(K9, dist5, x, y, &u, &v);
      const Tap t = quantise(u, v, rows, cols);
      map[(size_t)y * cols + x] = pack(t, cols);
      if (valid) valid[(size_t)y * cols + x] = (uint8_t)t.valid;
    }
}

// rules 1-5 for n images of one size; false: the arguments are refused
inline bool undistort(int n, int rows, int cols, int ch, const uint8_t* const* src, const double* K9, const double* dist5,
                      uint8_t* const* dst, uint8_t* valid) {
  if (n < 1 || rows < 1 || cols < 1 || (ch != 1 && ch != 3) || !src || !dst || !model_ok(K9, dist5)) return false;
  for (int i = 0; i < n; ++i)
    if (!src[i] || !dst[i]) return false;
  std::vector<Packed> map;
  make_map(rows, cols, K9, dist5, map, valid);
  const size_t px = (size_t)rows * cols;
  for (int i = 0; i < n; ++i)
    for (size_t p = 0; p < px; ++p)
      for (int c = 0; c < ch; ++c) dst[i][p * ch + c] = blend(src[i], cols, ch, c, map[p]);
  return true;
}

inline void level_mask(const uint8_t* valid0, int rows, int cols, int level, uint8_t* out) {
  const int r = rows >> level, c = cols >> level;
  for (int y = 0; y < r; ++y)
    for (int x = 0; x < c; ++x) out[(size_t)y * c + x] = level_valid(valid0, cols, level, x, y);
}

// rule 7 on one depth map (idx, depth, score nullable)
inline void seam(const uint8_t* valid, int rows, int cols, int window, int32_t* idx, float* depth, float* score) {
  for (int y = 0; y < rows; ++y)
    for (int x = 0; x < cols; ++x) {
      if (!touches_invalid(valid, rows, cols, window, x, y)) continue;
      const size_t i = (size_t)y * cols + x;
      if (idx) idx[i] = -1;
      if (depth) depth[i] = 0.0f;
      if (score) score[i] = 0.0f;
    }
}

}  // namespace host
#endif  // !__HIPCC__

}  // namespace sfmund
