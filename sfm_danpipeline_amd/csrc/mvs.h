// mvs.h -- dense multi-view stereo (map3D step 7): plane-sweep depth maps, then cross-view consistency fusion.
// The arithmetic of DESIGN.md f-10, shared by the HIP kernels (mvs.hip) and by a g++ build (tests/stub/mvs_capi.cpp);
// compiled without floating-point contraction on both sides.  Window sums are integers, every f64 step is written out
// in one order, so the device equals the host build bit for bit.  Parity with pmvs2 is UNPINNED (no patch expansion).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#ifndef __HIPCC__
#include <algorithm>
#include <thread>
#endif
#include <vector>

#if defined(__HIPCC__)
#define MVS_HD __host__ __device__ __forceinline__
#else
#define MVS_HD inline
#endif

namespace sfmmvs {

constexpr int MIN_PLANES = 3, MAX_PLANES = 256;
constexpr int MAX_WINDOW = 7;  // (2w+1)^2 * 4080^2 < 2^32 holds up to 2w+1 = 16: every window sum fits u32
constexpr int MAX_SRC = 8, MAX_BEST = 4;
constexpr int TILE = 16, TILE_MAX = TILE + 2 * MAX_WINDOW;
constexpr int INVALID = 0xFFFF;  // a 12-bit sample (0 ... 4080) that does not exist, in the u16 tiles

struct Opts {
  int n_planes, window, n_src, n_best, min_views;
  double ncc_min, eps, var_min;
};
// var_min: N * sum r^2 - (sum r)^2 of a window whose gray values have standard deviation 1 at w = 3 (49^2 * 16^2)
inline Opts default_opts() { return Opts{128, 3, 4, 2, 3, 0.7, 0.01, 614656.0}; }
inline bool opts_valid(const Opts& o) {
  return o.n_planes >= MIN_PLANES && o.n_planes <= MAX_PLANES && o.window >= 1 && o.window <= MAX_WINDOW && o.n_src >= 1 &&
         o.n_src <= MAX_SRC && o.n_best >= 1 && o.n_best <= MAX_BEST && o.min_views >= 1 && o.ncc_min >= -1.0 && o.ncc_min <= 1.0 &&
         o.eps >= 0.0 && o.eps < 1.0 && o.var_min >= 0.0;
}

struct Cam {  // K at the working level
  double fx, fy, cx, cy;
};

// rule 1: one 2x2 box mean
MVS_HD uint8_t box4(int a, int b, int c, int d) { return (uint8_t)((a + b + c + d + 2) >> 2); }
// K one level down: pixel centre x of the half image lies at 2x + 0.5 of the full one
inline Cam halve_cam(const Cam& k) { return Cam{k.fx * 0.5, k.fy * 0.5, (k.cx + 0.5) * 0.5 - 0.5, (k.cy + 0.5) * 0.5 - 0.5}; }

// rule 2: inverse depth of plane k; index 0 is the far plane
MVS_HD double plane_inv(double inv_far, double step, double k) { return inv_far + k * step; }
inline void plane_range(double dmin, double dmax, int D, double* inv_far, double* step) {
  *inv_far = 1.0 / dmax;
  *step = (1.0 / dmin - 1.0 / dmax) / (double)(D - 1);
}

// rule 3: the 12-bit sample of img at H * (x, y, 1), -1 when it does not exist
MVS_HD int warp_sample(const uint8_t* img, int rows, int cols, const double* H, int x, int y) {
  const double xd = (double)x, yd = (double)y;
  const double a = (H[0] * xd + H[1] * yd) + H[2];
  const double b = (H[3] * xd + H[4] * yd) + H[5];
  const double c = (H[6] * xd + H[7] * yd) + H[8];
  if (!(c > 0.0)) return -1;  // behind the source camera
  const double u = a / c, v = b / c;
  if (!(u >= 0.0 && v >= 0.0 && u < (double)cols && v < (double)rows)) return -1;
  const double fu = floor(u), fv = floor(v);
  int ix = (int)fu, iy = (int)fv;
  int wx = (int)floor((u - fu) * 32.0 + 0.5), wy = (int)floor((v - fv) * 32.0 + 0.5);
  if (wx == 32) wx = 0, ++ix;
  if (wy == 32) wy = 0, ++iy;
  if (ix + 1 >= cols || iy + 1 >= rows) return -1;
  const uint8_t* p = img + (size_t)iy * cols + ix;
  const int top = (int)p[0] * (32 - wx) + (int)p[1] * wx;
  const int bot = (int)p[cols] * (32 - wx) + (int)p[cols + 1] * wx;
  return (top * (32 - wy) + bot * wy + 32) >> 6;  // /1024 * 16, rounded: 8.4 fixed point
}

// rule 4: the variance term of a window, and the NCC of two windows
MVS_HD int64_t var_term(int N, uint32_t s, uint32_t ss) { return (int64_t)N * (int64_t)ss - (int64_t)s * (int64_t)s; }
MVS_HD bool ncc(int N, uint32_t sr, int64_t vr, uint32_t sq, uint32_t sqq, uint32_t srq, double* out) {
  const int64_t vq = var_term(N, sq, sqq);
  if (vq <= 0 || vr <= 0) return false;
  const int64_t num = (int64_t)N * (int64_t)srq - (int64_t)sr * (int64_t)sq;
  *out = (double)num / sqrt((double)vr * (double)vq);
  return true;
}

// the n_best largest values seen, in descending order
struct Top {
  double v[MAX_BEST];
  int n;
  MVS_HD void clear() {
    for (int i = 0; i < MAX_BEST; ++i) v[i] = -4.0;
    n = 0;
  }
  MVS_HD void add(double x) {
    double c = x;
#pragma unroll
    for (int i = 0; i < MAX_BEST; ++i)
      if (c > v[i]) {
        const double t = v[i];
        v[i] = c;
        c = t;
      }
    ++n;
  }
  MVS_HD bool score(int nb, double* s) const {
    if (n < nb) return false;
    double a = v[0];
#pragma unroll
    for (int i = 1; i < MAX_BEST; ++i)
      if (i < nb) a = a + v[i];
    *s = a / (double)nb;
    return true;
  }
};

// rule 5: the running winner over the planes, with the scores on both sides of it
struct Winner {
  double best, prev, bprev, bnext;
  int bk;
  bool prev_ok, bprev_ok, bnext_ok;
  MVS_HD void clear() {
    best = prev = bprev = bnext = 0.0;
    bk = -1;
    prev_ok = bprev_ok = bnext_ok = false;
  }
  MVS_HD void step(int k, bool ok, double s) {
    if (bk >= 0 && k == bk + 1) bnext = s, bnext_ok = ok;
    if (ok && (bk < 0 || s > best)) best = s, bk = k, bprev = prev, bprev_ok = prev_ok, bnext_ok = false;
    prev = s, prev_ok = ok;
  }
  MVS_HD void finish(int D, double inv_far, double step, double ncc_min, int32_t* idx, float* depth, float* score) const {
    if (bk < 0 || !(best >= ncc_min)) {
      *idx = -1, *depth = 0.0f, *score = 0.0f;
      return;
    }
    double off = 0.0;
    if (bk > 0 && bk < D - 1 && bprev_ok && bnext_ok) {
      const double den = (bprev - 2.0 * best) + bnext;
      if (den < 0.0) off = 0.5 * (bprev - bnext) / den;
      if (off > 0.5) off = 0.5;
      if (off < -0.5) off = -0.5;
    }
    *idx = bk;
    *depth = (float)(1.0 / plane_inv(inv_far, step, (double)bk + off));
    *score = (float)best;
  }
};

// rule 7: pixel (x, y) of view r against every other view's depth map.  poses: [R | t] row-major 3x4 per view (x_cam = R X + t).
MVS_HD bool fuse_pixel(int r, int x, int y, int n_views, int rows, int cols, const Cam K, const double* poses, const float* depth,
                       double eps, int min_views, float* xyz, float* nrm) {
  const size_t px = (size_t)rows * cols;
  const double z = (double)depth[(size_t)r * px + (size_t)y * cols + x];
  if (!(z > 0.0)) return false;
  const double* P = poses + 12 * r;
  const double a = ((double)x - K.cx) / K.fx * z - P[3], b = ((double)y - K.cy) / K.fy * z - P[7], c = z - P[11];
  const double X = (P[0] * a + P[4] * b) + P[8] * c, Y = (P[1] * a + P[5] * b) + P[9] * c, Z = (P[2] * a + P[6] * b) + P[10] * c;
  int count = 1;
  bool owner = true;
  for (int v = 0; v < n_views; ++v) {
    if (v == r) continue;
    const double* Q = poses + 12 * v;
    const double zi = ((Q[8] * X + Q[9] * Y) + Q[10] * Z) + Q[11];
    if (!(zi > 0.0)) continue;
    const double xi = ((Q[0] * X + Q[1] * Y) + Q[2] * Z) + Q[3], yi = ((Q[4] * X + Q[5] * Y) + Q[6] * Z) + Q[7];
    const double pu = floor((K.fx * (xi / zi) + K.cx) + 0.5), pv = floor((K.fy * (yi / zi) + K.cy) + 0.5);
    if (!(pu >= 0.0 && pv >= 0.0 && pu < (double)cols && pv < (double)rows)) continue;
    const double zv = (double)depth[(size_t)v * px + (size_t)(int)pv * cols + (int)pu];
    if (zv > 0.0 && fabs(zv - zi) <= eps * zi) {
      ++count;
      if (v < r) owner = false;
    }
  }
  if (count < min_views || !owner) return false;
  xyz[0] = (float)X, xyz[1] = (float)Y, xyz[2] = (float)Z;
  // the unit vector from X to the centre of r, C = -R^T t
  const double dx = -((P[0] * P[3] + P[4] * P[7]) + P[8] * P[11]) - X, dy = -((P[1] * P[3] + P[5] * P[7]) + P[9] * P[11]) - Y,
               dz = -((P[2] * P[3] + P[6] * P[7]) + P[10] * P[11]) - Z;
  const double len = sqrt((dx * dx + dy * dy) + dz * dz);
  nrm[0] = len > 0.0 ? (float)(dx / len) : 0.0f, nrm[1] = len > 0.0 ? (float)(dy / len) : 0.0f, nrm[2] = len > 0.0 ? (float)(dz / len) : 0.0f;
  return true;
}

MVS_HD uint32_t pack_rgb(const uint8_t* gray, const uint8_t* bgr, size_t i) {
  if (bgr) return ((uint32_t)bgr[3 * i + 2] << 16) | ((uint32_t)bgr[3 * i + 1] << 8) | (uint32_t)bgr[3 * i];
  return (uint32_t)gray[i] * 0x010101u;
}

// ------------------------------------------------------------------------------------------------ host only
// rule 2: H[k][s] (9 doubles each), reference pixel -> pixel of source s on plane k
inline void make_homographies(const Cam& K, const double* poses, int ref, int n_src, const int32_t* src, int D, double inv_far,
                              double step, std::vector<double>& H) {
  H.assign((size_t)D * n_src * 9, 0.0);
  const double* Pr = poses + 12 * ref;
  for (int s = 0; s < n_src; ++s) {
    const double* Ps = poses + 12 * src[s];
    double R[9], t[3];  // Rs Rr^T, ts - (Rs Rr^T) tr
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) R[3 * i + j] = (Ps[4 * i] * Pr[4 * j] + Ps[4 * i + 1] * Pr[4 * j + 1]) + Ps[4 * i + 2] * Pr[4 * j + 2];
    for (int i = 0; i < 3; ++i) t[i] = Ps[4 * i + 3] - ((R[3 * i] * Pr[3] + R[3 * i + 1] * Pr[7]) + R[3 * i + 2] * Pr[11]);
    for (int k = 0; k < D; ++k) {
      const double inv = plane_inv(inv_far, step, (double)k);
      double M[9], A[9];
      for (int i = 0; i < 9; ++i) M[i] = R[i];
      for (int i = 0; i < 3; ++i) M[3 * i + 2] = R[3 * i + 2] + t[i] * inv;
      for (int j = 0; j < 3; ++j) {
        A[j] = K.fx * M[j] + K.cx * M[6 + j];
        A[3 + j] = K.fy * M[3 + j] + K.cy * M[6 + j];
        A[6 + j] = M[6 + j];
      }
      double* h = &H[((size_t)k * n_src + s) * 9];
      for (int i = 0; i < 3; ++i) {
        h[3 * i] = A[3 * i] / K.fx;
        h[3 * i + 1] = A[3 * i + 1] / K.fy;
        h[3 * i + 2] = (A[3 * i + 2] - h[3 * i] * K.cx) - h[3 * i + 1] * K.cy;
      }
    }
  }
}

// rule 6: the n_src nearest camera centres, ties by lower index; returns how many there are
inline int choose_sources(const double* poses, int n_views, int ref, int n_src, int32_t* src) {
  double C[3 * 64];
  std::vector<double> big;
  double* c = C;
  if (n_views > 64) big.resize(3 * (size_t)n_views), c = big.data();
  for (int v = 0; v < n_views; ++v) {
    const double* P = poses + 12 * v;
    for (int a = 0; a < 3; ++a) c[3 * v + a] = -((P[a] * P[3] + P[4 + a] * P[7]) + P[8 + a] * P[11]);
  }
  int n = 0;
  std::vector<char> used((size_t)n_views, 0);
  used[ref] = 1;
  for (; n < n_src && n < n_views - 1; ++n) {
    int best = -1;
    double bd = 0.0;
    for (int v = 0; v < n_views; ++v) {
      if (used[v]) continue;
      const double dx = c[3 * v] - c[3 * ref], dy = c[3 * v + 1] - c[3 * ref + 1], dz = c[3 * v + 2] - c[3 * ref + 2];
      const double d = (dx * dx + dy * dy) + dz * dz;
      if (best < 0 || d < bd) best = v, bd = d;
    }
    used[best] = 1;
    src[n] = best;
  }
  return n;
}

inline bool depthmap_args_ok(int n_views, int ref, int n_src, const int32_t* src, double dmin, double dmax, const Opts& o) {
  if (!opts_valid(o) || ref < 0 || ref >= n_views || n_src < 1 || n_src > MAX_SRC || !src) return false;
  if (!(dmin > 0.0) || !(dmin < dmax) || !(dmax < INFINITY)) return false;
  for (int s = 0; s < n_src; ++s) {
    if (src[s] < 0 || src[s] >= n_views || src[s] == ref) return false;
    for (int q = 0; q < s; ++q)
      if (src[q] == src[s]) return false;
  }
  return true;
}

#ifndef __HIPCC__
namespace host {

struct Scene {
  int n = 0, rows = 0, cols = 0;
  Cam K{};
  bool colour = false;
  std::vector<double> poses;
  std::vector<uint8_t> gray, bgr;
  std::vector<float> depth;
  std::vector<float> xyz, nrm;
  std::vector<uint32_t> rgb;
};

inline void halve(const std::vector<uint8_t>& in, int rows, int cols, int ch, std::vector<uint8_t>& out) {
  const int r2 = rows >> 1, c2 = cols >> 1;
  out.assign((size_t)r2 * c2 * ch, 0);
  for (int y = 0; y < r2; ++y)
    for (int x = 0; x < c2; ++x)
      for (int c = 0; c < ch; ++c) {
        const uint8_t* p = &in[((size_t)(2 * y) * cols + 2 * x) * ch + c];
        out[((size_t)y * c2 + x) * ch + c] = box4(p[0], p[ch], p[(size_t)cols * ch], p[(size_t)cols * ch + ch]);
      }
}

// false: the arguments are refused (the library's SFMHIP_ERR_ARG)
inline bool build(Scene& S, int n_views, int rows, int cols, const uint8_t* const* gray, const uint8_t* const* bgr, const double* K9,
                  const double* poses12, int level) {
  if (n_views < 2 || rows < 1 || cols < 1 || !gray || !K9 || !poses12 || level < 0 || level > 8) return false;
  if ((rows >> level) < 1 || (cols >> level) < 1) return false;
  S.n = n_views;
  S.colour = bgr != nullptr;
  S.K = Cam{K9[0], K9[4], K9[2], K9[5]};
  for (int l = 0; l < level; ++l) S.K = halve_cam(S.K);
  S.rows = rows >> level, S.cols = cols >> level;
  S.poses.assign(poses12, poses12 + 12 * (size_t)n_views);
  const size_t px = (size_t)S.rows * S.cols;
  S.gray.assign(px * n_views, 0);
  S.bgr.assign(S.colour ? 3 * px * n_views : 0, 0);
  S.depth.assign(px * n_views, 0.0f);
  for (int v = 0; v < n_views; ++v)
    for (int ch = 1; ch <= (S.colour ? 3 : 1); ch += 2) {
      const uint8_t* in = ch == 1 ? gray[v] : bgr[v];
      std::vector<uint8_t> a(in, in + (size_t)rows * cols * ch), b;
      int r = rows, c = cols;
      for (int l = 0; l < level; ++l, r >>= 1, c >>= 1) {
        halve(a, r, c, ch, b);
        a.swap(b);
      }
      memcpy(ch == 1 ? &S.gray[px * v] : &S.bgr[3 * px * v], a.data(), px * ch);
    }
  return true;
}

// rules 2-5 for one reference view, rows [y0, y1): separable integer box sums (equal to the plain double loop, being integers)
inline void depthmap_band(const Scene& S, int ref, int n_src, const int32_t* src, const std::vector<double>& H, double inv_far, double step,
                          const Opts& o, int y0, int y1, int32_t* idx, float* depth, float* score) {
  const int rows = S.rows, cols = S.cols, w = o.window, N = (2 * w + 1) * (2 * w + 1), D = o.n_planes;
  const size_t px = (size_t)rows * cols;
  const uint8_t* I = &S.gray[px * ref];
  const int ya = std::max(0, y0 - w), yb = std::min(rows, y1 + w), nb = yb - ya;
  const size_t bp = (size_t)(y1 - y0) * cols;
  std::vector<uint16_t> q((size_t)nb * cols);
  std::vector<uint32_t> hq((size_t)nb * cols), hqq((size_t)nb * cols), hrq((size_t)nb * cols);
  std::vector<uint16_t> hbad((size_t)nb * cols);
  std::vector<uint32_t> sr(bp, 0);
  std::vector<int64_t> vr(bp, 0);
  std::vector<char> rok(bp, 0);
  std::vector<Winner> win(bp);
  std::vector<Top> top(bp);
  for (auto& x : win) x.clear();
  for (int y = std::max(y0, w); y < std::min(y1, rows - w); ++y)
    for (int x = w; x < cols - w; ++x) {
      uint32_t s = 0, ss = 0;
      for (int dy = -w; dy <= w; ++dy)
        for (int dx = -w; dx <= w; ++dx) {
          const uint32_t r = 16u * I[(size_t)(y + dy) * cols + x + dx];
          s += r, ss += r * r;
        }
      const size_t i = (size_t)(y - y0) * cols + x;
      sr[i] = s, vr[i] = var_term(N, s, ss);
      rok[i] = vr[i] > 0 && (double)vr[i] >= o.var_min;
    }
  for (int k = 0; k < D; ++k) {
    for (auto& t : top) t.clear();
    for (int s = 0; s < n_src; ++s) {
      const uint8_t* J = &S.gray[px * src[s]];
      const double* h = &H[((size_t)k * n_src + s) * 9];
      for (int y = ya; y < yb; ++y)
        for (int x = 0; x < cols; ++x) {
          const int v = warp_sample(J, rows, cols, h, x, y);
          q[(size_t)(y - ya) * cols + x] = (uint16_t)(v < 0 ? INVALID : v);
        }
      for (int y = ya; y < yb; ++y)
        for (int x = w; x < cols - w; ++x) {
          uint32_t a = 0, b = 0, c = 0, bad = 0;
          for (int dx = -w; dx <= w; ++dx) {
            const uint32_t v = q[(size_t)(y - ya) * cols + x + dx], r = 16u * I[(size_t)y * cols + x + dx];
            if (v == (uint32_t)INVALID) ++bad;
            else a += v, b += v * v, c += r * v;
          }
          const size_t i = (size_t)(y - ya) * cols + x;
          hq[i] = a, hqq[i] = b, hrq[i] = c, hbad[i] = (uint16_t)bad;
        }
      for (int y = std::max(y0, w); y < std::min(y1, rows - w); ++y)
        for (int x = w; x < cols - w; ++x) {
          const size_t i = (size_t)(y - y0) * cols + x;
          if (!rok[i]) continue;
          uint32_t a = 0, b = 0, c = 0, bad = 0;
          for (int dy = -w; dy <= w; ++dy) {
            const size_t j = (size_t)(y + dy - ya) * cols + x;
            a += hq[j], b += hqq[j], c += hrq[j], bad += hbad[j];
          }
          double v;
          if (bad == 0 && ncc(N, sr[i], vr[i], a, b, c, &v)) top[i].add(v);
        }
    }
    for (size_t i = 0; i < bp; ++i) {
      double sc = 0.0;
      const bool ok = rok[i] && top[i].score(o.n_best, &sc);
      win[i].step(k, ok, sc);
    }
  }
  for (size_t i = 0; i < bp; ++i) {
    int32_t a;
    float d, sc;
    win[i].finish(D, inv_far, step, o.ncc_min, &a, &d, &sc);
    const size_t g = (size_t)y0 * cols + i;
    if (idx) idx[g] = a;
    if (score) score[g] = sc;
    depth[g] = d;
  }
}

// the depth map of view ref into the scene (and into idx / depth / score where given)
inline bool depthmap(Scene& S, int ref, int n_src, const int32_t* src, double dmin, double dmax, const Opts& o, int32_t* idx, float* depth,
                     float* score, int threads) {
  if (!depthmap_args_ok(S.n, ref, n_src, src, dmin, dmax, o)) return false;
  double inv_far, step;
  plane_range(dmin, dmax, o.n_planes, &inv_far, &step);
  std::vector<double> H;
  make_homographies(S.K, S.poses.data(), ref, n_src, src, o.n_planes, inv_far, step, H);
  const size_t px = (size_t)S.rows * S.cols;
  float* out = &S.depth[px * ref];
  threads = std::max(1, std::min(threads, (S.rows + 7) / 8));
  std::vector<std::thread> th;
  for (int t = 0; t < threads; ++t) {
    const int y0 = (int)((long long)S.rows * t / threads), y1 = (int)((long long)S.rows * (t + 1) / threads);
    th.emplace_back([&, y0, y1] { depthmap_band(S, ref, n_src, src, H, inv_far, step, o, y0, y1, idx, out, score); });
  }
  for (auto& t : th) t.join();
  if (depth) memcpy(depth, out, px * sizeof(float));
  return true;
}

// rule 7 over the depth maps the scene holds; returns the points
inline int fuse(Scene& S, const Opts& o) {
  S.xyz.clear(), S.nrm.clear(), S.rgb.clear();
  const size_t px = (size_t)S.rows * S.cols;
  for (int r = 0; r < S.n; ++r)
    for (int y = 0; y < S.rows; ++y)
      for (int x = 0; x < S.cols; ++x) {
        float p[3], n[3];
        if (!fuse_pixel(r, x, y, S.n, S.rows, S.cols, S.K, S.poses.data(), S.depth.data(), o.eps, o.min_views, p, n)) continue;
        S.xyz.insert(S.xyz.end(), p, p + 3);
        S.nrm.insert(S.nrm.end(), n, n + 3);
        S.rgb.push_back(pack_rgb(S.gray.data(), S.colour ? S.bgr.data() : nullptr, px * r + (size_t)y * S.cols + x));
      }
  return (int)S.rgb.size();
}

// rule 6, every depth map, rule 7; -1: arguments refused
inline int run(Scene& S, const double* dmin, const double* dmax, const Opts& o, int threads) {
  if (!opts_valid(o) || !dmin || !dmax) return -1;
  for (int v = 0; v < S.n; ++v)
    if (!(dmin[v] > 0.0) || !(dmin[v] < dmax[v]) || !(dmax[v] < INFINITY)) return -1;
  for (int v = 0; v < S.n; ++v) {
    int32_t src[MAX_SRC];
    const int n = choose_sources(S.poses.data(), S.n, v, o.n_src, src);
    if (!depthmap(S, v, n, src, dmin[v], dmax[v], o, nullptr, nullptr, nullptr, threads)) return -1;
  }
  return fuse(S, o);
}

}  // namespace host
#endif  // !__HIPCC__

}  // namespace sfmmvs
