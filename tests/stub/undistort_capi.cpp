// C entry points over sfm_danpipeline_amd/csrc/undistort.h for the CPU tests (tests/test_undistort_cpu.py) and for the GPU
// tests' bit-for-bit comparison: the g++ build of the header the device code is compiled from.
// -DUND_MAIN: a stand-alone driver for the sanitizer run (its pictures come from a fixed generator).
#include "../../sfm_danpipeline_amd/csrc/undistort.h"
#include <cstdio>
#include <utility>

using namespace sfmund;

extern "C" {

// rule 1 for one destination pixel
void und_distort_pixel(const double* K9, const double* dist5, int x, int y, double* uv) { distort_pixel(K9, dist5, x, y, &uv[0], &uv[1]); }

// rules 2-3 for one position: out5 = ix, iy, wx, wy, valid
void und_quantise(double u, double v, int rows, int cols, int32_t* out5) {
  const Tap t = quantise(u, v, rows, cols);
  out5[0] = t.ix, out5[1] = t.iy, out5[2] = t.wx, out5[3] = t.wy, out5[4] = t.valid;
}

// rules 2-4: channel c of a rows x cols x ch picture at (u, v); -1: invalid
int und_sample(const uint8_t* img, int rows, int cols, int ch, int c, double u, double v) {
  const Tap t = quantise(u, v, rows, cols);
  return t.valid ? (int)blend(img, cols, ch, c, pack(t, cols)) : -1;
}

// rules 1-5; -3 (the library's SFMHIP_ERR_ARG) for refused arguments
int und_undistort(int n, int rows, int cols, int ch, const uint8_t* const* src, const double* K9, const double* dist5, uint8_t* const* dst,
                  uint8_t* valid) {
  return host::undistort(n, rows, cols, ch, src, K9, dist5, dst, valid) ? 0 : -3;
}

// rule 6: out is (rows >> level) x (cols >> level)
void und_level_mask(const uint8_t* valid0, int rows, int cols, int level, uint8_t* out) { host::level_mask(valid0, rows, cols, level, out); }

// rule 7 on one depth map of the mask's size
void und_seam(const uint8_t* valid, int rows, int cols, int window, int32_t* idx, float* depth, float* score) {
  host::seam(valid, rows, cols, window, idx, depth, score);
}

}  // extern "C"

#ifdef UND_MAIN
int main() {
  const double K[9] = {61.3, 0, 25.7, 0, 59.9, 18.1, 0, 0, 1};
  const double sets[4][5] = {{-0.25, 0.08, 0.002, -0.0015, 0}, {0.2, -0.05, -0.002, 0.001, 0.01}, {0, 0, 0.05, -0.04, 0}, {0, 0, 0, 0, 0}};
  uint32_t seed = 12345u;
  long sum = 0;
  for (int ch : {1, 3})
    for (const auto& size : {std::pair<int, int>{9, 11}, {37, 53}, {1, 1}, {2, 64}})
      for (const auto& d : sets) {
        const int rows = size.first, cols = size.second, n = 3;
        const size_t bytes = (size_t)rows * cols * ch;
        std::vector<std::vector<uint8_t>> in(n, std::vector<uint8_t>(bytes)), out(n, std::vector<uint8_t>(bytes));
        std::vector<const uint8_t*> ip;
        std::vector<uint8_t*> op;
        for (int i = 0; i < n; ++i) {
          for (auto& b : in[i]) b = (uint8_t)((seed = seed * 1664525u + 1013904223u) >> 24);
          ip.push_back(in[i].data()), op.push_back(out[i].data());
        }
        std::vector<uint8_t> valid((size_t)rows * cols);
        if (und_undistort(n, rows, cols, ch, ip.data(), K, d, op.data(), valid.data())) return 1;
        for (int level = 0; level <= 2; ++level) {
          const int r = rows >> level, c = cols >> level;
          if (r < 1 || c < 1) continue;
          std::vector<uint8_t> m((size_t)r * c);
          und_level_mask(valid.data(), rows, cols, level, m.data());
          std::vector<int32_t> idx((size_t)r * c, 5);
          std::vector<float> depth((size_t)r * c, 1.0f), score((size_t)r * c, 1.0f);
          for (int w : {1, 3, 7}) und_seam(m.data(), r, c, w, idx.data(), depth.data(), score.data());
          for (int32_t a : idx) sum += a;
        }
        for (uint8_t b : out[n - 1]) sum += b;
      }
  // the corners of rules 2-3: far outside, non-finite, the last row and column, the carry at both borders
  const uint8_t img[6] = {1, 2, 3, 4, 5, 6};
  for (double u : {-1e300, -1.0, -1e-15, 0.0, 1.0, 2.0 - 1e-15, 2.0, 2.5, 3.0, 1e300, (double)NAN, (double)INFINITY})
    for (double v : {-1e300, -1e-15, 0.0, 1.0 - 1e-15, 1.0, 1.5, 2.0, (double)NAN}) sum += und_sample(img, 2, 3, 1, 0, u, v);
  std::printf("checksum %ld\n", sum);
  return 0;
}
#endif
