// cloud_filter_capi.cpp -- a C surface over csrc/cloud_filter.h for tests/test_cloud_filter_cpu.py and
// tests/test_gpu_cloud_filter.py (built with g++ -O2 -ffp-contract=off -pthread) and, with -DCLOUD_FILTER_MAIN, a
// stand-alone driver that runs both filters on clouds of its own under the sanitizers.  The sort, the run walk and the
// neighbour search here are the CPU's own (std::stable_sort, a hash grid with a brute-force fallback), independent of
// cloud_filter.hip's; only the arithmetic and the rules come from the header.  Status codes are include/sfmhip.h's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/cloud_filter.h"

namespace {

constexpr int OK = 0, ERR_ARG = -3, ERR_UNSUPPORTED = -5;

struct HashGrid {
  double cell = 1;
  std::unordered_map<long long, std::vector<int>> cells;
  static long long pack(long long x, long long y, long long z) {
    return ((x + (1ll << 20)) << 42) | ((y + (1ll << 20)) << 21) | (z + (1ll << 20));
  }
  static long long coord(float v, double cell) {
    double f = std::floor((double)v / cell);
    f = std::max(-(double)(1 << 20) + 1, std::min((double)(1 << 20) - 1, f));  // (clamped: a far point joins a border cell)
    return (long long)f;
  }
  void build(int n, const float* xyz, double c) {
    cell = c;
    cells.clear();
    for (int i = 0; i < n; ++i) {
      const float* p = xyz + 3 * (size_t)i;
      if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
      cells[pack(coord(p[0], c), coord(p[1], c), coord(p[2], c))].push_back(i);
    }
  }
  const std::vector<int>* at(long long x, long long y, long long z) const {
    auto it = cells.find(pack(x, y, z));
    return it == cells.end() ? nullptr : &it->second;
  }
};

template <typename F>
void parallel(int n, F f) {
  const int T = n < 4096 ? 1 : 16;
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      for (int i = t; i < n; i += T) f(i);
    });
  for (auto& x : th) x.join();
}

// the box of the finite points as floats; returns their count
int box(int n, const float* xyz, float mn[3], float mx[3]) {
  int nv = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
    for (int a = 0; a < 3; ++a) {
      mn[a] = nv ? std::min(mn[a], p[a]) : p[a];
      mx[a] = nv ? std::max(mx[a], p[a]) : p[a];
    }
    ++nv;
  }
  if (!nv)
    for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0f;
  return nv;
}

int plan_status(int pr) { return pr == sfmfilter::PLAN_ARG ? ERR_ARG : pr == sfmfilter::PLAN_UNSUPPORTED ? ERR_UNSUPPORTED : OK; }

template <int C>
struct Reader {  // V5's get(j, v) over the sorted order of one run
  const float* xyz;
  const float* nrm;
  const int* order;
  void operator()(int j, float* v) const {
    const size_t i = (size_t)order[j];
    v[0] = xyz[3 * i], v[1] = xyz[3 * i + 1], v[2] = xyz[3 * i + 2];
    if (C == 6) v[3] = nrm[3 * i], v[4] = nrm[3 * i + 1], v[5] = nrm[3 * i + 2];
  }
};

// S1: the mean_k + 1 smallest d2 of every finite point, ascending: rings of a hash grid until the last one is below the
// searched block's inner radius (with a margin), brute force over all points after 24 rings
void nearest_d2(int n, int nv, const float* xyz, int K, std::vector<float>& out /* n K */) {
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], (double)p[a]);
      hi[a] = std::max(hi[a], (double)p[a]);
    }
  }
  double ext = 0;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, nv ? hi[a] - lo[a] : 0.0);
  HashGrid g;
  g.build(n, xyz, ext > 0 ? ext / std::max(1.0, std::cbrt(nv / 8.0)) : 1.0);
  out.assign((size_t)n * K, 0.0f);
  parallel(n, [&](int i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) return;
    std::vector<float> c;
    const long long cx = HashGrid::coord(p[0], g.cell), cy = HashGrid::coord(p[1], g.cell), cz = HashGrid::coord(p[2], g.cell);
    bool brute = true;
    for (long long R = 0; R <= 24; ++R) {
      for (long long z = cz - R; z <= cz + R; ++z)
        for (long long y = cy - R; y <= cy + R; ++y)
          for (long long x = cx - R; x <= cx + R; ++x) {
            if (std::max(std::max(std::llabs(x - cx), std::llabs(y - cy)), std::llabs(z - cz)) != R) continue;
            const std::vector<int>* v = g.at(x, y, z);
            if (!v) continue;
            for (int j : *v) {
              const float* q = xyz + 3 * (size_t)j;
              c.push_back(sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]));
            }
          }
      if ((int)c.size() >= K) {
        std::nth_element(c.begin(), c.begin() + (K - 1), c.end());
        const double inner = R * g.cell * (1.0 - 1e-4);
        if ((double)c[K - 1] < inner * inner) {
          brute = false;
          break;
        }
      }
    }
    if (brute) {
      c.clear();
      for (int j = 0; j < n; ++j) {
        const float* q = xyz + 3 * (size_t)j;
        if (sfmcloud::finite3(q[0], q[1], q[2])) c.push_back(sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]));
      }
    }
    std::partial_sort(c.begin(), c.begin() + K, c.end());
    for (int s = 0; s < K; ++s) out[(size_t)i * K + s] = c[s];
  });
}

}  // namespace

extern "C" {

// V1-V3: keys[i] = the voxel index of point i, -1 for a non-finite point; div3 = the grid's extents
int cf_voxel_keys(int n, const float* xyz, const float* leaf, int32_t* keys, int32_t* div3) {
  float mn[3], mx[3];
  const int nv = box(n, xyz, mn, mx);
  sfmfilter::VoxelPlan p;
  const int rc = plan_status(sfmfilter::voxel_plan(leaf, mn, mx, p));
  if (rc != OK) return rc;
  for (int a = 0; a < 3; ++a) div3[a] = nv ? p.div[a] : 0;
  for (int i = 0; i < n; ++i) {
    const float* q = xyz + 3 * (size_t)i;
    keys[i] = sfmcloud::finite3(q[0], q[1], q[2]) ? sfmfilter::voxel_key(p, q[0], q[1], q[2]) : -1;
  }
  return OK;
}

// sfmhip_cloud_voxel_grid without the handle: rgb / normals / out_* / voxel_of may be NULL
int cf_voxel_grid(int n, const float* xyz, const float* leaf, int min_points, const uint32_t* rgb, const float* normals,
                  float* out_xyz, uint32_t* out_rgb, float* out_normals, int32_t* voxel_of, int32_t* n_out) {
  if (n < 0 || !leaf || !n_out || min_points < 0) return ERR_ARG;
  float mn[3], mx[3];
  const int nv = box(n, xyz, mn, mx);
  sfmfilter::VoxelPlan p;
  const int rc = plan_status(sfmfilter::voxel_plan(leaf, mn, mx, p));
  if (rc != OK) return rc;
  std::vector<int> key((size_t)n), order;
  order.reserve((size_t)nv);
  for (int i = 0; i < n; ++i) {
    const float* q = xyz + 3 * (size_t)i;
    if (voxel_of) voxel_of[i] = -1;
    if (!sfmcloud::finite3(q[0], q[1], q[2])) continue;
    key[i] = sfmfilter::voxel_key(p, q[0], q[1], q[2]);
    order.push_back(i);
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return key[a] < key[b]; });
  int m = 0;
  for (size_t s = 0; s < order.size();) {
    size_t e = s;
    while (e < order.size() && key[order[e]] == key[order[s]]) ++e;
    const int cnt = (int)(e - s);
    if (cnt >= min_points) {
      float t[6] = {0, 0, 0, 0, 0, 0};
      if (normals) {
        sfmfilter::run_sum<6>(cnt, Reader<6>{xyz, normals, &order[s]}, t);
      } else {
        float t3[3];
        sfmfilter::run_sum<3>(cnt, Reader<3>{xyz, nullptr, &order[s]}, t3);
        for (int a = 0; a < 3; ++a) t[a] = t3[a];
      }
      for (int a = 0; a < 3 && out_xyz; ++a) out_xyz[3 * (size_t)m + a] = sfmfilter::centroid(t[a], cnt);
      if (rgb && out_rgb) {
        uint64_t cs[3] = {0, 0, 0};
        for (size_t j = s; j < e; ++j) sfmfilter::rgb_add(cs, rgb[order[j]]);
        out_rgb[m] = sfmfilter::rgb_mean(cs, cnt);
      }
      if (normals && out_normals) sfmfilter::normal_mean(t + 3, out_normals + 3 * (size_t)m);
      for (size_t j = s; j < e && voxel_of; ++j) voxel_of[order[j]] = m;
      ++m;
    }
    s = e;
  }
  *n_out = m;
  return OK;
}

// sfmhip_cloud_statistical_outlier without the handle: mean_dist / threshold may be NULL
int cf_statistical_outlier(int n, const float* xyz, int mean_k, double std_mul, int negative, int32_t* idx_out, int32_t* n_out,
                           float* mean_dist, double* threshold) {
  if (n < 0 || mean_k < 1 || mean_k > sfmfilter::MEAN_K_MAX || !(std_mul - std_mul == 0.0) || !n_out) return ERR_ARG;
  int nv = 0;
  for (int i = 0; i < n; ++i) nv += sfmcloud::finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]) ? 1 : 0;
  if (nv > 0 && nv <= mean_k) return ERR_ARG;
  *n_out = 0;
  if (threshold) *threshold = 0.0;
  std::vector<float> md((size_t)n + 1, 0.0f);
  if (nv > 0) {
    const int K = mean_k + 1;
    std::vector<float> d2;
    nearest_d2(n, nv, xyz, K, d2);
    for (int i = 0; i < n; ++i) {
      if (!sfmcloud::finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2])) continue;
      double sum = 0.0;
      for (int k = 1; k <= mean_k; ++k) sum += sfmfilter::dist_term(d2[(size_t)i * K + k]);
      md[i] = sfmfilter::mean_dist(sum, mean_k);
    }
    const long long n_part = (n + (long long)sfmfilter::SUM_BLOCK - 1) / sfmfilter::SUM_BLOCK;
    std::vector<double> part((size_t)2 * n_part);
    for (long long b = 0; b < n_part; ++b)
      sfmfilter::stat_partial(md.data(), b * sfmfilter::SUM_BLOCK, std::min<long long>(n, (b + 1) * sfmfilter::SUM_BLOCK), part[2 * b],
                              part[2 * b + 1]);
    const double thr = sfmfilter::threshold(part.data(), n_part, nv, std_mul);
    int m = 0;
    for (int i = 0; i < n; ++i) {
      const bool fin = sfmcloud::finite3(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
      if (fin && sfmfilter::stat_keep(md[i], thr, negative != 0)) idx_out[m++] = i;
    }
    *n_out = m;
    if (threshold) *threshold = thr;
  }
  for (int i = 0; mean_dist && i < n; ++i) mean_dist[i] = md[i];
  return OK;
}

}  // extern "C"

#ifdef CLOUD_FILTER_MAIN
// Both filters on clouds made here: a noisy sheet with NaN points, colours and normals through three leaf sizes and
// min_points, one voxel of 300 points, the refusals, the tiny clouds; then the outlier removal at several mean_k,
// negative, identical points and n = mean_k + 1.  Prints a digest of each.
namespace {
uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
float unit(uint32_t& s) { return (float)(lcg(s) >> 8) / 16777216.0f; }
}  // namespace

int main() {
  uint32_t seed = 7;
  const int n = 6000;
  std::vector<float> xyz((size_t)3 * n), nrm((size_t)3 * n);
  std::vector<uint32_t> rgb((size_t)n);
  for (int i = 0; i < n; ++i) {
    xyz[3 * i] = unit(seed) - 0.3f, xyz[3 * i + 1] = unit(seed), xyz[3 * i + 2] = 0.05f * unit(seed);
    nrm[3 * i] = 0.1f * unit(seed), nrm[3 * i + 1] = 0.1f * unit(seed), nrm[3 * i + 2] = 1.0f;
    rgb[i] = lcg(seed) & 0xFFFFFFu;
    if (i % 97 == 0) xyz[3 * i + (i % 3)] = NAN;
    if (i % 211 == 0) nrm[3 * i] = NAN;
  }
  std::vector<float> oxyz((size_t)3 * n), onrm((size_t)3 * n), md((size_t)n);
  std::vector<uint32_t> orgb((size_t)n);
  std::vector<int32_t> vo((size_t)n), idx((size_t)n), keys((size_t)n);
  int32_t m = 0, div3[3];
  for (float lf : {0.02f, 0.11f, 5.0f})
    for (int mp : {0, 2, 3}) {
      const float leaf[3] = {lf, lf * 1.5f, lf};
      if (cf_voxel_grid(n, xyz.data(), leaf, mp, rgb.data(), nrm.data(), oxyz.data(), orgb.data(), onrm.data(), vo.data(), &m) != 0) return 1;
      long long s = 0;
      for (int i = 0; i < n; ++i) s += vo[i];
      std::printf("leaf %.2f min_points %d voxels %d voxel_of %lld\n", lf, mp, m, s);
    }
  const float one[3] = {1.0f, 1.0f, 1.0f};
  if (cf_voxel_grid(n, xyz.data(), one, 0, nullptr, nullptr, oxyz.data(), nullptr, nullptr, nullptr, &m) != 0) return 1;
  if (cf_voxel_keys(n, xyz.data(), one, keys.data(), div3) != 0) return 1;
  std::printf("plain voxels %d div %d %d %d\n", m, div3[0], div3[1], div3[2]);
  std::vector<float> same((size_t)3 * 300, 0.25f);
  if (cf_voxel_grid(300, same.data(), one, 0, nullptr, nullptr, oxyz.data(), nullptr, nullptr, vo.data(), &m) != 0 || m != 1) return 1;
  const float far[6] = {0, 0, 0, 1290.5f, 1290.5f, 1290.5f}, huge[6] = {3e9f, 0, 0, 3e9f, 1, 1}, bad[3] = {1.0f, 0.0f, 1.0f};
  std::printf("refusals %d %d %d\n", cf_voxel_grid(2, far, one, 0, nullptr, nullptr, oxyz.data(), nullptr, nullptr, nullptr, &m),
              cf_voxel_grid(2, huge, one, 0, nullptr, nullptr, oxyz.data(), nullptr, nullptr, nullptr, &m),
              cf_voxel_grid(2, far, bad, 0, nullptr, nullptr, oxyz.data(), nullptr, nullptr, nullptr, &m));
  for (int k = 0; k <= 1; ++k)
    if (cf_voxel_grid(k, xyz.data() + 3, one, 0, nullptr, nullptr, oxyz.data(), nullptr, nullptr, vo.data(), &m) != 0 || m != k) return 1;
  double thr = 0;
  for (int mk : {1, 8, 31, 32, 63})
    for (int neg = 0; neg <= 1; ++neg) {
      if (cf_statistical_outlier(n, xyz.data(), mk, 1.0, neg, idx.data(), &m, md.data(), &thr) != 0) return 1;
      std::printf("mean_k %d negative %d kept %d thr %.9g\n", mk, neg, m, thr);
    }
  if (cf_statistical_outlier(300, same.data(), 16, 1.0, 0, idx.data(), &m, md.data(), &thr) != 0 || m != 300 || thr != 0.0) return 1;
  std::printf("edge %d %d %d\n", cf_statistical_outlier(17, xyz.data() + 3, 16, 0.0, 0, idx.data(), &m, md.data(), &thr),
              cf_statistical_outlier(16, xyz.data() + 3, 16, 1.0, 0, idx.data(), &m, md.data(), &thr),
              cf_statistical_outlier(0, xyz.data(), 16, 1.0, 0, idx.data(), &m, md.data(), &thr));
  std::printf("done\n");
  return 0;
}
#endif
