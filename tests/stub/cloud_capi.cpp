// cloud_capi.cpp -- a C surface over csrc/cloud.h for tests/test_cloud_cpu.py and tests/test_gpu_cloud.py (built with
// g++ -O2 -ffp-contract=off -pthread), the PCD reader of csrc/host/pcllite.h, and, with -DCLOUD_MAIN, a driver that
// runs every operation on one cloud from a file under the sanitizers.  The spatial search here is the CPU's own (a hash
// grid, a brute-force fallback), independent of cloud.hip's; only the arithmetic and the rules come from the header.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/cloud.h"
#include "../../sfm_danpipeline_amd/csrc/host/pcllite.h"

namespace {

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

void radius_counts(int n, const float* xyz, double r, int cap, int32_t* counts) {
  HashGrid g;
  g.build(n, xyz, r * (1.0 + 1.0 / 1024.0));
  const float r2 = sfmcloud::radius2(r);
  parallel(n, [&](int i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) {
      counts[i] = 0;
      return;
    }
    const long long cx = HashGrid::coord(p[0], g.cell), cy = HashGrid::coord(p[1], g.cell), cz = HashGrid::coord(p[2], g.cell);
    int k = 0;
    for (long long z = cz - 1; z <= cz + 1; ++z)
      for (long long y = cy - 1; y <= cy + 1; ++y)
        for (long long x = cx - 1; x <= cx + 1; ++x) {
          const std::vector<int>* v = g.at(x, y, z);
          if (!v) continue;
          for (int j : *v) {
            const float* q = xyz + 3 * (size_t)j;
            k += sfmcloud::in_radius(sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]), r2) ? 1 : 0;
          }
        }
    counts[i] = cap > 0 ? std::min(k, cap) : k;
  });
}

struct Cand {
  float d;
  int i;
};
bool cand_less(const Cand& a, const Cand& b) { return sfmcloud::knn_less(a.d, a.i, b.d, b.i); }

// the k nearest of every point: rings of a hash grid until the k-th d2 is below the searched block's inner radius
// (with a margin), brute force over all points after 24 rings
void knn_lists(int n, const float* xyz, int k, std::vector<Cand>& out /* n k */, std::vector<int>& nfound) {
  int nv = 0;
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
    ++nv;
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], (double)p[a]);
      hi[a] = std::max(hi[a], (double)p[a]);
    }
  }
  double ext = 0;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, nv ? hi[a] - lo[a] : 0.0);
  HashGrid g;
  g.build(n, xyz, ext > 0 ? ext / std::max(1.0, std::cbrt(nv / 8.0)) : 1.0);
  out.assign((size_t)n * k, Cand{sfmcloud::bits_f(0x7F800000u), -1});
  nfound.assign(n, 0);
  parallel(n, [&](int i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) return;
    const int kk = std::min(k, nv);
    std::vector<Cand> c;
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
              c.push_back(Cand{sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]), j});
            }
          }
      if ((int)c.size() >= kk) {
        std::nth_element(c.begin(), c.begin() + (kk - 1), c.end(), cand_less);
        const double inner = R * g.cell * (1.0 - 1e-4);
        if ((double)c[kk - 1].d < inner * inner) {
          brute = false;
          break;
        }
      }
    }
    if (brute) {
      c.clear();
      for (int j = 0; j < n; ++j) {
        const float* q = xyz + 3 * (size_t)j;
        if (sfmcloud::finite3(q[0], q[1], q[2])) c.push_back(Cand{sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]), j});
      }
    }
    std::sort(c.begin(), c.end(), cand_less);
    for (int s = 0; s < kk; ++s) out[(size_t)i * k + s] = c[s];
    nfound[i] = kk;
  });
}

void normal_of(const float* xyz, const Cand* list, int cnt, const float* p, const float* vp, float* out4) {
  sfmcloud::Accu acc;
  sfmcloud::accu_zero(acc);
  for (int s = 0; s < cnt; ++s) {
    const float* q = xyz + 3 * (size_t)list[s].i;
    sfmcloud::accu_add(acc, q[0], q[1], q[2]);
  }
  float cov[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  if (cnt >= 3) sfmcloud::accu_covariance(acc, cnt, cov);
  sfmcloud::normal_from_cov(cov, cnt, p[0], p[1], p[2], vp, out4);
}

}  // namespace

extern "C" {

float cloud_dist2(float ax, float ay, float az, float bx, float by, float bz) { return sfmcloud::dist2(ax, ay, az, bx, by, bz); }
float cloud_radius2(double r) { return sfmcloud::radius2(r); }
double cloud_atan2(double y, double x) { return sfmcloud::atan2_own(y, x); }
double cloud_cos(double x) { return sfmcloud::cos_own(x); }
double cloud_sin(double x) { return sfmcloud::sin_own(x); }
void cloud_roots(const float* m, float* r) { sfmcloud::roots3(m, r); }
void cloud_eigen33(const float* cov, float* value, float* vec) { sfmcloud::eigen33(cov, *value, vec); }
void cloud_normal_from_cov(const float* cov, int count, const float* p, const float* vp, float* out4) {
  sfmcloud::normal_from_cov(cov, count, p[0], p[1], p[2], vp, out4);
}
// the normal of the first `count` points of `nb` (the neighbour list, in list order) at point p
void cloud_normal_of_list(const float* nb, int count, const float* p, const float* vp, float* out4) {
  std::vector<Cand> l((size_t)count);
  for (int s = 0; s < count; ++s) l[s] = Cand{0.f, s};
  normal_of(nb, l.data(), count, p, vp, out4);
}

int cloud_passthrough(int n, const float* xyz, int axis, float lo, float hi, int negative, int32_t* idx_out) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (sfmcloud::passthrough_keep(p[0], p[1], p[2], axis, lo, hi, negative != 0)) idx_out[m++] = i;
  }
  return m;
}

void cloud_radius_count(int n, const float* xyz, double r, int cap, int32_t* counts) { radius_counts(n, xyz, r, cap, counts); }

int cloud_radius_outlier(int n, const float* xyz, double r, int min_pts, int32_t* idx_out) {
  std::vector<int32_t> cnt((size_t)std::max(n, 1));
  radius_counts(n, xyz, r, 0, cnt.data());
  int m = 0;
  for (int i = 0; i < n; ++i)
    if (sfmcloud::radius_keep(cnt[i], min_pts)) idx_out[m++] = i;
  return m;
}

void cloud_knn(int n, const float* xyz, int k, int32_t* idx, float* d2) {
  std::vector<Cand> l;
  std::vector<int> nf;
  knn_lists(n, xyz, k, l, nf);
  for (size_t s = 0; s < l.size(); ++s) {
    idx[s] = l[s].i;
    d2[s] = l[s].d;
  }
}

void cloud_normals(int n, const float* xyz, int k, const float* vp, float* out4) {
  std::vector<Cand> l;
  std::vector<int> nf;
  knn_lists(n, xyz, k, l, nf);
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) {
      for (int c = 0; c < 4; ++c) out4[4 * (size_t)i + c] = sfmcloud::qnan();
      continue;
    }
    normal_of(xyz, &l[(size_t)i * k], nf[i], p, vp, out4 + 4 * (size_t)i);
  }
}

// pcl::io::loadPCDFile into xyz (capacity cap points); returns the point count, or -1; info = width, height, is_dense,
// and the sensor origin's bits follow in origin[3]
int cloud_load_pcd(const char* path, float* xyz, int cap, int32_t* info, float* origin) {
  pcl::PointCloud<pcl::PointXYZ> c;
  if (pcl::io::loadPCDFile(path, c) != 0) return -1;
  const int n = (int)c.size();
  for (int i = 0; i < n && i < cap; ++i) {
    xyz[3 * (size_t)i] = c.points[i].x;
    xyz[3 * (size_t)i + 1] = c.points[i].y;
    xyz[3 * (size_t)i + 2] = c.points[i].z;
  }
  info[0] = (int32_t)c.width;
  info[1] = (int32_t)c.height;
  info[2] = c.is_dense ? 1 : 0;
  for (int a = 0; a < 3; ++a) origin[a] = c.sensor_origin_[a];
  return n;
}

}  // extern "C"

#ifdef CLOUD_MAIN
// in.bin: i32 n, n x f32 xyz[3].  Runs the passthrough (x in [0.003, 0.83]), the radius counts (r 0.07, exact and
// capped at 151), the outlier removal (150), the 10 nearest and the normals (vp 0) and prints a digest of each.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<float> xyz((size_t)3 * n + 1);
  if (n && fread(xyz.data(), 4, (size_t)3 * n, f) != (size_t)3 * n) return 2;
  fclose(f);
  std::vector<int32_t> idx((size_t)n + 1), cnt((size_t)n + 1), kid((size_t)n * 10 + 1);
  std::vector<float> kd((size_t)n * 10 + 1), nrm((size_t)n * 4 + 1);
  const float vp[3] = {0, 0, 0};
  const int m_pt = cloud_passthrough(n, xyz.data(), 0, 0.003f, 0.83f, 0, idx.data());
  cloud_radius_count(n, xyz.data(), 0.07, 0, cnt.data());
  long long sum = 0;
  for (int i = 0; i < n; ++i) sum += cnt[i];
  cloud_radius_count(n, xyz.data(), 0.07, 151, cnt.data());
  long long sum_cap = 0;
  for (int i = 0; i < n; ++i) sum_cap += cnt[i];
  const int m_ro = cloud_radius_outlier(n, xyz.data(), 0.07, 150, idx.data());
  cloud_knn(n, xyz.data(), 10, kid.data(), kd.data());
  long long ksum = 0;
  for (size_t s = 0; s < (size_t)n * 10; ++s) ksum += kid[s];
  cloud_normals(n, xyz.data(), 10, vp, nrm.data());
  int nan = 0;
  for (int i = 0; i < n; ++i) nan += nrm[4 * (size_t)i] != nrm[4 * (size_t)i];
  std::printf("passthrough %d counts %lld capped %lld outlier_kept %d knn %lld nan %d\n", m_pt, sum, sum_cap, m_ro, ksum, nan);
  return 0;
}
#endif
