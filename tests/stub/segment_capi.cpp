// segment_capi.cpp -- a C surface over csrc/segment.h for tests/test_segment_cpu.py and tests/test_gpu_segment.py
// (built with g++ -O2 -ffp-contract=off -pthread), the XYZRGB PCD reader of csrc/host/pcllite.h, and, with
// -DSEGMENT_MAIN, a driver that runs the whole call on one cloud from a file under the sanitizers.  What the device
// does in parallel is done here the way PCL does it: a hash-grid search of its own for the neighbours, the literal
// queue for the growth, a dense-style pass with a heap for the segment neighbours; only the arithmetic and the region
// steps (rules 8-10) come from the header.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <queue>
#include <thread>
#include <unordered_map>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/segment.h"
#include "../../sfm_danpipeline_amd/csrc/host/pcllite.h"

namespace {

struct Cand {
  float d;
  int i;
};
bool cand_less(const Cand& a, const Cand& b) { return sfmcloud::knn_less(a.d, a.i, b.d, b.i); }

long long cell_key(long long x, long long y, long long z) {
  return ((x + (1ll << 20)) << 42) | ((y + (1ll << 20)) << 21) | (z + (1ll << 20));
}
long long cell_coord(float v, double cell) {
  double f = std::floor((double)v / cell);
  f = std::max(-(double)(1 << 20) + 1, std::min((double)(1 << 20) - 1, f));
  return (long long)f;
}

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

// the k nearest (d2, position) among the m gathered points, for each of them: rings of a hash grid until the k-th d2
// is inside the searched block, brute force after 12 rings.  out: m x k, position -1 / +inf padded; a non-finite point
// has no list and is in nobody's.
void knn_positions(int m, const float* p3, int k, std::vector<int>& idx, std::vector<float>& d2) {
  idx.assign((size_t)m * k, -1);
  d2.assign((size_t)m * k, sfmcloud::bits_f(0x7F800000u));
  int nv = 0;
  double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
  for (int i = 0; i < m; ++i) {
    const float* p = p3 + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
    ++nv;
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], (double)p[a]);
      hi[a] = std::max(hi[a], (double)p[a]);
    }
  }
  if (!nv) return;
  double ext = 0;
  for (int a = 0; a < 3; ++a) ext = std::max(ext, hi[a] - lo[a]);
  const double cell = ext > 0 ? ext / std::max(1.0, std::sqrt(nv / 24.0)) : 1.0;  // (surfaces: ~24 points per occupied cell)
  std::unordered_map<long long, std::vector<int>> cells;
  for (int i = 0; i < m; ++i) {
    const float* p = p3 + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
    cells[cell_key(cell_coord(p[0], cell), cell_coord(p[1], cell), cell_coord(p[2], cell))].push_back(i);
  }
  const int kk = std::min(k, nv);
  parallel(m, [&](int i) {
    const float* p = p3 + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) return;
    std::vector<Cand> c;
    const long long cx = cell_coord(p[0], cell), cy = cell_coord(p[1], cell), cz = cell_coord(p[2], cell);
    bool brute = true;
    for (long long R = 0; R <= 12; ++R) {
      for (long long z = cz - R; z <= cz + R; ++z)
        for (long long y = cy - R; y <= cy + R; ++y)
          for (long long x = cx - R; x <= cx + R; ++x) {
            if (std::max(std::max(std::llabs(x - cx), std::llabs(y - cy)), std::llabs(z - cz)) != R) continue;
            auto it = cells.find(cell_key(x, y, z));
            if (it == cells.end()) continue;
            for (int j : it->second) {
              const float* q = p3 + 3 * (size_t)j;
              c.push_back(Cand{sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]), j});
            }
          }
      if ((int)c.size() >= kk) {
        std::nth_element(c.begin(), c.begin() + (kk - 1), c.end(), cand_less);
        const double inner = R * cell * (1.0 - 1e-4);
        if ((double)c[kk - 1].d < inner * inner) {
          brute = false;
          break;
        }
      }
    }
    if (brute) {
      c.clear();
      for (int j = 0; j < m; ++j) {
        const float* q = p3 + 3 * (size_t)j;
        if (sfmcloud::finite3(q[0], q[1], q[2])) c.push_back(Cand{sfmcloud::dist2(p[0], p[1], p[2], q[0], q[1], q[2]), j});
      }
    }
    std::partial_sort(c.begin(), c.begin() + kk, c.end(), cand_less);
    for (int s = 0; s < kk; ++s) {
      idx[(size_t)i * k + s] = c[s].i;
      d2[(size_t)i * k + s] = c[s].d;
    }
  });
}

bool indices_valid(int n, const int32_t* ind, int m) {
  if (!ind || m < 1 || m > n) return false;
  for (int r = 0; r < m; ++r)
    if (ind[r] < 0 || ind[r] >= n || (r > 0 && ind[r] <= ind[r - 1])) return false;
  return true;
}

void gather(const float* xyz, const int32_t* ind, int m, std::vector<float>& out) {
  out.resize((size_t)3 * m + 1);
  for (int r = 0; r < m; ++r)
    for (int a = 0; a < 3; ++a) out[3 * (size_t)r + a] = xyz[3 * (size_t)ind[r] + a];
}

// rule 4 as PCL runs it: seeds in list order, a queue, the first `nn` entries of the current point
int grow_queue(int m, int k, int nn, const int* idx, const uint32_t* rgb, float p2p2, std::vector<int>& seg) {
  seg.assign((size_t)m, -1);
  int n_seg = 0;
  std::queue<int> q;
  for (int seed = 0; seed < m; ++seed) {
    if (seg[seed] != -1 || idx[(size_t)seed * k] < 0) continue;
    seg[seed] = n_seg;
    q.push(seed);
    while (!q.empty()) {
      const int u = q.front();
      q.pop();
      for (int s = 0; s < nn && s < k; ++s) {
        const int v = idx[(size_t)u * k + s];
        if (v < 0) break;
        if (seg[v] != -1) continue;
        if (!sfmseg::point_joins(rgb[u], rgb[v], p2p2)) continue;
        seg[v] = n_seg;
        q.push(v);
      }
    }
    ++n_seg;
  }
  return n_seg;
}

// rules 5-7: counts, colours, and findRegionsKNN's pass per segment (a distance per other segment, then the heap)
void tables(int m, int k, int keep, const int* idx, const float* d2, const uint32_t* rgb, const std::vector<int>& seg, int n_seg,
            sfmseg::SegTables& t) {
  t.n_seg = n_seg;
  t.count.assign((size_t)n_seg, 0);
  t.colour.assign((size_t)3 * n_seg, 0);
  std::vector<unsigned> sum((size_t)3 * n_seg, 0);
  std::vector<std::vector<int>> pts((size_t)n_seg);
  for (int u = 0; u < m; ++u) {
    if (seg[u] < 0) continue;
    pts[seg[u]].push_back(u);
    ++t.count[seg[u]];
    sum[3 * (size_t)seg[u]] += (rgb[u] >> 16) & 255u;
    sum[3 * (size_t)seg[u] + 1] += (rgb[u] >> 8) & 255u;
    sum[3 * (size_t)seg[u] + 2] += rgb[u] & 255u;
  }
  for (size_t e = 0; e < sum.size(); ++e) t.colour[e] = sfmseg::seg_channel(sum[e], (unsigned)t.count[e / 3]);
  t.nbr_off.assign((size_t)n_seg + 1, 0);
  t.nbr_seg.clear();
  t.nbr_d2.clear();
  std::vector<float> dist((size_t)n_seg, FLT_MAX);
  std::vector<int> touched;
  for (int s = 0; s < n_seg; ++s) {
    touched.clear();
    for (int u : pts[s])
      for (int e = 0; e < k; ++e) {
        const int v = idx[(size_t)u * k + e];
        if (v < 0) break;
        const int b = seg[v];
        if (b == s) continue;
        if (dist[b] == FLT_MAX) touched.push_back(b);
        if (dist[b] > d2[(size_t)u * k + e]) dist[b] = d2[(size_t)u * k + e];
      }
    std::sort(touched.begin(), touched.end());
    std::priority_queue<std::pair<float, int>> heap;
    for (int b : touched) {
      if (dist[b] < FLT_MAX) {
        heap.push(std::make_pair(dist[b], b));
        if ((int)heap.size() > keep) heap.pop();
      }
      dist[b] = FLT_MAX;
    }
    while (!heap.empty()) {
      t.nbr_d2.push_back(heap.top().first);
      t.nbr_seg.push_back(heap.top().second);
      heap.pop();
    }
    t.nbr_off[(size_t)s + 1] = (int)t.nbr_seg.size();
  }
}

sfmseg::Opts opts_of(const int32_t* oi, const float* of) { return sfmseg::Opts{oi[0], oi[1], oi[2], oi[3], of[0], of[1], of[2]}; }

}  // namespace

extern "C" {

void seg_reference_opts(int32_t* oi /* 4 */, float* of /* 3 */) {
  const sfmseg::Opts o = sfmseg::reference_opts();
  oi[0] = o.region_neighbour_number;
  oi[1] = o.neighbour_number;
  oi[2] = o.min_cluster_size;
  oi[3] = o.max_cluster_size;
  of[0] = o.distance_threshold;
  of[1] = o.point_color_threshold;
  of[2] = o.region_color_threshold;
}

int seg_colour_diff(uint32_t a, uint32_t b) { return sfmseg::colour_diff(a, b); }
unsigned seg_channel(unsigned sum, unsigned count) { return sfmseg::seg_channel(sum, count); }

// rule 2: n_idx x k cloud indices and d2; -3 for an empty or malformed list
int seg_subset_knn(int n, const float* xyz, const int32_t* ind, int m, int k, int32_t* idx, float* d2) {
  if (k < 1 || k > sfmseg::KMAX || !indices_valid(n, ind, m)) return -3;
  std::vector<float> p;
  gather(xyz, ind, m, p);
  std::vector<int> ki;
  std::vector<float> kd;
  knn_positions(m, p.data(), k, ki, kd);
  for (size_t e = 0; e < ki.size(); ++e) {
    idx[e] = ki[e] >= 0 ? ind[ki[e]] : -1;
    d2[e] = kd[e];
  }
  return 0;
}

// rules 2-4: segment per cloud point (-1 outside the list); returns the segment count, or -3
int seg_grow(int n, const float* xyz, const uint32_t* rgb, const int32_t* ind, int m, const int32_t* oi, const float* of,
             int32_t* segment) {
  const sfmseg::Opts o = opts_of(oi, of);
  if (!sfmseg::opts_valid(o) || !indices_valid(n, ind, m)) return -3;
  std::vector<float> p;
  gather(xyz, ind, m, p);
  std::vector<int> ki, seg;
  std::vector<float> kd;
  const int k = o.region_neighbour_number;
  knn_positions(m, p.data(), k, ki, kd);
  std::vector<uint32_t> c((size_t)m);
  for (int r = 0; r < m; ++r) c[r] = rgb[ind[r]] & 0x00FFFFFFu;
  const int n_seg = grow_queue(m, k, o.neighbour_number, ki.data(), c.data(), sfmseg::squared(o.point_color_threshold), seg);
  for (int i = 0; i < n; ++i) segment[i] = -1;
  for (int r = 0; r < m; ++r) segment[ind[r]] = seg[r];
  return n_seg;
}

// the whole call: labels per cloud point, *n_clusters, stats = (n_idx used, segments, regions, 0); 0, or -3
int seg_segment_rgb(int n, const float* xyz, const uint32_t* rgb, const int32_t* ind, int m, const int32_t* oi, const float* of,
                    int32_t* labels, int32_t* n_clusters, int32_t* stats, int32_t* seg_region_out /* n_idx, or NULL */) {
  const sfmseg::Opts o = opts_of(oi, of);
  if (!sfmseg::opts_valid(o) || !indices_valid(n, ind, m)) return -3;
  std::vector<float> p;
  gather(xyz, ind, m, p);
  std::vector<int> ki, seg;
  std::vector<float> kd;
  const int k = o.region_neighbour_number;
  knn_positions(m, p.data(), k, ki, kd);
  std::vector<uint32_t> c((size_t)m);
  for (int r = 0; r < m; ++r) c[r] = rgb[ind[r]] & 0x00FFFFFFu;
  const int n_seg = grow_queue(m, k, o.neighbour_number, ki.data(), c.data(), sfmseg::squared(o.point_color_threshold), seg);
  sfmseg::SegTables t;
  tables(m, k, o.region_neighbour_number, ki.data(), kd.data(), c.data(), seg, n_seg, t);
  std::vector<int> seg_region, point_cluster;
  int n_regions = 0, nc = 0;
  sfmseg::regions_from_tables(o, t, seg.data(), m, seg_region, n_regions, point_cluster, nc);
  for (int i = 0; i < n; ++i) labels[i] = -1;
  int used = 0;
  for (int r = 0; r < m; ++r) {
    labels[ind[r]] = point_cluster[r];
    used += seg[r] >= 0;
    if (seg_region_out) seg_region_out[r] = seg[r] >= 0 ? seg_region[seg[r]] : -1;
  }
  *n_clusters = nc;
  stats[0] = used;
  stats[1] = n_seg;
  stats[2] = n_regions;
  stats[3] = 0;
  return 0;
}

// rules 8-10 alone on tables built by hand
void seg_regions(const int32_t* oi, const float* of, int n_seg, const int32_t* count, const uint32_t* colour, const int32_t* nbr_off,
                 const int32_t* nbr_seg, const float* nbr_d2, const int32_t* point_seg, int n_s, int32_t* seg_region, int32_t* n_regions,
                 int32_t* point_cluster, int32_t* n_clusters) {
  sfmseg::SegTables t;
  t.n_seg = n_seg;
  t.count.assign(count, count + n_seg);
  t.colour.assign(colour, colour + 3 * (size_t)n_seg);
  t.nbr_off.assign(nbr_off, nbr_off + n_seg + 1);
  t.nbr_seg.assign(nbr_seg, nbr_seg + nbr_off[n_seg]);
  t.nbr_d2.assign(nbr_d2, nbr_d2 + nbr_off[n_seg]);
  std::vector<int> sr, pc;
  int nr = 0, nc = 0;
  sfmseg::regions_from_tables(opts_of(oi, of), t, point_seg, n_s, sr, nr, pc, nc);
  for (int s = 0; s < n_seg; ++s) seg_region[s] = sr[s];
  for (int i = 0; i < n_s; ++i) point_cluster[i] = pc[i];
  *n_regions = nr;
  *n_clusters = nc;
}

void seg_minmax(int n, const float* xyz, float* mn, float* mx, double* height) {
  sfmseg::minmax_host(n, xyz, mn, mx);
  *height = sfmseg::height(mn, mx);
}

// cloud.h's ordered keys as segment.h sees them: key[i] = ord_key(f[i]), back[i] = ord_val(key[i])
void seg_ord_keys(int n, const float* f, uint32_t* key, float* back) {
  for (int i = 0; i < n; ++i) {
    key[i] = sfmcloud::ord_key(f[i]);
    back[i] = sfmcloud::ord_val(key[i]);
  }
}

// pcl::io::loadPCDFile for PointXYZRGB; returns the point count or -1; info = width, height, is_dense
int seg_load_pcd(const char* path, float* xyz, uint32_t* rgb, int cap, int32_t* info) {
  pcl::PointCloud<pcl::PointXYZRGB> c;
  if (pcl::io::loadPCDFile(path, c) != 0) return -1;
  const int n = (int)c.size();
  for (int i = 0; i < n && i < cap; ++i) {
    xyz[3 * (size_t)i] = c.points[i].x;
    xyz[3 * (size_t)i + 1] = c.points[i].y;
    xyz[3 * (size_t)i + 2] = c.points[i].z;
    rgb[i] = c.points[i].rgba;
  }
  info[0] = (int32_t)c.width;
  info[1] = (int32_t)c.height;
  info[2] = c.is_dense ? 1 : 0;
  return n;
}

}  // extern "C"

#ifdef SEGMENT_MAIN
// in.bin: i32 n, n x f32 xyz[3], n x u32 rgb.  PassThrough on z in [0, 14], the whole call with the reference's
// options but min_cluster_size 50, the bounds; prints a digest.
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int n = 0;
  if (fread(&n, 4, 1, f) != 1 || n < 0) return 2;
  std::vector<float> xyz((size_t)3 * n + 1);
  std::vector<uint32_t> rgb((size_t)n + 1);
  if (n && fread(xyz.data(), 4, (size_t)3 * n, f) != (size_t)3 * n) return 2;
  if (n && fread(rgb.data(), 4, (size_t)n, f) != (size_t)n) return 2;
  fclose(f);
  std::vector<int32_t> ind;
  for (int i = 0; i < n; ++i)
    if (sfmcloud::passthrough_keep(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2], 2, 0.0f, 14.0f, false)) ind.push_back(i);
  int32_t oi[4];
  float of[3];
  seg_reference_opts(oi, of);
  oi[2] = 50;
  std::vector<int32_t> labels((size_t)n + 1);
  int32_t nc = 0, stats[4] = {0, 0, 0, 0};
  const int rc = seg_segment_rgb(n, xyz.data(), rgb.data(), ind.data(), (int)ind.size(), oi, of, labels.data(), &nc, stats, nullptr);
  float mn[3], mx[3];
  double h = 0;
  seg_minmax(n, xyz.data(), mn, mx, &h);
  long long in_cluster = 0;
  for (int i = 0; i < n; ++i) in_cluster += labels[i] >= 0;
  std::printf("segment rc %d indexed %d segments %d regions %d clusters %d clustered %lld height %.6f\n", rc, stats[0], stats[1],
              stats[2], nc, in_cluster, h);
  return 0;
}
#endif
