// segment.h -- the rules of the colour region growing that follows map3D (reference src/Segmentation.cpp:3-66:
// pcl::RegionGrowingRGB behind a PassThrough on z) and of Dendrometry::estimate's bounds (src/DendrometryE.cpp:3-29:
// pcl::getMinMax3D and cv::norm), as code that hipcc and a plain g++ both compile.  The device code (segment.hip) and
// the CPU test stub (tests/stub/segment_capi.cpp) share these bodies: the per-point and per-segment arithmetic is
// __host__ __device__, the region steps (rules 8-10 of DESIGN.md f-8), which run over segments and depend on their
// order, are host code that the C call runs on the downloaded segment tables.  C++14.
// PARITY UNPINNED: PCL is not in the image; the rules are recalled from PCL 1.8.1's region_growing.hpp /
// region_growing_rgb.hpp.
#pragma once
#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>
#include "cloud.h"

namespace sfmseg {

constexpr int KMAX = 128;  // largest neighbour count of the subset k-NN

// the seven numbers of RegionGrowingRGB the reference sets or leaves at their defaults (rule 1)
struct Opts {
  int region_neighbour_number;   // 100: neighbours searched per point, and segment neighbours kept
  int neighbour_number;          // 30: entries of a point's list the growth looks at
  int min_cluster_size;          // 600
  int max_cluster_size;          // INT_MAX
  float distance_threshold;      // 10 (stored squared)
  float point_color_threshold;   // 6 (stored squared)
  float region_color_threshold;  // 5 (stored squared)
};
inline Opts reference_opts() { return Opts{100, 30, 600, INT_MAX, 10.0f, 6.0f, 5.0f}; }
inline bool opts_valid(const Opts& o) {
  return o.region_neighbour_number >= 1 && o.region_neighbour_number <= KMAX && o.neighbour_number >= 1 &&
         o.min_cluster_size >= 1 && o.max_cluster_size >= o.min_cluster_size && o.distance_threshold >= 0.0f &&
         o.point_color_threshold >= 0.0f && o.region_color_threshold >= 0.0f;
}
// the setters store thresh * thresh in float
SFM_CLOUD_INLINE float squared(float t) { return t * t; }

// calculateColorimetricalDifference on packed 0x00RRGGBB: the integer sum of the squared channel differences
SFM_CLOUD_INLINE int colour_diff(uint32_t a, uint32_t b) {
  const int dr = (int)((a >> 16) & 255u) - (int)((b >> 16) & 255u);
  const int dg = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u);
  const int db = (int)(a & 255u) - (int)(b & 255u);
  return dr * dr + dg * dg + db * db;
}
// validatePoint: the neighbour joins unless the difference to the CURRENT point is > the squared threshold
SFM_CLOUD_INLINE bool point_joins(uint32_t cu, uint32_t cv, float p2p2) { return !((float)colour_diff(cu, cv) > p2p2); }
// a segment's colour channel: unsigned(float(sum) / float(count))
SFM_CLOUD_INLINE unsigned seg_channel(unsigned sum, unsigned count) { return (unsigned)((float)sum / (float)count); }
SFM_CLOUD_INLINE int seg_colour_diff(const unsigned* a, const unsigned* b) {
  const int dr = (int)a[0] - (int)b[0], dg = (int)a[1] - (int)b[1], db = (int)a[2] - (int)b[2];
  return dr * dr + dg * dg + db * db;
}

// Dendrometry::estimate's "Total Height": cv::norm of the Point3f difference = sqrt of the double sum of squares
inline double height(const float mn[3], const float mx[3]) {
  const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
  return std::sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
}
// pcl::getMinMax3D over the finite points (min starts at FLT_MAX, max at -FLT_MAX, which an empty cloud keeps)
inline void minmax_host(int n, const float* xyz, float mn[3], float mx[3]) {
  uint32_t lo[3], hi[3];
  for (int a = 0; a < 3; ++a) {
    lo[a] = sfmcloud::ord_key(FLT_MAX);
    hi[a] = sfmcloud::ord_key(-FLT_MAX);
  }
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!sfmcloud::finite3(p[0], p[1], p[2])) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = std::min(lo[a], sfmcloud::ord_key(p[a]));
      hi[a] = std::max(hi[a], sfmcloud::ord_key(p[a]));
    }
  }
  for (int a = 0; a < 3; ++a) {
    mn[a] = sfmcloud::ord_val(lo[a]);
    mx[a] = sfmcloud::ord_val(hi[a]);
  }
}

// ---- the segment tables the region steps read (what the device produces and the C call downloads)
struct SegTables {
  int n_seg = 0;
  std::vector<int> count;        // points per segment
  std::vector<unsigned> colour;  // 3 per segment (rule 7)
  std::vector<int> nbr_off;      // n_seg + 1: segment s's neighbours are entries nbr_off[s] .. nbr_off[s + 1] - 1,
  std::vector<int> nbr_seg;      //   in stored order: descending (d2, segment), at most region_neighbour_number
  std::vector<float> nbr_d2;
};

typedef std::pair<float, int> DistSeg;
inline bool dist_seg_less(const DistSeg& a, const DistSeg& b) { return sfmcloud::knn_less(a.first, a.second, b.first, b.second); }

// Rules 8-10.  point_seg: the segment of each of the n_s indexed points (list order), -1 for a point with no list.
// Out: seg_region (the region of every segment after the small-region step), n_regions (regions the homogeneous
// merging opened), point_cluster (n_s: the final cluster of each indexed point, -1 = in no cluster) and n_clusters.
// Linear in the neighbour entries but for the lists a chain of small regions hands on.
inline void regions_from_tables(const Opts& o, const SegTables& t, const int* point_seg, int n_s, std::vector<int>& seg_region,
                                int& n_regions, std::vector<int>& point_cluster, int& n_clusters) {
  const float dist2 = squared(o.distance_threshold), r2r2 = squared(o.region_color_threshold);
  const int S = t.n_seg;
  seg_region.assign((size_t)S, -1);
  std::vector<long long> reg_pts;
  // rule 8: homogeneous merging
  for (int s = 0; s < S; ++s) {
    int cur;
    if (seg_region[s] == -1) {
      cur = (int)reg_pts.size();
      seg_region[s] = cur;
      reg_pts.push_back(t.count[s]);
    } else {
      cur = seg_region[s];
    }
    for (int e = t.nbr_off[s]; e < t.nbr_off[s + 1] && e - t.nbr_off[s] < o.region_neighbour_number; ++e) {
      if (t.nbr_d2[e] > dist2) continue;
      const int q = t.nbr_seg[e];
      if (seg_region[q] != -1) continue;
      if ((float)seg_colour_diff(&t.colour[3 * (size_t)s], &t.colour[3 * (size_t)q]) < r2r2) {
        seg_region[q] = cur;
        reg_pts[cur] += t.count[q];
      }
    }
  }
  const int R = (int)reg_pts.size();
  n_regions = R;
  // rule 9: the regions' neighbour lists, then the small regions
  std::vector<std::vector<int>> reg_segs((size_t)R);
  for (int s = 0; s < S; ++s) reg_segs[seg_region[s]].push_back(s);
  std::vector<std::vector<DistSeg>> nb((size_t)R);
  std::vector<char> stale((size_t)R, 0);  // a receiver's list is cleaned and sorted again when it is next read
  for (int r = 0; r < R; ++r) {
    for (int s : reg_segs[r])
      for (int e = t.nbr_off[s]; e < t.nbr_off[s + 1]; ++e) {
        if (t.nbr_d2[e] == FLT_MAX) continue;
        if (seg_region[t.nbr_seg[e]] != r) nb[r].push_back(DistSeg(t.nbr_d2[e], t.nbr_seg[e]));
      }
    std::sort(nb[r].begin(), nb[r].end(), dist_seg_less);
  }
  for (int r = 0; r < R; ++r) {
    if (!(reg_pts[r] < o.min_cluster_size)) continue;
    if (stale[r]) {  // (the entries that point into the region itself since it last received: (FLT_MAX, 0), then the sort)
      for (DistSeg& d : nb[r])
        if (seg_region[d.second] == r) d = DistSeg(FLT_MAX, 0);
      std::sort(nb[r].begin(), nb[r].end(), dist_seg_less);
      stale[r] = 0;
    }
    if (nb[r].empty() || nb[r][0].first == FLT_MAX) continue;
    const int to = seg_region[nb[r][0].second];
    if (to == r) continue;  // (cannot happen: such an entry was set to FLT_MAX above)
    for (int s : reg_segs[r]) {
      reg_segs[to].push_back(s);
      seg_region[s] = to;
    }
    reg_segs[r].clear();
    reg_pts[to] += reg_pts[r];
    reg_pts[r] = 0;
    for (const DistSeg& d : nb[r])
      if (seg_region[d.second] != to) nb[to].push_back(d);
    nb[r].clear();
    stale[to] = 1;
  }
  // rule 10: assembly in region order, the compaction of empty regions, the size limits
  std::vector<int> order((size_t)R);
  for (int r = 0; r < R; ++r) order[r] = r;
  if (R > 0) {
    int i = 0, j = R - 1;
    while (i < j) {
      while (reg_pts[order[i]] != 0 && i < j) ++i;
      while (reg_pts[order[j]] == 0 && i < j) --j;
      if (i != j) std::swap(order[i], order[j]);
    }
  }
  std::vector<int> cluster_of((size_t)R, -1);
  n_clusters = 0;
  for (int p = 0; p < R; ++p) {
    const long long m = reg_pts[order[p]];
    if (m == 0 || m < o.min_cluster_size || m > o.max_cluster_size) continue;
    cluster_of[order[p]] = n_clusters++;
  }
  point_cluster.assign((size_t)n_s, -1);
  for (int i = 0; i < n_s; ++i)
    if (point_seg[i] >= 0) point_cluster[i] = cluster_of[seg_region[point_seg[i]]];
}

}  // namespace sfmseg
