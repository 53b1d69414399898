// pcllite.h -- the few PCL 1.8.1 types map3D's step 10 passes around (reference src/Sfm.cpp:94-102, include/Sfm.h:182-186),
// as plain stand-ins next to cvlite.h (PCL is not a dependency of this build), and the PCD reader that loads MAP3D.pcd
// into them (pcl::io::loadPCDFile for PointXYZ and PointXYZRGB), and pcl::VoxelGrid / pcl::StatisticalOutlierRemoval /
// pcl::IterativeClosestPoint / pcl::transformPointCloud over the C ABI.  Header-only and C++14: the host mirror and the CPU
// tests include it.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>
#include "../../../include/sfmhip.h"  // (the filter classes at the end forward to the C ABI)

sfmhip_ctx* sfm_hip_context();  // hip_backend.h: the process-wide context of the host classes

namespace pcl {

struct PointXYZ {
  float x, y, z;
  PointXYZ() : x(0), y(0), z(0) {}
  PointXYZ(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

// x, y, z and the packed colour 0x00RRGGBB (PCL's rgba member; its float view `rgb` is what a PCD's rgb field of TYPE F holds)
struct PointXYZRGB {
  float x, y, z;
  uint32_t rgba;
  PointXYZRGB() : x(0), y(0), z(0), rgba(0) {}
  PointXYZRGB(float x_, float y_, float z_, uint32_t c) : x(x_), y(y_), z(z_), rgba(c) {}
  uint8_t r() const { return (uint8_t)(rgba >> 16); }
  uint8_t g() const { return (uint8_t)(rgba >> 8); }
  uint8_t b() const { return (uint8_t)rgba; }
};

// one cluster: the indices of its points in the input cloud
struct PointIndices {
  std::vector<int> indices;
};

struct Normal {
  float normal_x, normal_y, normal_z, curvature;
  Normal() : normal_x(0), normal_y(0), normal_z(0), curvature(0) {}
};

template <typename T>
struct PointCloud {
  std::vector<T> points;
  uint32_t width = 0, height = 0;  // an unorganised cloud: width = size, height = 1
  bool is_dense = true;            // false when a point may hold a non-finite value
  float sensor_origin_[4] = {0, 0, 0, 0};  // the PCD's VIEWPOINT translation (Eigen::Vector4f in PCL)
  typedef std::shared_ptr<PointCloud<T>> Ptr;
  size_t size() const { return points.size(); }
  bool empty() const { return points.empty(); }
  void push_back(const T& p) {
    points.push_back(p);
    width = (uint32_t)points.size();
    height = 1;
  }
};

// a point with its normal: what create_mesh hands to pcl::Poisson (pcl::concatenateFields of the cloud and its normals)
struct PointNormal {
  float x, y, z, normal_x, normal_y, normal_z, curvature;
  PointNormal() : x(0), y(0), z(0), normal_x(0), normal_y(0), normal_z(0), curvature(0) {}
};

// one polygon: indices into the mesh's cloud
struct Vertices {
  std::vector<uint32_t> vertices;
};

// pcl::PolygonMesh keeps its vertices as a PCLPointCloud2 blob; the stand-in keeps them as the PointXYZ cloud that
// pcl::fromPCLPointCloud2 would read out of it.  polygons: triangles (Poisson's outputPolygons is off).  colours (0x00RRGGBB) and
// normals: one per vertex after StructFromMotion::finishMesh (in PCL further fields of the blob), empty in every other mesh
struct PolygonMesh {
  PointCloud<PointXYZ> cloud;
  std::vector<Vertices> polygons;
  std::vector<uint32_t> colours;
  std::vector<Normal> normals;
};

namespace io {

// The reader behind both loadPCDFile overloads: PCD v0.5-0.7, DATA ascii or binary (little-endian records), fields x,
// y, z of TYPE F and SIZE 4 or 8 and, when `colour` is asked for, a field rgb or rgba of SIZE 4 (TYPE F: the packed
// colour's bits as a float, what convertPLYtoPCD writes; TYPE U / I: the packed integer); other fields are skipped and
// a file without a colour field gives colour 0; binary_compressed is refused with a message.  Returns 0, or -1 when
// the file is missing, malformed or truncated.  is_dense = every point finite.
struct PcdRecord {
  float v[3];
  uint32_t c;
};
struct PcdFile {
  std::vector<PcdRecord> points;
  uint32_t width = 0, height = 0;
  bool is_dense = true;
  float origin[3] = {0, 0, 0};
};
inline int readPCD(const std::string& path, bool colour, PcdFile& file) {
  file = PcdFile();
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::fprintf(stderr, "[pcd] cannot open %s\n", path.c_str());
    return -1;
  }
  std::vector<char> buf;
  char tmp[65536];
  size_t got;
  while ((got = std::fread(tmp, 1, sizeof tmp, f)) > 0) buf.insert(buf.end(), tmp, tmp + got);
  std::fclose(f);
  size_t pos = 0;
  std::vector<std::string> names, types;
  std::vector<int> sizes, counts;
  long long width = -1, height = 1, points = -1;
  float vp[7] = {0, 0, 0, 1, 0, 0, 0};
  std::string data;
  while (pos < buf.size()) {
    size_t e = pos;
    while (e < buf.size() && buf[e] != '\n') ++e;
    std::string l(&buf[pos], e - pos);
    pos = e + 1;
    if (!l.empty() && l.back() == '\r') l.pop_back();
    if (l.empty() || l[0] == '#') continue;
    std::istringstream is(l);
    std::string w, v;
    is >> w;
    if (w == "VERSION") continue;
    if (w == "FIELDS" || w == "COLUMNS") {
      while (is >> v) names.push_back(v);
    } else if (w == "SIZE") {
      int s;
      while (is >> s) sizes.push_back(s);
    } else if (w == "TYPE") {
      while (is >> v) types.push_back(v);
    } else if (w == "COUNT") {
      int s;
      while (is >> s) counts.push_back(s);
    } else if (w == "WIDTH") {
      is >> width;
    } else if (w == "HEIGHT") {
      is >> height;
    } else if (w == "VIEWPOINT") {
      for (int k = 0; k < 7; ++k) is >> vp[k];
    } else if (w == "POINTS") {
      is >> points;
    } else if (w == "DATA") {
      is >> data;
      break;
    } else {
      std::fprintf(stderr, "[pcd] %s: unknown header line '%s'\n", path.c_str(), l.c_str());
      return -1;
    }
  }
  if (counts.empty()) counts.assign(names.size(), 1);
  if (points < 0 && width >= 0) points = width * height;
  if (names.empty() || sizes.size() != names.size() || types.size() != names.size() || counts.size() != names.size() ||
      points < 0 || width < 0 || height < 0 || width * height != points || points > (1ll << 31) - 1) {
    std::fprintf(stderr, "[pcd] %s: malformed header\n", path.c_str());
    return -1;
  }
  if (data == "binary_compressed") {
    std::fprintf(stderr, "[pcd] %s: DATA binary_compressed is not supported (save the cloud as ascii or binary)\n",
                 path.c_str());
    return -1;
  }
  if (data != "ascii" && data != "binary") {
    std::fprintf(stderr, "[pcd] %s: unknown DATA '%s'\n", path.c_str(), data.c_str());
    return -1;
  }
  int col[4] = {-1, -1, -1, -1}, off[4] = {0, 0, 0, 0}, fsz[4] = {0, 0, 0, 0};
  bool colour_is_float = true;
  int ncol = 0, rec = 0;
  for (size_t i = 0; i < names.size(); ++i) {
    const int a = names[i] == "x" ? 0 : names[i] == "y" ? 1 : names[i] == "z" ? 2 : -1;
    if (colour && (names[i] == "rgb" || names[i] == "rgba")) {
      if (sizes[i] != 4 || counts[i] != 1 || (types[i] != "F" && types[i] != "U" && types[i] != "I")) {
        std::fprintf(stderr, "[pcd] %s: field %s must be one 4-byte value\n", path.c_str(), names[i].c_str());
        return -1;
      }
      col[3] = ncol;
      off[3] = rec;
      fsz[3] = 4;
      colour_is_float = types[i] == "F";
    }
    if (a >= 0) {
      if (types[i] != "F" || (sizes[i] != 4 && sizes[i] != 8) || counts[i] != 1) {
        std::fprintf(stderr, "[pcd] %s: field %s must be one float\n", path.c_str(), names[i].c_str());
        return -1;
      }
      col[a] = ncol;
      off[a] = rec;
      fsz[a] = sizes[i];
    }
    if (sizes[i] <= 0 || counts[i] <= 0) {
      std::fprintf(stderr, "[pcd] %s: malformed header\n", path.c_str());
      return -1;
    }
    ncol += counts[i];
    rec += sizes[i] * counts[i];
  }
  if (col[0] < 0 || col[1] < 0 || col[2] < 0) {
    std::fprintf(stderr, "[pcd] %s: no x y z fields\n", path.c_str());
    return -1;
  }
  PcdFile out;
  out.points.resize((size_t)points);
  bool dense = true;
  if (data == "binary") {
    if (buf.size() < pos || (unsigned long long)(buf.size() - pos) < (unsigned long long)points * rec) {
      std::fprintf(stderr, "[pcd] %s: truncated binary data\n", path.c_str());
      return -1;
    }
    for (long long k = 0; k < points; ++k) {
      const char* r = &buf[pos] + (size_t)k * rec;
      float v[3];
      for (int a = 0; a < 3; ++a) {
        if (fsz[a] == 4) {
          std::memcpy(&v[a], r + off[a], 4);
        } else {
          double d;
          std::memcpy(&d, r + off[a], 8);
          v[a] = (float)d;
        }
      }
      PcdRecord q = {{v[0], v[1], v[2]}, 0};
      if (col[3] >= 0) std::memcpy(&q.c, r + off[3], 4);
      out.points[(size_t)k] = q;
    }
  } else {
    const char* p = buf.empty() ? "" : &buf[0];
    const char* end = p + buf.size();
    p += std::min(pos, buf.size());
    std::string tok;
    for (long long k = 0; k < points; ++k) {
      float v[3] = {0, 0, 0};
      uint32_t packed = 0;
      for (int c = 0; c < ncol; ++c) {
        while (p < end && (*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) ++p;
        const char* s = p;
        while (p < end && !(*p == ' ' || *p == '\t' || *p == '\r' || *p == '\n')) ++p;
        if (s == p) {
          std::fprintf(stderr, "[pcd] %s: truncated ascii data (point %lld)\n", path.c_str(), k);
          return -1;
        }
        for (int a = 0; a < 3; ++a)
          if (c == col[a]) {
            tok.assign(s, p - s);
            char* q = nullptr;
            v[a] = std::strtof(tok.c_str(), &q);
            if (q == tok.c_str()) {
              std::fprintf(stderr, "[pcd] %s: bad number '%s'\n", path.c_str(), tok.c_str());
              return -1;
            }
          }
        if (c == col[3]) {
          tok.assign(s, p - s);
          char* q = nullptr;
          if (colour_is_float) {
            const float fc = std::strtof(tok.c_str(), &q);  // (8 digits give the packed bits back, subnormals included)
            std::memcpy(&packed, &fc, 4);
          } else {
            packed = (uint32_t)std::strtoll(tok.c_str(), &q, 10);
          }
          if (q == tok.c_str()) {
            std::fprintf(stderr, "[pcd] %s: bad number '%s'\n", path.c_str(), tok.c_str());
            return -1;
          }
        }
      }
      PcdRecord q = {{v[0], v[1], v[2]}, packed};
      out.points[(size_t)k] = q;
    }
  }
  for (const PcdRecord& q : out.points) dense = dense && std::isfinite(q.v[0]) && std::isfinite(q.v[1]) && std::isfinite(q.v[2]);
  out.width = (uint32_t)width;
  out.height = (uint32_t)height;
  out.is_dense = dense;
  for (int k = 0; k < 3; ++k) out.origin[k] = vp[k];
  file = out;
  return 0;
}

template <typename T, typename F>
inline int loadPCDInto(const std::string& path, bool colour, PointCloud<T>& cloud, F make) {
  cloud = PointCloud<T>();
  PcdFile f;
  if (readPCD(path, colour, f) != 0) return -1;
  cloud.points.resize(f.points.size());
  for (size_t k = 0; k < f.points.size(); ++k) cloud.points[k] = make(f.points[k]);
  cloud.width = f.width;
  cloud.height = f.height;
  cloud.is_dense = f.is_dense;
  for (int k = 0; k < 3; ++k) cloud.sensor_origin_[k] = f.origin[k];
  cloud.sensor_origin_[3] = 0;
  return 0;
}

// pcl::io::loadPCDFile(path, cloud) for PointXYZ and for PointXYZRGB (the cloud is left empty on failure)
inline int loadPCDFile(const std::string& path, PointCloud<PointXYZ>& cloud) {
  return loadPCDInto(path, false, cloud, [](const PcdRecord& q) { return PointXYZ(q.v[0], q.v[1], q.v[2]); });
}
inline int loadPCDFile(const std::string& path, PointCloud<PointXYZRGB>& cloud) {
  return loadPCDInto(path, true, cloud, [](const PcdRecord& q) { return PointXYZRGB(q.v[0], q.v[1], q.v[2], q.c & 0x00FFFFFFu); });
}

}  // namespace io

// ---- pcl::VoxelGrid and pcl::StatisticalOutlierRemoval with PCL's setters and filter(output), forwarding to
// sfmhip_cloud_voxel_grid / sfmhip_cloud_statistical_outlier (include/sfmhip.h, rules V1-V7 and S1-S5): code written
// against PCL compiles against these.  Templates, so a program that never filters (the CPU tests) links without the library.
namespace detail {

template <typename T>
struct Attr {  // what setDownsampleAllData averages besides x, y, z
  static const bool rgb = false, normal = false;
  static uint32_t colour(const T&) { return 0; }
  static void set_colour(T&, uint32_t) {}
  static void get_normal(const T&, float*) {}
  static void set_normal(T&, const float*) {}
};
template <>
struct Attr<PointXYZRGB> {
  static const bool rgb = true, normal = false;
  static uint32_t colour(const PointXYZRGB& p) { return p.rgba; }
  static void set_colour(PointXYZRGB& p, uint32_t c) { p.rgba = c; }
  static void get_normal(const PointXYZRGB&, float*) {}
  static void set_normal(PointXYZRGB&, const float*) {}
};
template <>
struct Attr<PointNormal> {  // (the curvature is not averaged: it is left 0)
  static const bool rgb = false, normal = true;
  static uint32_t colour(const PointNormal&) { return 0; }
  static void set_colour(PointNormal&, uint32_t) {}
  static void get_normal(const PointNormal& p, float* n) { n[0] = p.normal_x, n[1] = p.normal_y, n[2] = p.normal_z; }
  static void set_normal(PointNormal& p, const float* n) { p.normal_x = n[0], p.normal_y = n[1], p.normal_z = n[2]; }
};

inline void filter_check(int rc, const char* what) {
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[pcl] %s: %s\n", what, sfmhip_error_string(rc));
    std::abort();  // (no CPU fallback behind the drop-in)
  }
}

template <typename T>
inline sfmhip_cloud* upload(const PointCloud<T>& c) {
  std::vector<float> xyz(3 * c.size() + 3);
  for (size_t i = 0; i < c.size(); ++i) xyz[3 * i] = c.points[i].x, xyz[3 * i + 1] = c.points[i].y, xyz[3 * i + 2] = c.points[i].z;
  sfmhip_cloud* h = nullptr;
  filter_check(sfmhip_cloud_create(sfm_hip_context(), (int)c.size(), xyz.data(), &h), "sfmhip_cloud_create");
  return h;
}

template <typename T>
inline void like(const PointCloud<T>& in, size_t m, PointCloud<T>& out) {
  out.points.resize(m);
  out.width = (uint32_t)m;
  out.height = 1;
  out.is_dense = true;  // (both filters drop the non-finite points)
  for (int a = 0; a < 4; ++a) out.sensor_origin_[a] = in.sensor_origin_[a];
}

}  // namespace detail

template <typename PointT>
class VoxelGrid {
 public:
  void setInputCloud(const typename PointCloud<PointT>::Ptr& cloud) { input_ = cloud; }
  void setLeafSize(float lx, float ly, float lz) { leaf_[0] = lx, leaf_[1] = ly, leaf_[2] = lz; }
  void setMinimumPointsNumberPerVoxel(unsigned int min_points) { min_points_ = min_points; }
  void setDownsampleAllData(bool downsample) { all_data_ = downsample; }
  // the centroids in ascending voxel index; a grid of more than INT32_MAX voxels warns and copies the input, as PCL does
  void filter(PointCloud<PointT>& output) {
    typedef detail::Attr<PointT> A;
    const PointCloud<PointT> in = input_ ? *input_ : PointCloud<PointT>();
    const size_t n = in.size();
    const bool rgb = all_data_ && A::rgb, nrm = all_data_ && A::normal;
    std::vector<uint32_t> col(rgb ? n + 1 : 0), ocol(rgb ? n + 1 : 0);
    std::vector<float> nv(nrm ? 3 * n + 3 : 0), onv(nrm ? 3 * n + 3 : 0), oxyz(3 * n + 3);
    for (size_t i = 0; i < n && rgb; ++i) col[i] = A::colour(in.points[i]);
    for (size_t i = 0; i < n && nrm; ++i) A::get_normal(in.points[i], &nv[3 * i]);
    sfmhip_cloud* h = detail::upload(in);
    int32_t m = 0;
    const int rc = sfmhip_cloud_voxel_grid(h, leaf_, (int)min_points_, rgb ? col.data() : nullptr, nrm ? nv.data() : nullptr, oxyz.data(),
                                           rgb ? ocol.data() : nullptr, nrm ? onv.data() : nullptr, nullptr, &m, nullptr);
    sfmhip_cloud_destroy(h);
    if (rc == SFMHIP_ERR_UNSUPPORTED) {
      std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
      output = in;
      return;
    }
    detail::filter_check(rc, "sfmhip_cloud_voxel_grid");
    PointCloud<PointT> out;
    detail::like(in, (size_t)m, out);
    for (int32_t r = 0; r < m; ++r) {
      PointT p = PointT();
      p.x = oxyz[3 * r], p.y = oxyz[3 * r + 1], p.z = oxyz[3 * r + 2];
      if (rgb) A::set_colour(p, ocol[r]);
      if (nrm) A::set_normal(p, &onv[3 * r]);
      out.points[r] = p;
    }
    output = out;
  }

 private:
  typename PointCloud<PointT>::Ptr input_;
  float leaf_[3] = {0, 0, 0};
  unsigned int min_points_ = 0;
  bool all_data_ = true;
};

template <typename PointT>
class StatisticalOutlierRemoval {
 public:
  void setInputCloud(const typename PointCloud<PointT>::Ptr& cloud) { input_ = cloud; }
  void setMeanK(int mean_k) { mean_k_ = mean_k; }
  void setStddevMulThresh(double std_mul) { std_mul_ = std_mul; }
  void setNegative(bool negative) { negative_ = negative; }
  // the kept points in input order (mean_k in 1..63; more finite points than mean_k)
  void filter(PointCloud<PointT>& output) {
    const PointCloud<PointT> in = input_ ? *input_ : PointCloud<PointT>();
    std::vector<int32_t> idx(in.size() + 1);
    int32_t m = 0;
    sfmhip_cloud* h = detail::upload(in);
    const int rc = sfmhip_cloud_statistical_outlier(h, mean_k_, std_mul_, negative_ ? 1 : 0, idx.data(), &m, nullptr, nullptr);
    sfmhip_cloud_destroy(h);
    detail::filter_check(rc, "sfmhip_cloud_statistical_outlier");
    PointCloud<PointT> out;
    detail::like(in, (size_t)m, out);
    for (int32_t r = 0; r < m; ++r) out.points[r] = in.points[idx[r]];
    output = out;
  }

 private:
  typename PointCloud<PointT>::Ptr input_;
  int mean_k_ = 1;          // PCL's defaults
  double std_mul_ = 0.0;
  bool negative_ = false;
};

// pcl::MovingLeastSquares without upsampling (NONE, SIMPLE projection) over sfmhip_cloud_mls (include/sfmhip.h rules M1-M7,
// DESIGN.md f-23).  PCL 1.8.1's defaults: no polynomial fit (order 0 in the library's terms), order 2 once it is on, normals
// off, the Gaussian's parameter r * r unless set.  setSearchMethod is accepted and ignored: the search is the library's grid.
template <typename PointInT, typename PointOutT>
class MovingLeastSquares {
 public:
  void setInputCloud(const typename PointCloud<PointInT>::Ptr& cloud) { input_ = cloud; }
  template <typename Tree>
  void setSearchMethod(const Tree&) {}
  void setSearchRadius(double radius) { radius_ = radius; }
  void setPolynomialFit(bool fit) { fit_ = fit; }
  void setPolynomialOrder(int order) { order_ = order; }
  void setSqrGaussParam(double g) { gauss_ = g; }
  void setComputeNormals(bool compute) { normals_ = compute; }
  // the smoothed points in input order; points with fewer than 3 neighbours and non-finite points are left out
  void process(PointCloud<PointOutT>& output) {
    const PointCloud<PointInT> in = input_ ? *input_ : PointCloud<PointInT>();
    const size_t n = in.size();
    sfmhip_mls_opts o;
    sfmhip_mls_default_opts(&o);
    o.search_radius = radius_;
    o.polynomial_order = fit_ ? order_ : 0;
    o.compute_normals = normals_ ? 1 : 0;
    o.sqr_gauss_param = gauss_;
    std::vector<float> xyz(3 * n + 3), n4(4 * n + 4, 0.0f);
    std::vector<int32_t> src(n + 1);
    int32_t m = 0;
    sfmhip_cloud* h = detail::upload(in);
    const int rc = sfmhip_cloud_mls(h, &o, xyz.data(), n4.data(), src.data(), &m, nullptr, nullptr);
    sfmhip_cloud_destroy(h);
    detail::filter_check(rc, "sfmhip_cloud_mls");
    PointCloud<PointOutT> out;
    out.points.resize((size_t)m);
    out.width = (uint32_t)m;
    out.height = 1;
    out.is_dense = true;
    for (int a = 0; a < 4; ++a) out.sensor_origin_[a] = in.sensor_origin_[a];
    for (int32_t r = 0; r < m; ++r) {
      PointOutT p = PointOutT();
      p.x = xyz[3 * r], p.y = xyz[3 * r + 1], p.z = xyz[3 * r + 2];
      p.normal_x = n4[4 * r], p.normal_y = n4[4 * r + 1], p.normal_z = n4[4 * r + 2], p.curvature = n4[4 * r + 3];
      out.points[r] = p;
    }
    indices_.reset(new PointIndices);
    indices_->indices.assign(src.begin(), src.begin() + m);
    output = out;
  }
  // the input index of every output row (of the last process())
  std::shared_ptr<PointIndices> getCorrespondingIndices() const { return indices_; }

 private:
  typename PointCloud<PointInT>::Ptr input_;
  double radius_ = 0.0, gauss_ = 0.0;
  bool fit_ = false, normals_ = false;
  int order_ = 2;
  std::shared_ptr<PointIndices> indices_{new PointIndices};
};

// ---- pcl::IterativeClosestPoint, its similarity form and pcl::transformPointCloud with PCL's setters, forwarding to
// sfmhip_cloud_register / sfmhip_cloud_transform (include/sfmhip.h, DESIGN.md f-17 rules 1-8).  The matrix is the 4 x 4 float
// one PCL code reads the result from.  Not mirrored: reciprocal correspondences, RANSAC rejection, the Euclidean fitness epsilon.
// The rejectors of DESIGN.md f-22 are setters here (setTrimFraction: CorrespondenceRejectorTrimmed's overlap ratio; setOneToOne:
// CorrespondenceRejectorOneToOne), and pcl::IterativeClosestPointWithNormals is its point-to-plane metric; a call that uses
// any of them goes through sfmhip_cloud_register_icp, every other call through sfmhip_cloud_register as before.
}  // namespace pcl

namespace Eigen {
struct Matrix4f {
  float m[16];
  Matrix4f() {
    for (int i = 0; i < 16; ++i) m[i] = 0.0f;
  }
  static Matrix4f Identity() {
    Matrix4f M;
    M.m[0] = M.m[5] = M.m[10] = M.m[15] = 1.0f;
    return M;
  }
  float& operator()(int r, int c) { return m[4 * r + c]; }
  float operator()(int r, int c) const { return m[4 * r + c]; }
};
}  // namespace Eigen

namespace pcl {
namespace detail {

// the similarity of a 4 x 4 [s R | t]: s = cbrt(det), R = the block / s (the library wants finite entries and s > 0)
inline sfmhip_transform to_transform(const Eigen::Matrix4f& M) {
  const double a[9] = {M(0, 0), M(0, 1), M(0, 2), M(1, 0), M(1, 1), M(1, 2), M(2, 0), M(2, 1), M(2, 2)};
  const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
  sfmhip_transform T;
  T.scale = std::cbrt(det);
  for (int i = 0; i < 9; ++i) T.R[i] = a[i] / T.scale;
  for (int r = 0; r < 3; ++r) T.t[r] = M(r, 3);
  return T;
}
inline Eigen::Matrix4f to_matrix(const sfmhip_transform& T) {
  Eigen::Matrix4f M = Eigen::Matrix4f::Identity();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) M(r, c) = (float)(T.scale * T.R[3 * r + c]);
    M(r, 3) = (float)T.t[r];
  }
  return M;
}
template <typename T>
inline void download_into(sfmhip_cloud* h, const PointCloud<T>& in, PointCloud<T>& out) {
  std::vector<float> xyz(3 * in.size() + 3);
  filter_check(sfmhip_cloud_download(h, xyz.data()), "sfmhip_cloud_download");
  PointCloud<T> r = in;  // (every other field rides along)
  for (size_t i = 0; i < in.size(); ++i) r.points[i].x = xyz[3 * i], r.points[i].y = xyz[3 * i + 1], r.points[i].z = xyz[3 * i + 2];
  out = r;
}

}  // namespace detail

// x -> M x for every point (rule 2: f64, rounded once; a non-finite point stays), on the device
template <typename PointT>
inline void transformPointCloud(const PointCloud<PointT>& in, PointCloud<PointT>& out, const Eigen::Matrix4f& M) {
  const sfmhip_transform T = detail::to_transform(M);
  sfmhip_cloud *h = detail::upload(in), *moved = nullptr;
  const int rc = sfmhip_cloud_transform(h, &T, &moved);
  sfmhip_cloud_destroy(h);
  detail::filter_check(rc, "sfmhip_cloud_transform");
  detail::download_into(moved, in, out);
  sfmhip_cloud_destroy(moved);
}

template <typename PointSource, typename PointTarget>
class IterativeClosestPoint {
 public:
  void setInputSource(const typename PointCloud<PointSource>::Ptr& cloud) { source_ = cloud; }
  void setInputTarget(const typename PointCloud<PointTarget>::Ptr& cloud) { target_ = cloud; }
  void setMaxCorrespondenceDistance(double d) { max_dist_ = d; }
  void setMaximumIterations(int n) { max_iters_ = n; }
  void setTransformationEpsilon(double e) { eps_ = e; }
  void setEstimateScale(bool on) { with_scale_ = on; }  // (ours: TransformationEstimationSVDScale in place of ...SVD)
  void setTrimFraction(double keep) { trim_ = keep; }    // (ours: the kept fraction of the surviving pairs, (0, 1]; 1: off)
  void setOneToOne(bool on) { one_to_one_ = on; }        // (ours: a target point keeps only its best source)
  void align(PointCloud<PointSource>& output) { align(output, Eigen::Matrix4f::Identity()); }
  // the source under the final transformation; a guess must be a similarity with finite entries
  void align(PointCloud<PointSource>& output, const Eigen::Matrix4f& guess) {
    const PointCloud<PointSource> src = source_ ? *source_ : PointCloud<PointSource>();
    const PointCloud<PointTarget> tgt = target_ ? *target_ : PointCloud<PointTarget>();
    sfmhip_register_opts o;
    sfmhip_register_default_opts(&o);
    o.max_iters = max_iters_, o.with_scale = with_scale_ ? 1 : 0, o.max_dist = max_dist_, o.eps = eps_;
    const sfmhip_transform init = detail::to_transform(guess);
    sfmhip_cloud *hs = detail::upload(src), *ht = detail::upload(tgt), *moved = nullptr;
    int rc;
    if (metric_ == 0 && trim_ == 1.0 && !one_to_one_) {
      rc = sfmhip_cloud_register(ht, hs, &o, &init, &result_, nullptr);
      icp_result_ = sfmhip_icp_result();
    } else {  // f-22: the rejectors and the plane metric
      sfmhip_icp_opts io;
      sfmhip_icp_default_opts(&io);
      io.max_iters = o.max_iters, io.with_scale = o.with_scale, io.max_dist = o.max_dist, io.eps = o.eps;
      io.metric = metric_, io.one_to_one = one_to_one_ ? 1 : 0, io.trim = trim_, io.normal_stride = 3;
      if (metric_ == 1) io.min_pairs = with_scale_ ? 7 : 6, io.eps = eps_ > 0.0 ? eps_ : 1e-9;  // (the metric needs an eps)
      rc = sfmhip_cloud_register_icp(ht, hs, metric_ == 1 ? normals_.data() : nullptr, &io, &init, &icp_result_, nullptr);
      result_.T = icp_result_.T, result_.iterations = icp_result_.iterations, result_.pairs = icp_result_.pairs;
      result_.converged = icp_result_.converged, result_.flags = icp_result_.flags, result_.mse = icp_result_.mse;
    }
    if (rc == SFMHIP_OK) rc = sfmhip_cloud_transform(hs, &result_.T, &moved);
    sfmhip_cloud_destroy(hs);
    sfmhip_cloud_destroy(ht);
    detail::filter_check(rc, "sfmhip_cloud_register");
    detail::download_into(moved, src, output);
    sfmhip_cloud_destroy(moved);
  }
  bool hasConverged() const { return result_.flags == 0; }  // (PCL counts the iteration limit as a criterion met)
  double getFitnessScore() const { return result_.mse; }
  Eigen::Matrix4f getFinalTransformation() const { return detail::to_matrix(result_.T); }
  const sfmhip_register_result& result() const { return result_; }  // (ours: the f64 transform, the counts and the flags)
  const sfmhip_icp_result& icpResult() const { return icp_result_; }  // (ours: plane_mse and trim_d2 too; zeros after an f-17 call)

 protected:
  typename PointCloud<PointSource>::Ptr source_;
  typename PointCloud<PointTarget>::Ptr target_;
  double max_dist_ = INFINITY, eps_ = 0.0;  // PCL: sqrt(DBL_MAX) and 0
  int max_iters_ = 10;                      // PCL's default
  bool with_scale_ = false, one_to_one_ = false;
  double trim_ = 1.0;
  int metric_ = 0;               // 1: set by IterativeClosestPointWithNormals
  std::vector<float> normals_;   // ... with the target's normals, 3 floats a point
  sfmhip_register_result result_ = sfmhip_register_result();
  sfmhip_icp_result icp_result_ = sfmhip_icp_result();
};

// (ours) the similarity form under a name of its own
template <typename PointSource, typename PointTarget>
class IterativeClosestPointWithScale : public IterativeClosestPoint<PointSource, PointTarget> {
 public:
  IterativeClosestPointWithScale() { this->with_scale_ = true; }
};

// pcl::IterativeClosestPointWithNormals: the point-to-plane metric (f-22 rule 8) against the normals the target's points carry
// (a PointNormal target); a target row whose normal is zero or non-finite takes no part
template <typename PointSource, typename PointTarget>
class IterativeClosestPointWithNormals : public IterativeClosestPoint<PointSource, PointTarget> {
 public:
  IterativeClosestPointWithNormals() { this->metric_ = 1; }
  void align(PointCloud<PointSource>& output) { align(output, Eigen::Matrix4f::Identity()); }
  void align(PointCloud<PointSource>& output, const Eigen::Matrix4f& guess) {
    const size_t n = this->target_ ? this->target_->size() : 0;
    this->normals_.assign(3 * n + 3, 0.0f);
    for (size_t i = 0; i < n; ++i) {
      const PointTarget& p = this->target_->points[i];
      this->normals_[3 * i] = p.normal_x, this->normals_[3 * i + 1] = p.normal_y, this->normals_[3 * i + 2] = p.normal_z;
    }
    IterativeClosestPoint<PointSource, PointTarget>::align(output, guess);
  }
};

}  // namespace pcl
