// SfmCloud.cpp -- map3D's step 10 on the dense cloud (reference src/Sfm.cpp:94-102, bodies :1323-1383) in the host
// mirror: cloudPointFilter, removePoints, create_mesh (normals, then Poisson) and finishMesh over sfmhip_cloud_* (cloud.hip, poisson.hip, mesh.hip).  Kept out
// of Sfm.cpp / SfmIO.cpp, which the oracle's sanitizer builds link against a CPU stub of the C ABI.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "Sfm.h"
#include "hip_backend.h"

namespace {

// the one device cloud the three calls share: the handle of the last cloud asked for, keyed by its point count and an
// FNV-1a hash of its bytes (so a cloud edited in place gets a fresh upload).  Replaced, never freed at exit.
struct DeviceCloud {
  sfmhip_cloud* h = nullptr;
  size_t n = 0;
  uint64_t hash = 0;
};

uint64_t hash_points(const std::vector<pcl::PointXYZ>& p) {
  const unsigned char* b = reinterpret_cast<const unsigned char*>(p.data());
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < p.size() * sizeof(pcl::PointXYZ); ++i) h = (h ^ b[i]) * 1099511628211ull;
  return h;
}

sfmhip_cloud* device_cloud(const pcl::PointCloud<pcl::PointXYZ>& c) {
  static DeviceCloud cache;
  const uint64_t h = hash_points(c.points);
  if (cache.h && cache.n == c.size() && cache.hash == h) return cache.h;
  if (cache.h) sfmhip_cloud_destroy(cache.h);
  cache = DeviceCloud();
  static_assert(sizeof(pcl::PointXYZ) == 12, "PointXYZ is three packed floats");
  const int rc = sfmhip_cloud_create(sfm_hip_context(), (int)c.size(), c.size() ? &c.points[0].x : nullptr, &cache.h);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_create: %s\n", sfmhip_error_string(rc));
    std::abort();
  }
  cache.n = c.size();
  cache.hash = h;
  return cache.h;
}

void check(int rc, const char* what) {
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] %s: %s\n", what, sfmhip_error_string(rc));
    std::abort();  // (no CPU fallback behind the drop-in)
  }
}

void take(const pcl::PointCloud<pcl::PointXYZ>& in, const std::vector<int32_t>& idx, int32_t m,
          pcl::PointCloud<pcl::PointXYZ>& out) {
  pcl::PointCloud<pcl::PointXYZ> r;
  r.points.resize((size_t)m);
  for (int32_t i = 0; i < m; ++i) r.points[i] = in.points[idx[i]];
  r.width = (uint32_t)m;
  r.height = 1;
  r.is_dense = in.is_dense;
  for (int a = 0; a < 4; ++a) r.sensor_origin_[a] = in.sensor_origin_[a];
  out = r;
}

// create_mesh's second half on a device cloud `h` whose normals (rows of 4 floats, flipped already) are `nrm`: pcl::Poisson
// with the reference's setters, the mesh read back into `mesh`
void poisson_mesh(sfmhip_cloud* h, const std::vector<float>& nrm, pcl::PolygonMesh& mesh, double* cell = nullptr) {
  sfmhip_poisson_opts o;
  sfmhip_poisson_default_opts(&o);  // setDepth(7), setPointWeight(4), setScale(1.1); rows of 4 floats
  // the default cap of 4 * 2^depth steps ends conjugate gradients short of cg_rtol at depth 7 (about
  // 6 * 2^depth steps are needed); twice the default lets the solve converge
  o.cg_max_iter = 8 << o.depth;
  sfmhip_mesh* m = nullptr;
  sfmhip_poisson_summary s;
  check(sfmhip_cloud_poisson(h, nrm.data(), &o, &m, &s), "sfmhip_cloud_poisson");
  if (s.cg_iterations >= o.cg_max_iter && s.cg_relative_residual > o.cg_rtol)
    std::fprintf(stderr, "create_mesh: the Poisson solve stopped at its cap of %d steps with relative residual %.3e (cg_rtol %.1e)\n",
                 (int)o.cg_max_iter, s.cg_relative_residual, o.cg_rtol);
  std::vector<float> v(3 * (size_t)s.n_vertices + 3);
  std::vector<int32_t> t(3 * (size_t)s.n_triangles + 3);
  check(sfmhip_mesh_download(m, v.data(), t.data()), "sfmhip_mesh_download");
  sfmhip_mesh_destroy(m);
  if (cell) *cell = s.cell;
  mesh = pcl::PolygonMesh();
  mesh.cloud.points.resize((size_t)s.n_vertices);
  for (int i = 0; i < s.n_vertices; ++i) mesh.cloud.points[i] = pcl::PointXYZ(v[3 * i], v[3 * i + 1], v[3 * i + 2]);
  mesh.cloud.width = (uint32_t)s.n_vertices;
  mesh.cloud.height = 1;
  mesh.polygons.resize((size_t)s.n_triangles);
  for (int i = 0; i < s.n_triangles; ++i)
    mesh.polygons[i].vertices = {(uint32_t)t[3 * i], (uint32_t)t[3 * i + 1], (uint32_t)t[3 * i + 2]};
}

}  // namespace

void StructFromMotion::cloudPointFilter(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud,
                                        pcl::PointCloud<pcl::PointXYZ>::Ptr& filterCloud) {
  std::vector<int32_t> idx(cloud->size() + 1);
  int32_t m = 0;
  check(sfmhip_cloud_passthrough(device_cloud(*cloud), 0, 0.003f, 0.83f, 0, idx.data(), &m), "sfmhip_cloud_passthrough");
  if (!filterCloud) filterCloud.reset(new pcl::PointCloud<pcl::PointXYZ>);
  take(*cloud, idx, m, *filterCloud);
}

void StructFromMotion::removePoints(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud,
                                    pcl::PointCloud<pcl::PointXYZ>::Ptr& filterCloud) {
  std::vector<int32_t> idx(cloud->size() + 1);
  int32_t m = 0;
  check(sfmhip_cloud_radius_outlier(device_cloud(*cloud), 0.07, 150, idx.data(), &m), "sfmhip_cloud_radius_outlier");
  if (!filterCloud) filterCloud.reset(new pcl::PointCloud<pcl::PointXYZ>);
  take(*cloud, idx, m, *filterCloud);
}

void StructFromMotion::computeNormals(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PointCloud<pcl::Normal>::Ptr& normals) {
  const size_t n = cloud->size();
  std::vector<float> out(4 * n + 4);
  const float vp[3] = {cloud->sensor_origin_[0], cloud->sensor_origin_[1], cloud->sensor_origin_[2]};  // (use_sensor_origin_)
  check(sfmhip_cloud_normals(device_cloud(*cloud), 10, vp, out.data()), "sfmhip_cloud_normals");
  if (!normals) normals.reset(new pcl::PointCloud<pcl::Normal>);
  pcl::PointCloud<pcl::Normal> r;
  r.points.resize(n);
  bool dense = true;
  for (size_t i = 0; i < n; ++i) {
    pcl::Normal& q = r.points[i];
    q.normal_x = -out[4 * i];  // create_mesh: every normal times -1 (src/Sfm.cpp:1358-1362)
    q.normal_y = -out[4 * i + 1];
    q.normal_z = -out[4 * i + 2];
    q.curvature = out[4 * i + 3];
    dense = dense && q.normal_x == q.normal_x;
  }
  r.width = (uint32_t)n;
  r.height = 1;
  r.is_dense = dense;
  for (int a = 0; a < 4; ++a) r.sensor_origin_[a] = cloud->sensor_origin_[a];
  *normals = r;
}

void StructFromMotion::create_mesh(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PolygonMesh& mesh) {
  pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
  computeNormals(cloud, normals);  // (flipped already)
  // pcl::concatenateFields(*cloud, *normals, *cloud_smoothed_normals): the points are on the device already, so only
  // the normals are laid out, in the 4-float rows sfmhip_cloud_poisson reads
  std::vector<float> nrm(4 * cloud->size() + 4);
  for (size_t i = 0; i < cloud->size(); ++i) {
    const pcl::Normal& q = normals->points[i];
    nrm[4 * i] = q.normal_x, nrm[4 * i + 1] = q.normal_y, nrm[4 * i + 2] = q.normal_z, nrm[4 * i + 3] = q.curvature;
  }
  poisson_mesh(device_cloud(*cloud), nrm, mesh);
}

void StructFromMotion::smoothCloud(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, double radius, int order,
                                   pcl::PointCloud<pcl::PointNormal>::Ptr& smoothed) {
  pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> mls;
  mls.setInputCloud(cloud);
  mls.setSearchRadius(radius);
  mls.setPolynomialFit(order > 0);
  if (order > 0) mls.setPolynomialOrder(order);
  mls.setComputeNormals(true);
  if (!smoothed) smoothed.reset(new pcl::PointCloud<pcl::PointNormal>);
  mls.process(*smoothed);
}

void StructFromMotion::create_mesh(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PolygonMesh& mesh, double smooth_radius) {
  // the pass the reference's create_mesh left commented out (`ne.setInputCloud (cloud_smoothed)`): MovingLeastSquares at
  // order 2, then the normals and Poisson on the smoothed cloud, which stays on the device from the smoothing to the mesh
  sfmhip_mls_opts mo;
  sfmhip_mls_default_opts(&mo);
  mo.search_radius = smooth_radius;
  mo.compute_normals = 0;
  int32_t m = 0;
  sfmhip_cloud* sm = nullptr;
  check(sfmhip_cloud_mls(device_cloud(*cloud), &mo, nullptr, nullptr, nullptr, &m, nullptr, &sm), "sfmhip_cloud_mls");
  std::vector<float> nrm(4 * (size_t)m + 4);
  const float vp[3] = {cloud->sensor_origin_[0], cloud->sensor_origin_[1], cloud->sensor_origin_[2]};
  const int rc = sfmhip_cloud_normals(sm, 10, vp, nrm.data());
  if (rc != SFMHIP_OK) sfmhip_cloud_destroy(sm);
  check(rc, "sfmhip_cloud_normals");
  for (int32_t i = 0; i < m; ++i)
    for (int a = 0; a < 3; ++a) nrm[4 * (size_t)i + a] = -nrm[4 * (size_t)i + a];  // create_mesh: every normal times -1
  poisson_mesh(sm, nrm, mesh);
  sfmhip_cloud_destroy(sm);
}

namespace {

// the positions of a coloured cloud as the PointXYZ cloud the device cache is keyed by, and its colours
void split_colours(const pcl::PointCloud<pcl::PointXYZRGB>& in, pcl::PointCloud<pcl::PointXYZ>& xyz, std::vector<uint32_t>& rgb) {
  xyz.points.resize(in.size());
  rgb.resize(in.size() + 1);
  for (size_t i = 0; i < in.size(); ++i) {
    xyz.points[i] = pcl::PointXYZ(in.points[i].x, in.points[i].y, in.points[i].z);
    rgb[i] = in.points[i].rgba & 0x00FFFFFFu;
  }
  xyz.width = (uint32_t)in.size();
  xyz.height = 1;
  xyz.is_dense = in.is_dense;
  for (int a = 0; a < 4; ++a) xyz.sensor_origin_[a] = in.sensor_origin_[a];
}

sfmhip_mesh_finish_summary finish_mesh(sfmhip_cloud* h, const std::vector<uint32_t>& rgb, pcl::PolygonMesh& mesh, const sfmhip_mesh_finish_opts& opts) {
  const size_t nv = mesh.cloud.size(), nt = mesh.polygons.size();
  std::vector<float> v(3 * nv + 3);
  std::vector<int32_t> t(3 * nt + 3);
  for (size_t i = 0; i < nv; ++i) v[3 * i] = mesh.cloud.points[i].x, v[3 * i + 1] = mesh.cloud.points[i].y, v[3 * i + 2] = mesh.cloud.points[i].z;
  for (size_t i = 0; i < nt; ++i) {
    if (mesh.polygons[i].vertices.size() != 3) {
      std::fprintf(stderr, "[sfm] finishMesh: polygon %zu is not a triangle\n", i);
      std::abort();
    }
    for (int k = 0; k < 3; ++k) t[3 * i + k] = (int32_t)mesh.polygons[i].vertices[k];
  }
  sfmhip_mesh *in = nullptr, *out = nullptr;
  check(sfmhip_mesh_create(v.data(), (int)nv, t.data(), (int)nt, &in), "sfmhip_mesh_create");
  sfmhip_mesh_finish_summary s;
  const int rc = sfmhip_cloud_mesh_finish(h, rgb.data(), in, &opts, &out, &s);
  sfmhip_mesh_destroy(in);
  check(rc, "sfmhip_cloud_mesh_finish");
  std::vector<float> ov(3 * (size_t)s.n_vertices + 3), on(3 * (size_t)s.n_vertices + 3);
  std::vector<int32_t> ot(3 * (size_t)s.n_triangles + 3);
  std::vector<uint32_t> oc((size_t)s.n_vertices + 1);
  check(sfmhip_mesh_download(out, ov.data(), ot.data()), "sfmhip_mesh_download");
  check(sfmhip_mesh_attributes(out, on.data(), oc.data(), nullptr, nullptr, nullptr, nullptr, nullptr), "sfmhip_mesh_attributes");
  sfmhip_mesh_destroy(out);
  mesh = pcl::PolygonMesh();
  mesh.cloud.points.resize((size_t)s.n_vertices);
  mesh.colours.assign(oc.begin(), oc.begin() + s.n_vertices);
  mesh.normals.resize((size_t)s.n_vertices);
  for (int i = 0; i < s.n_vertices; ++i) {
    mesh.cloud.points[i] = pcl::PointXYZ(ov[3 * i], ov[3 * i + 1], ov[3 * i + 2]);
    mesh.normals[i].normal_x = on[3 * i], mesh.normals[i].normal_y = on[3 * i + 1], mesh.normals[i].normal_z = on[3 * i + 2];
  }
  mesh.cloud.width = (uint32_t)s.n_vertices;
  mesh.cloud.height = 1;
  mesh.polygons.resize((size_t)s.n_triangles);
  for (int i = 0; i < s.n_triangles; ++i) mesh.polygons[i].vertices = {(uint32_t)ot[3 * i], (uint32_t)ot[3 * i + 1], (uint32_t)ot[3 * i + 2]};
  return s;
}

}  // namespace

sfmhip_mesh_finish_summary StructFromMotion::finishMesh(const pcl::PointCloud<pcl::PointXYZRGB>& cloud, pcl::PolygonMesh& mesh,
                                                        const sfmhip_mesh_finish_opts& opts) {
  pcl::PointCloud<pcl::PointXYZ> xyz;
  std::vector<uint32_t> rgb;
  split_colours(cloud, xyz, rgb);
  return finish_mesh(device_cloud(xyz), rgb, mesh, opts);
}

void StructFromMotion::create_mesh(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloud, pcl::PolygonMesh& mesh, sfmhip_mesh_finish_summary* summary) {
  pcl::PointCloud<pcl::PointXYZ>::Ptr xyz(new pcl::PointCloud<pcl::PointXYZ>);
  std::vector<uint32_t> rgb;
  split_colours(*cloud, *xyz, rgb);
  pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
  computeNormals(xyz, normals);  // (flipped already)
  std::vector<float> nrm(4 * xyz->size() + 4);
  for (size_t i = 0; i < xyz->size(); ++i) {
    const pcl::Normal& q = normals->points[i];
    nrm[4 * i] = q.normal_x, nrm[4 * i + 1] = q.normal_y, nrm[4 * i + 2] = q.normal_z, nrm[4 * i + 3] = q.curvature;
  }
  double cell = 0.0;
  poisson_mesh(device_cloud(*xyz), nrm, mesh, &cell);
  sfmhip_mesh_finish_opts o;
  sfmhip_mesh_finish_default_opts(&o);  // min_support 1, the component filters off
  o.support_radius = cell > 0.0 ? 1.5 * cell : 1.0;  // (no sample: no cube, an empty mesh)
  const sfmhip_mesh_finish_summary s = finish_mesh(device_cloud(*xyz), rgb, mesh, o);
  if (summary) *summary = s;
}

double StructFromMotion::registerCloud(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, const pcl::PointCloud<pcl::PointXYZ>& reference,
                                       double* scale_out, double max_dist, const sfmhip_transform* guess, sfmhip_register_result* result) {
  sfmhip_cloud* ref = nullptr;
  check(sfmhip_cloud_create(sfm_hip_context(), (int)reference.size(), reference.size() ? &reference.points[0].x : nullptr, &ref),
        "sfmhip_cloud_create");
  sfmhip_register_opts o;
  sfmhip_register_default_opts(&o);
  o.with_scale = 1;
  o.max_dist = max_dist;
  sfmhip_register_result res;
  const int rc = sfmhip_cloud_register(ref, device_cloud(*cloud), &o, guess, &res, nullptr);
  sfmhip_cloud_destroy(ref);
  check(rc, "sfmhip_cloud_register");
  const double scale = res.flags == 0 ? res.T.scale : 0.0;
  if (scale_out) *scale_out = scale;
  if (result) *result = res;
  return scale;
}

double StructFromMotion::registerCloud(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, const pcl::PointCloud<pcl::PointXYZ>& reference,
                                       const sfmhip_icp_opts& opts, const float* reference_normals, const sfmhip_transform* guess,
                                       sfmhip_icp_result* result) {
  sfmhip_cloud* ref = nullptr;
  check(sfmhip_cloud_create(sfm_hip_context(), (int)reference.size(), reference.size() ? &reference.points[0].x : nullptr, &ref),
        "sfmhip_cloud_create");
  sfmhip_icp_opts o = opts;
  std::vector<float> own;
  int rc = SFMHIP_OK;
  if (o.metric == 1 && !reference_normals) {  // the reference's own normals, towards the origin as create_mesh takes them
    own.resize(4 * reference.size() + 4);
    const float vp[3] = {0.0f, 0.0f, 0.0f};
    rc = sfmhip_cloud_normals(ref, 10, vp, own.data());
    reference_normals = own.data();
    o.normal_stride = 4;
  }
  sfmhip_icp_result res;
  if (rc == SFMHIP_OK) rc = sfmhip_cloud_register_icp(ref, device_cloud(*cloud), reference_normals, &o, guess, &res, nullptr);
  sfmhip_cloud_destroy(ref);
  check(rc, "sfmhip_cloud_register_icp");
  if (result) *result = res;
  return res.flags == 0 ? res.T.scale : 0.0;
}

int StructFromMotion::alignPlots(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, const pcl::PointCloud<pcl::PointXYZ>& reference,
                                 const sfmhip_align_opts& opts, sfmhip_align_result* result, const sfmhip_ground_opts* ground) {
  sfmhip_cloud* ref = nullptr;
  check(sfmhip_cloud_create(sfm_hip_context(), (int)reference.size(), reference.size() ? &reference.points[0].x : nullptr, &ref),
        "sfmhip_cloud_create");
  sfmhip_cloud* src = device_cloud(*cloud);
  sfmhip_ground_result g[2];
  sfmhip_frame f[2];
  sfmhip_ground_opts go;
  sfmhip_ground_default_opts(&go);
  if (ground) go = *ground;
  int rc = sfmhip_cloud_ground_plane(ref, nullptr, 0, &go, nullptr, 0, &g[0]);
  if (rc == SFMHIP_OK) rc = sfmhip_cloud_ground_plane(src, nullptr, 0, &go, nullptr, 0, &g[1]);
  const bool planes = rc == SFMHIP_OK && sfmhip_frame_from_ground(&g[0], &f[0]) == SFMHIP_OK && sfmhip_frame_from_ground(&g[1], &f[1]) == SFMHIP_OK;
  sfmhip_align_result res;
  if (planes) rc = sfmhip_cloud_align(ref, src, &f[0], &f[1], &opts, &res);
  sfmhip_cloud_destroy(ref);
  check(rc, planes ? "sfmhip_cloud_align" : "sfmhip_cloud_ground_plane");
  if (!planes) return -1;
  if (result) *result = res;
  return res.flags;
}
