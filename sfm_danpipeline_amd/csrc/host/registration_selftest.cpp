// registration_selftest.cpp -- two reconstructions of one plot become one cloud in metres, written against
// PCL's classes as pcllite.h mirrors them and the host mirror's registerCloud; needs the GPU, takes no input:
//   registration_selftest [scale]
//   registration_selftest --icp     (the plane metric and the rejectors on the same two plots, see run_icp)
// A planted plot in metres (a ground disc with three trees: plot A) and a second sampling of it in another gauge (plot B:
// every second point, moved by the inverse of a 4 degree, 0.3 m motion and divided by `scale`, 1.04 without the argument).
// pcl::IterativeClosestPointWithScale aligns B to A, StructFromMotion::registerCloud gives the metres per unit of B,
// pcl::transformPointCloud moves B, sfmhip_cloud_concat joins the two on the device, sfmhip_cloud_voxel_grid thins the sum
// without an upload, and Dendrometry::estimatePlot measures its trees.  One line per step ("<step>: ..."), estimatePlot's own
// lines between the last two.  Exit 3: the registration has a flag set; 4: a step after it failed.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "DendrometryE.h"
#include "Sfm.h"
#include "hip_backend.h"

static uint32_t rng_state = 2024u;
static double rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) / 16777216.0;
}
static double gauss() {
  double s = 0;
  for (int i = 0; i < 12; ++i) s += rnd();
  return s - 6.0;
}

// --icp: pcl::IterativeClosestPointWithNormals against A with its planted normals (the ground's up, a trunk's radial, a
// crown shell's gradient), then with the trimmed and with the one-to-one rejector, then registerCloud's options overload with
// the similarity plane metric on the reference's own k-NN normals.  One line per step; exit 3: a flag is set
static int run_icp(const pcl::PointCloud<pcl::PointXYZ>::Ptr& A, const pcl::PointCloud<pcl::PointXYZ>::Ptr& B, const std::vector<float>& normals,
                   double scale) {
  pcl::PointCloud<pcl::PointNormal>::Ptr An(new pcl::PointCloud<pcl::PointNormal>);
  for (size_t i = 0; i < A->size(); ++i) {
    pcl::PointNormal p;
    p.x = A->points[i].x, p.y = A->points[i].y, p.z = A->points[i].z;
    p.normal_x = normals[3 * i], p.normal_y = normals[3 * i + 1], p.normal_z = normals[3 * i + 2];
    An->push_back(p);
  }
  Eigen::Matrix4f guess = Eigen::Matrix4f::Identity();
  for (int i = 0; i < 3; ++i) guess(i, i) = (float)scale;  // (the rigid metric keeps the scale of its start)
  const char* names[3] = {"plane", "plane trimmed", "plane one-to-one"};
  for (int v = 0; v < 3; ++v) {
    pcl::IterativeClosestPointWithNormals<pcl::PointXYZ, pcl::PointNormal> icp;
    icp.setInputSource(B);
    icp.setInputTarget(An);
    icp.setMaxCorrespondenceDistance(1.0);
    icp.setMaximumIterations(50);
    icp.setTransformationEpsilon(1e-6);
    if (v == 1) icp.setTrimFraction(0.8);
    if (v == 2) icp.setOneToOne(true);
    pcl::PointCloud<pcl::PointXYZ> aligned;
    icp.align(aligned, guess);
    const sfmhip_icp_result& r = icp.icpResult();
    std::printf("%s: iterations %d pairs %d converged %d flags %d rmse %.3g plane rmse %.3g tau %.3g\n", names[v], r.iterations, r.pairs, r.converged,
                r.flags, std::sqrt(r.mse), std::sqrt(r.plane_mse), r.trim_d2);
    if (!icp.hasConverged()) return 3;
  }
  StructFromMotion sfm;
  sfmhip_icp_opts o;
  sfmhip_icp_default_opts(&o);
  o.metric = 1, o.with_scale = 1, o.min_pairs = 7, o.eps = 1e-6, o.max_dist = 1.0, o.normal_stride = 3;
  sfmhip_icp_result res;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud = B;
  const double metres = sfm.registerCloud(cloud, *A, o, normals.data(), nullptr, &res);
  std::printf("registerCloud: %.12f metres per unit, iterations %d converged %d flags %d\n", metres, res.iterations, res.converged, res.flags);
  if (!(metres > 0)) return 3;
  const double own = sfm.registerCloud(cloud, *A, o, nullptr, nullptr, &res);  // the reference's own k-NN normals
  std::printf("registerCloud own normals: %.12f metres per unit, iterations %d converged %d flags %d\n", own, res.iterations, res.converged,
              res.flags);
  return own > 0 ? 0 : 3;
}

int main(int argc, char** argv) {
  const bool icp_mode = argc > 1 && std::string(argv[1]) == "--icp";
  const double PI = 3.14159265358979323846, scale = argc > 1 && !icp_mode ? std::atof(argv[1]) : 1.04;
  std::vector<float> normals;  // A's planted normals (read by --icp only)
  pcl::PointCloud<pcl::PointXYZ>::Ptr A(new pcl::PointCloud<pcl::PointXYZ>), B(new pcl::PointCloud<pcl::PointXYZ>);
  for (int i = 0; i < 40000; ++i) {  // ground disc, noise 0.01
    const double a = 2 * PI * rnd(), r = 9.0 * std::sqrt(rnd());
    A->push_back(pcl::PointXYZ((float)(r * std::cos(a)), (float)(r * std::sin(a)), (float)(0.01 * gauss())));
    normals.insert(normals.end(), {0.0f, 0.0f, 1.0f});
  }
  const double centres[3][2] = {{-4, -2}, {3, -3}, {1, 4.5}};
  for (const double* c : {centres[0], centres[1], centres[2]}) {
    for (int i = 0; i < 6000; ++i) {  // trunk
      const double a = 2 * PI * rnd();
      A->push_back(pcl::PointXYZ((float)(c[0] + 0.15 * std::cos(a)), (float)(c[1] + 0.15 * std::sin(a)), (float)(4.0 * rnd())));
      normals.insert(normals.end(), {(float)std::cos(a), (float)std::sin(a), 0.0f});
    }
    for (int i = 0; i < 8000; ++i) {  // crown shell
      const double a = 2 * PI * rnd(), u = 2 * rnd() - 1, s = std::sqrt(1 - u * u);
      A->push_back(pcl::PointXYZ((float)(c[0] + 2.0 * s * std::cos(a)), (float)(c[1] + 1.5 * s * std::sin(a)), (float)(6.5 + 2.5 * u)));
      normals.insert(normals.end(), {(float)(s * std::cos(a) / 2.0), (float)(s * std::sin(a) / 1.5), (float)(u / 2.5)});  // (the ellipsoid's gradient: used as given)
    }
  }
  // B = R^T (A - t) / scale over every second point: the motion (scale, R, t) brings it back
  const double ang = 4.0 * PI / 180.0, t[3] = {0.3, -0.21, 0.15};
  double ax[3] = {0.3, -0.2, 0.93};
  const double l = std::sqrt(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
  for (double& v : ax) v /= l;
  const double c = std::cos(ang), s = std::sin(ang), C = 1 - c;
  const double R[9] = {c + ax[0] * ax[0] * C,         ax[0] * ax[1] * C - ax[2] * s, ax[0] * ax[2] * C + ax[1] * s,
                       ax[1] * ax[0] * C + ax[2] * s, c + ax[1] * ax[1] * C,         ax[1] * ax[2] * C - ax[0] * s,
                       ax[2] * ax[0] * C - ax[1] * s, ax[2] * ax[1] * C + ax[0] * s, c + ax[2] * ax[2] * C};
  for (size_t i = 0; i < A->size(); i += 2) {
    const pcl::PointXYZ& p = A->points[i];
    const double y[3] = {(p.x - t[0]) / scale, (p.y - t[1]) / scale, (p.z - t[2]) / scale};
    B->push_back(pcl::PointXYZ((float)(R[0] * y[0] + R[3] * y[1] + R[6] * y[2]), (float)(R[1] * y[0] + R[4] * y[1] + R[7] * y[2]),
                               (float)(R[2] * y[0] + R[5] * y[1] + R[8] * y[2])));
  }
  std::printf("plots: A %d B %d\n", (int)A->size(), (int)B->size());
  if (icp_mode) return run_icp(A, B, normals, scale);

  pcl::IterativeClosestPointWithScale<pcl::PointXYZ, pcl::PointXYZ> icp;
  icp.setInputSource(B);
  icp.setInputTarget(A);
  icp.setMaxCorrespondenceDistance(1.0);
  icp.setMaximumIterations(50);
  pcl::PointCloud<pcl::PointXYZ> aligned;
  icp.align(aligned);
  const sfmhip_register_result& r = icp.result();
  std::printf("register: iterations %d pairs %d converged %d flags %d rmse %.3g fitness %.3g\n", r.iterations, r.pairs, r.converged, r.flags,
              std::sqrt(r.mse), icp.getFitnessScore());
  if (!icp.hasConverged()) return 3;

  StructFromMotion sfm;
  double metres = 0;
  sfm.registerCloud(B, *A, &metres, 1.0);
  std::printf("scale: %.12f metres per unit\n", metres);
  if (!(metres > 0)) return 3;

  pcl::PointCloud<pcl::PointXYZ> moved;
  pcl::transformPointCloud(*B, moved, icp.getFinalTransformation());
  double dev = 0;
  for (size_t i = 0; i < moved.size(); ++i) {
    const pcl::PointXYZ &a = A->points[2 * i], &m = moved.points[i];
    dev = std::fmax(dev, std::fmax(std::fabs(a.x - m.x), std::fmax(std::fabs(a.y - m.y), std::fabs(a.z - m.z))));
  }
  std::printf("transform: %d points, farthest from its own point in A %.3g\n", (int)moved.size(), dev);

  // the rest without the host in between: handles, the f64 transform, concat, voxel grid
  sfmhip_cloud *ha = nullptr, *hb = nullptr, *hm = nullptr, *hc = nullptr;
  if (sfmhip_cloud_create(sfm_hip_context(), (int)A->size(), &A->points[0].x, &ha) != SFMHIP_OK) return 4;
  if (sfmhip_cloud_create(sfm_hip_context(), (int)B->size(), &B->points[0].x, &hb) != SFMHIP_OK) return 4;
  if (sfmhip_cloud_transform(hb, &r.T, &hm) != SFMHIP_OK || sfmhip_cloud_concat(ha, hm, &hc) != SFMHIP_OK) return 4;
  int32_t n_all = 0, n_vox = 0;
  sfmhip_cloud_size(hc, &n_all, nullptr);
  std::printf("concat: %d points\n", n_all);
  const float leaf[3] = {0.05f, 0.05f, 0.05f};
  std::vector<float> vox(3 * (size_t)n_all + 3);
  if (sfmhip_cloud_voxel_grid(hc, leaf, 0, nullptr, nullptr, vox.data(), nullptr, nullptr, nullptr, &n_vox, nullptr) != SFMHIP_OK) return 4;
  std::printf("voxel grid: %d voxels of 0.05\n", n_vox);
  for (sfmhip_cloud* h : {ha, hb, hm, hc}) sfmhip_cloud_destroy(h);

  pcl::PointCloud<pcl::PointXYZRGB>::Ptr plot(new pcl::PointCloud<pcl::PointXYZRGB>);
  for (int i = 0; i < n_vox; ++i) plot->push_back(pcl::PointXYZRGB(vox[3 * i], vox[3 * i + 1], vox[3 * i + 2], 0x00808080u));
  Dendrometry den;
  sfmhip_ground_opts gopts;
  sfmhip_ground_default_opts(&gopts);
  gopts.inlier_tol = 0.04;
  const int rc = den.estimatePlot(plot, gopts, nullptr, 0);
  std::printf("estimatePlot: status %d trees %d\n", rc, rc == SFMHIP_OK ? den.trees().n_trees : 0);
  return rc == SFMHIP_OK ? 0 : 4;
}
