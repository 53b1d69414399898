// align_selftest.cpp -- two reconstructions of one plot in unrelated gauges brought together without a starting guess
// (DESIGN.md f-18), written against the host mirror's alignPlots and registerCloud; needs the GPU, takes no input:
//   align_selftest [scale]
// A planted plot in metres (a ground disc with three trees of different heights: plot A) and a second sampling of it in
// another gauge (plot B: every second point, moved by the inverse of a motion of 115 degrees about a tilted axis and (11, -7,
// 3) m, and divided by `scale`, 2.3 without the argument).  Each plot is levelled by its own ground plane, alignPlots votes
// for scale, yaw and shift and runs ICP from every candidate on the points above the ground, and registerCloud refines the
// winner on the whole clouds.  One line per step ("<step>: ...").  Exit 3: no winner; 4: the registration from it has a flag
// set or has not reached its fixed point; 5: the scale is off by more than 0.1 %.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include "Sfm.h"
#include "hip_backend.h"

static uint32_t rng_state = 2025u;
static double rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) / 16777216.0;
}
static double gauss() {
  double s = 0;
  for (int i = 0; i < 12; ++i) s += rnd();
  return s - 6.0;
}

int main(int argc, char** argv) {
  const double PI = 3.14159265358979323846, scale = argc > 1 ? std::atof(argv[1]) : 2.3;
  pcl::PointCloud<pcl::PointXYZ>::Ptr A(new pcl::PointCloud<pcl::PointXYZ>), B(new pcl::PointCloud<pcl::PointXYZ>);
  for (int i = 0; i < 20000; ++i) {  // ground disc, noise 0.01
    const double a = 2 * PI * rnd(), r = 9.0 * std::sqrt(rnd());
    A->push_back(pcl::PointXYZ((float)(r * std::cos(a)), (float)(r * std::sin(a)), (float)(0.01 * gauss())));
  }
  const double trees[3][3] = {{-4, -2, 6.5}, {3, -3, 8.0}, {1, 4.5, 5.0}};  // (x, y, crown centre height)
  for (const double* c : {trees[0], trees[1], trees[2]}) {
    for (int i = 0; i < 3000; ++i) {  // trunk
      const double a = 2 * PI * rnd();
      A->push_back(pcl::PointXYZ((float)(c[0] + 0.15 * std::cos(a)), (float)(c[1] + 0.15 * std::sin(a)), (float)((c[2] - 2.0) * rnd())));
    }
    for (int i = 0; i < 4000; ++i) {  // crown shell
      const double a = 2 * PI * rnd(), u = 2 * rnd() - 1, s = std::sqrt(1 - u * u);
      A->push_back(pcl::PointXYZ((float)(c[0] + 2.0 * s * std::cos(a)), (float)(c[1] + 1.5 * s * std::sin(a)), (float)(c[2] + 2.5 * u)));
    }
  }
  // B = R^T (A - t) / scale over every second point: the motion (scale, R, t) brings it back
  const double ang = 115.0 * PI / 180.0, t[3] = {11.0, -7.0, 3.0};
  double ax[3] = {0.5, -0.4, 0.77};
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

  // the two ground planes, for the record (alignPlots fits them again)
  sfmhip_ground_opts go;
  sfmhip_ground_default_opts(&go);
  const char* names[2] = {"A", "B"};
  pcl::PointCloud<pcl::PointXYZ>::Ptr clouds[2] = {A, B};
  for (int k = 0; k < 2; ++k) {
    sfmhip_cloud* h = nullptr;
    sfmhip_ground_result g;
    if (sfmhip_cloud_create(sfm_hip_context(), (int)clouds[k]->size(), &clouds[k]->points[0].x, &h) != SFMHIP_OK) return 2;
    const int rc = sfmhip_cloud_ground_plane(h, nullptr, 0, &go, nullptr, 0, &g);
    sfmhip_cloud_destroy(h);
    if (rc != SFMHIP_OK || g.flags != 0) return 2;
    std::printf("ground %s: up %.4f %.4f %.4f offset %.4f inliers %d\n", names[k], g.up[0], g.up[1], g.up[2], g.offset, g.inliers);
  }

  StructFromMotion sfm;
  sfmhip_align_opts o;
  sfmhip_align_default_opts(&o);
  o.scale_lo = 0.65 * scale, o.scale_hi = 1.52 * scale, o.h_tol = 0.3;
  o.src_samples = 800, o.tgt_samples = 600;
  sfmhip_align_result ar;
  const int flags = sfm.alignPlots(B, *A, o, &ar);
  if (flags < 0) return 2;
  std::printf("align: flags %d candidates %d winner %d (same %d) votes %d pairs %d of %d scale %.5f\n", flags, ar.n_cand, ar.cand_index, ar.n_same,
              ar.cand.votes, ar.reg.pairs, ar.stats.n_src, ar.reg.T.scale);
  if (flags != 0) return 3;

  double metres = 0;
  sfmhip_register_result r;
  sfm.registerCloud(B, *A, &metres, 0.6, &ar.reg.T, &r);
  std::printf("register: iterations %d pairs %d converged %d flags %d rmse %.3g\n", r.iterations, r.pairs, r.converged, r.flags, std::sqrt(r.mse));
  std::printf("scale: %.9f metres per unit\n", metres);
  if (r.flags != 0 || r.converged != 1) return 4;
  return std::fabs(metres / scale - 1) <= 1e-3 ? 0 : 5;
}
