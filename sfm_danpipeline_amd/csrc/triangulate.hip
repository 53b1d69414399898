// triangulate.hip -- two-view DLT triangulation + reprojection filter on gfx950.
//
// Replaces the numeric body of StructFromMotion::triangulateViews (reference
// src/Sfm.cpp:812-860): cv::undistortPoints -> cv::triangulatePoints (4x4 homogeneous DLT,
// smallest right singular vector by one-sided Jacobi) -> convertPointsFromHomogeneous ->
// cv::projectPoints in both views -> float 6 px test.  One lane per match, f64 throughout,
// contraction off so the arithmetic is operation-for-operation the restated OpenCV sequence.
// HBM-bound by construction (2 x 16 B in, 24 B + 1 B (+8 B) out per match); the track /
// visibility bookkeeping (Point3D::idxImage, src/Sfm.cpp:862-873) is the host mirror's job.
#include "common.h"
#include "camera.h"
#include "pose.h"
#include <float.h>

namespace {

using sfmpose::dlt_null_vector;  // (pose.h: shared with the pose kernels and the CPU test stub)
using sfmcam::project_point;     // (camera.h: shared with the PnP kernels and their CPU test stub)
using sfmcam::undistort_point;

struct TriParams {
  double P1[12], P2[12], K[9], dist[5];
  float max_err;
};

__global__ __launch_bounds__(256) void triangulate_kernel(TriParams p, const double2* __restrict__ xy1,
                                                          const double2* __restrict__ xy2, int m,
                                                          double* __restrict__ X, float* __restrict__ err,
                                                          unsigned char* __restrict__ keep) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < m;
  const double2 a = live ? xy1[i] : make_double2(0, 0);
  const double2 b = live ? xy2[i] : make_double2(0, 0);
  double x1, y1, x2, y2;
  undistort_point(p.K, p.dist, a.x, a.y, x1, y1);
  undistort_point(p.K, p.dist, b.x, b.y, x2, y2);
  double At[4][4];  // At[c][r] = A[r][c]
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    At[k][0] = x1 * p.P1[8 + k] - p.P1[0 + k];
    At[k][1] = y1 * p.P1[8 + k] - p.P1[4 + k];
    At[k][2] = x2 * p.P2[8 + k] - p.P2[0 + k];
    At[k][3] = y2 * p.P2[8 + k] - p.P2[4 + k];
  }
  double v[4];
  dlt_null_vector(At, v);
  const double scale = v[3] != 0 ? 1. / v[3] : 1.;
  const double Xi[3] = {v[0] * scale, v[1] * scale, v[2] * scale};
  double u1, v1, u2, v2;
  project_point(p.P1, p.K, p.dist, Xi, u1, v1);
  project_point(p.P2, p.K, p.dist, Xi, u2, v2);
  const double dx1 = u1 - a.x, dy1 = v1 - a.y, dx2 = u2 - b.x, dy2 = v2 - b.y;
  const float e1 = (float)sqrt(dx1 * dx1 + dy1 * dy1);
  const float e2 = (float)sqrt(dx2 * dx2 + dy2 * dy2);
  if (live) {
    X[3 * i] = Xi[0];
    X[3 * i + 1] = Xi[1];
    X[3 * i + 2] = Xi[2];
    if (err) {
      err[2 * i] = e1;
      err[2 * i + 1] = e2;
    }
    keep[i] = !(p.max_err < e1 || p.max_err < e2);
  }
}

}  // namespace

extern "C" int sfmhip_triangulate(sfmhip_ctx* ctx, const double P1[12], const double P2[12], const double K[9],
                                  const double dist[5], const double* xy1, const double* xy2, int m, float max_err,
                                  double* X, float* err, uint8_t* keep) {
  if (!ctx || !P1 || !P2 || !K || !dist || m < 0) return SFMHIP_ERR_ARG;
  if (m == 0) return SFMHIP_OK;
  if (!xy1 || !xy2 || !X || !keep) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  TriParams p;
  for (int i = 0; i < 12; ++i) {
    p.P1[i] = P1[i];
    p.P2[i] = P2[i];
  }
  for (int i = 0; i < 9; ++i) p.K[i] = K[i];
  for (int i = 0; i < 5; ++i) p.dist[i] = dist[i];
  p.max_err = max_err;
  const size_t n = (size_t)m;
  // one device slab: xy1 | xy2 | X | err | keep
  const size_t off_xy2 = n * 16, off_X = off_xy2 + n * 16, off_err = off_X + n * 24, off_keep = off_err + n * 8;
  const size_t bytes = off_keep + n;
  DevBufs bufs;
  unsigned char* d = nullptr;
  SFM_TRY(bufs.alloc(&d, bytes));
  hipStream_t st = ctx->stream;
  SFM_HIP_TRY(hipMemcpyAsync(d, xy1, n * 16, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d + off_xy2, xy2, n * 16, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(triangulate_kernel, dim3((m + 255) / 256), dim3(256), 0, st, p, (const double2*)d,
                     (const double2*)(d + off_xy2), m, (double*)(d + off_X), (float*)(d + off_err), d + off_keep);
  SFM_HIP_TRY(hipGetLastError());
  SFM_HIP_TRY(hipMemcpyAsync(X, d + off_X, n * 24, hipMemcpyDeviceToHost, st));
  if (err) SFM_HIP_TRY(hipMemcpyAsync(err, d + off_err, n * 8, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(keep, d + off_keep, n, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}
