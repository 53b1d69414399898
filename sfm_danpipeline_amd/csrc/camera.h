// camera.h -- the pinhole + distortion model of OpenCV 3.4.1 as __host__ __device__ code: cv::undistortPoints and
// cv::projectPoints for one point, f64, operation for operation the restated library sequence.  The triangulation kernel
// (triangulate.hip), the PnP kernels (pnp.hip) and the CPU stub of the latter share these bodies.  Compile with
// -ffp-contract=off.
#pragma once
#include <cmath>

#ifdef __HIPCC__
#define SFM_CAM_INLINE __host__ __device__ __forceinline__
#else
#define SFM_CAM_INLINE inline __attribute__((always_inline))
#endif

namespace sfmcam {

// cv::undistortPoints for one pixel (imgproc/undistort.cpp, 3.4.1: five fixed-point iterations, no R, no P)
SFM_CAM_INLINE void undistort_point(const double* K, const double* dist, double u, double v, double& xo, double& yo) {
  const double ifx = 1. / K[0], ify = 1. / K[4];
  double x = (u - K[2]) * ifx, y = (v - K[5]) * ify;
  const double x0 = x, y0 = y;
  const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
#pragma unroll 1
  for (int j = 0; j < 5; ++j) {
    const double r2 = x * x + y * y;
    const double icdist = 1. / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
    const double deltaX = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
    const double deltaY = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  xo = x;
  yo = y;
}

// cv::projectPoints for one point under P = [R|t] (calib3d/calibration.cpp cvProjectPoints2, k1 k2 p1 p2 k3)
SFM_CAM_INLINE void project_point(const double* P, const double* K, const double* dist, const double X[3], double& u, double& v) {
  double x = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  double y = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  z = z ? 1. / z : 1;
  x *= z;
  y *= z;
  const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
  const double r2 = x * x + y * y, r4 = r2 * r2, r6 = r4 * r2;
  const double a1 = 2 * x * y, a2 = r2 + 2 * x * x, a3 = r2 + 2 * y * y;
  const double cdist = 1 + k1 * r2 + k2 * r4 + k3 * r6;
  const double xd = x * cdist + p1 * a1 + p2 * a2;
  const double yd = y * cdist + p1 * a3 + p2 * a1;
  u = xd * K[0] + K[2];
  v = yd * K[4] + K[5];
}

}  // namespace sfmcam
