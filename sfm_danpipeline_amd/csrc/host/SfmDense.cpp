// SfmDense.cpp -- map3D's step 7 in the host mirror.  The reference shells out to pmvs2 (src/Sfm.cpp:62-67); here the dense
// cloud comes from sfmhip_mvs_run (plane-sweep depth maps and cross-view fusion; pmvs2 parity UNPINNED) and
// is written where step 8 (convertPLYtoPCD) reads it.  Kept out of Sfm.cpp so that the drivers without step 7 link as before.
#include <algorithm>
#include <cstdio>
#include "Sfm.h"
#include "hip_backend.h"

size_t StructFromMotion::densify(const std::string& plyPath) {
  std::vector<const uint8_t*> gray, bgr;
  std::vector<double> poses, dmin, dmax;
  int rows = 0, cols = 0;
  bool colour = true;
  for (int v : nGoodViews) {  // the registered views, ascending
    if (v < 0 || (size_t)v >= nCameraPoses.size() || (size_t)v >= mGrayImages.size() || mGrayImages[v].empty()) continue;
    const cv::Matx34d& P = nCameraPoses[v];
    double lo = 0.0, hi = 0.0;
    int seen = 0;
    for (const Point3D& p : nReconstructionCloud) {
      if (!p.idxImage.count(v)) continue;
      const double z = (P(2, 0) * p.pt.x + P(2, 1) * p.pt.y) + (P(2, 2) * p.pt.z + P(2, 3));
      if (!(z > 0.0)) continue;
      lo = seen ? std::min(lo, z) : z;
      hi = seen ? std::max(hi, z) : z;
      ++seen;
    }
    if (seen < 8) continue;  // too few sparse points to bound the sweep
    const cv::Mat& g = mGrayImages[v];
    if (gray.empty()) rows = g.rows, cols = g.cols;
    if (g.rows != rows || g.cols != cols || g.channels() != 1) {
      std::fprintf(stderr, "densify: view %d is not a %d x %d gray image; skipped\n", v, cols, rows);
      continue;
    }
    const bool has_bgr = (size_t)v < mColorImages.size() && mColorImages[v].rows == rows && mColorImages[v].cols == cols &&
                         mColorImages[v].channels() == 3;
    colour = colour && has_bgr;
    gray.push_back(g.ptr());
    bgr.push_back(has_bgr ? mColorImages[v].ptr() : nullptr);
    poses.insert(poses.end(), P.val, P.val + 12);
    dmin.push_back(lo / 1.25);  // the sparse depths, widened by 25 %
    dmax.push_back(hi * 1.25);
  }
  if (gray.size() < 2 || cameraMatrix.K.rows != 3 || cameraMatrix.K.cols != 3) {
    std::fprintf(stderr, "densify: %zu usable views\n", gray.size());
    return 0;
  }
  sfmhip_mvs_opts o;
  sfmhip_mvs_default_opts(&o);
  o.min_views = 5;  // options.txt: minImageNum 5
  sfmhip_mvs* m = nullptr;
  int32_t n = 0;
  // the calibration file's distortion coefficients (k1 k2 p1 p2 k3): with any of them set the views are undistorted on the
  // device first; all zero is the pinhole call, bit for bit what it always was
  double dist[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 5 && i < (int)cameraMatrix.distCoef.data.size(); ++i) dist[i] = cameraMatrix.distCoef.data[i];
  const bool distorted = std::any_of(dist, dist + 5, [](double d) { return d != 0.0; });
  const int level = 1;  // options.txt: level 1
  int rc = distorted ? sfmhip_mvs_create_distorted(sfm_hip_context(), (int)gray.size(), rows, cols, gray.data(), colour ? bgr.data() : nullptr,
                                                   cameraMatrix.K.data.data(), dist, poses.data(), level, &m)
                     : sfmhip_mvs_create(sfm_hip_context(), (int)gray.size(), rows, cols, gray.data(), colour ? bgr.data() : nullptr,
                                         cameraMatrix.K.data.data(), poses.data(), level, &m);
  if (rc == SFMHIP_OK) rc = sfmhip_mvs_run(m, dmin.data(), dmax.data(), &o, &n);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "densify: %s\n", sfmhip_error_string(rc));
    sfmhip_mvs_destroy(m);
    return 0;
  }
  std::vector<float> xyz(3 * (size_t)n + 3), nrm(3 * (size_t)n + 3);
  std::vector<uint32_t> rgb((size_t)n + 1);
  sfmhip_mvs_download(m, xyz.data(), nrm.data(), rgb.data());
  sfmhip_mvs_destroy(m);
  FILE* f = std::fopen(plyPath.c_str(), "wb");
  if (!f) {
    std::fprintf(stderr, "densify: cannot write %s\n", plyPath.c_str());
    return 0;
  }
  std::fprintf(f, "ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\n"
                  "property uchar blue\nend_header\n", (int)n);
  for (int i = 0; i < n; ++i) {
    const unsigned char c[3] = {(unsigned char)(rgb[i] >> 16), (unsigned char)(rgb[i] >> 8), (unsigned char)rgb[i]};
    std::fwrite(&xyz[3 * (size_t)i], 4, 3, f);
    std::fwrite(&nrm[3 * (size_t)i], 4, 3, f);
    std::fwrite(c, 1, 3, f);
  }
  std::fclose(f);
  std::printf("densify: %zu views%s, %d points -> %s\n", gray.size(), distorted ? " (undistorted)" : "", (int)n, plyPath.c_str());
  return (size_t)n;
}
