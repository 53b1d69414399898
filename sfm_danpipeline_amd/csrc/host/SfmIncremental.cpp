// SfmIncremental.cpp -- the incremental loop of StructFromMotion: addMoreViews and findCameraPosePNP (reference
// src/Sfm.cpp:893-1006, 1137-1210) over sfmhip_pnp_ransac.  The wrapper's cv::projectPoints and cv::Rodrigues use the
// arithmetic the kernels use (../camera.h, ../pnp.h).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>
#include "../pnp.h"
#include "Sfm.h"
#include "hip_backend.h"

bool StructFromMotion::findCameraPosePNP(const Intrinsics& intrinsics, const std::vector<cv::Point3d>& pts3D,
                                         const std::vector<cv::Point2d>& pts2D, cv::Matx34d& P) {
  pnpInliers.clear();
  if (pts3D.size() <= 7 || pts2D.size() <= 7 || pts3D.size() != pts2D.size()) {
    // something went wrong aligning 3D to 2D points..
    std::cerr << "couldn't find [enough] corresponding cloud points... (only " << pts3D.size() << ")" << std::endl;
    return false;
  }
  if (intrinsics.K.data.size() < 9) {
    std::cerr << "Intrinsics matrix (K) must be initialized." << std::endl;
    return false;
  }
  // cv::minMaxIdx(pts2D): the largest of all x and y (the array is taken as single-channel)
  double maxVal = -1.7976931348623157e308;
  for (const cv::Point2d& p : pts2D) maxVal = std::max(maxVal, std::max(p.x, p.y));
  double dist[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 5 && i < (int)intrinsics.distCoef.data.size(); ++i) dist[i] = intrinsics.distCoef.data[i];
  const double* K = intrinsics.K.data.data();
  static_assert(sizeof(cv::Point3d) == 3 * sizeof(double) && sizeof(cv::Point2d) == 2 * sizeof(double), "packed points");
  // solvePnPRansac(pts3D, pts2D, K, distCoef, rvec, T, true, 1000, 0.006 * maxVal, 0.99, inliers, CV_EPNP); rvec and T stay
  // zero when it returns false
  const int32_t offsets[2] = {0, (int32_t)pts3D.size()};
  const double thr = 0.006 * maxVal;
  int32_t status = 0, n_in = 0;
  double rvec[3] = {0, 0, 0}, T[3] = {0, 0, 0};
  std::vector<uint8_t> mask(pts3D.size());
  const int rc = sfmhip_pnp_ransac(sfm_hip_context(), 1, offsets, &pts3D[0].x, &pts2D[0].x, K, dist, &thr, 0.99, 1000, &status, rvec, T,
                                   nullptr, nullptr, nullptr, nullptr, &n_in, mask.data(), nullptr);
  if (rc != SFMHIP_OK) {
    std::cerr << "findCameraPosePNP: " << sfmhip_error_string(rc) << std::endl;
    return false;
  }
  if (status == 1)
    for (size_t i = 0; i < mask.size(); ++i)
      if (mask[i]) pnpInliers.push_back((int)i);
  // cv::projectPoints(pts3D, rvec, T, K, distCoef, projected3D)
  double Pm[12];
  sfmpnp::pose_matrix(rvec, T, Pm);
  if (pnpInliers.size() == 0) {  // get inliers
    for (size_t i = 0; i < pts3D.size(); i++) {
      const double X[3] = {pts3D[i].x, pts3D[i].y, pts3D[i].z};
      double u, v;
      sfmcam::project_point(Pm, K, dist, X, u, v);
      const double dx = u - pts2D[i].x, dy = v - pts2D[i].y;
      if (std::sqrt(dx * dx + dy * dy) < 8.0) pnpInliers.push_back((int)i);
    }
  }
  if (std::sqrt(T[0] * T[0] + T[1] * T[1] + T[2] * T[2]) > 200.0) {
    // this is bad...
    std::cerr << "estimated camera movement is too big, skip this camera\r\n";
    return false;
  }
  cv::Mat R(3, 3, CV_64F);
  sfmpnp::rodrigues_to_matrix(rvec, &R.at<double>(0, 0));  // cv::Rodrigues(rvec, R)
  if (!CheckCoherentRotation(R)) {
    std::cerr << "rotation is incoherent. we should try a different base view..." << std::endl;
    return false;
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P(r, c) = R.at<double>(r, c);
    P(r, 3) = T[r];
  }
  std::cout << "found t = [" << T[0] << ", " << T[1] << ", " << T[2] << "] with " << pnpInliers.size() << " inliers" << std::endl;
  return true;
}

bool StructFromMotion::addMoreViews() {
  std::vector<cv::Point3d> points3D;
  std::vector<cv::Point2d> points2D;
  const int nImg = (int)nImages.size();

  while (nDoneViews.size() != mGrayImages.size()) {
    std::set<int> newFrames;
    for (int newViewstoAdd : nDoneViews) {
      int i;
      int j;
      if (newViewstoAdd == 0) {
        i = newViewstoAdd;
        j = std::abs(newViewstoAdd + 1);
      } else if (newViewstoAdd == nImg) {
        i = std::abs(newViewstoAdd - 1);
        j = newViewstoAdd;
      } else {
        i = std::abs(newViewstoAdd - 1);
        j = std::abs(newViewstoAdd + 1);
      }
      if (nDoneViews.count(i) == 1) {
        if (nDoneViews.count(j) == 1) {
          continue;
        } else {
          newFrames.insert(j);
        }
      } else {
        newFrames.insert(i);
        if (nDoneViews.count(j) == 1) {
          continue;
        } else {
          newFrames.insert(j);
        }
      }
    }
    // DEVIATION: a view that does not exist is dropped (the reference would throw in .at()), and a round that has no new
    // view to try ends the loop (the reference would go round for ever)
    bool any = false;
    for (auto it = newFrames.begin(); it != newFrames.end();) {
      if (*it < 0 || *it >= nImg) {
        it = newFrames.erase(it);
        continue;
      }
      any = any || nDoneViews.find(*it) == nDoneViews.end();
      ++it;
    }
    if (!any) break;

    for (int NEW_VIEW : newFrames) {
      if (nDoneViews.find(NEW_VIEW) != nDoneViews.end()) continue;  // Skip done views

      std::cout << "\n" << "====================================" << std::endl;
      std::cout << "ESTIMATING MORE CAMERAS PROJECTION..." << std::endl;
      std::cout << "Extracting 2d3d correspondences..." << std::endl;
      std::cout << "Possible view:" << " image --> " << NEW_VIEW << std::endl;

      Matching bestMatches;
      int DONE_VIEW;
      find2D3DMatches(NEW_VIEW, points3D, points2D, bestMatches, DONE_VIEW);
      std::cout << "Adding " << NEW_VIEW << " to existing [";
      for (auto it = nDoneViews.begin(); it != nDoneViews.end(); ++it) std::cout << (it == nDoneViews.begin() ? "" : ", ") << *it;
      std::cout << "]" << std::endl;
      nDoneViews.insert(NEW_VIEW);

      std::cout << "Estimating camera pose..." << std::endl;
      cv::Matx34d newCameraPose;
      newCameraPose(0, 0) = newCameraPose(1, 1) = newCameraPose(2, 2) = 1.0;
      bool success = findCameraPosePNP(cameraMatrix, points3D, points2D, newCameraPose);

      if (not success) {
        std::cout << "Failed. Could not get a good pose estimation. skip view" << std::endl;
        continue;
      }

      if (nCameraPoses.size() < (size_t)nImg) nCameraPoses.resize((size_t)nImg);
      nCameraPoses[NEW_VIEW] = newCameraPose;

      std::vector<Point3D> new_triangulated;

      for (int good_view : nGoodViews) {
        int queryImage, trainImage;
        if (NEW_VIEW < good_view) {
          queryImage = NEW_VIEW;
          trainImage = good_view;
        } else {
          queryImage = good_view;
          trainImage = NEW_VIEW;
        }

        Matching matches;
        getMatching(queryImage, trainImage, &matches);

        bool good_triangulation = triangulateViews(imagesPts2D.at(queryImage), imagesPts2D.at(trainImage), nCameraPoses[queryImage],
                                                   nCameraPoses[trainImage], matches, cameraMatrix,
                                                   std::make_pair(queryImage, trainImage), new_triangulated);
        if (not good_triangulation) {
          continue;
        }

        std::cout << "Before triangulation: " << nReconstructionCloud.size() << std::endl;
        mergeNewPoints(new_triangulated);
        std::cout << "After triangulation: " << nReconstructionCloud.size() << std::endl;
      }

      nGoodViews.insert(NEW_VIEW);
      adjustCurrentBundle();
    }
    continue;
  }
  std::cout << "\n" << "=============================== " << std::endl;
  std::cout << "Images processed = " << nDoneViews.size() << " of " << nImages.size() << std::endl;
  std::cout << "PointCloud size = " << nReconstructionCloud.size() << " pts3D" << std::endl;
  return true;
}
