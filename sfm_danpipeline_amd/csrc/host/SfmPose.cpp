// SfmPose.cpp -- the pose step of StructFromMotion: baseReconstruction, getCameraPose and the helpers it calls (reference
// src/Sfm.cpp:408-492, 610-662, 713-799, 1119-1131) over sfmhip_essential_pose / sfmhip_score_homography.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include "../pose.h"
#include "Sfm.h"
#include "hip_backend.h"

namespace {

// operator<< of a cv::Mat / cv::Matx of doubles, OpenCV's default formatter: "[a, b, c;\n d, e, f]", %.16g
void printMat(std::ostream& os, const double* v, int rows, int cols) {
  char buf[64];
  os << "[";
  for (int r = 0; r < rows; ++r) {
    for (int c = 0; c < cols; ++c) {
      std::snprintf(buf, sizeof buf, "%.16g", v[r * cols + c]);
      os << buf << (c + 1 < cols ? ", " : "");
    }
    os << (r + 1 < rows ? ";\n " : "]");
  }
}

}  // namespace

double StructFromMotion::determinante(cv::Mat& relativeRotationCam) {
  return sfmpose::fullpivlu_det3(&relativeRotationCam.at<double>(0, 0));
}

bool StructFromMotion::CheckCoherentRotation(cv::Mat& R) {
  if (!sfmpose::coherent_det(determinante(R))) {  // fabsf(determinante(R)) - 1.0 > 1e-07
    std::cout << "det(R) != +-1.0, this is not a rotation matrix" << std::endl;
    return false;
  }
  return true;
}

void StructFromMotion::prunedMatchingWithHomography(const int& idx_query, const int& idx_train, const Matching& goodMatches,
                                                    Matching* prunedMatch) {
  // keypointstoPoints of the matched keypoints = the matched rows of imagesPts2D
  Points2d query_points, train_points;
  AlignedPointsFromMatch(imagesPts2D.at(idx_query), imagesPts2D.at(idx_train), goodMatches, query_points, train_points);
  const double ransac_thresh = 2.5;
  std::vector<uint8_t> mask;
  if (goodMatches.size() >= 4) {
    const int32_t offsets[2] = {0, (int32_t)query_points.size()};
    int32_t inl = 0;
    mask.resize(query_points.size());
    const int rc = sfmhip_score_homography(sfm_hip_context(), 1, offsets, &query_points[0].x, &train_points[0].x, &ransac_thresh,
                                           0.995, 2000, &inl, mask.data(), nullptr);
    if (rc != SFMHIP_OK) {
      std::cerr << "prunedMatchingWithHomography: " << sfmhip_error_string(rc) << std::endl;
      mask.clear();
    }
  }
  std::cout << "Homography inliers mask:" << mask.size() << " inliers" << std::endl;
  for (size_t i = 0; i < mask.size(); ++i)
    if (mask[i]) prunedMatch->push_back(goodMatches[i]);
}

// one sfmhip_essential_pose call over the pairs (K = cameraMatrix.K; findEssentialMat(0.999, 1.0), recoverPose with fx)
bool StructFromMotion::essentialPoses(const std::vector<Points2d>& left, const std::vector<Points2d>& right,
                                      std::vector<PoseOutcome>& out) {
  const int n = (int)left.size();
  out.assign(n, PoseOutcome());
  if (n == 0) return true;
  std::vector<int32_t> offsets(1, 0);
  std::vector<double> l, r;
  for (int p = 0; p < n; ++p) {
    for (size_t i = 0; i < left[p].size(); ++i) {
      l.push_back(left[p][i].x);
      l.push_back(left[p][i].y);
      r.push_back(right[p][i].x);
      r.push_back(right[p][i].y);
    }
    offsets.push_back((int32_t)(l.size() / 2));
  }
  if (l.empty()) {
    l.assign(2, 0.0);
    r.assign(2, 0.0);
  }
  std::vector<double> E(9 * (size_t)n), R(9 * (size_t)n), T(3 * (size_t)n);
  std::vector<int32_t> inl(n), ng(n);
  std::vector<uint8_t> mask((size_t)offsets[n] + 1);
  const cv::Mat_<double>& K = cameraMatrix.K;
  const int rc = sfmhip_essential_pose(sfm_hip_context(), n, offsets.data(), l.data(), r.data(), K(0, 0), K(1, 1), K(0, 2), K(1, 2),
                                       0.999, 1.0, E.data(), inl.data(), R.data(), T.data(), ng.data(), mask.data());
  if (rc != SFMHIP_OK) {
    std::cerr << "getCameraPose: " << sfmhip_error_string(rc) << std::endl;
    return false;
  }
  for (int p = 0; p < n; ++p) {
    PoseOutcome& o = out[p];
    for (int k = 0; k < 9; ++k) o.E[k] = E[9 * (size_t)p + k];
    for (int k = 0; k < 9; ++k) o.R[k] = R[9 * (size_t)p + k];
    for (int k = 0; k < 3; ++k) o.T[k] = T[3 * (size_t)p + k];
    o.inliers = inl[p];
    o.n_good = ng[p];
    o.mask.assign(mask.begin() + offsets[p], mask.begin() + offsets[p + 1]);
  }
  return true;
}

// src/Sfm.cpp:720-789 from the pruning on, with the pair's essential_pose outcome (nullptr: computed here from
// alignedLeft / alignedRight, the caller's points)
bool StructFromMotion::cameraPoseFrom(const int& idx_query, const int& idx_train, const Matching& matches,
                                      const Points2d& alignedLeft, const Points2d& alignedRight, const PoseOutcome* outcome,
                                      cv::Matx34d& Pleft, cv::Matx34d& Pright) {
  Matching prunedMatches;
  prunedMatchingWithHomography(idx_query, idx_train, matches, &prunedMatches);
  std::cout << "pruned matches:" << prunedMatches.size() << std::endl;
  std::cout << "aligned: " << alignedLeft.size() << " and " << alignedRight.size() << std::endl;
  if (alignedLeft.size() <= 7 || alignedRight.size() <= 7) {
    std::cout << "Sorry. not enough points for findEssentialMat function. matches size is " << prunedMatches.size() << std::endl;
    return false;
  }
  std::vector<PoseOutcome> mine;
  if (!outcome) {
    if (!essentialPoses(std::vector<Points2d>(1, alignedLeft), std::vector<Points2d>(1, alignedRight), mine)) return false;
    outcome = &mine[0];
  }
  if (outcome->n_good < 0) {  // (the reference throws in decomposeEssentialMat: see Sfm.h)
    std::cerr << "getCameraPose: findEssentialMat found no model for " << idx_query << "," << idx_train << std::endl;
    return false;
  }
  std::cout << "Essential matrix:\n";
  printMat(std::cout, outcome->E, 3, 3);
  std::cout << std::endl;
  cv::Mat R(3, 3, CV_64F, outcome->R);
  const bool success = CheckCoherentRotation(R);
  std::cout << "R:\n";
  printMat(std::cout, outcome->R, 3, 3);
  std::cout << std::endl << "T:\n";
  printMat(std::cout, outcome->T, 3, 1);
  std::cout << std::endl;
  if (!success) {
    std::cerr << "Bad rotation." << std::endl;
    return false;
  }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Pright(r, c) = outcome->R[3 * r + c];
    Pright(r, 3) = outcome->T[r];
  }
  Pleft = cv::Matx34d();
  Pleft(0, 0) = Pleft(1, 1) = Pleft(2, 2) = 1.0;
  std::cout << "Pright:\n";
  printMat(std::cout, Pright.val, 3, 4);
  std::cout << std::endl;
  return true;
}

bool StructFromMotion::getCameraPose(const Intrinsics& intrinsics, const int& idx_query, const int& idx_train,
                                     const Matching& matches, const Points2d& left, const Points2d& right, cv::Matx34d& Pleft,
                                     cv::Matx34d& Pright) {
  if (intrinsics.K.data.empty()) {
    std::cerr << "Intrinsics matrix (K) must be initialized." << std::endl;
    return false;
  }
  Points2d alignedLeft, alignedRight;
  AlignedPointsFromMatch(left, right, matches, alignedLeft, alignedRight);
  const Intrinsics keep = cameraMatrix;  // (essentialPoses reads cameraMatrix)
  cameraMatrix = intrinsics;
  const bool ok = cameraPoseFrom(idx_query, idx_train, matches, alignedLeft, alignedRight, nullptr, Pleft, Pright);
  cameraMatrix = keep;
  return ok;
}

bool StructFromMotion::baseReconstruction() {
  const std::map<float, std::pair<int, int>> bestViews = findBestPair();
  lastBasePose = BasePose();
  if (bestViews.empty()) {
    std::cout << "Could not obtain a good pair for baseline reconstruction." << std::endl;
    return false;
  }
  // every entry's getCameraPose numerics in one call: each pair's outcome is independent of the others
  std::vector<Matching> matches;
  std::vector<Points2d> left, right;
  for (const auto& bp : bestViews) {
    Matching m;
    getMatching(bp.second.first, bp.second.second, &m);
    Points2d l, r;
    AlignedPointsFromMatch(imagesPts2D.at(bp.second.first), imagesPts2D.at(bp.second.second), m, l, r);
    matches.push_back(m);
    left.push_back(l);
    right.push_back(r);
  }
  std::vector<PoseOutcome> outcomes;
  const bool haveK = !cameraMatrix.K.data.empty();
  if (haveK && !essentialPoses(left, right, outcomes)) return false;  // (a device error: not the same as "no pair passed")
  size_t e = 0;
  for (auto it = bestViews.begin(); it != bestViews.end(); ++it, ++e) {
    const int queryImage = it->second.first, trainImage = it->second.second;
    std::cout << "Best pair:" << "[" << queryImage << "," << trainImage << "]" << " has:" << matches[e].size() << " matches"
              << " and " << it->first << " inliers." << std::endl;
    cv::Matx34d Pleft, Pright;
    Pleft(0, 0) = Pleft(1, 1) = Pleft(2, 2) = 1.0;
    Pright = Pleft;
    std::cout << "Estimating camera pose with Essential Matrix..." << std::endl;
    bool success = false;
    if (!haveK)
      std::cerr << "Intrinsics matrix (K) must be initialized." << std::endl;
    else
      success = cameraPoseFrom(queryImage, trainImage, matches[e], left[e], right[e], &outcomes[e], Pleft, Pright);
    if (!success) {
      std::cerr << "Failed. stereo view could not be obtained " << queryImage << "," << trainImage << ", something wrong."
                << std::endl;
      continue;
    }
    std::cout << "Camera:" << queryImage << "\n";
    printMat(std::cout, Pleft.val, 3, 4);
    std::cout << std::endl << "Camera:" << trainImage << "\n";
    printMat(std::cout, Pright.val, 3, 4);
    std::cout << std::endl;
    std::cout << "Showing matches between " << "image:" << queryImage << " and image:" << trainImage << std::endl;
    std::vector<Point3D> pointcloud;
    success = triangulateViews(imagesPts2D.at(queryImage), imagesPts2D.at(trainImage), Pleft, Pright, matches[e], cameraMatrix,
                               std::make_pair(queryImage, trainImage), pointcloud);
    if (!success) {
      std::cerr << "Could not triangulate image:" << queryImage << " and image:" << trainImage << std::endl;
      continue;
    }
    nReconstructionCloud = pointcloud;
    const size_t need = (size_t)std::max(queryImage, trainImage) + 1;
    if (nCameraPoses.size() < std::max(need, nImages.size())) nCameraPoses.resize(std::max(need, nImages.size()));
    nCameraPoses[queryImage] = Pleft;
    nCameraPoses[trainImage] = Pright;
    nDoneViews.insert(queryImage);
    nDoneViews.insert(trainImage);
    nGoodViews.insert(queryImage);
    nGoodViews.insert(trainImage);
    BasePose& b = lastBasePose;
    b.query = queryImage;
    b.train = trainImage;
    b.n_good = outcomes[e].n_good;
    for (int k = 0; k < 9; ++k) b.E[k] = outcomes[e].E[k];
    for (int k = 0; k < 9; ++k) b.R[k] = outcomes[e].R[k];
    for (int k = 0; k < 3; ++k) b.T[k] = outcomes[e].T[k];
    b.mask = outcomes[e].mask;
    break;
  }
  return true;
}
