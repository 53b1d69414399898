// SfmTracks.cpp -- StructFromMotion::consolidateTracks: the multi-view tracks of the registered views (sfmhip_tracks_*,
// DESIGN.md f-16) in place of the two-view points triangulateViews and mergeNewPoints leave.  The reference has no
// counterpart (parity UNPINNED); nothing calls this by default.  With `verify` the lists first pass the two-view verification
// (sfmhip_matchplan_verify / sfmhip_verify_lists) and the tracks are built from what it keeps.
#include <iostream>
#include "Sfm.h"
#include "hip_backend.h"

namespace {
// every image's pixels one after the other, as sfmhip_tracks_triangulate and the verification take them
void packPixels(const std::vector<Points2d>& pts, std::vector<int32_t>& xyPtr, std::vector<double>& xy) {
  xyPtr.assign(pts.size() + 1, 0);
  xy.clear();
  for (size_t i = 0; i < pts.size(); ++i) {
    xyPtr[i + 1] = xyPtr[i] + (int32_t)pts[i].size();
    for (const cv::Point2d& p : pts[i]) {
      xy.push_back(p.x);
      xy.push_back(p.y);
    }
  }
}
}  // namespace

size_t StructFromMotion::consolidateTracks(int minViews, bool verify) {
  const int nImg = (int)imagesPts2D.size();
  std::vector<int32_t> good(nGoodViews.begin(), nGoodViews.end()), pairs, nFeat((size_t)nImg);
  for (int i = 0; i < nImg; ++i) nFeat[i] = (int32_t)imagesPts2D[i].size();
  for (size_t a = 0; a < good.size(); ++a)
    for (size_t b = a + 1; b < good.size(); ++b) {
      if (good[a] < 0 || good[b] >= nImg) continue;
      pairs.push_back(good[a]);
      pairs.push_back(good[b]);
    }
  const int nPairs = (int)(pairs.size() / 2);
  if (nPairs == 0) return nReconstructionCloud.size();
  sfmhip_tracks_opts opts;
  sfmhip_tracks_default_opts(&opts);
  opts.min_len = minViews;
  sfmhip_tracks* tracks = nullptr;
  sfmhip_verified* verified = nullptr;
  std::vector<int32_t> xyPtr;
  std::vector<double> xy;
  packPixels(imagesPts2D, xyPtr, xy);
  int rc = SFMHIP_OK;
  // descriptors of one kind, one row per 2-D point: the resident image set (made here as getMatching makes it) and one plan
  // over every pair, whose lists are read where they lie on the device
  bool resident = !imagesDescriptors.empty() && (int)imagesDescriptors.size() == nImg && imagesDescriptors[0].cols > 0;
  for (int i = 0; resident && i < nImg; ++i)
    resident = imagesDescriptors[i].cols == imagesDescriptors[0].cols && imagesDescriptors[i].type() == imagesDescriptors[0].type() &&
               imagesDescriptors[i].rows == nFeat[i];
  if (resident) {
    if (!devSet) {
      const cv::Mat& d0 = imagesDescriptors[0];
      rc = sfmhip_imageset_create(sfm_hip_context(), nImg, nFeat.data(), d0.cols, d0.type() == CV_32F ? SFMHIP_F32 : SFMHIP_U8, SFMHIP_L2,
                                  &devSet);
      for (int i = 0; rc == SFMHIP_OK && i < nImg; ++i) rc = uploadOrAdopt(devSet, i);
      if (rc == SFMHIP_OK) rc = sfmhip_imageset_prepare_async(devSet);
      if (rc == SFMHIP_OK) rc = sfmhip_matchplan_create(devSet, pairs.data(), 1, &devPlan);  // (getMatching's one-pair plan)
      if (rc != SFMHIP_OK) releaseDeviceSet();
    }
    sfmhip_matchplan* plan = nullptr;
    if (rc == SFMHIP_OK) rc = sfmhip_matchplan_create(devSet, pairs.data(), nPairs, &plan);
    if (rc == SFMHIP_OK) rc = sfmhip_matchplan_run_async(plan, NN_MATCH_RATIO);
    if (rc == SFMHIP_OK && verify) rc = sfmhip_matchplan_verify(plan, xyPtr.data(), xy.data(), cameraMatrix.K.data.data(), nullptr, &verified);
    if (rc == SFMHIP_OK) rc = verify ? sfmhip_tracks_build_from_verified(verified, &opts, &tracks) : sfmhip_tracks_build_from_plan(plan, &opts, &tracks);
    if (plan) sfmhip_matchplan_destroy(plan);
  } else {  // the pair cache, or one matcher call per pair: host lists
    std::vector<int32_t> counts, q, t;
    for (int p = 0; p < nPairs; ++p) {
      Matching m;
      getMatching(pairs[2 * p], pairs[2 * p + 1], &m);
      counts.push_back((int32_t)m.size());
      for (const cv::DMatch& d : m) {
        q.push_back(d.queryIdx);
        t.push_back(d.trainIdx);
      }
    }
    if (verify) {
      rc = sfmhip_verify_lists(sfm_hip_context(), nImg, nFeat.data(), nPairs, pairs.data(), counts.data(), q.data(), t.data(), xyPtr.data(),
                               xy.data(), cameraMatrix.K.data.data(), nullptr, &verified);
      if (rc == SFMHIP_OK) rc = sfmhip_tracks_build_from_verified(verified, &opts, &tracks);
    } else {
      rc = sfmhip_tracks_build(sfm_hip_context(), nImg, nFeat.data(), nPairs, pairs.data(), counts.data(), q.data(), t.data(), &opts, &tracks);
    }
  }
  if (verified) {
    sfmhip_verified_counts(verified, &verifyStats);
    sfmhip_verified_destroy(verified);
    std::cout << "verify: " << verifyStats.pairs_kept << " of " << verifyStats.pairs << " pairs kept (" << verifyStats.pairs_no_model
              << " without a model), " << verifyStats.matches_out << " of " << verifyStats.matches_in << " matches" << std::endl;
  }
  if (rc != SFMHIP_OK) {
    std::cerr << "consolidateTracks: " << sfmhip_error_string(rc) << std::endl;
    return nReconstructionCloud.size();
  }
  sfmhip_tracks_stats st;
  sfmhip_tracks_counts(tracks, &st);
  std::vector<double> poses(12 * (size_t)nImg, 0.0), X(3 * (size_t)st.n_tracks);
  std::vector<uint8_t> hasPose((size_t)nImg, 0), keep((size_t)st.n_tracks);
  std::vector<int32_t> ptr((size_t)st.n_tracks + 1), view((size_t)st.n_obs), feat((size_t)st.n_obs);
  for (int i = 0; i < nImg; ++i) {
    if (nGoodViews.count(i) && (size_t)i < nCameraPoses.size()) {
      hasPose[i] = 1;
      for (int k = 0; k < 12; ++k) poses[12 * (size_t)i + k] = nCameraPoses[i].val[k];
    }
  }
  double dist[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < 5 && i < (int)cameraMatrix.distCoef.data.size(); ++i) dist[i] = cameraMatrix.distCoef.data[i];
  const float MIN_REPROJECTION_ERROR = 6.0;  // triangulateViews' bound
  rc = sfmhip_tracks_triangulate(tracks, poses.data(), hasPose.data(), cameraMatrix.K.data.data(), dist, xyPtr.data(), xy.data(),
                                 MIN_REPROJECTION_ERROR, minViews, X.data(), nullptr, nullptr, keep.data());
  if (rc == SFMHIP_OK) rc = sfmhip_tracks_download(tracks, ptr.data(), view.data(), feat.data(), nullptr);
  sfmhip_tracks_destroy(tracks);
  if (rc != SFMHIP_OK) {
    std::cerr << "consolidateTracks: " << sfmhip_error_string(rc) << std::endl;
    return nReconstructionCloud.size();
  }
  std::vector<Point3D> cloud;
  for (int64_t k = 0; k < st.n_tracks; ++k) {
    if (!keep[k]) continue;
    Point3D p;
    p.pt = cv::Point3d(X[3 * (size_t)k], X[3 * (size_t)k + 1], X[3 * (size_t)k + 2]);
    for (int j = ptr[k]; j < ptr[k + 1]; ++j) {
      if (!hasPose[view[j]]) continue;
      p.idxImage[view[j]] = feat[j];
      p.pt2D[view[j]] = imagesPts2D[view[j]][feat[j]];
    }
    cloud.push_back(p);
  }
  std::cout << "consolidateTracks: " << st.n_tracks << " tracks (" << st.conflicting << " conflicting, " << st.short_tracks << " short), "
            << cloud.size() << " points for " << nReconstructionCloud.size() << std::endl;
  nReconstructionCloud.swap(cloud);
  return nReconstructionCloud.size();
}
