// essential_dev.h -- the RANSAC of sfmhip_score_essential (score.hip) as an internal routine whose results stay on the
// device, so that the pose step (pose.hip, sfmhip_essential_pose) reads E and the inlier mask where they are.
#pragma once
#include <vector>
#include "common.h"

struct EssentialDev {
  DevBufs bufs;  // every buffer below is freed with the object
  double* d_left = nullptr;   // the pixel coordinates as given: 2 doubles per match
  double* d_right = nullptr;
  double* d_p1 = nullptr;     // normalised with (fx, fy, cx, cy): findEssentialMat's points
  double* d_p2 = nullptr;
  double* d_bestE = nullptr;  // 9 per pair, row-major; zero where has[pair] == 0
  int* d_off = nullptr;       // offsets (n_pairs + 1)
  unsigned char* d_has = nullptr;   // per pair: 0 no model, 1 a RANSAC model, 2 exactly five matches
  unsigned char* d_mask = nullptr;  // the RANSAC mask, 1 byte per match (want_mask only)
  std::vector<unsigned char> has;
};

// findEssentialMat(left, right, K, RANSAC, prob, threshold) for a batch of pairs (arguments checked by the caller).
// Fills inliers (and iterations when non-null) on the host, ctx->score_flags, and dev; the work is ordered on
// ctx->stream and is complete when the call returns.
int sfm_essential_ransac(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy, const double* right_xy,
                         double fx, double fy, double cx, double cy, double prob, double threshold, int32_t* inliers,
                         int32_t* iterations, bool want_mask, EssentialDev& dev);

// The same from normalised points already on the device: the caller has allocated dev.d_p1 / dev.d_p2 from dev.bufs
// (2 doubles per match, at least one match's worth) and filled them on ctx->stream (verify.hip gathers them from the match
// lists).  d_left / d_right stay null.  sfm_essential_ransac is its upload and normalisation followed by this.
int sfm_essential_ransac_points(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, double fx, double fy, double prob,
                                double threshold, int32_t* inliers, int32_t* iterations, bool want_mask, EssentialDev& dev);
