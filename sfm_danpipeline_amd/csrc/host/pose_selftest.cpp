// pose_selftest.cpp -- drives the base reconstruction of the C++ host mirror (needs the GPU):
//   pose_selftest <image dir> <calibration.xml> <out.bin>
// imagesLOAD -> getCameraMatrix -> extractFeature -> baseReconstruction (findBestPair, then getCameraPose over the map:
// sfmhip_essential_pose, and triangulateViews on the first pair whose pose passes) -> adjustCurrentBundle.  out.bin:
//   i32 q, i32 t (-1, -1: no pair passed; nothing follows), i32 n_good, f64 E[9], f64 R[9], f64 T[3]   the chosen pair
//   i32 n; n bytes: recoverPose's output mask over the pair's matches (getMatching order)
//   f64 Pq[12], f64 Pt[12]                                                                              nCameraPoses
//   i32 n_cloud, n_cloud x (f64 xyz[3], i32 fq, i32 ft)                                                 the seeded cloud
//   after adjustCurrentBundle: f64 K[9], f64 Pq[12], f64 Pt[12], n_cloud x f64 xyz[3]
//   pose_selftest --get-camera-pose <calibration.xml> <in.bin> <out.bin>
// getCameraPose(K, 0, 1, matches, left, right) on a caller's points: in.bin = i32 n, n x f64 left[2], n x f64 right[2], then
// the members imagesPts2D[0] and [1] (n x f64 [2] each, what the homography pruning reads); the matches are (i, i).
// out.bin = i32 ok, f64 Pleft[12], f64 Pright[12].  Exit 5 when baseReconstruction (or the batched pose call) fails.
#include <cstdio>
#include <string>
#include <vector>
#include "Sfm.h"

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  if (std::string(argv[1]) == "--get-camera-pose") {
    if (argc < 5) return 2;
    StructFromMotion sfm;
    if (!sfm.getCameraMatrix(argv[2])) return 4;
    FILE* fi = fopen(argv[3], "rb");
    if (!fi) return 2;
    int n = 0;
    if (fread(&n, 4, 1, fi) != 1 || n < 0) return 2;
    std::vector<Points2d> pts(4, Points2d((size_t)n));
    for (Points2d& p : pts)
      for (cv::Point2d& q : p)
        if (fread(&q.x, 8, 2, fi) != 2) return 2;
    fclose(fi);
    sfm.setPoints2D(std::vector<Points2d>{pts[2], pts[3]});
    Matching m;
    for (int i = 0; i < n; ++i) m.push_back(cv::DMatch(i, i, 0.f));
    cv::Matx34d Pl, Pr;
    const int ok = sfm.getCameraPose(sfm.intrinsics(), 0, 1, m, pts[0], pts[1], Pl, Pr) ? 1 : 0;
    FILE* o = fopen(argv[4], "wb");
    if (!o) return 2;
    fwrite(&ok, 4, 1, o);
    fwrite(Pl.val, 8, 12, o);
    fwrite(Pr.val, 8, 12, o);
    fclose(o);
    return 0;
  }
  StructFromMotion sfm;
  if (!sfm.imagesLOAD(argv[1])) return 3;
  if (!sfm.getCameraMatrix(argv[2])) return 4;
  sfm.extractFeature();
  if (!sfm.baseReconstruction()) return 5;
  FILE* o = fopen(argv[3], "wb");
  if (!o) return 2;
  const StructFromMotion::BasePose& b = sfm.basePose();
  fwrite(&b.query, 4, 1, o);
  fwrite(&b.train, 4, 1, o);
  if (b.query < 0) {
    fclose(o);
    return 0;
  }
  const int q = b.query, t = b.train;
  fwrite(&b.n_good, 4, 1, o);
  fwrite(b.E, 8, 9, o);
  fwrite(b.R, 8, 9, o);
  fwrite(b.T, 8, 3, o);
  const int nm = (int)b.mask.size();
  fwrite(&nm, 4, 1, o);
  fwrite(b.mask.data(), 1, b.mask.size(), o);
  fwrite(sfm.cameraPoses()[q].val, 8, 12, o);
  fwrite(sfm.cameraPoses()[t].val, 8, 12, o);
  const int nc = (int)sfm.nReconstructionCloud.size();
  fwrite(&nc, 4, 1, o);
  for (const Point3D& p : sfm.nReconstructionCloud) {
    fwrite(&p.pt.x, 8, 3, o);
    const int fq = p.idxImage.at(q), ft = p.idxImage.at(t);
    fwrite(&fq, 4, 1, o);
    fwrite(&ft, 4, 1, o);
  }
  sfm.adjustCurrentBundle();
  fwrite(sfm.intrinsics().K.data.data(), 8, 9, o);
  fwrite(sfm.cameraPoses()[q].val, 8, 12, o);
  fwrite(sfm.cameraPoses()[t].val, 8, 12, o);
  for (const Point3D& p : sfm.nReconstructionCloud) fwrite(&p.pt.x, 8, 3, o);
  fclose(o);
  return 0;
}
