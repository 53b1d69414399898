// tracks_selftest.cpp -- drives the track consolidation of the C++ host mirror (needs the GPU): baseReconstruction(),
// addMoreViews(), consolidateTracks(minViews), adjustBundle().
//   tracks_selftest --scene <scene.bin> <out prefix> [minViews]
//   tracks_selftest --images <image dir> <calibration.xml> <out prefix> [minViews]
// With --verify among the arguments the lists pass the two-view verification first (consolidateTracks(minViews, true);
// DESIGN.md f-19), and a line "verified: pairs P kept K no_model N matches A -> B" precedes "consolidated:".
// The inputs are incr_selftest's.  Writes <out prefix>.before (the state after addMoreViews) and <out prefix>.after (after the
// consolidation and one more bundle adjustment), both in incr_selftest's out.bin layout.  A line "consolidated: N" goes to
// stdout and to stderr before that last bundle adjustment, so that its messages can be told from the earlier ones.
// Exit 5 when baseReconstruction fails or finds no base pair, 6 when addMoreViews does, 7 when no track is kept.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>
#include "Sfm.h"

namespace {
bool rd(FILE* f, void* p, size_t bytes) { return bytes == 0 || fread(p, bytes, 1, f) == 1; }

bool write_state(const std::string& path, const StructFromMotion& sfm, int n_img, int base_cloud) {
  FILE* o = fopen(path.c_str(), "wb");
  if (!o) return false;
  const StructFromMotion::BasePose& b = sfm.basePose();
  fwrite(&n_img, 4, 1, o);
  fwrite(&b.query, 4, 1, o);
  fwrite(&b.train, 4, 1, o);
  fwrite(&base_cloud, 4, 1, o);
  for (int i = 0; i < n_img; ++i) {
    const cv::Matx34d P = (size_t)i < sfm.cameraPoses().size() ? sfm.cameraPoses()[i] : cv::Matx34d();
    fwrite(P.val, 8, 12, o);
  }
  fwrite(sfm.intrinsics().K.data.data(), 8, 9, o);
  for (const std::set<int>* s : {&sfm.doneViews(), &sfm.goodViews()}) {
    const int n = (int)s->size();
    fwrite(&n, 4, 1, o);
    for (int v : *s) fwrite(&v, 4, 1, o);
  }
  const int nc = (int)sfm.nReconstructionCloud.size();
  fwrite(&nc, 4, 1, o);
  for (const Point3D& p : sfm.nReconstructionCloud) {
    fwrite(&p.pt.x, 8, 3, o);
    const int nt = (int)p.idxImage.size();
    fwrite(&nt, 4, 1, o);
    for (const auto& kv : p.idxImage) {
      const int vf[2] = {kv.first, kv.second};
      fwrite(vf, 4, 2, o);
    }
  }
  return fclose(o) == 0;
}
}  // namespace

int main(int argc, char** argv) {
  bool verify = false;  // --verify, wherever it stands, is taken out of the arguments
  for (int i = 1; i < argc; ++i)
    if (std::string(argv[i]) == "--verify") {
      verify = true;
      for (int j = i; j + 1 < argc; ++j) argv[j] = argv[j + 1];
      --argc;
      --i;
    }
  if (argc < 4) return 2;
  StructFromMotion sfm;
  std::string out;
  int n_img = 0, next = 4;
  if (std::string(argv[1]) == "--scene") {
    FILE* fi = fopen(argv[2], "rb");
    if (!fi) return 2;
    Intrinsics in;
    in.K = cv::Mat_<double>(3, 3);
    in.distCoef = cv::Mat_<double>(1, 5);
    if (!rd(fi, &n_img, 4) || n_img < 2 || !rd(fi, in.K.data.data(), 72) || !rd(fi, in.distCoef.data.data(), 40)) return 2;
    std::vector<Points2d> pts((size_t)n_img);
    for (Points2d& p : pts) {
      int n = 0;
      if (!rd(fi, &n, 4) || n < 0) return 2;
      p.resize((size_t)n);
      if (!rd(fi, p.data(), 16 * (size_t)n)) return 2;
    }
    sfm.setDescriptors(std::vector<cv::Mat>((size_t)n_img));
    sfm.setImageCount(n_img);
    sfm.setPoints2D(pts);
    sfm.setCameraMatrix(in);
    int n_pairs = 0;
    if (!rd(fi, &n_pairs, 4) || n_pairs < 0) return 2;
    for (int p = 0; p < n_pairs; ++p) {
      int hdr[3];
      if (!rd(fi, hdr, 12) || hdr[0] < 0 || hdr[1] <= hdr[0] || hdr[1] >= n_img || hdr[2] < 0) return 2;
      std::vector<int> qt(2 * (size_t)hdr[2]);
      if (!rd(fi, qt.data(), 8 * (size_t)hdr[2])) return 2;
      Matching m;
      for (int i = 0; i < hdr[2]; ++i) {
        if (qt[2 * i] < 0 || qt[2 * i] >= (int)pts[hdr[0]].size() || qt[2 * i + 1] < 0 || qt[2 * i + 1] >= (int)pts[hdr[1]].size()) return 2;
        m.push_back(cv::DMatch(qt[2 * i], qt[2 * i + 1], 0.f));
      }
      sfm.setPairMatches(hdr[0], hdr[1], m);
    }
    fclose(fi);
    out = argv[3];
  } else if (std::string(argv[1]) == "--images") {
    if (argc < 5) return 2;
    if (!sfm.imagesLOAD(argv[2])) return 3;
    if (!sfm.getCameraMatrix(argv[3])) return 4;
    sfm.extractFeature();
    n_img = (int)sfm.grayImages().size();
    out = argv[4];
    next = 5;
  } else {
    return 2;
  }
  const int min_views = argc > next ? std::atoi(argv[next]) : 2;
  if (!sfm.baseReconstruction() || sfm.basePose().query < 0) return 5;
  const int base_cloud = (int)sfm.nReconstructionCloud.size();
  if (!sfm.addMoreViews()) return 6;
  if (!write_state(out + ".before", sfm, n_img, base_cloud)) return 2;
  const size_t n = verify ? sfm.consolidateTracks(min_views, true) : sfm.consolidateTracks(min_views);
  if (verify) {
    const sfmhip_verify_stats& vs = sfm.lastVerifyStats();
    std::cout << "verified: pairs " << vs.pairs << " kept " << vs.pairs_kept << " no_model " << vs.pairs_no_model << " matches " << vs.matches_in
              << " -> " << vs.matches_out << std::endl;
  }
  std::cout << "consolidated: " << n << std::endl;
  std::cerr << "consolidated: " << n << std::endl;
  if (n == 0) return 7;
  sfm.adjustCurrentBundle();
  return write_state(out + ".after", sfm, n_img, base_cloud) ? 0 : 2;
}
