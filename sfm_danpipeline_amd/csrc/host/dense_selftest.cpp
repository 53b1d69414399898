// dense_selftest.cpp -- map3D's step 7 in the host mirror, needs the GPU:
//   dense_selftest <image dir> <calib.xml> <poses+cloud.bin> <out dir>
// imagesLOAD -> getCameraMatrix -> the poses and the sparse cloud from the file -> StructFromMotion::densify, which writes
// <out dir>/models/options.txt.ply (the directories are made here, as PMVS2() makes them under denseCloud/).
// poses+cloud.bin, little-endian:  i32 n_views, 9 f64 K (all zero: the calibration file's K stays; else the K the poses were
//                                  adjusted with), per view (i32 registered, 12 f64 [R|t] row-major);
//                                  i32 n_points, per point (3 f64 xyz, i32 n_obs, n_obs x i32 view)
// Exit 3: the images or the calibration do not load; 4: the file is short; 5: the dense cloud is empty.
#include <sys/stat.h>
#include <cstdio>
#include <memory>
#include <string>
#include "Sfm.h"

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  StructFromMotion sfm;
  if (!sfm.imagesLOAD(argv[1]) || !sfm.getCameraMatrix(argv[2])) return 3;
  const std::unique_ptr<FILE, int (*)(FILE*)> file(std::fopen(argv[3], "rb"), std::fclose);  // closed on every return
  FILE* f = file.get();
  if (!f) return 4;
  int32_t nv = 0, np = 0;
  if (std::fread(&nv, 4, 1, f) != 1 || nv < 0 || (size_t)nv != sfm.grayImages().size()) return 4;
  double K[9];
  if (std::fread(K, 8, 9, f) != 9) return 4;
  if (K[0] != 0.0) {
    Intrinsics in = sfm.intrinsics();
    for (int i = 0; i < 9; ++i) in.K.data[i] = K[i];
    sfm.setCameraMatrix(in);
  }
  std::vector<cv::Matx34d> poses((size_t)nv);
  std::set<int> good;
  for (int v = 0; v < nv; ++v) {
    int32_t reg = 0;
    if (std::fread(&reg, 4, 1, f) != 1 || std::fread(poses[v].val, 8, 12, f) != 12) return 4;
    if (reg) good.insert(v);
  }
  if (std::fread(&np, 4, 1, f) != 1 || np < 0) return 4;
  for (int i = 0; i < np; ++i) {
    Point3D p;
    double x[3];
    int32_t no = 0;
    if (std::fread(x, 8, 3, f) != 3 || std::fread(&no, 4, 1, f) != 1 || no < 0) return 4;
    p.pt = cv::Point3d(x[0], x[1], x[2]);
    for (int k = 0; k < no; ++k) {
      int32_t v = 0;
      if (std::fread(&v, 4, 1, f) != 1) return 4;
      p.idxImage[v] = 0;
    }
    sfm.nReconstructionCloud.push_back(p);
  }
  sfm.setCameraPoses(poses);
  sfm.setGoodViews(good);
  sfm.setDoneViews(good);
  const std::string out = argv[4];
  mkdir(out.c_str(), 0777);
  mkdir((out + "/models").c_str(), 0777);
  const size_t n = sfm.densify(out + "/models/options.txt.ply");
  std::printf("views %d registered %zu sparse %d dense %zu\n", (int)nv, good.size(), (int)np, n);
  return n ? 0 : 5;
}
