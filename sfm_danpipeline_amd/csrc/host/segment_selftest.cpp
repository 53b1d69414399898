// segment_selftest.cpp -- the two steps the reference's main runs after map3D (main.cpp:65-84), needs the GPU:
//   segment_selftest <MAP3D.pcd> <out.bin>
// Segmentation::color_based_growing_segmentation() on the PCD, then Dendrometry::estimate() on the cloud it loaded.
// out.bin: i32 n, i32 clusters, n x i32 label (-1 = in no cluster), 3 x f32 min, 3 x f32 max, f64 total height.
// Exit 3: the cloud is empty or no cluster came out (where the reference exits with -1).
#include <cstdio>
#include "DendrometryE.h"
#include "Segmentation.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  Segmentation seg;
  seg.setInputFile(argv[1]);
  if (seg.color_based_growing_segmentation() != 0) return 3;
  Dendrometry den;
  den.estimate(seg.cloud());
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const int n = (int)seg.labels().size(), nc = (int)seg.clusters().size();
  fwrite(&n, 4, 1, o);
  fwrite(&nc, 4, 1, o);
  fwrite(seg.labels().data(), 4, (size_t)n, o);
  fwrite(den.minPt(), 4, 3, o);
  fwrite(den.maxPt(), 4, 3, o);
  const double h = den.totalHeight();
  fwrite(&h, 8, 1, o);
  fclose(o);
  return 0;
}
