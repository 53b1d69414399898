// cloud_filter_selftest.cpp -- the two filters between a dense cloud and everything after it, written against PCL's
// classes as pcllite.h mirrors them; needs the GPU:
//   cloud_filter_selftest <in.pcd> <leaf> <mean_k> <std_mul> <out.pcd>
// loadPCDFile -> pcl::VoxelGrid (setLeafSize(leaf, leaf, leaf)) -> pcl::StatisticalOutlierRemoval (setMeanK, setStddevMulThresh)
// -> computeNormals (create_mesh's first half: 10 nearest, negated) -> out.pcd: DATA binary, fields x y z normal_x normal_y
// normal_z curvature.  Prints "points <n> voxels <m> kept <k>".  Exit 4: the PCD does not load.
#include <cstdio>
#include <cstdlib>
#include <string>
#include "Sfm.h"

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>);
  if (pcl::io::loadPCDFile(argv[1], *cloud) != 0) return 4;
  const float leaf = std::strtof(argv[2], nullptr);
  pcl::PointCloud<pcl::PointXYZ>::Ptr thin(new pcl::PointCloud<pcl::PointXYZ>), kept(new pcl::PointCloud<pcl::PointXYZ>);
  pcl::VoxelGrid<pcl::PointXYZ> vg;
  vg.setInputCloud(cloud);
  vg.setLeafSize(leaf, leaf, leaf);
  vg.filter(*thin);
  pcl::StatisticalOutlierRemoval<pcl::PointXYZ> sor;
  sor.setInputCloud(thin);
  sor.setMeanK(std::atoi(argv[3]));
  sor.setStddevMulThresh(std::atof(argv[4]));
  sor.filter(*kept);
  StructFromMotion sfm;
  pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
  sfm.computeNormals(kept, normals);
  FILE* o = fopen(argv[5], "wb");
  if (!o) return 2;
  const int k = (int)kept->size();
  std::fprintf(o, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z curvature\n"
                  "SIZE 4 4 4 4 4 4 4\nTYPE F F F F F F F\nCOUNT 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\n"
                  "DATA binary\n", k, k);
  for (int i = 0; i < k; ++i) {
    fwrite(&kept->points[i].x, 4, 3, o);
    fwrite(&normals->points[i].normal_x, 4, 4, o);
  }
  fclose(o);
  std::printf("points %d voxels %d kept %d\n", (int)cloud->size(), (int)thin->size(), k);
  return 0;
}
