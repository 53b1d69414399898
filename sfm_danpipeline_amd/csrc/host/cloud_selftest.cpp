// cloud_selftest.cpp -- map3D's steps 8-10 in the reference's order (src/Sfm.cpp:69-81, 94-102), needs the GPU:
//   cloud_selftest <in.ply> <work dir> <out.bin>
// convertPLYtoPCD(in.ply, <work dir>/MAP3D.pcd) -> loadPCDFile -> cloudPointFilter(cloudXYZ, filterCloud) ->
// removePoints(cloudXYZ, filterCloud) -> computeNormals(cloudXYZ) (create_mesh's first half), every call on the
// UNFILTERED cloud as the reference makes them.  out.bin:
//   i32 n, n x f32 xyz[3]            the loaded cloud
//   i32 m1, m1 x f32 xyz[3]          filterCloud after cloudPointFilter
//   i32 m2, m2 x f32 xyz[3]          filterCloud after removePoints (what the reference keeps)
//   i32 n, n x f32 (nx, ny, nz, curvature)   the normals create_mesh would pass on (negated)
// Exit 3: the PLY is empty (the reference's "ply file is empty"); 4: the PCD does not load.
#include <cstdio>
#include <string>
#include <vector>
#include "Sfm.h"

static void put_cloud(FILE* o, const pcl::PointCloud<pcl::PointXYZ>& c) {
  const int n = (int)c.size();
  fwrite(&n, 4, 1, o);
  for (const pcl::PointXYZ& p : c.points) fwrite(&p.x, 4, 3, o);
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  const std::string pcd = std::string(argv[2]) + "/MAP3D.pcd";
  if (StructFromMotion::convertPLYtoPCD(argv[1], pcd) == 0) return 3;
  StructFromMotion sfm;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloudXYZ(new pcl::PointCloud<pcl::PointXYZ>);
  if (pcl::io::loadPCDFile(pcd, *cloudXYZ) != 0) return 4;
  pcl::PointCloud<pcl::PointXYZ>::Ptr filterCloud(new pcl::PointCloud<pcl::PointXYZ>);
  FILE* o = fopen(argv[3], "wb");
  if (!o) return 2;
  put_cloud(o, *cloudXYZ);
  sfm.cloudPointFilter(cloudXYZ, filterCloud);
  put_cloud(o, *filterCloud);
  const size_t m1 = filterCloud->size();
  sfm.removePoints(cloudXYZ, filterCloud);
  put_cloud(o, *filterCloud);
  pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
  sfm.computeNormals(cloudXYZ, normals);
  const int n = (int)normals->size();
  fwrite(&n, 4, 1, o);
  for (const pcl::Normal& q : normals->points) fwrite(&q.normal_x, 4, 4, o);
  fclose(o);
  std::printf("points %d passthrough %zu radius %zu normals %d\n", (int)cloudXYZ->size(), m1, filterCloud->size(), n);
  return 0;
}
