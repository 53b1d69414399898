// smooth_selftest.cpp -- the smoothing pass the reference's create_mesh names and does not run (src/Sfm.cpp:1347-1383), written
// against PCL's class as pcllite.h mirrors it; needs the GPU:
//   smooth_selftest <in.pcd> <radius> <order> <out.pcd> [<mesh.ply> [<mesh_plain.ply>]]
// loadPCDFile -> StructFromMotion::smoothCloud (pcl::MovingLeastSquares: setSearchRadius, setPolynomialFit / setPolynomialOrder,
// setComputeNormals) -> out.pcd: DATA binary, fields x y z normal_x normal_y normal_z curvature and, as an integer field,
// index: getCorrespondingIndices.  With mesh.ply: create_mesh(cloud, mesh, radius) -- the smoothing at order 2, the normals
// and Poisson without the smoothed points leaving the device -- as a binary PLY; with mesh_plain.ply: the two-argument
// create_mesh beside it.  Prints "points <n> smoothed <m>" and a line per mesh.  Exit 4: the PCD does not load.
#include <cstdio>
#include <cstdlib>
#include "Sfm.h"

static int write_ply(const char* path, const pcl::PolygonMesh& mesh) {
  FILE* o = fopen(path, "wb");
  if (!o) return 2;
  std::fprintf(o, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                  "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
               mesh.cloud.size(), mesh.polygons.size());
  for (const pcl::PointXYZ& p : mesh.cloud.points) fwrite(&p.x, 4, 3, o);
  for (const pcl::Vertices& f : mesh.polygons) {
    const unsigned char n = (unsigned char)f.vertices.size();
    fwrite(&n, 1, 1, o);
    for (uint32_t v : f.vertices) {
      const int32_t i = (int32_t)v;
      fwrite(&i, 4, 1, o);
    }
  }
  fclose(o);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>);
  if (pcl::io::loadPCDFile(argv[1], *cloud) != 0) return 4;
  const double radius = std::atof(argv[2]);
  StructFromMotion sfm;
  pcl::PointCloud<pcl::PointNormal>::Ptr smoothed;
  sfm.smoothCloud(cloud, radius, std::atoi(argv[3]), smoothed);
  // (smoothCloud keeps the class inside; the indices come from a second object run the same way)
  pcl::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> mls;
  mls.setInputCloud(cloud);
  mls.setSearchMethod(nullptr);
  mls.setSearchRadius(radius);
  mls.setPolynomialFit(std::atoi(argv[3]) > 0);
  mls.setPolynomialOrder(std::atoi(argv[3]) > 0 ? std::atoi(argv[3]) : 2);
  mls.setComputeNormals(true);
  pcl::PointCloud<pcl::PointNormal> again;
  mls.process(again);
  const std::vector<int>& idx = mls.getCorrespondingIndices()->indices;
  if (again.size() != smoothed->size() || idx.size() != again.size()) return 5;
  FILE* o = fopen(argv[4], "wb");
  if (!o) return 2;
  const int k = (int)smoothed->size();
  std::fprintf(o, "# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z normal_x normal_y normal_z curvature index\n"
                  "SIZE 4 4 4 4 4 4 4 4\nTYPE F F F F F F F I\nCOUNT 1 1 1 1 1 1 1 1\nWIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\n"
                  "DATA binary\n", k, k);
  for (int i = 0; i < k; ++i) {
    fwrite(&smoothed->points[i].x, 4, 7, o);
    const int32_t j = idx[i];
    fwrite(&j, 4, 1, o);
  }
  fclose(o);
  std::printf("points %d smoothed %d\n", (int)cloud->size(), k);
  if (argc > 5) {
    pcl::PolygonMesh mesh;
    sfm.create_mesh(cloud, mesh, radius);
    if (write_ply(argv[5], mesh) != 0) return 2;
    std::printf("smoothed mesh: vertices %zu triangles %zu\n", mesh.cloud.size(), mesh.polygons.size());
  }
  if (argc > 6) {
    pcl::PolygonMesh mesh;
    sfm.create_mesh(cloud, mesh);
    if (write_ply(argv[6], mesh) != 0) return 2;
    std::printf("plain mesh: vertices %zu triangles %zu\n", mesh.cloud.size(), mesh.polygons.size());
  }
  return 0;
}
