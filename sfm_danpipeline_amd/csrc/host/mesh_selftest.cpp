// mesh_selftest.cpp -- the last call of map3D's step 10 (reference src/Sfm.cpp:98-102), needs the GPU:
//   mesh_selftest <MAP3D.pcd> <out.ply>
// loadPCDFile -> StructFromMotion::create_mesh(cloudXYZ, mesh) -> a binary little-endian PLY of the mesh (float x y z
// vertices, `list uchar int vertex_indices` faces).  Exit 4: the PCD does not load.
#include <cstdio>
#include "Sfm.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  StructFromMotion sfm;
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloudXYZ(new pcl::PointCloud<pcl::PointXYZ>);
  if (pcl::io::loadPCDFile(argv[1], *cloudXYZ) != 0) return 4;
  pcl::PolygonMesh mesh;
  sfm.create_mesh(cloudXYZ, mesh);
  FILE* o = fopen(argv[2], "wb");
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
  std::printf("points %zu vertices %zu triangles %zu\n", cloudXYZ->size(), mesh.cloud.size(), mesh.polygons.size());
  return 0;
}
