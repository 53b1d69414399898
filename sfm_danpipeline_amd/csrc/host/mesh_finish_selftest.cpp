// mesh_finish_selftest.cpp -- create_mesh with the finishing behind it, needs the GPU:
//   mesh_finish_selftest <MAP3D.pcd> <out.ply>
// loadPCDFile (x y z and rgb; a file without colours gives colour 0) -> StructFromMotion::create_mesh(cloudRGB, mesh): the
// normals, their flip, Poisson at depth 7, then finishMesh with the mirror's defaults (support radius 1.5 cells, min_support
// 1) -> a binary little-endian PLY of the trimmed mesh: float x y z nx ny nz and uchar red green blue per vertex, `list uchar
// int vertex_indices` faces.  Prints the summary on one line.  Exit 4: the PCD does not load.
#include <cstdio>
#include "Sfm.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  StructFromMotion sfm;
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>);
  if (pcl::io::loadPCDFile(argv[1], *cloud) != 0) return 4;
  pcl::PolygonMesh mesh;
  sfmhip_mesh_finish_summary s;
  sfm.create_mesh(cloud, mesh, &s);
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  std::fprintf(o, "ply\nformat binary_little_endian 1.0\nelement vertex %zu\nproperty float x\nproperty float y\nproperty float z\n"
                  "property float nx\nproperty float ny\nproperty float nz\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
                  "element face %zu\nproperty list uchar int vertex_indices\nend_header\n",
               mesh.cloud.size(), mesh.polygons.size());
  for (size_t i = 0; i < mesh.cloud.size(); ++i) {
    const pcl::Normal& n = mesh.normals[i];
    const float f[6] = {mesh.cloud.points[i].x, mesh.cloud.points[i].y, mesh.cloud.points[i].z, n.normal_x, n.normal_y, n.normal_z};
    const unsigned char c[3] = {(unsigned char)(mesh.colours[i] >> 16), (unsigned char)(mesh.colours[i] >> 8), (unsigned char)mesh.colours[i]};
    fwrite(f, 4, 6, o);
    fwrite(c, 1, 3, o);
  }
  for (const pcl::Vertices& f : mesh.polygons) {
    const unsigned char n = (unsigned char)f.vertices.size();
    fwrite(&n, 1, 1, o);
    for (uint32_t v : f.vertices) {
      const int32_t i = (int32_t)v;
      fwrite(&i, 4, 1, o);
    }
  }
  fclose(o);
  std::printf("points %zu vertices %d -> %d triangles %d -> %d unsupported %d trimmed %d components %d kept %d area %.9g volume %.9g\n",
              cloud->size(), (int)s.n_vertices_in, (int)s.n_vertices, (int)s.n_triangles_in, (int)s.n_triangles, (int)s.n_unsupported_vertices,
              (int)s.n_trimmed_triangles, (int)s.n_components, (int)s.n_components_kept, s.area, s.volume);
  return 0;
}
