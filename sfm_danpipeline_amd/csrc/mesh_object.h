// mesh_object.h -- sfmhip_mesh, the host object behind the mesh handle of include/sfmhip.h: poisson.hip's extraction fills
// the geometry, sfmhip_mesh_create wraps a caller's arrays, and mesh.hip's finishing call adds the
// per-vertex and per-triangle attributes.  A mesh that did not come out of the finishing call has none.
#pragma once
#include <cstdint>
#include <vector>

struct sfmhip_mesh {
  std::vector<float> verts;
  std::vector<int32_t> tris;
  // ---- sfmhip_cloud_mesh_finish's output only
  bool finished = false, coloured = false;
  std::vector<float> normals, nearest_d2;                     // 3 nv, nv
  std::vector<uint32_t> rgb;                                  // nv, filled when the call was given colours
  std::vector<int32_t> support, nearest, vertex_src, triangle_src;  // nv, nv, nv, nt
};
