// mesh.hip -- the finishing of a mesh against the device-resident cloud it was made from (sfmhip_cloud_mesh_finish; DESIGN.md
// f-24) on gfx950, by the rules M1-M7 of include/sfmhip.h: the trim of the surface no point supports, the drop of small
// components, per-vertex colours and normals, area and volume.  The arithmetic is mesh.h's, which the CPU test stub compiles too,
// and every output is the same bits as that build's.
//
// msh_keys + the handle's cell_sort: the vertices in the order of their cell of the cloud's radius grid (reg_keys' idea: the
// lanes of a wave then read the same rows).  msh_support: a lane per vertex walks the 9 row spans around its cell -- ascending
// (cell key, input index), which is M2's order -- with the count, the best pair and the five f64 sums in registers; a row goes
// to its vertex index.  The vertex's cell is the clamped one: clamping is monotone and moves no two coordinates apart, so the
// points within the radius of a vertex outside the cloud's box are still in the block around the cell it lands in, and a
// vertex far outside finds an empty block or points that fail the distance test.
// msh_tri_flags, msh_unite (union_find.h), msh_sizes, msh_component_flags, msh_keep: M3 and M4; integer atomics only, each a
// minimum, a count or a store of 1.  The handle's scan and msh_scatter_*: M5.  msh_pairs + cell_sort (stable) + msh_ranges +
// msh_normals: M6's incidence lists and their fixed-order sums.  msh_sums: M7's block trees; the host adds the partials in
// ascending order.  No atomics on floats.
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include "block_sum.h"
#include "mesh.h"
#include "mesh_object.h"
#include "union_find.h"
#include <algorithm>
#include <climits>
#include <vector>

using namespace sfmgrid;

namespace {

enum { C_UNSUPPORTED, C_TRIMMED, C_WORDS };

struct MeshState {  // on the cloud handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::MESH;
  Grow<float> verts, nd2, o_verts, o_nd2, o_normals;
  Grow<uint32_t> rgb_in, rgb, o_rgb;
  Grow<int> tris, kin, kout, vin, order, support, nearest, sup, parent, size, cflag, coff, cpairs, vused, voff, tflag, toff, o_tris, o_support,
      o_nearest, vsrc, tsrc, pkin, pkout, pvin, pvout, vstart, vend, cnt;
  Grow<double> part;
  double ms[4] = {0, 0, 0, 0};  // search, trim + components, compaction + normals + sums, the whole call
};

__device__ __forceinline__ bool finite_vertex(const float* v, int i) { return sfmcloud::finite3(v[3 * (size_t)i], v[3 * (size_t)i + 1], v[3 * (size_t)i + 2]); }

// the cell of the cloud's grid every vertex lands in (a non-finite vertex: `invalid`, behind every cell) and its index
__global__ void msh_keys(GridDev g, const float* verts, int nv, int invalid, int* keys, int* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  int key = invalid;
  if (finite_vertex(verts, i))
    key = (cell_of((double)verts[3 * (size_t)i + 2], g.o[2], g.cell, g.D[2]) * g.D[1] + cell_of((double)verts[3 * (size_t)i + 1], g.o[1], g.cell, g.D[1])) *
              g.D[0] +
          cell_of((double)verts[3 * (size_t)i], g.o[0], g.cell, g.D[0]);
  keys[i] = key;
  vals[i] = i;
}

// M2 + M3's vertex test.  order: the vertex of every lane (the results do not depend on it)
__global__ __launch_bounds__(256) void msh_support(GridDev g, const float* verts, int nv, const int* order, const uint32_t* rgb_in, float r2,
                                                   double r2d, int min_support, int* support, int* nearest, float* nd2, uint32_t* rgb, int* sup,
                                                   int* cnt) {
  const int l = blockIdx.x * blockDim.x + threadIdx.x;
  bool unsupported = false;
  if (l < nv) {
    const int i = order[l];
    const float vx = verts[3 * (size_t)i], vy = verts[3 * (size_t)i + 1], vz = verts[3 * (size_t)i + 2];
    const bool fin = sfmcloud::finite3(vx, vy, vz);
    sfmmesh::Support s;
    sfmmesh::support_zero(s);
    if (fin) {
      const int c[3] = {cell_of((double)vx, g.o[0], g.cell, g.D[0]), cell_of((double)vy, g.o[1], g.cell, g.D[1]),
                        cell_of((double)vz, g.o[2], g.cell, g.D[2])};
      const int x0 = max(c[0] - 1, 0), x1 = min(c[0] + 1, g.D[0] - 1);
      for (int z = max(c[2] - 1, 0); z <= min(c[2] + 1, g.D[2] - 1); ++z)
        for (int y = max(c[1] - 1, 0); y <= min(c[1] + 1, g.D[1] - 1); ++y) {
          int b, e;
          row_span(g, (z * g.D[1] + y) * g.D[0], x0, x1, &b, &e);
          for (int j = b; j < e; ++j) {
            const float4 q = g.pts[j];
            const int qi = __float_as_int(q.w);
            sfmmesh::support_add(s, vx, vy, vz, q.x, q.y, q.z, qi, rgb_in ? rgb_in[qi] : 0u, rgb_in != nullptr, r2, r2d);
          }
        }
    }
    const bool ok = sfmmesh::vertex_supported(fin, s.count, min_support);
    support[i] = s.count;
    nearest[i] = sfmmesh::nearest_of(s);
    nd2[i] = s.best_d2;
    if (rgb_in) rgb[i] = sfmmesh::colour_of(s);
    sup[i] = ok ? 1 : 0;
    unsupported = !ok;
  }
  const int nu = __popcll(__ballot(unsupported));  // (an integer count: order-free)
  if ((threadIdx.x & 63) == 0 && nu) atomicAdd(cnt + C_UNSUPPORTED, nu);
}

// M3: the triangles that survive the trim; parent[v] = v for the union-find rides along on the vertex range
__global__ __launch_bounds__(256) void msh_tri_flags(const int* tris, int nt, const int* sup, int* tflag, int* cnt) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  bool trimmed = false;
  if (t < nt) {
    const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    const bool keep = sfmmesh::triangle_distinct(a, b, c) && sup[a] && sup[b] && sup[c];
    tflag[t] = keep ? 1 : 0;
    trimmed = !keep;
  }
  const int n = __popcll(__ballot(trimmed));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(cnt + C_TRIMMED, n);
}

__global__ void msh_iota(int* parent, int nv) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v < nv) parent[v] = v;
}

__global__ void msh_unite(const int* tris, int nt, const int* tflag, int* parent) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt || !tflag[t]) return;
  const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
  sfmuf::unite(parent, a, b);
  sfmuf::unite(parent, b, c);
}

// M4: a component's size at its id, the root of its vertices = its least vertex (an integer count)
__global__ void msh_sizes(const int* tris, int nt, const int* tflag, int* parent, int* size) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt || !tflag[t]) return;
  atomicAdd(size + sfmuf::root_of(parent, tris[3 * (size_t)t]), 1);
}

// cflag[v] = 1 where v is the id of a component that stays (any: of any component)
__global__ void msh_component_flags(const int* size, int nv, int min_triangles, int cut_size, int cut_id, int any, int* cflag) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  cflag[v] = (any ? size[v] > 0 : sfmmesh::component_kept(size[v], v, min_triangles, cut_size, cut_id)) ? 1 : 0;
}

// the (id, size) pairs of the components, ascending by id
__global__ void msh_component_pairs(const int* size, const int* cflag, const int* coff, int nv, int* pairs) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv || !cflag[v]) return;
  pairs[2 * (size_t)coff[v]] = v;
  pairs[2 * (size_t)coff[v] + 1] = size[v];
}

// the triangles of the output and the vertices they use (every writer of vused[v] stores 1)
__global__ void msh_keep(const int* tris, int nt, int* parent, const int* cflag, int* tflag, int* vused) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt || !tflag[t]) return;
  const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
  if (!cflag[sfmuf::root_of(parent, a)]) {
    tflag[t] = 0;
    return;
  }
  vused[a] = 1;
  vused[b] = 1;
  vused[c] = 1;
}

// M5: the rows of the kept vertices, in input order
__global__ void msh_scatter_vertices(const float* verts, const int* support, const int* nearest, const float* nd2, const uint32_t* rgb,
                                     const int* vused, const int* voff, int nv, float* o_verts, int* o_support, int* o_nearest, float* o_nd2,
                                     uint32_t* o_rgb, int* vsrc) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv || !vused[v]) return;
  const size_t r = (size_t)voff[v];
  for (int a = 0; a < 3; ++a) o_verts[3 * r + a] = verts[3 * (size_t)v + a];
  o_support[r] = support[v];
  o_nearest[r] = nearest[v];
  o_nd2[r] = nd2[v];
  if (rgb) o_rgb[r] = rgb[v];
  vsrc[r] = v;
}

// ... and of the kept triangles, renumbered; with them M6's (vertex, triangle) pairs in the order (triangle, corner)
__global__ void msh_scatter_triangles(const int* tris, const int* tflag, const int* toff, const int* voff, int nt, int* o_tris, int* tsrc,
                                      int* pair_keys, int* pair_vals) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nt || !tflag[t]) return;
  const size_t r = (size_t)toff[t];
  for (int k = 0; k < 3; ++k) {
    const int v = voff[tris[3 * (size_t)t + k]];
    o_tris[3 * r + k] = v;
    pair_keys[3 * r + k] = v;
    pair_vals[3 * r + k] = (int)r;
  }
  tsrc[r] = t;
}

// the range of every output vertex in the sorted pairs (every output vertex has a triangle)
__global__ void msh_ranges(const int* keys, int m, int* start, int* end) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m) return;
  const int k = keys[s];
  if (s == 0 || keys[s - 1] != k) start[k] = s;
  if (s == m - 1 || keys[s + 1] != k) end[k] = s + 1;
}

__device__ __forceinline__ void load_triangle(const float* verts, const int* tris, size_t t, float a[3], float b[3], float c[3]) {
  const size_t ia = (size_t)tris[3 * t], ib = (size_t)tris[3 * t + 1], ic = (size_t)tris[3 * t + 2];
  for (int k = 0; k < 3; ++k) a[k] = verts[3 * ia + k], b[k] = verts[3 * ib + k], c[k] = verts[3 * ic + k];
}

// M6: a lane per output vertex sums the crosses of its triangles, ascending by output triangle
__global__ __launch_bounds__(256) void msh_normals(const float* verts, const int* tris, const int* start, const int* end, const int* pair_tri,
                                                   int nv, float* normals) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nv) return;
  double s[3] = {0.0, 0.0, 0.0};
  for (int j = start[v]; j < end[v]; ++j) {
    float a[3], b[3], c[3];
    double x[3];
    load_triangle(verts, tris, (size_t)pair_tri[j], a, b, c);
    sfmmesh::triangle_cross(a, b, c, x);
    s[0] = s[0] + x[0];
    s[1] = s[1] + x[1];
    s[2] = s[2] + x[2];
  }
  float o[3];
  sfmmesh::normal_write(s, o);
  for (int k = 0; k < 3; ++k) normals[3 * (size_t)v + k] = o[k];
}

// M7: area and volume of every block of 256 output triangles by block_sum.h's tree
__global__ __launch_bounds__(sfmsum::CHUNK) void msh_sums(const float* verts, const int* tris, int nt, double* part) {
  __shared__ double sh[2][4];
  const int t = blockIdx.x * sfmsum::CHUNK + threadIdx.x;
  double v[2] = {0.0, 0.0};
  if (t < nt) {
    float a[3], b[3], c[3];
    load_triangle(verts, tris, (size_t)t, a, b, c);
    v[0] = sfmmesh::triangle_area(a, b, c);
    v[1] = sfmmesh::triangle_volume(a, b, c);
  }
  sfmsum::block_tree<2>(v, sh);
  if (threadIdx.x < 2) part[2 * (size_t)blockIdx.x + threadIdx.x] = threadIdx.x == 0 ? v[0] : v[1];
}

bool opts_valid(const sfmhip_mesh_finish_opts* o) {
  return o && o->support_radius > 0.0 && sfmmesh::finite_d(o->support_radius) && o->min_support >= 0 && o->min_component_triangles >= 0 &&
         o->keep_largest >= 0;
}

template <class T>
int upload(T* dst, const T* src, size_t n, hipStream_t st) {
  if (n) SFM_HIP_TRY(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyHostToDevice, st));
  return SFMHIP_OK;
}
template <class T>
int download(std::vector<T>& dst, const T* src, size_t n, hipStream_t st) {
  dst.resize(n);
  if (n) SFM_HIP_TRY(hipMemcpyAsync(dst.data(), src, sizeof(T) * n, hipMemcpyDeviceToHost, st));
  return SFMHIP_OK;
}

// the finishing of a mesh of nv >= 1 vertices against a cloud with a finite point
int finish(sfmhip_cloud* c, const uint32_t* rgb, const sfmhip_mesh* in, const sfmhip_mesh_finish_opts& o, MeshState* s, sfmhip_mesh* out,
           sfmhip_mesh_finish_summary& sum) {
  hipStream_t st = c->ctx->stream;
  const bool timing = c->ctx->timing;
  const int nv = (int)(in->verts.size() / 3), nt = (int)(in->tris.size() / 3), nt1 = std::max(nt, 1);
  const double radius = o.support_radius;
  // the input mesh and the colours go up (the mesh is a host object: what that costs is the call's time less its three stages)
  SFM_TRY(s->verts.need((size_t)3 * nv));
  SFM_TRY(s->tris.need((size_t)3 * nt1));
  SFM_TRY(upload(s->verts.p, in->verts.data(), (size_t)3 * nv, st));
  SFM_TRY(upload(s->tris.p, in->tris.data(), (size_t)3 * nt, st));
  if (rgb) {
    SFM_TRY(s->rgb_in.need((size_t)c->n));
    SFM_TRY(upload(s->rgb_in.p, rgb, (size_t)c->n, st));
    SFM_TRY(s->rgb.need((size_t)nv));
    SFM_TRY(s->o_rgb.need((size_t)nv));
  }
  for (Grow<int>* g : {&s->kin, &s->kout, &s->vin, &s->order, &s->support, &s->nearest, &s->sup, &s->parent, &s->size, &s->cflag, &s->coff,
                       &s->vused, &s->voff, &s->o_support, &s->o_nearest, &s->vsrc, &s->vstart, &s->vend})
    SFM_TRY(g->need((size_t)nv));
  SFM_TRY(s->cpairs.need((size_t)2 * nv));
  for (Grow<int>* g : {&s->tflag, &s->toff, &s->tsrc}) SFM_TRY(g->need((size_t)nt1));
  for (Grow<int>* g : {&s->o_tris, &s->pkin, &s->pkout, &s->pvin, &s->pvout}) SFM_TRY(g->need((size_t)3 * nt1));
  for (Grow<float>* g : {&s->nd2, &s->o_nd2}) SFM_TRY(g->need((size_t)nv));
  SFM_TRY(s->o_verts.need((size_t)3 * nv));
  SFM_TRY(s->o_normals.need((size_t)3 * nv));
  SFM_TRY(s->cnt.need(C_WORDS));
  SFM_TRY(s->part.need((size_t)2 * blocks(nt1, sfmsum::CHUNK)));
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t0 = sfm_now_ms();

  // ---- M2: the search
  SFM_TRY(radius_grid(c, radius));  // (waits for the build)
  const GridDev g = c->rg.dev(c->n_valid);
  const unsigned bv = blocks(nv, 256), bt = blocks(nt1, 256);
  SFM_HIP_TRY(hipMemsetAsync(s->cnt.p, 0, sizeof(int) * C_WORDS, st));
  hipLaunchKernelGGL(msh_keys, dim3(bv), dim3(256), 0, st, g, s->verts.p, nv, (int)c->rg.ncell, s->kin.p, s->vin.p);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(cell_sort(c, c->rg.ncell, s->kin.p, s->kout.p, s->vin.p, s->order.p, nv));
  hipLaunchKernelGGL(msh_support, dim3(bv), dim3(256), 0, st, g, s->verts.p, nv, s->order.p, rgb ? s->rgb_in.p : nullptr, sfmcloud::radius2(radius),
                     sfmmesh::radius2_d(radius), o.min_support, s->support.p, s->nearest.p, s->nd2.p, rgb ? s->rgb.p : nullptr, s->sup.p, s->cnt.p);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t1 = sfm_now_ms();

  // ---- M3 + M4: the trim and the components
  int n_components = 0, n_kept = 0;
  SFM_HIP_TRY(hipMemsetAsync(s->size.p, 0, sizeof(int) * (size_t)nv, st));
  SFM_HIP_TRY(hipMemsetAsync(s->vused.p, 0, sizeof(int) * (size_t)nv, st));
  hipLaunchKernelGGL(msh_iota, dim3(bv), dim3(256), 0, st, s->parent.p, nv);
  if (nt > 0) {
    hipLaunchKernelGGL(msh_tri_flags, dim3(bt), dim3(256), 0, st, s->tris.p, nt, s->sup.p, s->tflag.p, s->cnt.p);
    hipLaunchKernelGGL(msh_unite, dim3(bt), dim3(256), 0, st, s->tris.p, nt, s->tflag.p, s->parent.p);
    hipLaunchKernelGGL(msh_sizes, dim3(bt), dim3(256), 0, st, s->tris.p, nt, s->tflag.p, s->parent.p, s->size.p);
  } else {
    SFM_HIP_TRY(hipMemsetAsync(s->tflag.p, 0, sizeof(int), st));
  }
  SFM_HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(msh_component_flags, dim3(bv), dim3(256), 0, st, s->size.p, nv, 0, -1, 0, 1, s->cflag.p);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(scan(c, s->cflag.p, s->coff.p, (size_t)nv, &n_components));  // (waits)
  if (n_components < 0 || n_components > nv) return SFMHIP_ERR_STATE;
  int cut_size = -1, cut_id = 0;
  if (o.keep_largest > 0 && n_components > o.keep_largest) {  // the k-th component by (size descending, id ascending), on the host
    hipLaunchKernelGGL(msh_component_pairs, dim3(bv), dim3(256), 0, st, s->size.p, s->cflag.p, s->coff.p, nv, s->cpairs.p);
    SFM_HIP_TRY(hipGetLastError());
    std::vector<int> pairs((size_t)2 * n_components);
    SFM_HIP_TRY(hipMemcpyAsync(pairs.data(), s->cpairs.p, sizeof(int) * pairs.size(), hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    std::vector<std::pair<int, int>> by((size_t)n_components);  // (-size, id): ascending is the rule's order
    for (int k = 0; k < n_components; ++k) by[k] = {-pairs[2 * (size_t)k + 1], pairs[2 * (size_t)k]};
    std::nth_element(by.begin(), by.begin() + (o.keep_largest - 1), by.end());
    cut_size = -by[o.keep_largest - 1].first;
    cut_id = by[o.keep_largest - 1].second;
  }
  hipLaunchKernelGGL(msh_component_flags, dim3(bv), dim3(256), 0, st, s->size.p, nv, o.min_component_triangles, cut_size, cut_id, 0, s->cflag.p);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(scan(c, s->cflag.p, s->coff.p, (size_t)nv, &n_kept));
  if (nt > 0) hipLaunchKernelGGL(msh_keep, dim3(bt), dim3(256), 0, st, s->tris.p, nt, s->parent.p, s->cflag.p, s->tflag.p, s->vused.p);
  SFM_HIP_TRY(hipGetLastError());
  if (timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  const double t2 = sfm_now_ms();

  // ---- M5: the compaction through the handle's scan
  int mv = 0, mt = 0;
  SFM_TRY(scan(c, s->vused.p, s->voff.p, (size_t)nv, &mv));
  SFM_TRY(scan(c, s->tflag.p, s->toff.p, (size_t)nt1, &mt));
  if (mv < 0 || mv > nv || mt < 0 || mt > nt) return SFMHIP_ERR_STATE;
  const int nb = (int)blocks(mt, sfmsum::CHUNK);
  if (mt > 0) {
    hipLaunchKernelGGL(msh_scatter_vertices, dim3(bv), dim3(256), 0, st, s->verts.p, s->support.p, s->nearest.p, s->nd2.p, rgb ? s->rgb.p : nullptr,
                       s->vused.p, s->voff.p, nv, s->o_verts.p, s->o_support.p, s->o_nearest.p, s->o_nd2.p, rgb ? s->o_rgb.p : nullptr, s->vsrc.p);
    hipLaunchKernelGGL(msh_scatter_triangles, dim3(bt), dim3(256), 0, st, s->tris.p, s->tflag.p, s->toff.p, s->voff.p, nt, s->o_tris.p, s->tsrc.p,
                       s->pkin.p, s->pvin.p);
    SFM_HIP_TRY(hipGetLastError());
    // ---- M6: the incidence lists by a stable sort of the pairs, then the normals
    SFM_TRY(cell_sort(c, (long long)mv, s->pkin.p, s->pkout.p, s->pvin.p, s->pvout.p, 3 * mt));
    hipLaunchKernelGGL(msh_ranges, dim3(blocks(3ll * mt, 256)), dim3(256), 0, st, s->pkout.p, 3 * mt, s->vstart.p, s->vend.p);
    hipLaunchKernelGGL(msh_normals, dim3(blocks(mv, 256)), dim3(256), 0, st, s->o_verts.p, s->o_tris.p, s->vstart.p, s->vend.p, s->pvout.p, mv,
                       s->o_normals.p);
    // ---- M7
    hipLaunchKernelGGL(msh_sums, dim3((unsigned)nb), dim3(sfmsum::CHUNK), 0, st, s->o_verts.p, s->o_tris.p, mt, s->part.p);
    SFM_HIP_TRY(hipGetLastError());
  }
  int cnt[C_WORDS] = {0, 0};
  std::vector<double> part;
  SFM_HIP_TRY(hipMemcpyAsync(cnt, s->cnt.p, sizeof cnt, hipMemcpyDeviceToHost, st));
  SFM_TRY(download(part, s->part.p, (size_t)2 * nb, st));
  SFM_TRY(download(out->verts, s->o_verts.p, (size_t)3 * mv, st));
  SFM_TRY(download(out->tris, s->o_tris.p, (size_t)3 * mt, st));
  SFM_TRY(download(out->normals, s->o_normals.p, (size_t)3 * mv, st));
  SFM_TRY(download(out->support, s->o_support.p, (size_t)mv, st));
  SFM_TRY(download(out->nearest, s->o_nearest.p, (size_t)mv, st));
  SFM_TRY(download(out->nearest_d2, s->o_nd2.p, (size_t)mv, st));
  SFM_TRY(download(out->vertex_src, s->vsrc.p, (size_t)mv, st));
  SFM_TRY(download(out->triangle_src, s->tsrc.p, (size_t)mt, st));
  if (rgb) SFM_TRY(download(out->rgb, s->o_rgb.p, (size_t)mv, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  double area = 0.0, volume = 0.0;
  for (int b = 0; b < nb; ++b) area = area + part[2 * (size_t)b], volume = volume + part[2 * (size_t)b + 1];
  sum.n_vertices = mv;
  sum.n_triangles = mt;
  sum.n_unsupported_vertices = cnt[C_UNSUPPORTED];
  sum.n_trimmed_triangles = cnt[C_TRIMMED];
  sum.n_components = n_components;
  sum.n_components_kept = n_kept;
  sum.area = area;
  sum.volume = volume;
  if (timing) {
    s->ms[0] = t1 - t0;
    s->ms[1] = t2 - t1;
    s->ms[2] = sfm_now_ms() - t2;
  }
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_mesh_finish_default_opts(sfmhip_mesh_finish_opts* o) {
  if (!o) return;
  o->support_radius = 0.0;
  o->min_support = 1;
  o->min_component_triangles = 0;
  o->keep_largest = 0;
  o->reserved = 0;
}

extern "C" int sfmhip_mesh_create(const float* vertices, int nv, const int32_t* triangles, int nt, sfmhip_mesh** out) {
  if (!out || nv < 0 || nt < 0 || nt > INT_MAX / 3 || nv > INT_MAX / 3 || (nv > 0 && !vertices) || (nt > 0 && !triangles)) return SFMHIP_ERR_ARG;
  for (size_t k = 0; k < (size_t)3 * nt; ++k)
    if (triangles[k] < 0 || triangles[k] >= nv) return SFMHIP_ERR_ARG;
  sfmhip_mesh* m = new sfmhip_mesh();
  m->verts.assign(vertices, vertices + (size_t)3 * nv);
  m->tris.assign(triangles, triangles + (size_t)3 * nt);
  *out = m;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_mesh_finish(sfmhip_cloud* c, const uint32_t* rgb, const sfmhip_mesh* in, const sfmhip_mesh_finish_opts* opts,
                                        sfmhip_mesh** out, sfmhip_mesh_finish_summary* summary) {
  if (!c || !in || !out || !opts_valid(opts)) return SFMHIP_ERR_ARG;
  const size_t nv = in->verts.size() / 3, nt = in->tris.size() / 3;
  if (nv > (size_t)(INT_MAX / 3) || nt > (size_t)(INT_MAX / 3)) return SFMHIP_ERR_ARG;
  for (int32_t v : in->tris)  // (a mesh of the extraction or of sfmhip_mesh_create holds none: the kernels index by it)
    if (v < 0 || (size_t)v >= nv) return SFMHIP_ERR_ARG;
  *out = nullptr;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  MeshState* s = stage<MeshState>(c);
  for (double& m : s->ms) m = 0;
  const double t0 = sfm_now_ms();
  sfmhip_mesh_finish_summary sum = {};
  sum.n_vertices_in = (int32_t)nv;
  sum.n_triangles_in = (int32_t)nt;
  sfmhip_mesh* mesh = new sfmhip_mesh();
  mesh->finished = true;
  mesh->coloured = rgb != nullptr;
  if (c->n_valid > 0 && nv > 0) {
    const int rc = finish(c, rgb, in, *opts, s, mesh, sum);
    if (rc != SFMHIP_OK) {
      delete mesh;
      return rc;
    }
  } else {  // M1: no finite point or no vertex: nothing is supported, nothing comes out
    sum.n_unsupported_vertices = (int32_t)nv;
    sum.n_trimmed_triangles = (int32_t)nt;
  }
  if (c->ctx->timing) s->ms[3] = sfm_now_ms() - t0;
  if (summary) *summary = sum;
  *out = mesh;
  return SFMHIP_OK;
}

extern "C" int sfmhip_mesh_attributes(const sfmhip_mesh* m, float* normals, uint32_t* rgb, int32_t* support, int32_t* nearest, float* nearest_d2,
                                      int32_t* vertex_src, int32_t* triangle_src) {
  if (!m) return SFMHIP_ERR_ARG;
  const bool asked = normals || rgb || support || nearest || nearest_d2 || vertex_src || triangle_src;
  if (asked && !m->finished) return SFMHIP_ERR_STATE;
  auto put = [](void* dst, const void* src, size_t bytes) {
    if (dst && bytes) memcpy(dst, src, bytes);
  };
  put(normals, m->normals.data(), m->normals.size() * sizeof(float));
  put(rgb, m->rgb.data(), m->rgb.size() * sizeof(uint32_t));  // (empty without colours: rgb is left as it is)
  put(support, m->support.data(), m->support.size() * sizeof(int32_t));
  put(nearest, m->nearest.data(), m->nearest.size() * sizeof(int32_t));
  put(nearest_d2, m->nearest_d2.data(), m->nearest_d2.size() * sizeof(float));
  put(vertex_src, m->vertex_src.data(), m->vertex_src.size() * sizeof(int32_t));
  put(triangle_src, m->triangle_src.data(), m->triangle_src.size() * sizeof(int32_t));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_mesh_last_timing(sfmhip_cloud* c, double ms4[4]) {
  if (!c || !ms4) return SFMHIP_ERR_ARG;
  const MeshState* s = stage<MeshState>(c);
  for (int i = 0; i < 4; ++i) ms4[i] = s->ms[i];
  return SFMHIP_OK;
}
