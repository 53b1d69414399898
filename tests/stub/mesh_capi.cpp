// mesh_capi.cpp -- a C surface over csrc/mesh.h for tests/test_mesh_cpu.py and tests/test_gpu_mesh.py (built with g++ -O2
// -ffp-contract=off -pthread) and, with -DMESH_MAIN, a stand-alone driver that finishes meshes of its own under the sanitizers.
// Plain host loops: the search is brute force over all points, whose hits are then sorted by (M2's cell id, input index), or a
// walk of the 27 cells around the vertex's cell of M2's grid, which meets them in that order; the tests compare the two.  The
// union-find is a sequential one, the incidence lists are filled in triangle order, the block sums are block_sum.h's host tree.
// Only the grid's key function and the arithmetic come from the shared headers.  Status codes are include/sfmhip.h's.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <utility>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/block_sum.h"
#include "../../sfm_danpipeline_amd/csrc/mesh.h"

namespace {

constexpr int OK = 0, ERR_ARG = -3;

template <typename F>
void parallel(int n, int threads, F f) {
  const int T = std::max(1, std::min(threads, n));
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t)
    th.emplace_back([&, t] {
      for (int i = t; i < n; i += T) f(i);
    });
  for (auto& x : th) x.join();
}

bool finite_pt(const float* p) { return sfmcloud::finite3(p[0], p[1], p[2]); }

// M2's grid for radius r over the finite points; returns their count
int geometry(int n, const float* xyz, double r, sfmcloud::GridGeom& g) {
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  int nv = 0;
  for (int i = 0; i < n; ++i) {
    const float* p = xyz + 3 * (size_t)i;
    if (!finite_pt(p)) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = nv ? std::min(lo[a], (double)p[a]) : (double)p[a];
      hi[a] = nv ? std::max(hi[a], (double)p[a]) : (double)p[a];
    }
    ++nv;
  }
  sfmcloud::grid_geometry(lo, hi, nv, sfmcloud::radius_cell(r), g);
  return nv;
}

struct Mesh {
  std::vector<float> verts, normals, nd2;
  std::vector<int32_t> tris, support, nearest, vsrc, tsrc;
  std::vector<uint32_t> rgb;
  int32_t counts[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the summary's integers in its order
  double area = 0, volume = 0;
};

int find(std::vector<int>& parent, int x) {
  while (parent[x] != x) x = parent[x] = parent[parent[x]];
  return x;
}

}  // namespace

extern "C" {

// sfmhip_cloud_mesh_finish without the handles.  search: 0 = brute force up to 2048 points and the grid walk above, 1 = brute
// force, 2 = the grid walk.  rgb may be NULL.  *out: a Mesh for msh_counts / msh_get / msh_free
int msh_finish(int n, const float* xyz, const uint32_t* rgb, int nv, const float* verts, int nt, const int32_t* tris, double radius,
               int min_support, int min_component, int keep_largest, int search, int threads, void** out) {
  if (!out || n < 0 || nv < 0 || nt < 0 || !(radius > 0.0) || !sfmmesh::finite_d(radius) || min_support < 0 || min_component < 0 ||
      keep_largest < 0)
    return ERR_ARG;
  for (size_t k = 0; k < (size_t)3 * nt; ++k)
    if (tris[k] < 0 || tris[k] >= nv) return ERR_ARG;
  Mesh* m = new Mesh();
  *out = m;
  m->counts[0] = nv;
  m->counts[1] = nt;
  sfmcloud::GridGeom g;
  const int n_valid = geometry(n, xyz, radius, g);
  if (n_valid == 0 || nv == 0) {  // M1
    m->counts[4] = nv;
    m->counts[5] = nt;
    return OK;
  }
  // M2
  const float r2 = sfmcloud::radius2(radius);
  const double r2d = sfmmesh::radius2_d(radius);
  std::vector<int> key((size_t)n, -1);
  for (int i = 0; i < n; ++i)
    if (finite_pt(xyz + 3 * (size_t)i)) key[i] = sfmcloud::cell_key(g, xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
  const bool brute = search == 1 || (search == 0 && n <= 2048);
  std::vector<int> start, sorted;  // the grid walk's cells: start[c] .. start[c + 1] into `sorted`, ascending input index
  if (!brute) {
    start.assign((size_t)g.ncell + 1, 0);
    for (int i = 0; i < n; ++i)
      if (key[i] >= 0) ++start[(size_t)key[i] + 1];
    for (long long c = 0; c < g.ncell; ++c) start[(size_t)c + 1] += start[(size_t)c];
    sorted.resize((size_t)n_valid);
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int i = 0; i < n; ++i)
      if (key[i] >= 0) sorted[(size_t)at[(size_t)key[i]]++] = i;
  }
  std::vector<int32_t> support((size_t)nv), nearest((size_t)nv);
  std::vector<float> nd2((size_t)nv);
  std::vector<uint32_t> colour((size_t)nv, 0u);
  std::vector<char> sup((size_t)nv);
  parallel(nv, threads, [&](int v) {
    const float* p = verts + 3 * (size_t)v;
    const bool fin = finite_pt(p);
    sfmmesh::Support s;
    sfmmesh::support_zero(s);
    auto add = [&](int j) {
      sfmmesh::support_add(s, p[0], p[1], p[2], xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2], j, rgb ? rgb[j] : 0u, rgb != nullptr,
                           r2, r2d);
    };
    if (fin && brute) {
      std::vector<std::pair<int, int>> hit;
      for (int j = 0; j < n; ++j)
        if (key[j] >= 0 && sfmcloud::in_radius(sfmcloud::dist2(p[0], p[1], p[2], xyz[3 * (size_t)j], xyz[3 * (size_t)j + 1], xyz[3 * (size_t)j + 2]), r2))
          hit.emplace_back(key[j], j);
      std::sort(hit.begin(), hit.end());
      for (const auto& h : hit) add(h.second);
    } else if (fin) {
      const int c[3] = {sfmcloud::cell_of(p[0], g.o[0], g.cell, g.D[0]), sfmcloud::cell_of(p[1], g.o[1], g.cell, g.D[1]),
                        sfmcloud::cell_of(p[2], g.o[2], g.cell, g.D[2])};
      for (int z = std::max(c[2] - 1, 0); z <= std::min(c[2] + 1, g.D[2] - 1); ++z)
        for (int y = std::max(c[1] - 1, 0); y <= std::min(c[1] + 1, g.D[1] - 1); ++y)
          for (int x = std::max(c[0] - 1, 0); x <= std::min(c[0] + 1, g.D[0] - 1); ++x) {
            const size_t cell = ((size_t)z * g.D[1] + y) * g.D[0] + x;
            for (int k = start[cell]; k < start[cell + 1]; ++k) add(sorted[(size_t)k]);
          }
    }
    support[v] = s.count;
    nearest[v] = sfmmesh::nearest_of(s);
    nd2[v] = s.best_d2;
    if (rgb) colour[v] = sfmmesh::colour_of(s);
    sup[v] = sfmmesh::vertex_supported(fin, s.count, min_support) ? 1 : 0;
  });
  for (int v = 0; v < nv; ++v) m->counts[4] += !sup[v];
  // M3 + M4
  std::vector<char> tkeep((size_t)nt);
  std::vector<int> parent((size_t)nv), size((size_t)nv, 0), least((size_t)nv);
  for (int v = 0; v < nv; ++v) parent[v] = v;
  for (int t = 0; t < nt; ++t) {
    const int a = tris[3 * (size_t)t], b = tris[3 * (size_t)t + 1], c = tris[3 * (size_t)t + 2];
    tkeep[t] = sfmmesh::triangle_distinct(a, b, c) && sup[a] && sup[b] && sup[c];
    m->counts[5] += !tkeep[t];
    if (!tkeep[t]) continue;
    parent[find(parent, a)] = find(parent, b);
    parent[find(parent, b)] = find(parent, c);
  }
  for (int v = 0; v < nv; ++v) least[v] = nv;
  for (int v = 0; v < nv; ++v) least[find(parent, v)] = std::min(least[find(parent, v)], v);  // a component's id: its least vertex
  for (int t = 0; t < nt; ++t)
    if (tkeep[t]) ++size[(size_t)least[find(parent, tris[3 * (size_t)t])]];
  std::vector<std::pair<int, int>> comps;  // (-size, id)
  for (int v = 0; v < nv; ++v)
    if (size[v] > 0) comps.emplace_back(-size[v], v);
  m->counts[6] = (int32_t)comps.size();
  int cut_size = -1, cut_id = 0;
  if (keep_largest > 0 && (int)comps.size() > keep_largest) {
    std::sort(comps.begin(), comps.end());
    cut_size = -comps[(size_t)keep_largest - 1].first;
    cut_id = comps[(size_t)keep_largest - 1].second;
  }
  std::vector<char> ckeep((size_t)nv, 0);
  for (int v = 0; v < nv; ++v) {
    ckeep[v] = sfmmesh::component_kept(size[v], v, min_component, cut_size, cut_id);
    m->counts[7] += ckeep[v];
  }
  // M5
  std::vector<int> vnew((size_t)nv, -1);
  std::vector<char> used((size_t)nv, 0);
  for (int t = 0; t < nt; ++t) {
    if (tkeep[t] && !ckeep[(size_t)least[find(parent, tris[3 * (size_t)t])]]) tkeep[t] = 0;
    if (tkeep[t])
      for (int k = 0; k < 3; ++k) used[(size_t)tris[3 * (size_t)t + k]] = 1;
  }
  for (int v = 0; v < nv; ++v) {
    if (!used[v]) continue;
    vnew[v] = (int)m->vsrc.size();
    m->vsrc.push_back(v);
    for (int a = 0; a < 3; ++a) m->verts.push_back(verts[3 * (size_t)v + a]);
    m->support.push_back(support[v]);
    m->nearest.push_back(nearest[v]);
    m->nd2.push_back(nd2[v]);
    if (rgb) m->rgb.push_back(colour[v]);
  }
  for (int t = 0; t < nt; ++t) {
    if (!tkeep[t]) continue;
    m->tsrc.push_back(t);
    for (int k = 0; k < 3; ++k) m->tris.push_back(vnew[(size_t)tris[3 * (size_t)t + k]]);
  }
  const int mv = (int)m->vsrc.size(), mt = (int)m->tsrc.size();
  m->counts[2] = mv;
  m->counts[3] = mt;
  // M6: the sums grow in triangle order, which is every vertex's ascending order
  std::vector<double> acc((size_t)3 * mv, 0.0);
  for (int t = 0; t < mt; ++t) {
    const int32_t* q = m->tris.data() + 3 * (size_t)t;
    double x[3];
    sfmmesh::triangle_cross(m->verts.data() + 3 * (size_t)q[0], m->verts.data() + 3 * (size_t)q[1], m->verts.data() + 3 * (size_t)q[2], x);
    for (int k = 0; k < 3; ++k)
      for (int a = 0; a < 3; ++a) acc[3 * (size_t)q[k] + a] = acc[3 * (size_t)q[k] + a] + x[a];
  }
  m->normals.resize((size_t)3 * mv);
  for (int v = 0; v < mv; ++v) sfmmesh::normal_write(acc.data() + 3 * (size_t)v, m->normals.data() + 3 * (size_t)v);
  // M7
  for (int b = 0; b < mt; b += sfmsum::CHUNK) {
    double va[sfmsum::CHUNK], vv[sfmsum::CHUNK];
    for (int k = 0; k < sfmsum::CHUNK; ++k) {
      va[k] = vv[k] = 0.0;
      if (b + k >= mt) continue;
      const int32_t* q = m->tris.data() + 3 * (size_t)(b + k);
      const float *pa = m->verts.data() + 3 * (size_t)q[0], *pb = m->verts.data() + 3 * (size_t)q[1], *pc = m->verts.data() + 3 * (size_t)q[2];
      va[k] = sfmmesh::triangle_area(pa, pb, pc);
      vv[k] = sfmmesh::triangle_volume(pa, pb, pc);
    }
    m->area = m->area + sfmsum::chunk_tree(va);
    m->volume = m->volume + sfmsum::chunk_tree(vv);
  }
  return OK;
}

// counts8: the summary's integers; sums2: area, volume
void msh_counts(const void* h, int32_t* counts8, double* sums2) {
  const Mesh* m = (const Mesh*)h;
  for (int k = 0; k < 8; ++k) counts8[k] = m->counts[k];
  sums2[0] = m->area;
  sums2[1] = m->volume;
}

void msh_get(const void* h, float* verts, int32_t* tris, float* normals, uint32_t* rgb, int32_t* support, int32_t* nearest, float* nd2,
             int32_t* vsrc, int32_t* tsrc) {
  const Mesh* m = (const Mesh*)h;
  auto put = [](void* dst, const void* src, size_t bytes) {
    if (dst && bytes) memcpy(dst, src, bytes);
  };
  put(verts, m->verts.data(), m->verts.size() * 4);
  put(tris, m->tris.data(), m->tris.size() * 4);
  put(normals, m->normals.data(), m->normals.size() * 4);
  put(rgb, m->rgb.data(), m->rgb.size() * 4);
  put(support, m->support.data(), m->support.size() * 4);
  put(nearest, m->nearest.data(), m->nearest.size() * 4);
  put(nd2, m->nd2.data(), m->nd2.size() * 4);
  put(vsrc, m->vsrc.data(), m->vsrc.size() * 4);
  put(tsrc, m->tsrc.data(), m->tsrc.size() * 4);
}

void msh_free(void* h) { delete (Mesh*)h; }

// block_sum.h's fixed-order sum of n values: consecutive blocks of 256, the partials in ascending order (M7)
double msh_sum(const double* x, int n) {
  double s = 0.0;
  for (int b = 0; b < n; b += sfmsum::CHUNK) {
    double v[sfmsum::CHUNK];
    for (int k = 0; k < sfmsum::CHUNK; ++k) v[k] = b + k < n ? x[b + k] : 0.0;
    s = s + sfmsum::chunk_tree(v);
  }
  return s;
}

}  // extern "C"

#ifdef MESH_MAIN
// Meshes made here: a lat-long sphere of 4 608 triangles against a cloud on its lower part (with NaN and infinite rows in the
// cloud and among the vertices, a repeated-index triangle, colours) by both searches and at 1 and 16 threads, a blob beside it
// under the component filters, the tiny meshes and clouds, a vertex far away, the refusals.  Prints a digest of each.
namespace {
uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }
float unit(uint32_t& s) { return (float)(lcg(s) >> 8) / 16777216.0f; }

void sphere(float cx, float R, int rings, int seg, std::vector<float>& v, std::vector<int32_t>& t) {
  const int base = (int)(v.size() / 3);
  for (int i = 0; i <= rings; ++i)
    for (int j = 0; j < seg; ++j) {
      const double th = 3.141592653589793 * i / rings, ph = 2 * 3.141592653589793 * j / seg;
      v.insert(v.end(), {cx + R * (float)(std::sin(th) * std::cos(ph)), R * (float)(std::sin(th) * std::sin(ph)), R * (float)std::cos(th)});
    }
  for (int i = 0; i < rings; ++i)
    for (int j = 0; j < seg; ++j) {
      const int a = base + i * seg + j, b = base + i * seg + (j + 1) % seg, c = a + seg, d = b + seg;
      t.insert(t.end(), {a, c, b, b, c, d});
    }
}

int run(const char* name, const std::vector<float>& xyz, const std::vector<uint32_t>& rgb, const std::vector<float>& v, const std::vector<int32_t>& t,
        double r, int min_support, int min_component, int keep, int search, int threads) {
  void* h = nullptr;
  const int rc = msh_finish((int)(xyz.size() / 3), xyz.data(), rgb.empty() ? nullptr : rgb.data(), (int)(v.size() / 3), v.data(), (int)(t.size() / 3),
                            t.data(), r, min_support, min_component, keep, search, threads, &h);
  if (rc != OK) {
    std::printf("%s: rc %d\n", name, rc);
    return rc;
  }
  int32_t c[8];
  double s[2];
  msh_counts(h, c, s);
  std::vector<float> ov((size_t)3 * c[2] + 3), on((size_t)3 * c[2] + 3), od((size_t)c[2] + 1);
  std::vector<int32_t> ot((size_t)3 * c[3] + 3), os((size_t)c[2] + 1), oi((size_t)c[2] + 1), vs((size_t)c[2] + 1), ts((size_t)c[3] + 1);
  std::vector<uint32_t> oc((size_t)c[2] + 1);
  msh_get(h, ov.data(), ot.data(), on.data(), oc.data(), os.data(), oi.data(), od.data(), vs.data(), ts.data());
  msh_free(h);
  unsigned long long digest = 0;
  for (int i = 0; i < c[2]; ++i) digest += (unsigned long long)os[i] * 31u + oc[i] + (unsigned)oi[i];
  std::printf("%s: search %d threads %d in %d %d out %d %d unsupported %d trimmed %d components %d kept %d area %.9g volume %.9g digest %llu\n", name,
              search, threads, c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], s[0], s[1], digest);
  return OK;
}
}  // namespace

int main() {
  uint32_t seed = 5;
  std::vector<float> xyz, v;
  std::vector<uint32_t> rgb;
  std::vector<int32_t> t;
  for (int i = 0; i < 6000; ++i) {  // the unit sphere below z = 0.4
    float p[3];
    double l;
    do {
      for (float& x : p) x = 2.0f * unit(seed) - 1.0f;
      l = std::sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
    } while (l < 0.1 || l > 1.0 || p[2] / l > 0.4);
    xyz.insert(xyz.end(), {(float)(p[0] / l), (float)(p[1] / l), (float)(p[2] / l)});
    rgb.push_back(lcg(seed) & 0xFFFFFFu);
  }
  for (int i = 0; i < 6000; i += 97) xyz[3 * i + (i % 3)] = NAN;
  for (int i = 5; i < 6000; i += 211) xyz[3 * i + 1] = (i & 1) ? INFINITY : -INFINITY;
  sphere(0.0f, 1.0f, 48, 48, v, t);
  v[3 * 700] = NAN;
  v[3 * 900 + 2] = INFINITY;
  t.insert(t.end(), {100, 100, 101});
  for (int search = 1; search <= 2; ++search)
    for (int threads : {1, 16})
      if (run("sphere", xyz, rgb, v, t, 0.12, 1, 0, 0, search, threads) != OK) return 1;
  if (run("no colours", xyz, {}, v, t, 0.12, 3, 0, 0, 0, 16) != OK || run("no trim", xyz, rgb, v, t, 0.12, 0, 0, 0, 0, 16) != OK) return 1;
  std::vector<float> xyz2 = xyz, v2 = v;
  std::vector<uint32_t> rgb2 = rgb;
  std::vector<int32_t> t2 = t;
  for (int i = 0; i < 400; ++i) {  // a blob at x = 1.6
    float p[3];
    double l;
    do {
      for (float& x : p) x = 2.0f * unit(seed) - 1.0f;
      l = std::sqrt((double)p[0] * p[0] + (double)p[1] * p[1] + (double)p[2] * p[2]);
    } while (l < 0.1 || l > 1.0);
    xyz2.insert(xyz2.end(), {1.6f + 0.15f * (float)(p[0] / l), 0.15f * (float)(p[1] / l), 0.15f * (float)(p[2] / l)});
    rgb2.push_back(0xFF0000u);
  }
  sphere(1.6f, 0.15f, 8, 8, v2, t2);
  if (run("blob", xyz2, rgb2, v2, t2, 0.12, 1, 0, 0, 0, 16) != OK || run("blob largest", xyz2, rgb2, v2, t2, 0.12, 1, 0, 1, 0, 16) != OK ||
      run("blob min", xyz2, rgb2, v2, t2, 0.12, 1, 129, 0, 0, 16) != OK || run("blob many", xyz2, rgb2, v2, t2, 0.12, 1, 0, 9, 0, 16) != OK)
    return 1;
  const std::vector<float> tet = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1};
  const std::vector<int32_t> tt = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3};
  std::vector<float> far = tet;
  far.insert(far.end(), {1e6f, 1e6f, -1e6f});
  std::vector<int32_t> tf = tt;
  tf.insert(tf.end(), {0, 1, 4});
  if (run("tetrahedron", tet, {}, tet, tt, 0.5, 1, 0, 0, 0, 1) != OK || run("far vertex", tet, {}, far, tf, 0.5, 1, 0, 0, 2, 1) != OK ||
      run("empty cloud", {}, {}, tet, tt, 0.5, 0, 0, 0, 0, 1) != OK || run("empty mesh", tet, {}, {}, {}, 0.5, 1, 0, 0, 0, 1) != OK ||
      run("no triangle", tet, {}, tet, {}, 0.5, 1, 0, 0, 0, 1) != OK || run("one point", {0, 0, 0}, {0x102030u}, tet, tt, 2.0, 1, 0, 0, 0, 1) != OK)
    return 1;
  const std::vector<int32_t> bad = {0, 1, 4};
  void* h = nullptr;
  std::printf("refusals %d %d %d %d %d %d\n", msh_finish(4, tet.data(), nullptr, 4, tet.data(), 1, bad.data(), 0.5, 1, 0, 0, 0, 1, &h),
              msh_finish(4, tet.data(), nullptr, 4, tet.data(), 4, tt.data(), 0.0, 1, 0, 0, 0, 1, &h),
              msh_finish(4, tet.data(), nullptr, 4, tet.data(), 4, tt.data(), NAN, 1, 0, 0, 0, 1, &h),
              msh_finish(4, tet.data(), nullptr, 4, tet.data(), 4, tt.data(), 0.5, -1, 0, 0, 0, 1, &h),
              msh_finish(4, tet.data(), nullptr, 4, tet.data(), 4, tt.data(), 0.5, 1, -1, 0, 0, 1, &h),
              msh_finish(4, tet.data(), nullptr, 4, tet.data(), 4, tt.data(), 0.5, 1, 0, -1, 0, 1, &h));
  std::printf("done\n");
  return 0;
}
#endif
