// mesh.h -- the arithmetic of the mesh finishing (sfmhip_cloud_mesh_finish; include/sfmhip.h rules M1-M7) as
// __host__ __device__ code that hipcc and a plain g++ both compile: a vertex's support among the cloud's points with its nearest
// point and its weighted colour sums, the trim, a triangle's cross product, area and signed volume, and a vertex normal's last
// step.  mesh.hip and the CPU test stub (tests/stub/mesh_capi.cpp) share these bodies, so the device result is checked bit for
// bit against a CPU build.  Compile with -ffp-contract=off.  Everything is + - * / sqrt in float or double: no libm or
// device-library routine enters a result.  What is summed in which order is the caller's business and is written at the rule.
#pragma once
#include "cloud.h"

namespace sfmmesh {

SFM_CLOUD_INLINE bool finite_d(double x) { return x - x == 0.0; }
SFM_CLOUD_INLINE float inf_f() { return sfmcloud::bits_f(0x7F800000u); }

// M2's radius as the colour weights see it: the float the distance test uses, widened
SFM_CLOUD_INLINE double radius2_d(double r) { return (double)sfmcloud::radius2(r); }

// ---- M2: what one vertex gathers from the cloud's points within the radius
struct Support {
  int count;              // points with d2 < r2
  float best_d2;          // the least (d2, index) by knn_less among them (+inf, INT_MAX with none)
  int best;
  double sw, sr, sg, sb;  // the weights and the weighted channels, in the order the points are passed
};
SFM_CLOUD_INLINE void support_zero(Support& s) {
  s.count = 0;
  s.best_d2 = inf_f();
  s.best = INT_MAX;
  s.sw = s.sr = s.sg = s.sb = 0.0;
}
// one finite cloud point q (input index j, colour rgb = 0x00RRGGBB, read only with `colour`) against the finite vertex v
SFM_CLOUD_INLINE void support_add(Support& s, float vx, float vy, float vz, float qx, float qy, float qz, int j, uint32_t rgb, bool colour,
                                  float r2, double r2d) {
  const float d2 = sfmcloud::dist2(vx, vy, vz, qx, qy, qz);
  if (!sfmcloud::in_radius(d2, r2)) return;
  ++s.count;
  if (sfmcloud::knn_less(d2, j, s.best_d2, s.best)) s.best_d2 = d2, s.best = j;
  if (colour) {
    const double t = 1.0 - (double)d2 / r2d;  // (d2 < r2 as floats: t > 0, so sw > 0 with one point)
    const double w = t * t;
    s.sw = s.sw + w;
    s.sr = s.sr + w * (double)((rgb >> 16) & 255u);
    s.sg = s.sg + w * (double)((rgb >> 8) & 255u);
    s.sb = s.sb + w * (double)(rgb & 255u);
  }
}
SFM_CLOUD_INLINE uint32_t channel(double s, double sw) {
  const double q = s / sw + 0.5;
  return q < 0.0 ? 0u : q >= 256.0 ? 255u : (uint32_t)(int)q;
}
SFM_CLOUD_INLINE uint32_t colour_of(const Support& s) {
  if (s.count == 0) return 0u;
  return (channel(s.sr, s.sw) << 16) | (channel(s.sg, s.sw) << 8) | channel(s.sb, s.sw);
}
SFM_CLOUD_INLINE int nearest_of(const Support& s) { return s.count ? s.best : -1; }

// ---- M1 + M3
SFM_CLOUD_INLINE bool vertex_supported(bool finite, int support, int min_support) { return finite && support >= min_support; }
SFM_CLOUD_INLINE bool triangle_distinct(int a, int b, int c) { return a != b && b != c && a != c; }

// ---- M4: does a component of `size` surviving triangles and id `id` stay?  (cut_size, cut_id): the last component keep_largest
// admits in the order (size descending, id ascending); cut_size < 0: no such limit
SFM_CLOUD_INLINE bool component_kept(int size, int id, int min_triangles, int cut_size, int cut_id) {
  if (size <= 0 || size < min_triangles) return false;
  if (cut_size < 0) return true;
  return size > cut_size || (size == cut_size && id <= cut_id);
}

// ---- M6 / M7: a triangle's cross(b - a, c - a), its area and its signed volume, of the widened floats
SFM_CLOUD_INLINE void triangle_cross(const float a[3], const float b[3], const float c[3], double o[3]) {
  const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
  const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
  o[0] = uy * vz - uz * vy;
  o[1] = uz * vx - ux * vz;
  o[2] = ux * vy - uy * vx;
}
SFM_CLOUD_INLINE double length3(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }
SFM_CLOUD_INLINE double triangle_area(const float a[3], const float b[3], const float c[3]) {
  double x[3];
  triangle_cross(a, b, c, x);
  return 0.5 * length3(x);
}
SFM_CLOUD_INLINE double triangle_volume(const float a[3], const float b[3], const float c[3]) {
  const double bx = (double)b[0], by = (double)b[1], bz = (double)b[2], cx = (double)c[0], cy = (double)c[1], cz = (double)c[2];
  const double x0 = by * cz - bz * cy, x1 = bz * cx - bx * cz, x2 = bx * cy - by * cx;
  return (((double)a[0] * x0 + (double)a[1] * x1) + (double)a[2] * x2) / 6.0;
}
// the sum s of a vertex's triangle crosses -> its normal (a zero or non-finite length: the canonical NaN three times)
SFM_CLOUD_INLINE void normal_write(const double s[3], float out[3]) {
  const double l = length3(s);
  if (!(l > 0.0) || !finite_d(l)) {
    out[0] = out[1] = out[2] = sfmcloud::qnan();
    return;
  }
  out[0] = (float)(s[0] / l);
  out[1] = (float)(s[1] / l);
  out[2] = (float)(s[2] / l);
}

}  // namespace sfmmesh
