// tracks_capi.cpp -- a C surface over csrc/tracks.h for tests/test_tracks_cpu.py and tests/test_gpu_tracks.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off): the whole build and the triangulation in the header's plain loops, and, with
// -DTRACKS_MAIN, a driver that runs graphs and scenes of its own making under the sanitizers.
#include <cstdio>
#include <cstring>
#include "../../sfm_danpipeline_amd/csrc/tracks.h"

using namespace sfmtracks;

extern "C" {

void trk_default_opts(Opts* o) { *o = default_opts(); }
int trk_sizes(int* opts, int* stats) {
  *opts = (int)sizeof(Opts);
  *stats = (int)sizeof(Stats);
  return 0;
}

// 0: done; 1: refused, nothing written.  trk_ptr: room for nodes / 2 + 1 entries; trk_view, trk_feat, node_track: for nodes
int trk_build(int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs, const int32_t* counts, const int32_t* q, const int32_t* t,
              const Opts* o, Stats* st, int32_t* trk_ptr, int32_t* trk_view, int32_t* trk_feat, int32_t* node_track) {
  std::vector<int32_t> p, v, f, nt;
  Stats s;
  if (!build_host(n_images, n_feat, n_pairs, pairs, counts, q, t, *o, s, p, v, f, nt)) return 1;
  *st = s;
  if (trk_ptr) std::memcpy(trk_ptr, p.data(), sizeof(int32_t) * p.size());
  if (trk_view && !v.empty()) std::memcpy(trk_view, v.data(), sizeof(int32_t) * v.size());
  if (trk_feat && !f.empty()) std::memcpy(trk_feat, f.data(), sizeof(int32_t) * f.size());
  if (node_track && !nt.empty()) std::memcpy(node_track, nt.data(), sizeof(int32_t) * nt.size());
  return 0;
}

void trk_triangulate(int n_tracks, const int32_t* trk_ptr, const int32_t* trk_view, const int32_t* trk_feat, const double* views,
                     const uint8_t* has_pose, const double* K, const double* dist, const int32_t* xy_ptr, const double* xy, float max_err,
                     int min_views, int front_only, double* X, float* err, int32_t* n_used, uint8_t* keep) {
  triangulate_host(n_tracks, trk_ptr, trk_view, trk_feat, views, has_pose, K, dist, xy_ptr, xy, max_err, min_views, front_only, X, err, n_used,
                   keep);
}
}

#ifdef TRACKS_MAIN
// a match graph from world ids with false matches and an image without features, through three min_len values; empty inputs
// and the refusals; then a ring scene triangulated under pose masks, a NaN pixel, distortion and the cheirality option
static uint32_t rng_state = 4321u;
static uint32_t rnd32() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}
static double rnd() { return (double)rnd32() / 16777216.0; }

int main() {
  const int NI = 12, NW = 400;
  std::vector<int32_t> n_feat(NI), pairs, counts, q, t;
  // world point w is seen in an image with 0.6, under a feature of its own drawn at random; every 9th match is false
  std::vector<std::vector<int32_t>> feat_of(NI, std::vector<int32_t>(NW, -1));
  for (int i = 0; i < NI; ++i) {
    n_feat[i] = i == 5 ? 0 : 300 + 10 * i;
    std::vector<int32_t> used((size_t)n_feat[i], 0);
    for (int w = 0; w < NW && n_feat[i]; ++w) {
      if (rnd() < 0.4) continue;
      const int f = (int)(rnd32() % (uint32_t)n_feat[i]);
      if (used[f]) continue;
      used[f] = 1;
      feat_of[i][w] = f;
    }
  }
  for (int a = 0; a < NI; ++a)
    for (int b = a + 1; b < NI; ++b) {
      int c = 0;
      for (int w = 0; w < NW; ++w) {
        if (feat_of[a][w] < 0 || feat_of[b][w] < 0 || rnd() < 0.3) continue;
        int tb = feat_of[b][w];
        if (rnd32() % 9 == 0) tb = (int)(rnd32() % (uint32_t)n_feat[b]);
        q.push_back(feat_of[a][w]);
        t.push_back(tb);
        ++c;
      }
      pairs.push_back(a), pairs.push_back(b), counts.push_back(c);
    }
  const int np = (int)counts.size();
  Stats st;
  std::vector<int32_t> ptr, view, feat, nt;
  for (int min_len = 0; min_len <= 4; min_len += 2) {
    if (!build_host(NI, n_feat.data(), np, pairs.data(), counts.data(), q.data(), t.data(), Opts{min_len, 0}, st, ptr, view, feat, nt)) return 1;
    std::printf("min_len %d: nodes %lld edges %lld components %lld conflicting %lld short %lld tracks %lld obs %lld\n", min_len, (long long)st.nodes,
                (long long)st.edges, (long long)st.components, (long long)st.conflicting, (long long)st.short_tracks, (long long)st.n_tracks,
                (long long)st.n_obs);
    if (st.components != st.conflicting + st.short_tracks + st.n_tracks || (int64_t)ptr.size() != st.n_tracks + 1 || ptr.back() != st.n_obs) return 2;
    for (int64_t k = 0; k < st.n_tracks; ++k)
      for (int j = ptr[k] + 1; j < ptr[k + 1]; ++j)
        if (view[j] <= view[j - 1]) return 3;
  }
  // empty inputs and the refusals
  if (!build_host(0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, default_opts(), st, ptr, view, feat, nt) || st.n_tracks != 0) return 4;
  if (!build_host(NI, n_feat.data(), 0, nullptr, nullptr, nullptr, nullptr, default_opts(), st, ptr, view, feat, nt) || st.n_tracks != 0) return 4;
  {
    const int32_t two[2] = {3, 3}, pr[2] = {0, 1}, c1[1] = {1};
    int32_t qq[1] = {3}, tt[1] = {0};
    if (build_host(2, two, 1, pr, c1, qq, tt, default_opts(), st, ptr, view, feat, nt)) return 5;  // q == n_feat
    qq[0] = -1;
    if (build_host(2, two, 1, pr, c1, qq, tt, default_opts(), st, ptr, view, feat, nt)) return 5;
    qq[0] = 0;
    const int32_t self[2] = {1, 1}, far[2] = {0, 2};
    if (build_host(2, two, 1, self, c1, qq, tt, default_opts(), st, ptr, view, feat, nt)) return 5;
    if (build_host(2, two, 1, far, c1, qq, tt, default_opts(), st, ptr, view, feat, nt)) return 5;
    if (!build_host(2, two, 1, pr, c1, qq, tt, default_opts(), st, ptr, view, feat, nt) || st.n_tracks != 1) return 5;
  }
  std::printf("graphs done\n");

  // a ring of views around the origin looking inwards, the tracks of the first build above, pixels by projection + noise
  if (!build_host(NI, n_feat.data(), np, pairs.data(), counts.data(), q.data(), t.data(), default_opts(), st, ptr, view, feat, nt)) return 1;
  const double K[9] = {1520, 0, 960, 0, 1520, 540, 0, 0, 1}, PI = 3.14159265358979323846;
  std::vector<double> poses(12 * (size_t)NI), world(3 * (size_t)NW);
  for (int w = 0; w < NW; ++w)
    for (int a = 0; a < 3; ++a) world[3 * w + a] = 2 * rnd() - 1;
  for (int i = 0; i < NI; ++i) {
    const double a = 2 * PI * i / NI, c = std::cos(a), s = std::sin(a);
    const double R[9] = {c, 0, -s, 0, 1, 0, s, 0, c}, C[3] = {-10 * s, 0, -10 * c};  // camera at C looking at the origin
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) poses[12 * i + 4 * r + k] = R[3 * r + k];
      poses[12 * i + 4 * r + 3] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
    }
  }
  std::vector<int32_t> xy_ptr(NI + 1, 0);
  for (int i = 0; i < NI; ++i) xy_ptr[i + 1] = xy_ptr[i] + n_feat[i];
  std::vector<double> xy(2 * (size_t)xy_ptr[NI], 100.0);
  for (int variant = 0; variant < 5; ++variant) {
    double dist[5] = {0, 0, 0, 0, 0};
    if (variant == 1) dist[0] = -0.1, dist[1] = 0.02, dist[2] = 1e-3, dist[3] = -1e-3, dist[4] = 1e-3;
    for (int i = 0; i < NI; ++i)
      for (int w = 0; w < NW; ++w)
        if (feat_of[i][w] >= 0) {
          double u, v;
          sfmcam::project_point(poses.data() + 12 * i, K, dist, world.data() + 3 * w, u, v);
          xy[2 * ((size_t)xy_ptr[i] + feat_of[i][w])] = u + (rnd() - 0.5);
          xy[2 * ((size_t)xy_ptr[i] + feat_of[i][w]) + 1] = v + (rnd() - 0.5);
        }
    if (variant == 2) xy[2 * (size_t)xy_ptr[1]] = NAN;
    std::vector<uint8_t> has(NI, 1), keep((size_t)st.n_tracks);
    if (variant == 3)
      for (int i = 0; i < NI; i += 2) has[i] = 0;
    if (variant == 4) std::fill(has.begin() + 1, has.end(), 0);
    std::vector<double> X(3 * (size_t)st.n_tracks);
    std::vector<float> err((size_t)st.n_obs);
    std::vector<int32_t> used((size_t)st.n_tracks);
    triangulate_host((int)st.n_tracks, ptr.data(), view.data(), feat.data(), poses.data(), has.data(), K, dist, xy_ptr.data(), xy.data(), 6.0f,
                     variant == 3 ? 3 : 2, variant == 0, X.data(), err.data(), used.data(), keep.data());
    long long kept = 0, unused = 0;
    for (uint8_t k : keep) kept += k;
    for (float e : err) unused += e == -1.0f;
    std::printf("variant %d: kept %lld unused %lld\n", variant, kept, unused);
    if (variant == 4 && (kept != 0 || unused != st.n_obs)) return 6;
  }
  std::printf("done\n");
  return 0;
}
#endif
