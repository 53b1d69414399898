// verify_capi.cpp -- a C surface over csrc/verify.h for tests/test_verify_cpu.py and tests/test_gpu_verify.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off): the refusals (V6), the kept pairs and the stable compaction (V4, V5) from a mask
// the caller brings or from each pair's E by the header's gather, normalisation and inlier test (V1, V3), and, with
// -DVERIFY_MAIN, a driver that runs lists of its own making under the sanitizers.
#include <cstdio>
#include <cstring>
#include "../../sfm_danpipeline_amd/csrc/verify.h"

using namespace sfmverify;

extern "C" {

void vfy_default_opts(Opts* o) { *o = default_opts(); }
int vfy_sizes(int* opts, int* stats) {
  *opts = (int)sizeof(Opts);
  *stats = (int)sizeof(Stats);
  return 0;
}

// 0: accepted; 1: refused (V6)
int vfy_check(int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs, const int32_t* counts, const int32_t* q, const int32_t* t,
              const int32_t* xy_ptr, const double* xy, const double* K, const Opts* o) {
  if (!args_ok(n_images, n_feat, xy_ptr, K, *o)) return 1;
  return lists_ok(n_images, n_feat, n_pairs, pairs, counts, q, t, xy) ? 0 : 1;
}

// V4 + V5 from a mask, one byte per input match (packed like the lists).  out_q / out_t: room for every input match.
void vfy_compact_mask(int n_pairs, const int32_t* counts, const int32_t* q, const int32_t* t, const uint8_t* mask, const uint8_t* has,
                      const int32_t* inliers, int min_inliers, int32_t* out_counts, int32_t* out_q, int32_t* out_t, uint8_t* kept, Stats* st) {
  std::vector<int64_t> off((size_t)n_pairs + 1, 0);
  for (int p = 0; p < n_pairs; ++p) off[(size_t)p + 1] = off[p] + counts[p];
  compact_host(n_pairs, counts, q, t, has, inliers, min_inliers, [&](int p, int i) { return mask[off[p] + i] != 0; }, out_counts, out_q, out_t,
               kept, *st);
}

// V1 + V3 + V4 + V5 from each pair's E (9 doubles, row-major)
void vfy_compact_E(int n_pairs, const int32_t* pairs, const int32_t* counts, const int32_t* q, const int32_t* t, const int32_t* xy_ptr,
                   const double* xy, const double* K, double threshold, const double* E, const uint8_t* has, const int32_t* inliers,
                   int min_inliers, int32_t* out_counts, int32_t* out_q, int32_t* out_t, uint8_t* kept, Stats* st) {
  verify_host(n_pairs, pairs, counts, q, t, xy_ptr, xy, K, threshold, E, has, inliers, min_inliers, out_counts, out_q, out_t, kept, *st);
}
}

#ifdef VERIFY_MAIN
// three images (the middle one without features, slack in xy_ptr), pairs of 0 / 5 / 300 matches under E = [t]x of a pure
// sideways translation (a match is an inlier when its two pixels share a row), every has code, min_inliers at and around the
// inlier count, then the refusals
static uint32_t rng_state = 99u;
static uint32_t rnd32() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 8;
}

int main() {
  const int NI = 3, NF = 320;
  const int32_t n_feat[NI] = {NF, 0, NF}, xy_ptr[NI + 1] = {4, 4 + NF + 3, 4 + NF + 3, 4 + 2 * NF + 10};
  const double K[9] = {1400, 0, 310, 0, 1650, 235, 0, 0, 1};
  std::vector<double> xy(2 * (size_t)xy_ptr[NI], -1.0);
  for (int f = 0; f < NF; ++f) {
    const double x = 20 + rnd32() % 600, y = 20 + rnd32() % 440;
    xy[2 * (xy_ptr[0] + f)] = x, xy[2 * (xy_ptr[0] + f) + 1] = y;
    xy[2 * (xy_ptr[2] + f)] = x - 30 - rnd32() % 40, xy[2 * (xy_ptr[2] + f) + 1] = f % 3 == 0 ? y + 25 : y;  // every third: off its row
  }
  const int NP = 4;
  const int32_t pairs[2 * NP] = {0, 2, 2, 0, 0, 2, 0, 2}, counts[NP] = {300, 5, 0, 300};
  std::vector<int32_t> q, t;
  for (int p = 0; p < NP; ++p)
    for (int i = 0; i < counts[p]; ++i) q.push_back((7 * i + p) % NF), t.push_back((7 * i + p) % NF);
  const double Ex[9] = {0, 0, 0, 0, 0, -1, 0, 1, 0};
  std::vector<double> E;
  for (int p = 0; p < NP; ++p) E.insert(E.end(), Ex, Ex + 9);
  Opts o = default_opts();
  if (vfy_check(NI, n_feat, NP, pairs, counts, q.data(), t.data(), xy_ptr, xy.data(), K, &o)) return 1;
  std::vector<int32_t> oc(NP), oq(q.size()), ot(q.size());
  std::vector<uint8_t> kept(NP);
  Stats st;
  const uint8_t has[NP] = {1, 2, 0, 1};
  int32_t inl[NP] = {0, 5, 0, 0};
  for (int i = 0; i < 300; ++i) inl[0] += ((7 * i) % NF) % 3 != 0, inl[3] += ((7 * i + 3) % NF) % 3 != 0;
  for (int min_inl : {0, 5, 6, inl[0], inl[0] + 1, 1000}) {
    vfy_compact_E(NP, pairs, counts, q.data(), t.data(), xy_ptr, xy.data(), K, 1.0, E.data(), has, inl, min_inl, oc.data(), oq.data(), ot.data(),
                  kept.data(), &st);
    std::printf("min_inliers %d: kept %lld no_model %lld in %lld out %lld counts %d %d %d %d\n", min_inl, (long long)st.pairs_kept,
                (long long)st.pairs_no_model, (long long)st.matches_in, (long long)st.matches_out, oc[0], oc[1], oc[2], oc[3]);
    for (int p = 0; p < NP; ++p)
      if (kept[p] && oc[p] != inl[p]) return 2;  // V5: a kept pair's count is its inlier count
    int64_t k = 0;
    for (int p = 0; p < NP; ++p)
      for (int i = 0; i < oc[p]; ++i, ++k)
        if (oq[k] != ot[k] || (has[p] == 1 && oq[k] % 3 == 0)) return 3;
  }
  // the same through a mask
  std::vector<uint8_t> mask(q.size());
  for (size_t i = 0; i < q.size(); ++i) mask[i] = q[i] % 3 != 0;
  for (int i = 0; i < 5; ++i) mask[300 + i] = 1;
  std::vector<int32_t> mc(NP), mq(q.size()), mt(q.size());
  vfy_compact_mask(NP, counts, q.data(), t.data(), mask.data(), has, inl, 15, mc.data(), mq.data(), mt.data(), kept.data(), &st);
  vfy_compact_E(NP, pairs, counts, q.data(), t.data(), xy_ptr, xy.data(), K, 1.0, E.data(), has, inl, 15, oc.data(), oq.data(), ot.data(), kept.data(),
                &st);
  if (mc != oc || std::memcmp(mq.data(), oq.data(), 4 * (size_t)st.matches_out) || std::memcmp(mt.data(), ot.data(), 4 * (size_t)st.matches_out)) return 4;
  std::printf("mask == E: out %lld\n", (long long)st.matches_out);
  // empty inputs and the refusals
  if (vfy_check(NI, n_feat, 0, nullptr, nullptr, nullptr, nullptr, xy_ptr, nullptr, K, &o)) return 5;
  vfy_compact_mask(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 15, nullptr, nullptr, nullptr, nullptr, &st);
  if (st.pairs != 0 || st.matches_out != 0) return 5;
  {
    const int32_t pr[2] = {0, 2}, self[2] = {2, 2}, far[2] = {0, 3}, c1[1] = {1}, bad_ptr[NI + 1] = {0, NF, NF - 1, 2 * NF}, tight[NI + 1] = {0, NF - 1, NF - 1, 2 * NF};
    int32_t qq[1] = {NF}, tt[1] = {0};
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, xy.data(), K, &o)) return 6;  // q == n_feat
    qq[0] = 0, tt[0] = -1;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, xy.data(), K, &o)) return 6;
    tt[0] = 0;
    if (!vfy_check(NI, n_feat, 1, self, c1, qq, tt, xy_ptr, xy.data(), K, &o)) return 6;
    if (!vfy_check(NI, n_feat, 1, far, c1, qq, tt, xy_ptr, xy.data(), K, &o)) return 6;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, bad_ptr, xy.data(), K, &o)) return 6;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, tight, xy.data(), K, &o)) return 6;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, nullptr, K, &o)) return 6;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, xy.data(), nullptr, &o)) return 6;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, nullptr, xy.data(), K, &o)) return 6;
    Opts bad = o;
    bad.prob = 1.0;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, xy.data(), K, &bad)) return 6;
    bad.prob = 0.0;
    if (!vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, xy.data(), K, &bad)) return 6;
    if (vfy_check(NI, n_feat, 1, pr, c1, qq, tt, xy_ptr, xy.data(), K, &o)) return 6;
  }
  std::printf("done\n");
  return 0;
}
#endif
