// align_capi.cpp -- a C surface over csrc/align.h and csrc/register.h for tests/test_align_cpu.py and tests/test_gpu_align.py
// (built with g++ -O2 -std=c++17 -ffp-contract=off -pthread): the batch of ICP starts in the header's lock-step loop next to
// the single run, the vote and the whole alignment in the header's plain loops, and, with -DALIGN_MAIN, a driver that runs
// plots of its own making under the sanitizers.
#include <cstdio>
#include "../../sfm_danpipeline_amd/csrc/align.h"

using namespace sfmalign;
using sfmreg::Transform;

extern "C" {

void aln_default_opts(Opts* o) { *o = default_opts(); }
int aln_sizes(int* frame, int* opts, int* cand, int* stats, int* result) {
  *frame = (int)sizeof(Frame), *opts = (int)sizeof(Opts), *cand = (int)sizeof(Candidate), *stats = (int)sizeof(Stats), *result = (int)sizeof(Result);
  return 0;
}

// f-17 rule 6 from one start (0: done; 1: refused)
int aln_single(int n_tgt, const float* tgt, int n_src, const float* src, const sfmreg::Opts* o, const Transform* init, sfmreg::Result* res,
               int32_t* idx) {
  return sfmreg::run_host(n_tgt, tgt, n_src, src, o ? *o : sfmreg::default_opts(), init, *res, idx) ? 0 : 1;
}
// f-18 entry 1 (0: done; 1: refused, nothing written)
int aln_batch(int n_tgt, const float* tgt, int n_src, const float* src, const sfmreg::Opts* o, const Transform* inits, int n_init,
              sfmreg::Result* res, int32_t* idx, int* longest) {
  return sfmreg::run_host_batch(n_tgt, tgt, n_src, src, o ? *o : sfmreg::default_opts(), inits, n_init, res, idx, longest) ? 0 : 1;
}
// f-18 entry 2: cands has room for o->n_cand (0: done; 1: refused)
int aln_vote(int n_tgt, const float* tgt, int n_src, const float* src, const Frame* ft, const Frame* fs, const Opts* o, Candidate* cands,
             int32_t* n_out, Stats* st, int threads) {
  std::vector<Candidate> c;
  if (!vote_host(n_tgt, tgt, n_src, src, *ft, *fs, *o, c, *st, nullptr, threads)) return 1;
  for (size_t i = 0; i < c.size(); ++i) cands[i] = c[i];
  *n_out = (int32_t)c.size();
  return 0;
}
// f-18 entry 3 (0: done; 1: refused)
int aln_align(int n_tgt, const float* tgt, int n_src, const float* src, const Frame* ft, const Frame* fs, const Opts* o, Result* out, int threads) {
  return align_host(n_tgt, tgt, n_src, src, *ft, *fs, *o, *out, threads) ? 0 : 1;
}
}

#ifdef ALIGN_MAIN
// a plot of a ground disc and three "trees" (columns with a blob on top), its copy under a similarity with a yaw about the
// vertical, the whole and a part: the batch against single runs (starts that converge, hit the limit, end FEW and end
// DEGENERATE), the vote's edges, the whole alignment, the empty cases and the refusals
static uint32_t rng_state = 4321u;
static double rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return (double)(rng_state >> 8) / 16777216.0;
}
static Transform yaw_motion(double deg, double tx, double ty, double scale) {
  const double a = deg * 3.14159265358979323846 / 180.0;
  Transform T = sfmreg::identity();
  T.R[0] = std::cos(a), T.R[1] = -std::sin(a), T.R[3] = std::sin(a), T.R[4] = std::cos(a);
  T.t[0] = tx, T.t[1] = ty, T.scale = scale;
  return T;
}
int main() {
  std::vector<float> plot;
  const double cx[3] = {-4, 3, 1}, cy[3] = {-2, -3, 4.5}, top[3] = {6, 8, 5};
  for (int i = 0; i < 3000; ++i) {
    const double u = rnd(), v = rnd(), w = rnd();
    if (i % 3 == 0) {
      plot.push_back((float)(16 * u - 8)), plot.push_back((float)(16 * v - 8)), plot.push_back((float)(0.02 * w));
    } else {
      const int t = i % 3 + (i % 2), k = t % 3;
      const double r = w < 0.4 ? 0.15 : 1.5 * v, h = w < 0.4 ? top[k] * u : top[k] + 1.5 * (u - 0.5);
      plot.push_back((float)(cx[k] + r * std::cos(6.28 * v * 7))), plot.push_back((float)(cy[k] + r * std::sin(6.28 * v * 7))), plot.push_back((float)h);
    }
  }
  const int n_tgt = (int)plot.size() / 3;
  const Transform M = yaw_motion(137.0, 11.0, -7.0, 2.3);
  std::vector<float> src;
  for (int i = 0; i < n_tgt; i += 2) {
    double y[3];
    for (int a = 0; a < 3; ++a) y[a] = (plot[3 * i + a] - M.t[a]) / M.scale;
    for (int a = 0; a < 3; ++a) src.push_back((float)(M.R[a] * y[0] + M.R[3 + a] * y[1] + M.R[6 + a] * y[2]));
  }
  const int n_src = (int)src.size() / 3;
  // the batch against single runs
  {
    sfmreg::Opts o = sfmreg::default_opts();
    o.with_scale = 1, o.max_dist = 0.6, o.max_iters = 6;
    std::vector<Transform> inits = {M, yaw_motion(134.0, 10.8, -7.1, 2.25), yaw_motion(137.0, 300.0, -7.0, 2.3), yaw_motion(100.0, 11.0, -7.0, 2.3)};
    for (int B : {1, 2, 4}) {
      std::vector<sfmreg::Result> res(B);
      std::vector<int32_t> idx((size_t)B * n_src);
      int longest = -1;
      if (aln_batch(n_tgt, plot.data(), n_src, src.data(), &o, inits.data(), B, res.data(), idx.data(), &longest)) return 1;
      for (int b = 0; b < B; ++b) {
        sfmreg::Result one;
        std::vector<int32_t> i1(n_src);
        if (aln_single(n_tgt, plot.data(), n_src, src.data(), &o, &inits[b], &one, i1.data())) return 1;
        if (memcmp(&one, &res[b], sizeof one) || memcmp(i1.data(), &idx[(size_t)b * n_src], sizeof(int32_t) * n_src)) return 1;
        if (B == 4) std::printf("batch %d: iterations %d pairs %d converged %d flags %d\n", b, one.iterations, one.pairs, one.converged, one.flags);
      }
    }
    const float line[12] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3};
    sfmreg::Result two[2];
    const Transform id2[2] = {sfmreg::identity(), sfmreg::identity()};
    o = sfmreg::default_opts();
    if (aln_batch(4, line, 4, line, &o, id2, 2, two, nullptr, nullptr) || two[0].flags != sfmreg::F_DEGENERATE || two[1].flags != sfmreg::F_DEGENERATE) return 1;
    if (aln_batch(0, line, 0, line, &o, id2, 2, two, nullptr, nullptr) || two[1].flags != sfmreg::F_FEW) return 1;
    Transform bad[2] = {sfmreg::identity(), sfmreg::identity()};
    bad[1].scale = 0;
    if (!aln_batch(4, line, 4, line, &o, bad, 2, two, nullptr, nullptr) || !aln_batch(4, line, 4, line, &o, nullptr, 2, two, nullptr, nullptr) ||
        !aln_batch(4, line, 4, line, &o, id2, 0, two, nullptr, nullptr) || !aln_batch(4, line, 4, line, &o, id2, 1025, two, nullptr, nullptr))
      return 1;
  }
  // the vote and the whole alignment
  const double up[3] = {0, 0, 1}, north[3] = {0, 1, 0};
  const Frame ft = frame_from(up, north, 0.01), fs = frame_from(up, north, 0.01 / 2.3);
  Opts o = default_opts();
  o.scale_lo = 1.5, o.scale_hi = 3.5, o.h_tol = 0.3, o.n_scale = 5, o.n_yaw = 24, o.bins = 32, o.src_samples = 300, o.tgt_samples = 301, o.n_cand = 16;
  for (int threads : {1, 3}) {
    std::vector<Candidate> cands(o.n_cand);
    int32_t n = 0;
    Stats st;
    if (aln_vote(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &o, cands.data(), &n, &st, threads) || n < 1 || st.flags) return 2;
    std::printf("vote: %d candidates of %d, leader votes %d k %d m %d, samples %d x %d, w %.4f\n", n, st.n_hyp, cands[0].votes, cands[0].k, cands[0].m,
                st.n_src, st.n_tgt, st.w);
    Result out;
    if (aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &o, &out, threads)) return 2;
    std::printf("align: flags %d winner %d of %d (same %d) pairs %d scale %.5f\n", out.flags, out.cand_index, out.n_cand, out.n_same, out.reg.pairs,
                out.reg.T.scale);
    if (out.flags || std::fabs(out.reg.T.scale / 2.3 - 1) > 0.01) return 2;
  }
  for (int edge = 0; edge < 4; ++edge) {  // one scale, one yaw, the bin limits, one sample
    Opts e = o;
    if (edge == 0) e.n_scale = 1, e.scale_lo = e.scale_hi = 2.3;
    if (edge == 1) e.n_yaw = 1;
    if (edge == 2) e.bins = 4, e.window_rel = 0.3;
    if (edge == 3) e.bins = 128, e.src_samples = 1, e.tgt_samples = 1;
    Result out;
    if (aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &e, &out, 2)) return 3;
    std::printf("edge %d: flags %d candidates %d\n", edge, out.flags, out.n_cand);
  }
  {  // the empty cases: nothing above the ground, no point at all, every point NaN
    std::vector<float> flat(plot);
    for (int i = 0; i < n_tgt; ++i) flat[3 * i + 2] = -1.0f;
    const float nan3[3] = {NAN, 0, 0};
    Result out;
    if (aln_align(n_tgt, flat.data(), n_src, src.data(), &ft, &fs, &o, &out, 1) || out.flags != (F_EMPTY | F_NO_WINNER) || out.n_cand) return 4;
    if (aln_align(n_tgt, plot.data(), 0, src.data(), &ft, &fs, &o, &out, 1) || out.flags != (F_EMPTY | F_NO_WINNER)) return 4;
    if (aln_align(1, nan3, n_src, src.data(), &ft, &fs, &o, &out, 1) || out.flags != (F_EMPTY | F_NO_WINNER)) return 4;
    Opts far = o;  // candidates, but every ICP start without pairs
    far.icp_dist_bins = 1e-9;
    if (aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &far, &out, 1) || out.flags != F_NO_WINNER || out.n_cand < 1) return 4;
  }
  {  // the refusals
    Result out;
    Opts b = o;
    b.h_tol = 0;
    if (!aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &b, &out, 1)) return 5;
    b = o, b.scale_hi = 1.0;
    if (!aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &b, &out, 1)) return 5;
    b = o, b.bins = 129;
    if (!aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &fs, &b, &out, 1)) return 5;
    const double up2[3] = {0, 0, 1.1};
    const Frame bad = frame_from(up2, north, 0.0), par = frame_from(up, up, 0.0);
    if (!aln_align(n_tgt, plot.data(), n_src, src.data(), &bad, &fs, &o, &out, 1) || !aln_align(n_tgt, plot.data(), n_src, src.data(), &ft, &par, &o, &out, 1))
      return 5;
  }
  std::printf("done\n");
  return 0;
}
#endif
