// align.h -- the rules of the coarse plot alignment (two levelled clouds vote for a scale, a yaw and a
// horizontal shift by the heights of their points above the ground; ICP from every candidate picks the winner) as code that
// hipcc and a plain g++ both compile with -ffp-contract=off.  The device code (align.hip) and the CPU test stub
// (tests/stub/align_capi.cpp) share these bodies, so the device result is checked byte for byte against a CPU build.  Every
// count is an integer, every real expression is f64 in one written order, minima and maxima are exact: no result depends on
// the order in which points, pairs or hypotheses are visited.  The host part below the shared part holds what runs once per
// call on the host in the library AND in the stub (the tables, the window, the candidates, the winner) and the whole call in
// plain loops (vote_host, align_host).
#pragma once
#include <cstdint>
#include <cstring>
#include "cloud.h"
#include "register.h"

#ifdef __HIPCC__
#define SFM_ALN_INLINE __host__ __device__ __forceinline__
#else
#define SFM_ALN_INLINE inline __attribute__((always_inline))
#endif

namespace sfmalign {

using sfmreg::fin;
using sfmreg::Transform;

// the C ABI's structs (include/sfmhip.h), field for field
struct Frame {  // the fields of the ground plane's result that level a cloud
  double up[3], north[3], offset;
};
struct Opts {
  double scale_lo, scale_hi, clear_rel, h_tol, window_rel, icp_dist_bins;
  int32_t n_scale, n_yaw, bins, src_samples, tgt_samples, n_cand, icp_max_iters, reserved;
};
struct Candidate {
  Transform T;
  int32_t votes, k, m, bin;
};
struct Stats {
  double hmax_src, hmax_tgt, w, window;
  int32_t n_above_src, n_above_tgt, n_src, n_tgt, n_hyp, flags;
};
struct Result {
  sfmreg::Result reg;
  Candidate cand;
  int32_t cand_index, n_same, n_cand, flags;
  Stats stats;
};
enum { F_EMPTY = 1, F_NO_WINNER = 2 };
constexpr int MAX_SCALES = 64, MAX_YAWS = 720, MIN_BINS = 4, MAX_BINS = 128, MAX_SAMPLES = 8192, MAX_CAND = 1024;

struct Basis {  // rule V2's frame: the rows of E, and the ground's height along up
  double east[3], north[3], up[3], offset;
};
struct Samp {  // a sample point: (e, n) as float32 and d = (f64)h - offset
  float e, n;
  double d;
};
struct Peak {  // rule V8 for one hypothesis (votes 0: none)
  int32_t votes, bin;
  double te, tn;
};
struct Window {  // rule V6's part that all hypotheses share
  double mid_e, mid_n, W, w;
};

inline Opts default_opts() {
  Opts o;
  o.scale_lo = o.scale_hi = 0.0;  // required
  o.clear_rel = 0.1;
  o.h_tol = 0.0;  // required
  o.window_rel = 1.0;
  o.icp_dist_bins = 1.25;
  o.n_scale = 15, o.n_yaw = 72, o.bins = 64, o.src_samples = 2048, o.tgt_samples = 2048, o.n_cand = 64, o.icp_max_iters = 30, o.reserved = 0;
  return o;
}
// rule V1's table
inline bool valid_opts(const Opts& o) {
  const bool reals = fin(o.scale_lo) && o.scale_lo > 0.0 && fin(o.scale_hi) && o.scale_hi >= o.scale_lo && o.clear_rel >= 0.0 && o.clear_rel < 1.0 &&
                     fin(o.h_tol) && o.h_tol > 0.0 && fin(o.window_rel) && o.window_rel > 0.0 && fin(o.icp_dist_bins) && o.icp_dist_bins > 0.0;
  return reals && o.n_scale >= 1 && o.n_scale <= MAX_SCALES && o.n_yaw >= 1 && o.n_yaw <= MAX_YAWS && o.bins >= MIN_BINS && o.bins <= MAX_BINS &&
         o.src_samples >= 1 && o.src_samples <= MAX_SAMPLES && o.tgt_samples >= 1 && o.tgt_samples <= MAX_SAMPLES && o.n_cand >= 1 &&
         o.n_cand <= MAX_CAND && o.icp_max_iters >= 0;
}
// rule V1's frames: f-11 rule 1 (|up| within 1e-6 of 1, north not parallel to up; north is projected off up and normalised,
// east = north x up), and a finite offset
inline bool make_basis(const Frame& f, Basis& b) {
  const double uu = (f.up[0] * f.up[0] + f.up[1] * f.up[1]) + f.up[2] * f.up[2];
  if (!(fabs(uu - 1.0) <= 2e-6) || !fin(f.offset)) return false;
  const double d = (f.north[0] * f.up[0] + f.north[1] * f.up[1]) + f.north[2] * f.up[2];
  double n[3];
  for (int a = 0; a < 3; ++a) n[a] = f.north[a] - d * f.up[a];
  const double nn = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
  if (!(nn > 1e-9) || !fin(nn)) return false;
  for (int a = 0; a < 3; ++a) b.up[a] = f.up[a], b.north[a] = n[a] / nn;
  b.east[0] = b.north[1] * b.up[2] - b.north[2] * b.up[1];
  b.east[1] = b.north[2] * b.up[0] - b.north[0] * b.up[2];
  b.east[2] = b.north[0] * b.up[1] - b.north[1] * b.up[0];
  b.offset = f.offset;
  return true;
}

// rule V2: (e, n, h) of a point as float32 (f-11 rules 2 and 3); a point that is not finite before or after: NaN, false
SFM_ALN_INLINE bool frame_point(const Basis& b, const float* p, float out[3]) {
  bool ok = sfmcloud::finite3(p[0], p[1], p[2]);
  if (ok) {
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    out[0] = (float)((b.east[0] * x + b.east[1] * y) + b.east[2] * z);
    out[1] = (float)((b.north[0] * x + b.north[1] * y) + b.north[2] * z);
    out[2] = (float)((b.up[0] * x + b.up[1] * y) + b.up[2] * z);
    ok = sfmcloud::finite3(out[0], out[1], out[2]);
  }
  if (!ok) out[0] = out[1] = out[2] = sfmcloud::qnan();
  return ok;
}
SFM_ALN_INLINE double height(float h, double offset) { return (double)h - offset; }
SFM_ALN_INLINE double clearance(double clear_rel, double hmax) { return clear_rel * hmax; }
SFM_ALN_INLINE bool is_above(double d, double clear) { return d >= clear; }
// rule V3: the above points at positions 0, stride, 2 stride, ... of their list
SFM_ALN_INLINE int stride_of(int n_above, int K) { return (n_above + K - 1) / K; }
SFM_ALN_INLINE int samples_of(int n_above, int stride) { return (n_above + stride - 1) / stride; }

// rule V5
SFM_ALN_INLINE void moved(double s, double c, double sn, const Samp& p, double& qe, double& qn, double& hq) {
  const double e = (double)p.e, n = (double)p.n;
  qe = s * (c * e - sn * n);
  qn = s * (sn * e + c * n);
  hq = s * p.d;
}
// exact minimum / maximum (of numbers: no NaN reaches them from finite floats and a finite scale)
SFM_ALN_INLINE double lower(double a, double b) { return b < a ? b : a; }
SFM_ALN_INLINE double upper(double a, double b) { return b > a ? b : a; }
SFM_ALN_INLINE double midpoint(double lo, double hi) { return 0.5 * (lo + hi); }
// rule V6: lo of one axis from the target's midpoint and the moved source's box
SFM_ALN_INLINE double window_lo(double mid_t, double qmin, double qmax, double W) { return (mid_t - midpoint(qmin, qmax)) - W; }
// rule V7
SFM_ALN_INLINE bool height_votes(double dj, double hq, double h_tol) { return fabs(dj - hq) <= h_tol; }
SFM_ALN_INLINE int bin_of(double xt, double q, double lo, double w, int B) {
  const double f = floor(((xt - q) - lo) / w);
  return (f >= 0.0 && f < (double)B) ? (int)f : -1;
}
// rule V8: the largest count, the lowest bin id on a tie, as one key's maximum (0: no vote)
SFM_ALN_INLINE uint64_t peak_key(uint32_t count, uint32_t bin) { return count ? ((uint64_t)count << 32) | (uint64_t)(0xFFFFFFFFu - bin) : 0ull; }
SFM_ALN_INLINE double bin_centre(double lo, int b, double w) { return lo + ((double)b + 0.5) * w; }
SFM_ALN_INLINE Peak peak_of(uint64_t key, double lo_e, double lo_n, double w, int B) {
  Peak p;
  p.votes = (int32_t)(key >> 32);
  p.bin = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
  p.te = key ? bin_centre(lo_e, p.bin % B, w) : 0.0;
  p.tn = key ? bin_centre(lo_n, p.bin / B, w) : 0.0;
  return p;
}

}  // namespace sfmalign

// ---- the host part: what the library and the stub both run once per call
#include <algorithm>
#include <cmath>
#include <vector>

namespace sfmalign {

inline Frame frame_from(const double up[3], const double north[3], double offset) {
  Frame f;
  for (int a = 0; a < 3; ++a) f.up[a] = up[a], f.north[a] = north[a];
  f.offset = offset;
  return f;
}

// rule V4: the tables, by the host's pow, cos and sin (the device never evaluates them)
struct Tables {
  std::vector<double> scale, cosv, sinv;
};
inline Tables tables(const Opts& o) {
  Tables t;
  const double PI = 3.14159265358979323846;
  for (int k = 0; k < o.n_scale; ++k)
    t.scale.push_back(k == 0 ? o.scale_lo : o.scale_lo * std::pow(o.scale_hi / o.scale_lo, (double)k / (double)(o.n_scale - 1)));
  for (int m = 0; m < o.n_yaw; ++m) {
    const double a = 2.0 * PI * (double)m / (double)o.n_yaw;
    t.cosv.push_back(std::cos(a)), t.sinv.push_back(std::sin(a));
  }
  return t;
}

// rule V6's shared part from the target sample (n >= 1)
inline Window window_of(const Samp* tgt, int n, double window_rel, int B) {
  double lo_e = tgt[0].e, hi_e = tgt[0].e, lo_n = tgt[0].n, hi_n = tgt[0].n;
  for (int j = 1; j < n; ++j) {
    lo_e = lower(lo_e, (double)tgt[j].e), hi_e = upper(hi_e, (double)tgt[j].e);
    lo_n = lower(lo_n, (double)tgt[j].n), hi_n = upper(hi_n, (double)tgt[j].n);
  }
  Window win;
  win.mid_e = midpoint(lo_e, hi_e), win.mid_n = midpoint(lo_n, hi_n);
  win.W = window_rel * upper(hi_e - lo_e, hi_n - lo_n);
  win.w = 2.0 * win.W / (double)B;
  return win;
}

// rule V9's transform of hypothesis (s, cos, sin) with the translation (te, tn): R = E_t^T (Rz E_s), the inner product first;
// every entry (a0 b0 + a1 b1) + a2 b2
inline Transform candidate_transform(const Basis& bt, const Basis& bs, double s, double c, double sn, double te, double tn) {
  const double* Es[3] = {bs.east, bs.north, bs.up};
  const double* Et[3] = {bt.east, bt.north, bt.up};
  const double Rz[9] = {c, -sn, 0.0, sn, c, 0.0, 0.0, 0.0, 1.0};
  double M[9];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) M[3 * r + q] = (Rz[3 * r] * Es[0][q] + Rz[3 * r + 1] * Es[1][q]) + Rz[3 * r + 2] * Es[2][q];
  Transform T;
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) T.R[3 * r + q] = (Et[0][r] * M[q] + Et[1][r] * M[3 + q]) + Et[2][r] * M[6 + q];
  const double v[3] = {te, tn, bt.offset - s * bs.offset};
  for (int r = 0; r < 3; ++r) T.t[r] = (Et[0][r] * v[0] + Et[1][r] * v[1]) + Et[2][r] * v[2];
  T.scale = s;
  return T;
}

// rule V9: the hypotheses with votes by (votes descending, k ascending, m ascending), the first n_cand; *n_hyp: how many had votes
inline std::vector<Candidate> candidates(const Opts& o, const Tables& t, const Peak* peaks, const Basis& bt, const Basis& bs, int* n_hyp) {
  std::vector<int> order;
  for (int h = 0; h < o.n_scale * o.n_yaw; ++h)
    if (peaks[h].votes > 0) order.push_back(h);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return peaks[a].votes > peaks[b].votes; });  // (h = k n_yaw + m ascends)
  if (n_hyp) *n_hyp = (int)order.size();
  if ((int)order.size() > o.n_cand) order.resize(o.n_cand);
  std::vector<Candidate> out;
  for (int h : order) {
    Candidate c;
    c.k = h / o.n_yaw, c.m = h % o.n_yaw, c.votes = peaks[h].votes, c.bin = peaks[h].bin;
    c.T = candidate_transform(bt, bs, t.scale[c.k], t.cosv[c.m], t.sinv[c.m], peaks[h].te, peaks[h].tn);
    out.push_back(c);
  }
  return out;
}

// entry 3's ICP options and its winner: flags == 0, then (pairs descending, mse ascending, index ascending); -1: none.
// *n_same: the results whose transform has the winner's bytes
inline sfmreg::Opts icp_opts(const Opts& o, double w) {
  sfmreg::Opts r = sfmreg::default_opts();
  r.with_scale = o.n_scale > 1 ? 1 : 0;
  r.max_iters = o.icp_max_iters;
  r.max_dist = o.icp_dist_bins * w;
  return r;
}
inline int pick_winner(const sfmreg::Result* res, int n, int* n_same) {
  int best = -1;
  for (int i = 0; i < n; ++i) {
    if (res[i].flags != 0) continue;
    if (best < 0 || res[i].pairs > res[best].pairs || (res[i].pairs == res[best].pairs && res[i].mse < res[best].mse)) best = i;
  }
  int same = 0;
  for (int i = 0; best >= 0 && i < n; ++i) same += memcmp(&res[i].T, &res[best].T, sizeof(Transform)) == 0;
  if (n_same) *n_same = same;
  return best;
}
inline void empty_stats(Stats& st) {
  memset(&st, 0, sizeof st);
  st.hmax_src = st.hmax_tgt = st.w = st.window = sfmreg::qnan_d();
}
inline void finish_result(Result& out, const Stats& st, const std::vector<Candidate>& cands, const sfmreg::Result* res) {
  memset(&out, 0, sizeof out);
  out.stats = st;
  out.n_cand = (int32_t)cands.size();
  const int win = pick_winner(res, (int)cands.size(), &out.n_same);
  out.cand_index = win;
  out.flags = st.flags | (win < 0 ? F_NO_WINNER : 0);
  if (win >= 0) {
    out.reg = res[win], out.cand = cands[win];
  } else {
    out.reg.T = out.cand.T = sfmreg::identity();
    out.reg.mse = sfmreg::qnan_d();
    out.cand.k = out.cand.m = out.cand.bin = -1;
  }
}

}  // namespace sfmalign

#ifndef __HIPCC__
// ---- the whole call on the host: what the device is checked against
#include <thread>

namespace sfmalign {

// rules V2 + V3 for one cloud on the host
struct Side {
  std::vector<Samp> samp;
  std::vector<int32_t> index;  // the input index of every sample
  double hmax = 0;
  int n_above = 0;
  bool any = false;   // a finite point
  bool empty = true;  // no above point, or hmax <= 0
};
inline void sample_host(int n, const float* xyz, const Basis& b, double clear_rel, int K, Side& s) {
  std::vector<float> fr((size_t)3 * std::max(n, 1));
  s = Side();
  for (int i = 0; i < n; ++i)
    if (frame_point(b, xyz + 3 * (size_t)i, &fr[3 * (size_t)i])) {
      const double d = height(fr[3 * (size_t)i + 2], b.offset);
      s.hmax = s.any ? upper(s.hmax, d) : d;
      s.any = true;
    }
  if (!s.any || !(s.hmax > 0.0)) return;
  const double clear = clearance(clear_rel, s.hmax);
  std::vector<int32_t> above;
  for (int i = 0; i < n; ++i)
    if (fr[3 * (size_t)i] == fr[3 * (size_t)i] && is_above(height(fr[3 * (size_t)i + 2], b.offset), clear)) above.push_back(i);
  s.n_above = (int)above.size();
  if (s.n_above == 0) return;
  s.empty = false;
  const int stride = stride_of(s.n_above, K);
  for (int r = 0; r < s.n_above; r += stride) {
    const int i = above[r];
    Samp p;
    p.e = fr[3 * (size_t)i], p.n = fr[3 * (size_t)i + 1], p.d = height(fr[3 * (size_t)i + 2], b.offset);
    s.samp.push_back(p), s.index.push_back(i);
  }
}

// rules V5 - V8 for every hypothesis in plain loops.  The target sample is walked in the order of its heights so that a
// source point meets only the run that passes rule V7 (the run's ends by the rule's own comparison, which is monotone in
// d_j): the integer votes do not depend on the order
inline void peaks_host(const Opts& o, const Tables& t, const Window& win, const std::vector<Samp>& src, const std::vector<Samp>& tgt,
                       std::vector<Peak>& peaks, int threads) {
  const int H = o.n_scale * o.n_yaw, B = o.bins;
  peaks.assign((size_t)H, Peak());
  std::vector<Samp> byh(tgt);
  std::stable_sort(byh.begin(), byh.end(), [](const Samp& a, const Samp& b) { return a.d < b.d; });
  auto work = [&](int t0) {
    std::vector<int32_t> hist((size_t)B * B);
    for (int h = t0; h < H; h += threads) {
      const double s = t.scale[h / o.n_yaw], c = t.cosv[h % o.n_yaw], sn = t.sinv[h % o.n_yaw];
      double qe, qn, hq, e0 = 0, e1 = 0, n0 = 0, n1 = 0;
      for (size_t i = 0; i < src.size(); ++i) {
        moved(s, c, sn, src[i], qe, qn, hq);
        e0 = i ? lower(e0, qe) : qe, e1 = i ? upper(e1, qe) : qe, n0 = i ? lower(n0, qn) : qn, n1 = i ? upper(n1, qn) : qn;
      }
      const double lo_e = window_lo(win.mid_e, e0, e1, win.W), lo_n = window_lo(win.mid_n, n0, n1, win.W);
      std::fill(hist.begin(), hist.end(), 0);
      for (size_t i = 0; i < src.size(); ++i) {
        moved(s, c, sn, src[i], qe, qn, hq);
        const auto a = std::partition_point(byh.begin(), byh.end(), [&](const Samp& p) { return p.d - hq < -o.h_tol; });
        for (auto p = a; p != byh.end() && !(p->d - hq > o.h_tol); ++p) {
          if (!height_votes(p->d, hq, o.h_tol)) continue;  // (a NaN difference)
          const int bx = bin_of((double)p->e, qe, lo_e, win.w, B), by = bin_of((double)p->n, qn, lo_n, win.w, B);
          if (bx >= 0 && by >= 0) ++hist[(size_t)by * B + bx];
        }
      }
      uint64_t key = 0;
      for (int b = 0; b < B * B; ++b) key = std::max(key, peak_key((uint32_t)hist[b], (uint32_t)b));
      peaks[h] = peak_of(key, lo_e, lo_n, win.w, B);
    }
  };
  std::vector<std::thread> pool;
  for (int t0 = 1; t0 < threads; ++t0) pool.emplace_back(work, t0);
  work(0);
  for (auto& th : pool) th.join();
}

// entry 2 on the host.  false: rule V1 refuses.  src_side (nullable): the source's sample, for entry 3
inline bool vote_host(int n_tgt, const float* tgt, int n_src, const float* src, const Frame& ft, const Frame& fs, const Opts& o,
                      std::vector<Candidate>& cands, Stats& st, Side* src_side = nullptr, int threads = 1) {
  Basis bt, bs;
  if (!valid_opts(o) || !make_basis(ft, bt) || !make_basis(fs, bs)) return false;
  cands.clear();
  empty_stats(st);
  Side T, S;
  sample_host(n_tgt, tgt, bt, o.clear_rel, o.tgt_samples, T);
  sample_host(n_src, src, bs, o.clear_rel, o.src_samples, S);
  st.n_above_tgt = T.n_above, st.n_above_src = S.n_above;
  st.n_tgt = (int32_t)T.samp.size(), st.n_src = (int32_t)S.samp.size();
  if (T.any) st.hmax_tgt = T.hmax;
  if (S.any) st.hmax_src = S.hmax;
  if (T.empty || S.empty) {
    st.flags = F_EMPTY;
    if (src_side) *src_side = Side();
    return true;
  }
  const Tables tab = tables(o);
  const Window win = window_of(T.samp.data(), (int)T.samp.size(), o.window_rel, o.bins);
  st.w = win.w, st.window = win.W;
  std::vector<Peak> peaks;
  peaks_host(o, tab, win, S.samp, T.samp, peaks, std::max(threads, 1));
  int n_hyp = 0;
  cands = candidates(o, tab, peaks.data(), bt, bs, &n_hyp);
  st.n_hyp = n_hyp;
  if (src_side) *src_side = std::move(S);
  return true;
}

// entry 3 on the host
inline bool align_host(int n_tgt, const float* tgt, int n_src, const float* src, const Frame& ft, const Frame& fs, const Opts& o, Result& out,
                       int threads = 1) {
  std::vector<Candidate> cands;
  Stats st;
  Side S;
  if (!vote_host(n_tgt, tgt, n_src, src, ft, fs, o, cands, st, &S, threads)) return false;
  std::vector<sfmreg::Result> res(cands.size());
  if (!cands.empty()) {
    std::vector<float> sel;
    for (int32_t i : S.index)
      for (int a = 0; a < 3; ++a) sel.push_back(src[3 * (size_t)i + a]);
    std::vector<Transform> inits;
    for (const Candidate& c : cands) inits.push_back(c.T);
    if (!sfmreg::run_host_batch(n_tgt, tgt, (int)S.index.size(), sel.data(), icp_opts(o, st.w), inits.data(), (int)inits.size(), res.data(), nullptr))
      return false;
  }
  finish_result(out, st, cands, res.data());
  return true;
}

}  // namespace sfmalign
#endif
