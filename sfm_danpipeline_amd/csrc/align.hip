// align.hip -- the coarse alignment of two levelled clouds: the pose vote and, around register.hip's batch,
// the whole alignment.  The rules are align.h's, which the CPU test stub compiles too.
//
// A side (one cloud under its frame): aln_frame writes (e, n, h) per point, the handle's minmax gives the largest h (hmax is
// monotone in it), aln_flag + the handle's scan list the above points in input order, aln_emit keeps every stride-th.  The
// two samples (at most 8 192 points each) come to the host once: the target's box gives the window, the source's indices feed
// sfmhip_cloud_select.
// aln_vote: a workgroup of 256 per hypothesis (k, m).  Pass 1 moves the source sample and reduces its box (exact minima and
// maxima: shuffles, then LDS); pass 2 streams the target sample through LDS in tiles of TILE points, every lane tests its
// source points against the tile (all lanes read the same LDS word: a broadcast) and a passing pair adds 1 to its bin of the
// B x B histogram in LDS with an integer atomic; a key reduction (count, lowest bin) gives the peak.  Dynamic LDS: 4 B B + 16
// TILE bytes, 68 KB at B = 128 (above the 64 KB a launch gets unasked, so the attribute is raised once).  No float atomics,
// no spins, no hand-offs between workgroups.
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include "align.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmgrid;
using namespace sfmalign;

namespace {

constexpr int VOTE_BLOCK = 256;
constexpr int TILE = 256;  // target sample points per LDS tile

struct AlnState {  // a side's scratch on its own handle; the vote's on the target handle
  static constexpr sfmgrid::Stage slot = sfmgrid::ALIGN;
  Grow<float> fr;
  Grow<Samp> samp;
  Grow<int> index;
  Grow<double> tab;
  Grow<Peak> peaks;
  double ms[3] = {0, 0, 0};  // vote, batch ICP, the whole call
};

struct HostSide {
  std::vector<Samp> samp;
  std::vector<int32_t> index;
  const Samp* d_samp = nullptr;
  double hmax = 0;
  int n_above = 0;
  bool any = false, empty = true;
};

struct VoteArgs {
  Window win;
  double h_tol;
  int B, n_yaw;
};

__global__ __launch_bounds__(256) void aln_frame(const float* xyz, int n, Basis b, float* fr) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float p[3] = {xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]};
  float out[3];
  frame_point(b, p, out);
  for (int a = 0; a < 3; ++a) fr[3 * (size_t)i + a] = out[a];
}

__global__ __launch_bounds__(256) void aln_flag(const float* fr, int n, double offset, double clear, int* flag) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float e = fr[3 * (size_t)i], h = fr[3 * (size_t)i + 2];
  flag[i] = (e == e && is_above(height(h, offset), clear)) ? 1 : 0;
}

// the above point at list position r stride becomes sample r (at[i] < n_above, so r < samples_of(n_above, stride))
__global__ __launch_bounds__(256) void aln_emit(const float* fr, int n, const int* flag, const int* at, int stride, double offset, Samp* samp,
                                                int* index) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !flag[i] || at[i] % stride != 0) return;
  const int r = at[i] / stride;
  Samp p;
  p.e = fr[3 * (size_t)i], p.n = fr[3 * (size_t)i + 1], p.d = height(fr[3 * (size_t)i + 2], offset);
  samp[r] = p;
  index[r] = i;
}

__global__ __launch_bounds__(VOTE_BLOCK) void aln_vote(const Samp* __restrict__ src, int ns, const Samp* __restrict__ tgt, int nt,
                                                       const double* __restrict__ scale, const double* __restrict__ cosv,
                                                       const double* __restrict__ sinv, VoteArgs a, Peak* peaks) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  Samp* tile = (Samp*)lds;                              // TILE
  unsigned* hist = (unsigned*)(lds + sizeof(Samp) * TILE);  // B x B
  __shared__ double box[4][4];
  __shared__ double lo_sh[2];
  __shared__ unsigned long long kred[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int hyp = blockIdx.x, k = hyp / a.n_yaw, m = hyp % a.n_yaw;
  const double s = scale[k], c = cosv[m], sn = sinv[m];
  for (int b = tid; b < a.B * a.B; b += VOTE_BLOCK) hist[b] = 0u;
  // pass 1: the moved sample's box (ns >= 1; a lane without a point starts from sample 0, which is in the box)
  double qe, qn, hq;
  moved(s, c, sn, src[0], qe, qn, hq);
  double e0 = qe, e1 = qe, n0 = qn, n1 = qn;
  for (int i = tid; i < ns; i += VOTE_BLOCK) {
    moved(s, c, sn, src[i], qe, qn, hq);
    e0 = lower(e0, qe), e1 = upper(e1, qe), n0 = lower(n0, qn), n1 = upper(n1, qn);
  }
  for (int off = 32; off >= 1; off >>= 1) {
    e0 = lower(e0, __shfl_xor(e0, off)), e1 = upper(e1, __shfl_xor(e1, off));
    n0 = lower(n0, __shfl_xor(n0, off)), n1 = upper(n1, __shfl_xor(n1, off));
  }
  if (lane == 0) box[wave][0] = e0, box[wave][1] = e1, box[wave][2] = n0, box[wave][3] = n1;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < VOTE_BLOCK / 64; ++w)
      e0 = lower(e0, box[w][0]), e1 = upper(e1, box[w][1]), n0 = lower(n0, box[w][2]), n1 = upper(n1, box[w][3]);
    lo_sh[0] = window_lo(a.win.mid_e, e0, e1, a.win.W);
    lo_sh[1] = window_lo(a.win.mid_n, n0, n1, a.win.W);
  }
  __syncthreads();
  const double lo_e = lo_sh[0], lo_n = lo_sh[1];
  // pass 2
  for (int j0 = 0; j0 < nt; j0 += TILE) {
    const int nj = min(TILE, nt - j0);
    for (int j = tid; j < nj; j += VOTE_BLOCK) tile[j] = tgt[j0 + j];
    __syncthreads();
    for (int i = tid; i < ns; i += VOTE_BLOCK) {
      moved(s, c, sn, src[i], qe, qn, hq);
      for (int j = 0; j < nj; ++j) {
        const Samp t = tile[j];
        if (!height_votes(t.d, hq, a.h_tol)) continue;
        const int bx = bin_of((double)t.e, qe, lo_e, a.win.w, a.B), by = bin_of((double)t.n, qn, lo_n, a.win.w, a.B);
        if (bx >= 0 && by >= 0) atomicAdd(&hist[by * a.B + bx], 1u);
      }
    }
    __syncthreads();
  }
  // the peak
  unsigned long long key = 0ull;
  for (int b = tid; b < a.B * a.B; b += VOTE_BLOCK) {
    const unsigned long long kb = peak_key(hist[b], (unsigned)b);
    key = kb > key ? kb : key;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off);
    key = o > key ? o : key;
  }
  if (lane == 0) kred[wave] = key;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < VOTE_BLOCK / 64; ++w) key = kred[w] > key ? kred[w] : key;
    peaks[hyp] = peak_of(key, lo_e, lo_n, a.win.w, a.B);
  }
}

// rules V2 + V3 for one cloud: the sample on the device (its handle's state) and on the host
int prepare_side(sfmhip_cloud* c, const Basis& b, double clear_rel, int K, HostSide& out) {
  out = HostSide();
  const int n = c->n;
  if (n <= 0) return SFMHIP_OK;
  hipStream_t st = c->ctx->stream;
  AlnState* s = stage<AlnState>(c);
  SFM_TRY(ensure_ibuf(c));
  SFM_TRY(s->fr.need((size_t)3 * n));
  hipLaunchKernelGGL(aln_frame, dim3(blocks(n, 256)), dim3(256), 0, st, c->xyz, n, b, s->fr.p);
  SFM_HIP_TRY(hipGetLastError());
  unsigned mm[7];
  SFM_TRY(minmax(c, s->fr.p, n, FinitePoint(), mm));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (mm[6] == 0) return SFMHIP_OK;
  out.any = true;
  out.hmax = height(sfmcloud::ord_val(mm[5]), b.offset);  // (the largest d is the largest h's: the subtraction is monotone)
  if (!(out.hmax > 0.0)) return SFMHIP_OK;
  int *flag = c->ibuf[2], *at = c->ibuf[3];
  hipLaunchKernelGGL(aln_flag, dim3(blocks(n, 256)), dim3(256), 0, st, s->fr.p, n, b.offset, clearance(clear_rel, out.hmax), flag);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(scan(c, flag, at, (size_t)n, &out.n_above));
  if (out.n_above <= 0) return SFMHIP_OK;
  const int stride = stride_of(out.n_above, K), ns = samples_of(out.n_above, stride);
  SFM_TRY(s->samp.need(ns));
  SFM_TRY(s->index.need(ns));
  hipLaunchKernelGGL(aln_emit, dim3(blocks(n, 256)), dim3(256), 0, st, s->fr.p, n, flag, at, stride, b.offset, s->samp.p, s->index.p);
  SFM_HIP_TRY(hipGetLastError());
  out.samp.resize(ns), out.index.resize(ns);
  SFM_HIP_TRY(hipMemcpyAsync(out.samp.data(), s->samp.p, sizeof(Samp) * (size_t)ns, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(out.index.data(), s->index.p, sizeof(int) * (size_t)ns, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  out.d_samp = s->samp.p;
  out.empty = false;
  return SFMHIP_OK;
}

// rules V1 - V9; src_index (nullable): the source sample's input indices
int vote(sfmhip_cloud* tgt, sfmhip_cloud* src, const sfmhip_frame* ft, const sfmhip_frame* fs, const sfmhip_align_opts* opts,
         std::vector<Candidate>& cands, Stats& st, std::vector<int32_t>* src_index) {
  if (!tgt || !src || !ft || !fs || !opts || tgt->ctx != src->ctx || tgt == src) return SFMHIP_ERR_ARG;  // (a side's sample lives on its handle)
  const Opts o = mirror<Opts>(*opts);
  Basis bt, bs;
  if (!valid_opts(o) || !make_basis(mirror<Frame>(*ft), bt) || !make_basis(mirror<Frame>(*fs), bs)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(tgt->ctx->device));
  hipStream_t stream = tgt->ctx->stream;
  AlnState* s = stage<AlnState>(tgt);
  const double t0 = sfm_now_ms();
  s->ms[0] = s->ms[1] = s->ms[2] = 0;
  cands.clear();
  empty_stats(st);
  HostSide T, S;
  SFM_TRY(prepare_side(tgt, bt, o.clear_rel, o.tgt_samples, T));
  SFM_TRY(prepare_side(src, bs, o.clear_rel, o.src_samples, S));
  st.n_above_tgt = T.n_above, st.n_above_src = S.n_above;
  st.n_tgt = (int32_t)T.samp.size(), st.n_src = (int32_t)S.samp.size();
  if (T.any) st.hmax_tgt = T.hmax;
  if (S.any) st.hmax_src = S.hmax;
  if (src_index) src_index->clear();
  if (T.empty || S.empty) {
    st.flags = F_EMPTY;
    s->ms[0] = s->ms[2] = sfm_now_ms() - t0;
    return SFMHIP_OK;
  }
  const Tables tab = tables(o);
  const Window win = window_of(T.samp.data(), (int)T.samp.size(), o.window_rel, o.bins);
  st.w = win.w, st.window = win.W;
  const int H = o.n_scale * o.n_yaw;
  SFM_TRY(s->tab.need((size_t)o.n_scale + 2 * (size_t)o.n_yaw));
  SFM_TRY(s->peaks.need(H));
  double* d_scale = s->tab.p;
  double *d_cos = d_scale + o.n_scale, *d_sin = d_cos + o.n_yaw;
  SFM_HIP_TRY(hipMemcpyAsync(d_scale, tab.scale.data(), sizeof(double) * o.n_scale, hipMemcpyHostToDevice, stream));
  SFM_HIP_TRY(hipMemcpyAsync(d_cos, tab.cosv.data(), sizeof(double) * o.n_yaw, hipMemcpyHostToDevice, stream));
  SFM_HIP_TRY(hipMemcpyAsync(d_sin, tab.sinv.data(), sizeof(double) * o.n_yaw, hipMemcpyHostToDevice, stream));
  const size_t lds_max = sizeof(unsigned) * MAX_BINS * MAX_BINS + sizeof(Samp) * TILE;
  SFM_HIP_TRY(hipFuncSetAttribute((const void*)aln_vote, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_max));
  VoteArgs a;
  a.win = win, a.h_tol = o.h_tol, a.B = o.bins, a.n_yaw = o.n_yaw;
  const size_t lds = sizeof(unsigned) * o.bins * o.bins + sizeof(Samp) * TILE;
  hipLaunchKernelGGL(aln_vote, dim3(H), dim3(VOTE_BLOCK), lds, stream, S.d_samp, (int)S.samp.size(), T.d_samp, (int)T.samp.size(), d_scale, d_cos,
                     d_sin, a, s->peaks.p);
  SFM_HIP_TRY(hipGetLastError());
  std::vector<Peak> peaks((size_t)H);
  SFM_HIP_TRY(hipMemcpyAsync(peaks.data(), s->peaks.p, sizeof(Peak) * (size_t)H, hipMemcpyDeviceToHost, stream));
  SFM_HIP_TRY(hipStreamSynchronize(stream));
  int n_hyp = 0;
  cands = candidates(o, tab, peaks.data(), bt, bs, &n_hyp);
  st.n_hyp = n_hyp;
  if (src_index) *src_index = std::move(S.index);
  s->ms[0] = s->ms[2] = sfm_now_ms() - t0;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_align_default_opts(sfmhip_align_opts* o) {
  if (o) *o = mirror<sfmhip_align_opts>(default_opts());
}

extern "C" int sfmhip_frame_from_ground(const sfmhip_ground_result* g, sfmhip_frame* out) {
  if (!g || !out) return SFMHIP_ERR_ARG;
  const Frame f = frame_from(g->up, g->north, g->offset);
  Basis b;
  if (!make_basis(f, b)) return SFMHIP_ERR_ARG;  // (a result without a plane holds NaN)
  *out = mirror<sfmhip_frame>(f);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_align_vote(sfmhip_cloud* tgt, sfmhip_cloud* src, const sfmhip_frame* ft, const sfmhip_frame* fs,
                                       const sfmhip_align_opts* opts, sfmhip_align_candidate* cands, int32_t* n_out, sfmhip_align_stats* stats) {
  if (!cands || !n_out || !stats) return SFMHIP_ERR_ARG;
  std::vector<Candidate> c;
  Stats st;
  SFM_TRY(vote(tgt, src, ft, fs, opts, c, st, nullptr));
  for (size_t i = 0; i < c.size(); ++i) cands[i] = mirror<sfmhip_align_candidate>(c[i]);
  *n_out = (int32_t)c.size();
  *stats = mirror<sfmhip_align_stats>(st);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_align(sfmhip_cloud* tgt, sfmhip_cloud* src, const sfmhip_frame* ft, const sfmhip_frame* fs, const sfmhip_align_opts* opts,
                                  sfmhip_align_result* out) {
  if (!out) return SFMHIP_ERR_ARG;
  std::vector<Candidate> c;
  std::vector<int32_t> index;
  Stats st;
  const double t0 = sfm_now_ms();
  SFM_TRY(vote(tgt, src, ft, fs, opts, c, st, &index));
  AlnState* s = stage<AlnState>(tgt);
  std::vector<sfmreg::Result> res(c.size());
  if (!c.empty()) {
    const double t1 = sfm_now_ms();
    sfmhip_cloud* sel = nullptr;
    SFM_TRY(sfmhip_cloud_select(src, index.data(), (int)index.size(), &sel));
    const sfmhip_register_opts ro = mirror<sfmhip_register_opts>(icp_opts(mirror<Opts>(*opts), st.w));
    std::vector<sfmhip_transform> inits;
    for (const Candidate& k : c) inits.push_back(mirror<sfmhip_transform>(k.T));
    static_assert(sizeof(sfmhip_register_result) == sizeof(sfmreg::Result), "the C ABI mirrors register.h");
    const int rc = sfmhip_cloud_register_batch(tgt, sel, &ro, inits.data(), (int)inits.size(), (sfmhip_register_result*)res.data(), nullptr);
    sfmhip_cloud_destroy(sel);
    SFM_TRY(rc);
    s->ms[1] = sfm_now_ms() - t1;
  }
  Result r;
  finish_result(r, st, c, res.data());
  *out = mirror<sfmhip_align_result>(r);
  s->ms[2] = sfm_now_ms() - t0;
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_align_last_timing(sfmhip_cloud* tgt, double ms3[3]) {
  if (!tgt || !ms3) return SFMHIP_ERR_ARG;
  const AlnState* s = stage<AlnState>(tgt);
  for (int i = 0; i < 3; ++i) ms3[i] = s->ms[i];
  return SFMHIP_OK;
}
