// verify.hip -- two-view verification of match lists on gfx950 before the multi-view tracks.  The rules
// are verify.h's, which the CPU test stub compiles too; the RANSAC is score.hip's, entered after its upload
// (sfm_essential_ransac_points).
//
//   vfy_gather    V1 + V6: a workgroup per pair reads its list where it lies (a match plan's slots or packed host lists),
//                 checks the pair and every match (a flag, as tracks.hip's trk_check), and writes the two normalised points of
//                 each match into the packed p1 / p2 arrays the RANSAC kernels take; no pixel is stored per match;
//   the RANSAC    findEssentialMat's, per pair: the host reads the n_pairs counts once, forms the offsets, replays the chunks;
//   vfy_compact   V3 + V5: a workgroup per pair walks its list in blocks of 256 with a running base, evaluates is_inlier
//                 under the pair's best E and writes the survivors in order at p * stride of the handle's own lists; the
//                 place inside a block comes from wave ballots and popcounts;
//   vfy_pack      the handle's lists packed pair after pair for the download.
// No spin, no hand-off between workgroups, no atomic but the flag.  Launches are ordered by the stream alone.
#include "common.h"
#include "essential_dev.h"
#include "verify.h"
#include <algorithm>
#include <climits>
#include <vector>

using namespace sfmverify;

static_assert(sizeof(sfmhip_verify_opts) == sizeof(Opts), "sfmhip_verify_opts mirrors sfmverify::Opts");
static_assert(sizeof(sfmhip_verify_stats) == sizeof(Stats), "sfmhip_verify_stats mirrors sfmverify::Stats");

struct sfmhip_verified {
  sfmhip_ctx* ctx = nullptr;
  DevBufs B;
  int n_images = 0, n_pairs = 0, stride = 1;
  std::vector<int> n_feat;
  int *pairs = nullptr, *counts = nullptr, *q = nullptr, *t = nullptr;  // device: the layout of a match plan's lists
  std::vector<int32_t> h_counts, inliers, iterations;
  std::vector<double> E;
  std::vector<uint8_t> kept;
  Stats stats = {};
  double sec[4] = {0, 0, 0, 0};
};

int sfm_verified_device_lists(const sfmhip_verified* v, sfm_matchplan_lists* out) {
  if (!v || !out) return SFMHIP_ERR_ARG;
  out->ctx = v->ctx;
  out->n_images = v->n_images;
  out->n_rows = v->n_feat.data();
  out->n_pairs = v->n_pairs;
  out->pairs = v->pairs;
  out->counts = v->counts;
  out->q = v->q;
  out->t = v->t;
  out->stride = v->stride;
  return SFMHIP_OK;
}

namespace {

// workgroup per pair.  offs: the packed offsets the host formed from the counts (n_pairs + 1); stride > 0: the lists lie in
// slots of `stride` per pair.  A bad pair or match raises *bad and writes nothing for itself.
__global__ __launch_bounds__(256) void vfy_gather(const int* __restrict__ pairs, const int* __restrict__ offs, int stride, int n_images,
                                                  const int* __restrict__ n_feat, const int* __restrict__ q, const int* __restrict__ t,
                                                  const int* __restrict__ xy_ptr, const double* __restrict__ xy, Norm nm,
                                                  double* __restrict__ p1, double* __restrict__ p2, unsigned* bad) {
  const int p = blockIdx.x, a = pairs[2 * p], b = pairs[2 * p + 1];
  if (!pair_ok(a, b, n_images)) {
    if (threadIdx.x == 0) atomicOr(bad, 1u);
    return;
  }
  const int o = offs[p], c = offs[p + 1] - o, nfa = n_feat[a], nfb = n_feat[b];
  const long long src = list_start(offs, stride, p);
  bool any_bad = false;
  for (int k = threadIdx.x; k < c; k += blockDim.x) {
    const int qi = q[src + k], ti = t[src + k];
    if (!match_ok(qi, ti, nfa, nfb)) {
      any_bad = true;
      continue;
    }
    const size_t l = pixel_index(xy_ptr, a, qi), r = pixel_index(xy_ptr, b, ti), m = 2 * ((size_t)o + k);
    p1[m] = norm_x(nm, xy[l]);
    p1[m + 1] = norm_y(nm, xy[l + 1]);
    p2[m] = norm_x(nm, xy[r]);
    p2[m + 1] = norm_y(nm, xy[r + 1]);
  }
  if (any_bad) atomicOr(bad, 1u);
}

// workgroup per pair.  code: verify.h's pair_code (0: the pair keeps nothing).  out_counts[p] = the survivors.
__global__ __launch_bounds__(256) void vfy_compact(const int* __restrict__ offs, int stride_in, const int* __restrict__ q,
                                                   const int* __restrict__ t, const double* __restrict__ p1, const double* __restrict__ p2,
                                                   const double* __restrict__ best_E, const uint8_t* __restrict__ code, float bound,
                                                   int stride_out, int* __restrict__ out_q, int* __restrict__ out_t,
                                                   int* __restrict__ out_counts) {
  __shared__ double sE[9];
  __shared__ int s_wave[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int has = code[p];
  if (has == 0) {  // (the whole workgroup)
    if (tid == 0) out_counts[p] = 0;
    return;
  }
  if (tid < 9) sE[tid] = best_E[(size_t)p * 9 + tid];
  __syncthreads();
  const int o = offs[p], n = offs[p + 1] - o;
  const long long src = list_start(offs, stride_in, p), dst = (long long)p * stride_out;
  int base = 0;
  for (int b0 = 0; b0 < n; b0 += 256) {
    const int i = b0 + tid;
    bool in = false;
    if (i < n) {
      const size_t k = 2 * ((size_t)o + i);
      in = mask_of(has, has == 1 && is_inlier(sE, p1[k], p1[k + 1], p2[k], p2[k + 1], bound));
    }
    const unsigned long long bal = __ballot(in);
    if (lane == 0) s_wave[w] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
    for (int j = 0; j < 4; ++j) {
      const int s = s_wave[j];
      before += j < w ? s : 0;
      all += s;
    }
    if (in) {
      const int pos = base + before + __popcll(bal & ((1ull << lane) - 1ull));
      out_q[dst + pos] = q[src + i];
      out_t[dst + pos] = t[src + i];
    }
    base += all;
    __syncthreads();  // (s_wave is written again in the next block)
  }
  if (tid == 0) out_counts[p] = base;
}

__global__ __launch_bounds__(256) void vfy_pack(const int* __restrict__ out_offs, int stride, const int* __restrict__ q, const int* __restrict__ t,
                                                int* __restrict__ pq, int* __restrict__ pt) {
  const int p = blockIdx.x, o = out_offs[p], c = out_offs[p + 1] - o;
  const long long src = (long long)p * stride;
  for (int k = threadIdx.x; k < c; k += blockDim.x) {
    pq[o + k] = q[src + k];
    pt[o + k] = t[src + k];
  }
}

// everything after the lists are on the device.  h_counts: the host's copy of the counts, or null (a plan: read here, once).
// stride_in > 0: slots per pair; 0: packed lists.  The stage times are the host's clock between the call's three stream
// synchronisations (the flag, the RANSAC's end, the counts), so they need no timing switch.
int verify_device(sfmhip_ctx* ctx, int n_images, const int* n_feat, int n_pairs, const int* d_pairs, const int* d_counts,
                  const int32_t* h_counts, int stride_in, const int* d_q, const int* d_t, const int32_t* xy_ptr, const double* xy,
                  const double* K, const Opts& o, sfmhip_verified** out) {
  if (!args_ok(n_images, n_feat, xy_ptr, K, o)) return SFMHIP_ERR_ARG;
  hipStream_t st = ctx->stream;
  const double t0 = sfm_now_ms();
  ctx->score_flags = 0;
  std::vector<int32_t> counts((size_t)n_pairs), offs((size_t)n_pairs + 1, 0);
  if (n_pairs) {
    if (h_counts) std::copy(h_counts, h_counts + n_pairs, counts.begin());
    else {
      SFM_HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, sizeof(int) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
      SFM_HIP_TRY(hipStreamSynchronize(st));
    }
  }
  long long total = 0;
  int longest = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (counts[p] < 0 || (stride_in > 0 && counts[p] > stride_in)) return SFMHIP_ERR_ARG;
    total += counts[p];
    if (total > INT_MAX - 1) return SFMHIP_ERR_ARG;
    offs[(size_t)p + 1] = (int32_t)total;
    longest = std::max(longest, counts[p]);
  }
  if (total > 0 && !xy) return SFMHIP_ERR_ARG;
  const int stride_out = stride_in > 0 ? stride_in : std::max(longest, 1);
  const size_t n_xy = (size_t)xy_ptr[n_images];

  sfmhip_verified* h = new sfmhip_verified();
  struct Guard {  // a failing step below frees the handle
    sfmhip_verified* h;
    ~Guard() {
      if (h) sfmhip_verified_destroy(h);
    }
  } guard{h};
  h->ctx = ctx;
  h->n_images = n_images;
  h->n_pairs = n_pairs;
  h->stride = stride_out;
  h->n_feat.assign(n_feat, n_feat + n_images);
  h->h_counts.assign((size_t)n_pairs, 0);
  h->inliers.assign((size_t)n_pairs, 0);
  h->iterations.assign((size_t)n_pairs, 0);
  h->E.assign(9 * (size_t)n_pairs, 0.0);
  h->kept.assign((size_t)n_pairs, 0);
  h->stats = Stats{n_pairs, 0, 0, total, 0};
  SFM_TRY(h->B.alloc(&h->pairs, 2 * (size_t)n_pairs));
  SFM_TRY(h->B.alloc(&h->counts, (size_t)n_pairs));
  SFM_TRY(h->B.alloc(&h->q, (size_t)n_pairs * stride_out));
  SFM_TRY(h->B.alloc(&h->t, (size_t)n_pairs * stride_out));
  if (n_pairs == 0) {
    guard.h = nullptr;
    *out = h;
    return SFMHIP_OK;
  }
  SFM_HIP_TRY(hipMemcpyAsync(h->pairs, d_pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyDeviceToDevice, st));

  DevBufs T;  // this call's temporaries
  EssentialDev dev;
  int *d_offs = nullptr, *d_nf = nullptr, *d_xyp = nullptr;
  double* d_xy = nullptr;
  unsigned* d_bad = nullptr;
  uint8_t* d_code = nullptr;
  SFM_TRY(T.alloc(&d_offs, offs.size()));
  SFM_TRY(T.alloc(&d_nf, (size_t)n_images));
  SFM_TRY(T.alloc(&d_xyp, (size_t)n_images + 1));
  SFM_TRY(T.alloc(&d_xy, 2 * n_xy));
  SFM_TRY(T.alloc(&d_bad, 1));
  SFM_TRY(T.alloc(&d_code, (size_t)n_pairs));
  const size_t pts_n = 2 * (size_t)std::max<long long>(total, 1);
  SFM_TRY(dev.bufs.alloc(&dev.d_p1, pts_n));
  SFM_TRY(dev.bufs.alloc(&dev.d_p2, pts_n));
  SFM_HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), sizeof(int) * offs.size(), hipMemcpyHostToDevice, st));
  if (n_images) SFM_HIP_TRY(hipMemcpyAsync(d_nf, n_feat, sizeof(int) * (size_t)n_images, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_xyp, xy_ptr, sizeof(int) * ((size_t)n_images + 1), hipMemcpyHostToDevice, st));
  if (n_xy && xy) SFM_HIP_TRY(hipMemcpyAsync(d_xy, xy, sizeof(double) * 2 * n_xy, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(d_bad, 0, sizeof(unsigned), st));
  hipLaunchKernelGGL(vfy_gather, dim3(n_pairs), dim3(256), 0, st, d_pairs, (const int*)d_offs, stride_in, n_images, (const int*)d_nf, d_q, d_t,
                     (const int*)d_xyp, (const double*)d_xy, norm_of(K), dev.d_p1, dev.d_p2, d_bad);
  SFM_HIP_TRY(hipGetLastError());
  unsigned bad = 0;
  SFM_HIP_TRY(hipMemcpyAsync(&bad, d_bad, sizeof(unsigned), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  if (bad) return SFMHIP_ERR_ARG;
  const double t1 = sfm_now_ms();

  SFM_TRY(sfm_essential_ransac_points(ctx, n_pairs, offs.data(), K[0], K[4], o.prob, o.threshold, h->inliers.data(), h->iterations.data(),
                                      false, dev));
  const double t2 = sfm_now_ms();

  std::vector<uint8_t> code((size_t)n_pairs);
  for (int p = 0; p < n_pairs; ++p) {
    code[p] = pair_code(dev.has[p], h->inliers[p], o.min_inliers);
    h->kept[p] = code[p] ? 1 : 0;
    h->stats.pairs_kept += code[p] ? 1 : 0;
    h->stats.pairs_no_model += dev.has[p] == 0 ? 1 : 0;
  }
  SFM_HIP_TRY(hipMemcpyAsync(d_code, code.data(), (size_t)n_pairs, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(vfy_compact, dim3(n_pairs), dim3(256), 0, st, (const int*)d_offs, stride_in, d_q, d_t, (const double*)dev.d_p1,
                     (const double*)dev.d_p2, (const double*)dev.d_bestE, (const uint8_t*)d_code, error_bound(K[0], K[4], o.threshold),
                     stride_out, h->q, h->t, h->counts);
  SFM_HIP_TRY(hipGetLastError());
  SFM_HIP_TRY(hipMemcpyAsync(h->h_counts.data(), h->counts, sizeof(int) * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(h->E.data(), dev.d_bestE, sizeof(double) * 9 * (size_t)n_pairs, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  for (int p = 0; p < n_pairs; ++p) h->stats.matches_out += h->h_counts[p];
  const double t3 = sfm_now_ms();
  h->sec[0] = (t1 - t0) * 1e-3;
  h->sec[1] = (t2 - t1) * 1e-3;
  h->sec[2] = (t3 - t2) * 1e-3;
  h->sec[3] = (t3 - t0) * 1e-3;
  guard.h = nullptr;
  *out = h;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_verify_default_opts(sfmhip_verify_opts* o) {
  if (!o) return;
  const Opts d = default_opts();
  o->prob = d.prob;
  o->threshold = d.threshold;
  o->min_inliers = d.min_inliers;
  o->reserved = d.reserved;
}

static Opts opts_of(const sfmhip_verify_opts* opts) {
  return opts ? Opts{opts->prob, opts->threshold, opts->min_inliers, opts->reserved} : default_opts();
}

extern "C" int sfmhip_matchplan_verify(sfmhip_matchplan* plan, const int32_t* xy_ptr, const double* xy, const double K[9],
                                       const sfmhip_verify_opts* opts, sfmhip_verified** out) {
  if (!plan || !out) return SFMHIP_ERR_ARG;
  sfm_matchplan_lists l;
  SFM_TRY(sfm_matchplan_device_lists(plan, &l));
  SFM_HIP_TRY(hipSetDevice(l.ctx->device));
  return verify_device(l.ctx, l.n_images, l.n_rows, l.n_pairs, l.pairs, l.counts, nullptr, l.stride, l.q, l.t, xy_ptr, xy, K, opts_of(opts), out);
}

extern "C" int sfmhip_verify_lists(sfmhip_ctx* ctx, int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs,
                                   const int32_t* counts, const int32_t* match_q, const int32_t* match_t, const int32_t* xy_ptr,
                                   const double* xy, const double K[9], const sfmhip_verify_opts* opts, sfmhip_verified** out) {
  if (!ctx || !out || n_images < 0 || n_pairs < 0 || (n_images && !n_feat) || (n_pairs && (!pairs || !counts))) return SFMHIP_ERR_ARG;
  long long ne = 0;
  for (int p = 0; p < n_pairs; ++p) {
    if (counts[p] < 0) return SFMHIP_ERR_ARG;
    ne += counts[p];
    if (ne > INT_MAX - 1) return SFMHIP_ERR_ARG;
  }
  if (ne && (!match_q || !match_t)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBufs L;
  int *d_pairs = nullptr, *d_q = nullptr, *d_t = nullptr;
  SFM_TRY(L.alloc(&d_pairs, 2 * (size_t)n_pairs));
  SFM_TRY(L.alloc(&d_q, (size_t)ne));
  SFM_TRY(L.alloc(&d_t, (size_t)ne));
  if (n_pairs) SFM_HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, st));
  if (ne) {
    SFM_HIP_TRY(hipMemcpyAsync(d_q, match_q, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, st));
    SFM_HIP_TRY(hipMemcpyAsync(d_t, match_t, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, st));
  }
  const int rc = verify_device(ctx, n_images, n_feat, n_pairs, d_pairs, nullptr, counts, 0, d_q, d_t, xy_ptr, xy, K, opts_of(opts), out);
  hipStreamSynchronize(st);  // (the lists leave with this frame)
  return rc;
}

extern "C" int sfmhip_verified_counts(const sfmhip_verified* v, sfmhip_verify_stats* stats) {
  if (!v || !stats) return SFMHIP_ERR_ARG;
  stats->pairs = v->stats.pairs;
  stats->pairs_kept = v->stats.pairs_kept;
  stats->pairs_no_model = v->stats.pairs_no_model;
  stats->matches_in = v->stats.matches_in;
  stats->matches_out = v->stats.matches_out;
  return SFMHIP_OK;
}

extern "C" int sfmhip_verified_download(const sfmhip_verified* v, int32_t* counts, int32_t* match_q, int32_t* match_t, int32_t* inliers,
                                        int32_t* iterations, double* E, uint8_t* kept) {
  if (!v) return SFMHIP_ERR_ARG;
  const size_t np = (size_t)v->n_pairs;
  if (counts) std::copy(v->h_counts.begin(), v->h_counts.end(), counts);
  if (inliers) std::copy(v->inliers.begin(), v->inliers.end(), inliers);
  if (iterations) std::copy(v->iterations.begin(), v->iterations.end(), iterations);
  if (E) std::copy(v->E.begin(), v->E.end(), E);
  if (kept) std::copy(v->kept.begin(), v->kept.end(), kept);
  const long long ne = v->stats.matches_out;
  if ((!match_q && !match_t) || ne == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(v->ctx->device));
  hipStream_t st = v->ctx->stream;
  std::vector<int32_t> offs(np + 1, 0);
  for (size_t p = 0; p < np; ++p) offs[p + 1] = offs[p] + v->h_counts[p];
  DevBufs T;
  int *d_offs = nullptr, *d_pq = nullptr, *d_pt = nullptr;
  SFM_TRY(T.alloc(&d_offs, offs.size()));
  SFM_TRY(T.alloc(&d_pq, (size_t)ne));
  SFM_TRY(T.alloc(&d_pt, (size_t)ne));
  SFM_HIP_TRY(hipMemcpyAsync(d_offs, offs.data(), sizeof(int) * offs.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(vfy_pack, dim3(v->n_pairs), dim3(256), 0, st, (const int*)d_offs, v->stride, (const int*)v->q, (const int*)v->t, d_pq, d_pt);
  SFM_HIP_TRY(hipGetLastError());
  if (match_q) SFM_HIP_TRY(hipMemcpyAsync(match_q, d_pq, sizeof(int) * (size_t)ne, hipMemcpyDeviceToHost, st));
  if (match_t) SFM_HIP_TRY(hipMemcpyAsync(match_t, d_pt, sizeof(int) * (size_t)ne, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

extern "C" int sfmhip_verified_last_timing(const sfmhip_verified* v, double seconds[4]) {
  if (!v || !seconds) return SFMHIP_ERR_ARG;
  for (int i = 0; i < 4; ++i) seconds[i] = v->sec[i];
  return SFMHIP_OK;
}

extern "C" void sfmhip_verified_destroy(sfmhip_verified* v) {
  if (!v) return;
  hipSetDevice(v->ctx->device);
  delete v;
}
