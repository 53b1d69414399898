// tracks.hip -- multi-view feature tracks and their N-view triangulation on gfx950.  The rules are tracks.h's,
// which the CPU test stub compiles too; every output is the same bytes as that build's.
//
//   trk_check     T1 on the device: a bad pair, count or match raises a flag and the call is refused before anything is made;
//   trk_hook / trk_flatten   the components of the match graph by union_find.h's no-wait union-find (roots fall by atomicMin,
//                 a component ends at its least node id);
//   the handle's stable cell sort of the nodes by root, trk_heads + scan: the components in ascending root order, each in
//                 ascending (view, feature) order; trk_runs marks a component whose neighbours share an image (T3);
//   trk_classify + two scans   the kept components, their numbers and their places in the CSR (T4, T5); trk_emit writes it;
//   trk_lens + the cell sort   the permutation of the tracks by length; trk_wave_len + scan the slab offset of every wave;
//   trk_triangulate   one lane per track in that order: the lane's 4 x 2m system lies in a global slab interleaved at stride
//                 64 with a wave-uniform row length, so every access of the Jacobi is one coalesced 512-byte line per wave.
// No spin, no hand-off between workgroups, no float atomic.  Launches are ordered by the stream alone.
#include "common.h"
#include "cloud_grid.h"
#include "tracks.h"
#include "union_find.h"
#include <algorithm>
#include <climits>
#include <vector>

using namespace sfmtracks;
using sfmgrid::blocks;

static_assert(sizeof(sfmhip_tracks_opts) == sizeof(Opts), "sfmhip_tracks_opts mirrors sfmtracks::Opts");
static_assert(sizeof(sfmhip_tracks_stats) == sizeof(Stats), "sfmhip_tracks_stats mirrors sfmtracks::Stats");

struct sfmhip_tracks {
  sfmhip_ctx* ctx = nullptr;
  // (only its rocPRIM temporary storage, which frees itself with this struct: what sfmgrid::scan and sfmgrid::cell_sort work
  // through.  It is no handle of adopt_device: it has no min / max record (mm is null), so sfmgrid::minmax must not be called on it)
  sfmhip_cloud scratch;
  DevBufs B;
  int n_images = 0, n_nodes = 0, n_tracks = 0, n_obs = 0, n_waves = 0;
  long long slab_len = 0;  // sum over the waves of their longest track: the slab is 512 doubles per unit
  Opts opts = default_opts();
  Stats stats = {};
  std::vector<int> n_feat;
  int *trk_ptr = nullptr, *trk_view = nullptr, *trk_feat = nullptr, *node_track = nullptr;
  int *perm = nullptr, *woff = nullptr;
  double* slab = nullptr;  // made by the first triangulation
  double sec[SFMHIP_TRACKS_STAGES] = {0, 0, 0, 0, 0, 0};
};

namespace {

typedef unsigned long long u64;

struct Counters {
  u64 edges, components, conflicting, short_tracks;
  unsigned bad, pad;
};

struct Stamps {  // hipEvents between the stages when the context's timing is on
  hipStream_t st;
  bool on;
  std::vector<hipEvent_t> ev;
  Stamps(hipStream_t s, bool o) : st(s), on(o) {}
  ~Stamps() {
    for (hipEvent_t e : ev) hipEventDestroy(e);
  }
  void mark() {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) == hipSuccess) {
      hipEventRecord(e, st);
      ev.push_back(e);
    }
  }
  double seconds(size_t a) {  // between marks a and a + 1
    float ms = 0;
    if (!on || a + 1 >= ev.size() || hipEventSynchronize(ev[a + 1]) != hipSuccess || hipEventElapsedTime(&ms, ev[a], ev[a + 1]) != hipSuccess)
      return 0;
    return ms * 1e-3;
  }
};

// the first match of pair p: the plan keeps `stride` slots per pair, host lists are packed (off: their exclusive scan)
__device__ __forceinline__ long long list_start(const long long* off, int stride, int p) { return off ? off[p] : (long long)p * stride; }

__global__ __launch_bounds__(256) void trk_check(const int* pairs, const int* counts, const long long* off, int stride, int n_images,
                                                 const int* n_feat, const int* q, const int* t, Counters* cnt) {
  const int p = blockIdx.x, a = pairs[2 * p], b = pairs[2 * p + 1], c = counts[p];
  if (!pair_ok(a, b, n_images) || c < 0 || (!off && c > stride)) {
    if (threadIdx.x == 0) atomicOr(&cnt->bad, 1u);
    return;
  }
  const long long o = list_start(off, stride, p);
  const int nfa = n_feat[a], nfb = n_feat[b];
  bool bad = false;
  for (int k = threadIdx.x; k < c; k += blockDim.x) bad |= !match_ok(q[o + k], t[o + k], nfa, nfb);
  if (bad) atomicOr(&cnt->bad, 1u);
  if (threadIdx.x == 0 && c) atomicAdd(&cnt->edges, (u64)c);
}

__global__ __launch_bounds__(256) void trk_iota(int n, int* a, int* b) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a[i] = i;
  if (b) b[i] = i;
}

// the hook kernel: one edge per thread step, a workgroup per pair (checked before: every index is in range)
__global__ __launch_bounds__(256) void trk_hook(const int* pairs, const int* counts, const long long* off, int stride, const int* base,
                                                const int* q, const int* t, int* parent) {
  const int p = blockIdx.x, c = counts[p];
  const int ba = base[pairs[2 * p]], bb = base[pairs[2 * p + 1]];
  const long long o = list_start(off, stride, p);
  for (int k = threadIdx.x; k < c; k += blockDim.x) sfmuf::unite(parent, ba + q[o + k], bb + t[o + k]);
}

__global__ __launch_bounds__(256) void trk_flatten(int* parent, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int r = sfmuf::root_of(parent, i);
  __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void trk_heads(const int* root, int n, int* head) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k < n) head[k] = (k == 0 || root[k] != root[k - 1]) ? 1 : 0;
}

// position k of the sorted order lies in component hx[k] + head[k] - 1 (hx: the exclusive scan of head)
__global__ __launch_bounds__(256) void trk_runs(const int* node, const int* head, const int* hx, int n, int n_comp, const int* base, int n_images,
                                                int* cstart, int* conf) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (k == 0) cstart[n_comp] = n;
  const int c = hx[k] + head[k] - 1;
  if (head[k]) cstart[c] = k;
  else if (image_of(base, n_images, node[k]) == image_of(base, n_images, node[k - 1])) conf[c] = 1;  // (T3; every writer stores 1)
}

__global__ __launch_bounds__(256) void trk_classify(const int* cstart, const int* conf, int n_comp, int need, int* kept, int* lens, Counters* cnt) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  bool comp = false, cf = false, sh = false;
  if (c < n_comp) {
    const int len = cstart[c + 1] - cstart[c];
    comp = len >= 2;
    cf = comp && conf[c] != 0;
    sh = comp && !cf && len < need;
    const bool k = comp && !cf && !sh;
    kept[c] = k ? 1 : 0;
    lens[c] = k ? len : 0;
  }
  const unsigned nc = (unsigned)__popcll(__ballot(comp)), nf = (unsigned)__popcll(__ballot(cf)), ns = (unsigned)__popcll(__ballot(sh));
  if ((threadIdx.x & 63) == 0) {
    if (nc) atomicAdd(&cnt->components, (u64)nc);
    if (nf) atomicAdd(&cnt->conflicting, (u64)nf);
    if (ns) atomicAdd(&cnt->short_tracks, (u64)ns);
  }
}

__global__ __launch_bounds__(256) void trk_emit(const int* node, const int* head, const int* hx, int n, const int* cstart, const int* kept,
                                                const int* tno, const int* ooff, const int* base, int n_images, int n_tracks, int n_obs,
                                                int* trk_ptr, int* trk_view, int* trk_feat, int* node_track) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  if (k == 0) trk_ptr[n_tracks] = n_obs;
  const int c = hx[k] + head[k] - 1, nd = node[k];
  if (!kept[c]) {
    node_track[nd] = -1;
    return;
  }
  const int pos = ooff[c] + (k - cstart[c]), im = image_of(base, n_images, nd);
  if (pos < 0 || pos >= n_obs) return;  // (never: ooff is the scan of the kept lengths)
  trk_view[pos] = im;
  trk_feat[pos] = nd - base[im];
  node_track[nd] = tno[c];
  if (head[k]) trk_ptr[tno[c]] = ooff[c];
}

__global__ __launch_bounds__(256) void trk_lens(const int* trk_ptr, int nt, int* len, int* idx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nt) return;
  len[i] = trk_ptr[i + 1] - trk_ptr[i];
  idx[i] = i;
}

// a wave's row length: its longest track, the last of its lanes in ascending length order
__global__ __launch_bounds__(256) void trk_wave_len(const int* sorted_len, int nt, int n_waves, int* wlen) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n_waves) wlen[w] = sorted_len[min(64 * w + 63, nt - 1)];
}

// cam: K[9] then dist[5].  The slab of wave w starts at 512 * woff[w] doubles and holds 4 rows of 2 * (its longest track)
// entries for each of its 64 lanes, lane-interleaved.
__global__ __launch_bounds__(256) void trk_triangulate(int nt, const int* __restrict__ perm, const int* __restrict__ woff,
                                                       const int* __restrict__ trk_ptr, const int* __restrict__ trk_view,
                                                       const int* __restrict__ trk_feat, const double* __restrict__ cam,
                                                       const double* __restrict__ views, const uint8_t* __restrict__ has_pose,
                                                       const int* __restrict__ xy_ptr, const double* __restrict__ xy, float max_err,
                                                       int min_views, int front_only, double* slab, double* __restrict__ X,
                                                       float* __restrict__ err, int* __restrict__ n_used, uint8_t* __restrict__ keep) {
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  const int i = gw * 64 + lane;
  if (i >= nt) return;
  const int tl = perm[min(gw * 64 + 63, nt - 1)], lda = 2 * (trk_ptr[tl + 1] - trk_ptr[tl]);
  const int tr = perm[i];
  double* At = slab + (size_t)woff[gw] * 512 + lane;
  double Xi[3];
  int32_t m;
  uint8_t kp;
  triangulate_track<64>(trk_ptr[tr], trk_ptr[tr + 1], trk_view, trk_feat, views, has_pose, cam, cam + 9, xy_ptr, xy, max_err, min_views,
                        front_only, At, lda, Xi, err, &m, &kp);
  X[3 * (size_t)tr] = Xi[0];
  X[3 * (size_t)tr + 1] = Xi[1];
  X[3 * (size_t)tr + 2] = Xi[2];
  n_used[tr] = m;
  keep[tr] = kp;
}

// everything after the lists are on the device.  pairs, counts, q, t (and off, or stride) are device pointers.
int build_device(sfmhip_ctx* ctx, int n_images, const int* n_feat, int n_pairs, const int* d_pairs, const int* d_counts, const long long* d_off,
                 int stride, const int* d_q, const int* d_t, const Opts& o, Stamps& sp, sfmhip_tracks** out) {
  hipStream_t st = ctx->stream;
  std::vector<int> base((size_t)n_images + 1, 0);
  long long nn = 0;
  for (int i = 0; i < n_images; ++i) {
    if (n_feat[i] < 0) return SFMHIP_ERR_ARG;
    nn += n_feat[i];
    if (nn > INT_MAX - 1) return SFMHIP_ERR_ARG;
    base[(size_t)i + 1] = (int)nn;
  }
  const int n = (int)nn;
  DevBufs T;  // this call's temporaries
  int *d_base = nullptr, *d_nf = nullptr;
  Counters* d_cnt = nullptr;
  SFM_TRY(T.alloc(&d_base, (size_t)n_images + 1));
  SFM_TRY(T.alloc(&d_nf, (size_t)std::max(n_images, 1)));
  SFM_TRY(T.alloc(&d_cnt, 1));
  SFM_HIP_TRY(hipMemcpyAsync(d_base, base.data(), sizeof(int) * base.size(), hipMemcpyHostToDevice, st));
  if (n_images) SFM_HIP_TRY(hipMemcpyAsync(d_nf, n_feat, sizeof(int) * n_images, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(d_cnt, 0, sizeof(Counters), st));
  sp.mark();
  Counters cnt = {};
  if (n_pairs > 0) {
    hipLaunchKernelGGL(trk_check, dim3(n_pairs), dim3(256), 0, st, d_pairs, d_counts, d_off, stride, n_images, d_nf, d_q, d_t, d_cnt);
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, st));
  }
  SFM_HIP_TRY(hipStreamSynchronize(st));  // (n_feat and base are the caller's and this frame's)
  if (cnt.bad || cnt.edges > (u64)(INT_MAX - 1)) return SFMHIP_ERR_ARG;
  sp.mark();

  sfmhip_tracks* h = new sfmhip_tracks();
  struct Guard {  // a failing step below frees the handle
    sfmhip_tracks* h;
    ~Guard() {
      if (h) sfmhip_tracks_destroy(h);
    }
  } guard{h};
  h->ctx = ctx;
  h->scratch.ctx = ctx;
  h->n_images = n_images;
  h->n_nodes = n;
  h->opts = o;
  h->n_feat.assign(n_feat, n_feat + n_images);
  h->stats = Stats{n, (int64_t)cnt.edges, 0, 0, 0, 0, 0};
  SFM_TRY(h->B.alloc(&h->node_track, (size_t)std::max(n, 1)));
  int n_tracks = 0, n_obs = 0;
  if (n > 0) {
    const size_t N = (size_t)n;
    int *parent, *iota, *root, *node, *head, *hx, *cstart, *conf, *kept, *lens, *tno, *ooff;
    SFM_TRY(T.alloc(&parent, N));
    SFM_TRY(T.alloc(&iota, N));
    SFM_TRY(T.alloc(&root, N));
    SFM_TRY(T.alloc(&node, N));
    SFM_TRY(T.alloc(&head, N));
    SFM_TRY(T.alloc(&hx, N));
    SFM_TRY(T.alloc(&cstart, N + 1));
    SFM_TRY(T.alloc(&conf, N));
    SFM_TRY(T.alloc(&kept, N));
    SFM_TRY(T.alloc(&lens, N));
    SFM_TRY(T.alloc(&tno, N));
    SFM_TRY(T.alloc(&ooff, N));
    hipLaunchKernelGGL(trk_iota, dim3(blocks(n, 256)), dim3(256), 0, st, n, parent, iota);
    if (n_pairs > 0) hipLaunchKernelGGL(trk_hook, dim3(n_pairs), dim3(256), 0, st, d_pairs, d_counts, d_off, stride, d_base, d_q, d_t, parent);
    hipLaunchKernelGGL(trk_flatten, dim3(blocks(n, 256)), dim3(256), 0, st, parent, n);
    SFM_HIP_TRY(hipGetLastError());
    sp.mark();
    SFM_TRY(sfmgrid::cell_sort(&h->scratch, n, parent, root, iota, node, n));
    sp.mark();
    int n_comp = 0;
    hipLaunchKernelGGL(trk_heads, dim3(blocks(n, 256)), dim3(256), 0, st, root, n, head);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(sfmgrid::scan(&h->scratch, head, hx, N, &n_comp));
    SFM_HIP_TRY(hipMemsetAsync(conf, 0, sizeof(int) * N, st));
    hipLaunchKernelGGL(trk_runs, dim3(blocks(n, 256)), dim3(256), 0, st, node, head, hx, n, n_comp, d_base, n_images, cstart, conf);
    hipLaunchKernelGGL(trk_classify, dim3(blocks(n_comp, 256)), dim3(256), 0, st, cstart, conf, n_comp, need_len(o.min_len), kept, lens, d_cnt);
    SFM_HIP_TRY(hipGetLastError());
    SFM_TRY(sfmgrid::scan(&h->scratch, kept, tno, (size_t)n_comp, &n_tracks));
    SFM_TRY(sfmgrid::scan(&h->scratch, lens, ooff, (size_t)n_comp, &n_obs));
    SFM_TRY(h->B.alloc(&h->trk_ptr, (size_t)n_tracks + 1));
    SFM_TRY(h->B.alloc(&h->trk_view, (size_t)std::max(n_obs, 1)));
    SFM_TRY(h->B.alloc(&h->trk_feat, (size_t)std::max(n_obs, 1)));
    hipLaunchKernelGGL(trk_emit, dim3(blocks(n, 256)), dim3(256), 0, st, node, head, hx, n, cstart, kept, tno, ooff, d_base, n_images, n_tracks,
                       n_obs, h->trk_ptr, h->trk_view, h->trk_feat, h->node_track);
    SFM_HIP_TRY(hipGetLastError());
    SFM_HIP_TRY(hipMemcpyAsync(&cnt, d_cnt, sizeof(Counters), hipMemcpyDeviceToHost, st));
    sp.mark();
    if (n_tracks > 0) {  // the length buckets: the tracks in ascending length, the slab offset of every wave of 64
      const int n_waves = (n_tracks + 63) / 64;
      int slab_len = 0;
      int *len = lens, *idx = tno, *slen = kept, *wlen = head;  // (n_tracks <= n / 2: the temporaries are free again)
      SFM_TRY(h->B.alloc(&h->perm, (size_t)n_tracks));
      SFM_TRY(h->B.alloc(&h->woff, (size_t)n_waves));
      hipLaunchKernelGGL(trk_lens, dim3(blocks(n_tracks, 256)), dim3(256), 0, st, h->trk_ptr, n_tracks, len, idx);
      SFM_HIP_TRY(hipGetLastError());
      SFM_TRY(sfmgrid::cell_sort(&h->scratch, n_images, len, slen, idx, h->perm, n_tracks));
      hipLaunchKernelGGL(trk_wave_len, dim3(blocks(n_waves, 256)), dim3(256), 0, st, slen, n_tracks, n_waves, wlen);
      SFM_HIP_TRY(hipGetLastError());
      SFM_TRY(sfmgrid::scan(&h->scratch, wlen, h->woff, (size_t)n_waves, &slab_len));
      h->n_waves = n_waves;
      h->slab_len = slab_len;
    }
    sp.mark();
  } else {
    SFM_TRY(h->B.alloc(&h->trk_ptr, 1));
  }
  if (n_tracks == 0) SFM_HIP_TRY(hipMemsetAsync(h->trk_ptr, 0, sizeof(int), st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  h->n_tracks = n_tracks;
  h->n_obs = n_obs;
  h->stats.components = (int64_t)cnt.components;
  h->stats.conflicting = (int64_t)cnt.conflicting;
  h->stats.short_tracks = (int64_t)cnt.short_tracks;
  h->stats.n_tracks = n_tracks;
  h->stats.n_obs = n_obs;
  if (sp.on && n > 0) {
    h->sec[0] = sp.seconds(0);
    h->sec[1] = sp.seconds(1);
    h->sec[2] = sp.seconds(2);
    h->sec[3] = sp.seconds(3);
    h->sec[4] = sp.seconds(4);
  }
  guard.h = nullptr;
  *out = h;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_tracks_default_opts(sfmhip_tracks_opts* o) {
  if (!o) return;
  const Opts d = default_opts();
  o->min_len = d.min_len;
  o->front_only = d.front_only;
}

extern "C" int sfmhip_tracks_build(sfmhip_ctx* ctx, int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs,
                                   const int32_t* counts, const int32_t* match_q, const int32_t* match_t, const sfmhip_tracks_opts* opts,
                                   sfmhip_tracks** out) {
  if (!ctx || !out || n_images < 0 || n_pairs < 0 || (n_images && !n_feat) || (n_pairs && (!pairs || !counts))) return SFMHIP_ERR_ARG;
  Opts o = default_opts();
  if (opts) o = Opts{opts->min_len, opts->front_only};
  std::vector<long long> off((size_t)n_pairs + 1, 0);
  for (int p = 0; p < n_pairs; ++p) {
    if (counts[p] < 0) return SFMHIP_ERR_ARG;
    off[(size_t)p + 1] = off[p] + counts[p];
  }
  const long long ne = off[n_pairs];
  if (ne > INT_MAX - 1 || (ne && (!match_q || !match_t))) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Stamps sp(st, ctx->timing);
  DevBufs L;
  int *d_pairs = nullptr, *d_counts = nullptr, *d_q = nullptr, *d_t = nullptr;
  long long* d_off = nullptr;
  SFM_TRY(L.alloc(&d_pairs, 2 * (size_t)n_pairs));
  SFM_TRY(L.alloc(&d_counts, (size_t)n_pairs));
  SFM_TRY(L.alloc(&d_off, (size_t)n_pairs + 1));
  SFM_TRY(L.alloc(&d_q, (size_t)ne));
  SFM_TRY(L.alloc(&d_t, (size_t)ne));
  if (n_pairs) {
    SFM_HIP_TRY(hipMemcpyAsync(d_pairs, pairs, sizeof(int) * 2 * (size_t)n_pairs, hipMemcpyHostToDevice, st));
    SFM_HIP_TRY(hipMemcpyAsync(d_counts, counts, sizeof(int) * (size_t)n_pairs, hipMemcpyHostToDevice, st));
  }
  SFM_HIP_TRY(hipMemcpyAsync(d_off, off.data(), sizeof(long long) * off.size(), hipMemcpyHostToDevice, st));
  if (ne) {
    SFM_HIP_TRY(hipMemcpyAsync(d_q, match_q, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, st));
    SFM_HIP_TRY(hipMemcpyAsync(d_t, match_t, sizeof(int) * (size_t)ne, hipMemcpyHostToDevice, st));
  }
  const int rc = build_device(ctx, n_images, n_feat, n_pairs, d_pairs, d_counts, d_off, 0, d_q, d_t, o, sp, out);
  hipStreamSynchronize(st);  // (the lists and `off` leave with this frame)
  return rc;
}

extern "C" int sfmhip_tracks_build_from_plan(sfmhip_matchplan* plan, const sfmhip_tracks_opts* opts, sfmhip_tracks** out) {
  if (!plan || !out) return SFMHIP_ERR_ARG;
  sfm_matchplan_lists l;
  SFM_TRY(sfm_matchplan_device_lists(plan, &l));
  Opts o = default_opts();
  if (opts) o = Opts{opts->min_len, opts->front_only};
  SFM_HIP_TRY(hipSetDevice(l.ctx->device));
  Stamps sp(l.ctx->stream, l.ctx->timing);
  return build_device(l.ctx, l.n_images, l.n_rows, l.n_pairs, l.pairs, l.counts, nullptr, l.stride, l.q, l.t, o, sp, out);
}

extern "C" int sfmhip_tracks_build_from_verified(const sfmhip_verified* verified, const sfmhip_tracks_opts* opts, sfmhip_tracks** out) {
  if (!verified || !out) return SFMHIP_ERR_ARG;
  sfm_matchplan_lists l;
  SFM_TRY(sfm_verified_device_lists(verified, &l));
  Opts o = default_opts();
  if (opts) o = Opts{opts->min_len, opts->front_only};
  SFM_HIP_TRY(hipSetDevice(l.ctx->device));
  Stamps sp(l.ctx->stream, l.ctx->timing);
  return build_device(l.ctx, l.n_images, l.n_rows, l.n_pairs, l.pairs, l.counts, nullptr, l.stride, l.q, l.t, o, sp, out);
}

extern "C" int sfmhip_tracks_counts(const sfmhip_tracks* tr, sfmhip_tracks_stats* stats) {
  if (!tr || !stats) return SFMHIP_ERR_ARG;
  stats->nodes = tr->stats.nodes;
  stats->edges = tr->stats.edges;
  stats->components = tr->stats.components;
  stats->conflicting = tr->stats.conflicting;
  stats->short_tracks = tr->stats.short_tracks;
  stats->n_tracks = tr->stats.n_tracks;
  stats->n_obs = tr->stats.n_obs;
  return SFMHIP_OK;
}

extern "C" int sfmhip_tracks_download(const sfmhip_tracks* tr, int32_t* trk_ptr, int32_t* trk_view, int32_t* trk_feat, int32_t* node_track) {
  if (!tr) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(tr->ctx->device));
  hipStream_t st = tr->ctx->stream;
  if (trk_ptr) SFM_HIP_TRY(hipMemcpyAsync(trk_ptr, tr->trk_ptr, sizeof(int) * ((size_t)tr->n_tracks + 1), hipMemcpyDeviceToHost, st));
  if (trk_view && tr->n_obs) SFM_HIP_TRY(hipMemcpyAsync(trk_view, tr->trk_view, sizeof(int) * (size_t)tr->n_obs, hipMemcpyDeviceToHost, st));
  if (trk_feat && tr->n_obs) SFM_HIP_TRY(hipMemcpyAsync(trk_feat, tr->trk_feat, sizeof(int) * (size_t)tr->n_obs, hipMemcpyDeviceToHost, st));
  if (node_track && tr->n_nodes)
    SFM_HIP_TRY(hipMemcpyAsync(node_track, tr->node_track, sizeof(int) * (size_t)tr->n_nodes, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

extern "C" int sfmhip_tracks_triangulate(sfmhip_tracks* tr, const double* poses, const uint8_t* has_pose, const double K[9], const double dist[5],
                                         const int32_t* xy_ptr, const double* xy, float max_err, int min_views, double* X, float* err,
                                         int32_t* n_used, uint8_t* keep) {
  if (!tr || !K || !dist) return SFMHIP_ERR_ARG;
  const int ni = tr->n_images, nt = tr->n_tracks;
  if (ni && (!poses || !has_pose || !xy_ptr)) return SFMHIP_ERR_ARG;
  if (ni && xy_ptr[0] < 0) return SFMHIP_ERR_ARG;
  for (int v = 0; v < ni; ++v) {  // a view with a pose has a pixel for every feature
    if (xy_ptr[v + 1] < xy_ptr[v]) return SFMHIP_ERR_ARG;
    if (has_pose[v] && xy_ptr[v + 1] - xy_ptr[v] < tr->n_feat[v]) return SFMHIP_ERR_ARG;
  }
  tr->sec[5] = 0;
  if (nt == 0) return SFMHIP_OK;
  const size_t n_xy = (size_t)xy_ptr[ni];
  if (n_xy && !xy) return SFMHIP_ERR_ARG;
  sfmhip_ctx* ctx = tr->ctx;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (!tr->slab) SFM_TRY(tr->B.alloc(&tr->slab, 512 * (size_t)tr->slab_len));
  DevBufs T;
  double *d_cam, *d_views, *d_xy, *d_X;
  uint8_t *d_has, *d_keep;
  int *d_xyp, *d_used;
  float* d_err;
  SFM_TRY(T.alloc(&d_cam, 16));
  SFM_TRY(T.alloc(&d_views, 12 * (size_t)ni));
  SFM_TRY(T.alloc(&d_has, (size_t)ni));
  SFM_TRY(T.alloc(&d_xyp, (size_t)ni + 1));
  SFM_TRY(T.alloc(&d_xy, 2 * n_xy));
  SFM_TRY(T.alloc(&d_X, 3 * (size_t)nt));
  SFM_TRY(T.alloc(&d_err, (size_t)tr->n_obs));
  SFM_TRY(T.alloc(&d_used, (size_t)nt));
  SFM_TRY(T.alloc(&d_keep, (size_t)nt));
  double cam[16] = {0};
  for (int i = 0; i < 9; ++i) cam[i] = K[i];
  for (int i = 0; i < 5; ++i) cam[9 + i] = dist[i];
  SFM_HIP_TRY(hipMemcpyAsync(d_cam, cam, sizeof cam, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_views, poses, sizeof(double) * 12 * (size_t)ni, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_has, has_pose, (size_t)ni, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemcpyAsync(d_xyp, xy_ptr, sizeof(int) * ((size_t)ni + 1), hipMemcpyHostToDevice, st));
  if (n_xy) SFM_HIP_TRY(hipMemcpyAsync(d_xy, xy, sizeof(double) * 2 * n_xy, hipMemcpyHostToDevice, st));
  Stamps sp(st, ctx->timing);
  sp.mark();
  hipLaunchKernelGGL(trk_triangulate, dim3(blocks(tr->n_waves, 4)), dim3(256), 0, st, nt, tr->perm, tr->woff, tr->trk_ptr, tr->trk_view,
                     tr->trk_feat, d_cam, d_views, d_has, d_xyp, d_xy, max_err, min_views, tr->opts.front_only, tr->slab, d_X, d_err, d_used,
                     d_keep);
  SFM_HIP_TRY(hipGetLastError());
  sp.mark();
  if (X) SFM_HIP_TRY(hipMemcpyAsync(X, d_X, sizeof(double) * 3 * (size_t)nt, hipMemcpyDeviceToHost, st));
  if (err) SFM_HIP_TRY(hipMemcpyAsync(err, d_err, sizeof(float) * (size_t)tr->n_obs, hipMemcpyDeviceToHost, st));
  if (n_used) SFM_HIP_TRY(hipMemcpyAsync(n_used, d_used, sizeof(int) * (size_t)nt, hipMemcpyDeviceToHost, st));
  if (keep) SFM_HIP_TRY(hipMemcpyAsync(keep, d_keep, (size_t)nt, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  tr->sec[5] = sp.seconds(0);
  return SFMHIP_OK;
}

extern "C" int sfmhip_tracks_last_timing(const sfmhip_tracks* tr, double seconds[SFMHIP_TRACKS_STAGES]) {
  if (!tr || !seconds) return SFMHIP_ERR_ARG;
  for (int i = 0; i < SFMHIP_TRACKS_STAGES; ++i) seconds[i] = tr->sec[i];
  return SFMHIP_OK;
}

extern "C" void sfmhip_tracks_destroy(sfmhip_tracks* tr) {
  if (!tr) return;
  hipSetDevice(tr->ctx->device);
  delete tr;  // (the scratch handle's temporary storage frees itself)
}
