// crowns.hip -- the crown delineation on gfx950: tree tops and crowns from a canopy raster, a tree number per point.  The rules
// are DESIGN.md f-21's; the arithmetic is crowns.h's, which the CPU test stub compiles too, and every output is the same bytes
// as that build's.  Every quantity is a pure function of the raster, so the kernels iterate as suits them:
//
//   crn_smooth    rule 3, a thread per cell, one launch per pass from one buffer into the other; a wave reads three segments of
//                 TILE contiguous cells;
//   crn_up        rules 4 - 6: up(q) into root[q] (-1 for a cell that is not canopy), the summit flags, the canopy count;
//   crn_jump      pointer doubling in place, root[q] = root[root[q]]: whatever another thread has written by then is an ancestor
//                 of q on its path, so the fixed point is root() in any interleaving.  The count of cells each round moved is
//                 read back once per batch of BATCH rounds, and rounds after one that moved nothing move nothing;
//   the summits   compacted by the scan into a list in ascending cell id: only they pay for a window;
//   crn_window    rule 7, a wave per summit over the square around its disc, then a keyed wave butterfly (rule 5's order is total,
//                 so the maximum does not depend on the order of the comparisons); parent() as a position in the summit list;
//   crn_pjump     the summit forest by doubling from one buffer into the other (the depth of a chain is summed on the way, so a
//                 round reads only the round before), counters as for crn_jump;
//   crn_tops      rule 8 by a scan of the top flags over the list, rule 11's rows; crn_labels rule 9, a thread per cell, the
//                 counts by integer atomics; crn_points rule 10, a thread per point; crn_area the rows' areas.
// No spin, no hand-off between workgroups, no float atomic.  Launches are ordered by the stream alone.
#include "common.h"
#include "cloud_grid.h"
#include "crowns.h"
#include <algorithm>

using namespace sfmcrowns;
using sfmgrid::blocks;
using sfmgrid::Grow;
using sfmgrid::mirror;

namespace {

struct Counts {  // what the kernels count
  unsigned n_canopy, n_labelled_cells, n_labelled, max_depth;
};

// the device memory of one delineation, grow-only: on a cloud handle (CrnState) or on the context (the raster entry)
struct Core {
  Grow<float> H;         // 2 ncell: the smoothing's two buffers
  Grow<int> root;        // ncell
  Grow<int> flag, pos;   // ncell: the summit flags and their exclusive scan (a summit's position in the list)
  Grow<int> labels;      // ncell
  Grow<int> list;        // 5 ns: a summit's cell, R2, its number (-1: none), its top flag and the flags' exclusive scan
  Grow<int2> par;        // 2 ns: (parent's position in the list, parent steps to it)
  Grow<Top> tops;        // max_trees
  Grow<unsigned> cnt;    // Counts, then BATCH round counters
  const float* Hfin = nullptr;  // the last run's H (in H)
  int rounds_up = 0, rounds_parent = 0;
  double ms[6] = {0, 0, 0, 0, 0, 0};
};

struct Scan {  // the exclusive scan a run compacts with: the handle's, or the context state's own
  int (*fn)(void* who, const int* in, int* out, size_t n, int* total);
  void* who;
  int operator()(const int* in, int* out, size_t n, int* total) const { return fn(who, in, out, n, total); }
};

__global__ __launch_bounds__(256) void crn_smooth(const float* __restrict__ in, int De, int Dn, float* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= De * Dn) return;
  out[q] = smooth_value(in, q % De, q / De, De, Dn);
}

__global__ __launch_bounds__(256) void crn_up(const float* __restrict__ H, int De, int Dn, double min_h, int* __restrict__ root,
                                              int* __restrict__ flag, Counts* cnt) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  bool canopy = false;
  if (q < De * Dn) {
    canopy = is_canopy(H[q], min_h);
    const int u = canopy ? up_of(H, q % De, q / De, De, Dn, min_h) : -1;
    root[q] = u;
    flag[q] = u == q ? 1 : 0;
  }
  const unsigned m = (unsigned)__popcll(__ballot(canopy));
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt->n_canopy, m);
}

__global__ __launch_bounds__(256) void crn_jump(int* root, int ncell, unsigned* moved) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  bool m = false;
  if (q < ncell) {
    const int r = root[q];
    if (r >= 0 && r < ncell) {
      const int rr = root[r];
      if (rr != r && rr >= 0 && rr < ncell) root[q] = rr, m = true;
    }
  }
  const unsigned k = (unsigned)__popcll(__ballot(m));
  if ((threadIdx.x & 63) == 0 && k) atomicAdd(moved, k);
}

__global__ __launch_bounds__(256) void crn_compact(const int* __restrict__ flag, const int* __restrict__ pos, int n, int cap, int* __restrict__ out) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n || !flag[q]) return;
  const int k = pos[q];
  if (k >= 0 && k < cap) out[k] = q;
}

// rule 7 for summit k of the list: a wave over the square around its disc
__global__ __launch_bounds__(256) void crn_window(const float* __restrict__ H, int De, int Dn, Prep p, const int* __restrict__ scell, int ns,
                                                  const int* __restrict__ root, const int* __restrict__ pos, int2* __restrict__ par,
                                                  int* __restrict__ sR2, int* __restrict__ istop) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= ns) return;
  const int s = scell[k], ncell = De * Dn;
  if (s < 0 || s >= ncell) return;  // (never)
  const int sx = s % De, sy = s / De;
  const float hs = H[s];
  const int R2 = window_R2(hs, p), rad = int_radius(R2), w = 2 * rad + 1;
  float hb = hs;
  int best = s;
  for (int t = lane; t < w * w; t += 64) {
    const int dx = t % w - rad, dy = t / w - rad;
    const int xx = sx + dx, yy = sy + dy;
    if (xx < 0 || yy < 0 || xx >= De || yy >= Dn || dx * dx + dy * dy > R2) continue;
    const int r = yy * De + xx;
    const float v = H[r];
    if (is_canopy(v, p.min_h) && key_greater(v, r, hb, best)) hb = v, best = r;
  }
  for (int off = 32; off >= 1; off >>= 1) {
    const float ho = __shfl_xor(hb, off);
    const int bo = __shfl_xor(best, off);
    if (key_greater(ho, bo, hb, best)) hb = ho, best = bo;
  }
  if (lane != 0) return;
  int parent = k;
  if (best != s) {
    const int r = root[best];
    const int j = r >= 0 && r < ncell ? pos[r] : -1;
    if (j >= 0 && j < ns) parent = j;  // (always: the root of a canopy cell is a summit)
  }
  par[k] = make_int2(parent, parent == k ? 0 : 1);
  sR2[k] = R2;
  istop[k] = parent == k ? 1 : 0;
}

__global__ __launch_bounds__(256) void crn_pjump(const int2* __restrict__ in, int ns, int2* __restrict__ out, unsigned* moved) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  bool m = false;
  if (k < ns) {
    const int2 a = in[k];
    int2 o = a;
    if (a.x >= 0 && a.x < ns) {
      const int2 b = in[a.x];
      if (b.x != a.x && b.x >= 0 && b.x < ns) o = make_int2(b.x, a.y + b.y), m = true;
    }
    out[k] = o;
  }
  const unsigned c = (unsigned)__popcll(__ballot(m));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(moved, c);
}

// rule 8's numbers and rule 11's rows (without their counts), the longest chain
__global__ __launch_bounds__(256) void crn_tops(const int* __restrict__ scell, const int* __restrict__ istop, const int* __restrict__ tpos,
                                                const int* __restrict__ sR2, const int2* __restrict__ par, int ns, int max_trees,
                                                const float* __restrict__ Z, const float* __restrict__ H, int De, float e_min, float n_min,
                                                double c, int* __restrict__ number, Top* __restrict__ tops, Counts* cnt) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  unsigned depth = 0;
  if (k < ns) {
    depth = (unsigned)par[k].y;
    int j = -1;
    if (istop[k] && tpos[k] < max_trees) {
      j = tpos[k];
      Top t;
      fill_top(t, scell[k], De, e_min, n_min, c, Z[scell[k]], H[scell[k]], sR2[k]);
      t.cells = t.points = 0;
      t.area = 0.0;
      tops[j] = t;
    }
    number[k] = j;
  }
  for (int off = 32; off >= 1; off >>= 1) depth = max(depth, (unsigned)__shfl_xor(depth, off));
  if ((threadIdx.x & 63) == 0 && depth) atomicMax(&cnt->max_depth, depth);
}

// rule 9 for cell q
__global__ __launch_bounds__(256) void crn_labels(const float* __restrict__ H, const int* __restrict__ root, const int* __restrict__ pos,
                                                  const int2* __restrict__ par, const int* __restrict__ number, const int* __restrict__ scell,
                                                  int De, int Dn, int ns, int kept, Prep p, int* __restrict__ labels, Top* tops, Counts* cnt) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x, ncell = De * Dn;
  int lab = -1;
  if (q < ncell) {
    const int r = root[q];
    if (r >= 0 && r < ncell) {
      const int k = pos[r];
      const int t = k >= 0 && k < ns ? par[k].x : -1;
      const int j = t >= 0 && t < ns ? number[t] : -1;
      if (j >= 0 && j < kept) {
        const int tc = scell[t];
        if (in_crown(H[q], H[tc], q % De, q / De, tc % De, tc / De, p)) {
          lab = j;
          atomicAdd(&tops[j].cells, 1);
        }
      }
    }
    labels[q] = lab;
  }
  const unsigned m = (unsigned)__popcll(__ballot(lab >= 0));
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt->n_labelled_cells, m);
}

// rule 10 for point i
__global__ __launch_bounds__(256) void crn_points(const float* __restrict__ enh, const float* __restrict__ hag, int n, sfmterrain::Dims d, double c,
                                                  double clear, const int* __restrict__ labels, int kept, int* __restrict__ tree_of, Top* tops,
                                                  Counts* cnt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  int lab = -1;
  if (i < n) {
    const float e = enh[3 * (size_t)i], nn = enh[3 * (size_t)i + 1], h = enh[3 * (size_t)i + 2];
    if (h == h && above_clear(hag[i], clear)) {
      const int q = sfmterrain::cell_of(e, nn, d, c);
      if (q >= 0 && q < d.De * d.Dn) lab = labels[q];  // (always in range: the raster was sized by these points)
      if (lab >= kept) lab = -1;                       // (never)
      if (lab >= 0) atomicAdd(&tops[lab].points, 1);
    }
    tree_of[i] = lab;
  }
  const unsigned m = (unsigned)__popcll(__ballot(lab >= 0));
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt->n_labelled, m);
}

__global__ __launch_bounds__(256) void crn_area(Top* tops, int kept, double c) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < kept) tops[j].area = top_area(tops[j].cells, c);
}

#define CRN_LAUNCH(kernel, grid, ...)                                \
  do {                                                               \
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, __VA_ARGS__); \
    SFM_HIP_TRY(hipGetLastError());                                  \
  } while (0)

// doubling rounds in batches until one moves nothing; `round` enqueues one round that counts into its argument
template <class Round>
int doubling(hipStream_t st, unsigned* d_moved, int limit, int& rounds, Round round) {
  rounds = 0;
  for (bool open = true; open && rounds < limit;) {
    unsigned moved[BATCH];
    SFM_HIP_TRY(hipMemsetAsync(d_moved, 0, sizeof moved, st));
    for (int b = 0; b < BATCH; ++b) SFM_TRY(round(d_moved + b));
    SFM_HIP_TRY(hipMemcpyAsync(moved, d_moved, sizeof moved, hipMemcpyDeviceToHost, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    for (int b = 0; b < BATCH && open; ++b) {
      ++rounds;
      open = moved[b] != 0;
    }
  }
  return SFMHIP_OK;
}

struct Points {  // rule 10's inputs (the cloud entry), all on the device; n = 0: the raster entry
  const float *enh = nullptr, *hag = nullptr;
  int n = 0;
  int* tree_of = nullptr;  // n
  sfmterrain::Dims d = {0.0f, 0.0f, 0, 0};
};

// rules 3 - 11 on the device raster Z (De x Dn, ncell >= 1): labels and H stay in `k`, `kept` top rows in k.tops
int delineate(sfmhip_ctx* ctx, Core& k, const Scan& scan, const float* Z, int De, int Dn, const Prep& p, float e_min, float n_min,
              const Points& pts, Result& res, int& kept) {
  hipStream_t st = ctx->stream;
  const int ncell = De * Dn;
  const dim3 gc(blocks(ncell, 256));
  kept = 0;
  k.rounds_up = k.rounds_parent = 0;
  SFM_TRY(k.H.need(2 * (size_t)ncell));
  SFM_TRY(k.root.need((size_t)ncell));
  SFM_TRY(k.flag.need((size_t)ncell));
  SFM_TRY(k.pos.need((size_t)ncell));
  SFM_TRY(k.labels.need((size_t)ncell));
  SFM_TRY(k.cnt.need(sizeof(Counts) / sizeof(unsigned) + BATCH));
  Counts* cnt = (Counts*)k.cnt.p;
  unsigned* moved = k.cnt.p + sizeof(Counts) / sizeof(unsigned);
  const double t0 = sfm_now_ms();
  double t1 = t0, t2 = t0, t3 = t0, t4 = t0;
  auto stamp = [&](double t5) {
    k.ms[0] = t1 - t0, k.ms[1] = t2 - t1, k.ms[2] = t3 - t2, k.ms[3] = t4 - t3, k.ms[4] = t5 - t4, k.ms[5] = t5 - t0;
  };
  SFM_HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(Counts), st));
  // rule 3
  float* Hb[2] = {k.H.p, k.H.p + ncell};
  int cur = 0;
  if (p.smooth_passes == 0) {
    SFM_HIP_TRY(hipMemcpyAsync(Hb[0], Z, sizeof(float) * (size_t)ncell, hipMemcpyDeviceToDevice, st));
  } else {
    CRN_LAUNCH(crn_smooth, gc, Z, De, Dn, Hb[0]);
    for (int s = 1; s < p.smooth_passes; ++s, cur ^= 1) CRN_LAUNCH(crn_smooth, gc, Hb[cur], De, Dn, Hb[cur ^ 1]);
  }
  const float* H = k.Hfin = Hb[cur];
  if (ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t1 = t2 = t3 = t4 = sfm_now_ms();
  // rules 4 - 6, the summit list
  CRN_LAUNCH(crn_up, gc, H, De, Dn, p.min_h, k.root.p, k.flag.p, cnt);
  SFM_TRY(doubling(st, moved, 64, k.rounds_up, [&](unsigned* m) -> int {  // (a chain is shorter than 2^24 < 2^64 cells)
    CRN_LAUNCH(crn_jump, gc, k.root.p, ncell, m);
    return SFMHIP_OK;
  }));
  int ns = 0;
  SFM_TRY(scan(k.flag.p, k.pos.p, (size_t)ncell, &ns));
  res.n_summits = ns;
  if (ns == 0) {  // no canopy cell: every canopy has its greatest cell for a summit
    SFM_HIP_TRY(hipMemsetAsync(k.labels.p, 0xFF, sizeof(int) * (size_t)ncell, st));
    if (pts.n > 0) SFM_HIP_TRY(hipMemsetAsync(pts.tree_of, 0xFF, sizeof(int) * (size_t)pts.n, st));
    SFM_HIP_TRY(hipStreamSynchronize(st));
    t2 = t3 = t4 = sfm_now_ms();
    stamp(t2);
    return SFMHIP_OK;
  }
  res.flags = 0;
  SFM_TRY(k.list.need(5 * (size_t)ns));
  SFM_TRY(k.par.need(2 * (size_t)ns));
  SFM_TRY(k.tops.need((size_t)p.max_trees));
  int *scell = k.list.p, *sR2 = scell + ns, *number = sR2 + ns, *istop = number + ns, *tpos = istop + ns;
  const dim3 gs(blocks(ns, 256));
  CRN_LAUNCH(crn_compact, gc, k.flag.p, k.pos.p, ncell, ns, scell);
  if (ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t2 = t3 = t4 = sfm_now_ms();
  // rules 7, 8: the windows, the summit forest, the numbers
  int2* P[2] = {k.par.p, k.par.p + ns};
  CRN_LAUNCH(crn_window, dim3(blocks(ns, 4)), H, De, Dn, p, scell, ns, k.root.p, k.pos.p, P[0], sR2, istop);
  int pc = 0;
  SFM_TRY(doubling(st, moved, 64, k.rounds_parent, [&](unsigned* m) -> int {
    CRN_LAUNCH(crn_pjump, gs, P[pc], ns, P[pc ^ 1], m);
    pc ^= 1;
    return SFMHIP_OK;
  }));
  int n_trees = 0;
  SFM_TRY(scan(istop, tpos, (size_t)ns, &n_trees));
  res.n_trees = n_trees;
  kept = std::min(n_trees, (int)p.max_trees);
  if (n_trees > p.max_trees) res.flags |= F_OVERFLOW;
  CRN_LAUNCH(crn_tops, gs, scell, istop, tpos, sR2, P[pc], ns, (int)p.max_trees, Z, H, De, e_min, n_min, p.c, number, k.tops.p, cnt);
  if (ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t3 = t4 = sfm_now_ms();
  // rule 9
  CRN_LAUNCH(crn_labels, gc, H, k.root.p, k.pos.p, P[pc], number, scell, De, Dn, ns, kept, p, k.labels.p, k.tops.p, cnt);
  if (ctx->timing) SFM_HIP_TRY(hipStreamSynchronize(st));
  t4 = sfm_now_ms();
  // rules 10, 11
  if (pts.n > 0)
    CRN_LAUNCH(crn_points, dim3(blocks(pts.n, 256)), pts.enh, pts.hag, pts.n, pts.d, p.c, p.ground_clear, k.labels.p, kept, pts.tree_of, k.tops.p, cnt);
  CRN_LAUNCH(crn_area, dim3(blocks(kept, 256)), k.tops.p, kept, p.c);
  Counts c;
  SFM_HIP_TRY(hipMemcpyAsync(&c, cnt, sizeof c, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  res.n_canopy = (int32_t)c.n_canopy, res.n_labelled_cells = (int32_t)c.n_labelled_cells, res.n_labelled = (int32_t)c.n_labelled;
  res.max_depth = (int32_t)c.max_depth;
  stamp(sfm_now_ms());
  return SFMHIP_OK;
}

int fetch_tops(hipStream_t st, const Core& k, int kept, int cap, sfmhip_crown_top* tops) {
  static_assert(sizeof(sfmhip_crown_top) == sizeof(Top), "a struct of the C ABI mirrors the header's");
  const int m = std::min(kept, cap);
  if (m > 0 && tops) SFM_HIP_TRY(hipMemcpyAsync(tops, k.tops.p, sizeof(Top) * (size_t)m, hipMemcpyDeviceToHost, st));
  return SFMHIP_OK;
}

struct CrnState {  // on the cloud handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::CROWNS;
  Core k;
  Grow<int> tree_of;  // n
  bool has_call = false;
  int ncell = 0;
};

struct CtxState {  // on the context, for the raster entry, freed with it
  Core k;
  Grow<float> Z;             // the raster as uploaded
  Grow<unsigned char> tmp;   // the scan's temporary storage
  hipStream_t st = nullptr;
};

int scan_cloud(void* who, const int* in, int* out, size_t n, int* total) { return sfmgrid::scan((sfmhip_cloud*)who, in, out, n, total); }
int scan_ctx(void* who, const int* in, int* out, size_t n, int* total) {
  CtxState* s = (CtxState*)who;
  size_t need = 0;
  SFM_TRY(sfm_scan_bytes(n, s->st, &need));
  SFM_TRY(s->tmp.need(need));
  long long t = 0;
  SFM_TRY(sfm_exclusive_scan(s->tmp.p, s->tmp.cap, in, out, n, s->st, total ? &t : nullptr));
  if (total) *total = (int)t;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_crowns_default_opts(sfmhip_crowns_opts* o) {
  if (!o) return;
  *o = mirror<sfmhip_crowns_opts>(default_opts());
}

extern "C" int sfmhip_chm_crowns(sfmhip_ctx* ctx, const float* chm, int De, int Dn, double c, const sfmhip_crowns_opts* opts, int32_t* labels,
                                 float* smooth, int cap, sfmhip_crown_top* tops, sfmhip_crowns_result* out) {
  if (!ctx || !opts || !out || De < 0 || Dn < 0 || cap < 0) return SFMHIP_ERR_ARG;
  Prep p;
  if (!prepare(mirror<Opts>(*opts), c, p)) return SFMHIP_ERR_ARG;
  if (!((double)De * (double)Dn <= CELL_CAP)) return SFMHIP_ERR_ARG;
  Result res;
  empty_result(res, c, 0.0f, 0.0f, De, Dn);
  const int ncell = De * Dn;
  if (ncell > 0) {
    if (!chm) return SFMHIP_ERR_ARG;
    SFM_HIP_TRY(hipSetDevice(ctx->device));
    if (!ctx->crowns_state) {
      ctx->crowns_state = new CtxState();
      ctx->crowns_state_free = [](void* s) { delete (CtxState*)s; };
    }
    CtxState* s = (CtxState*)ctx->crowns_state;
    hipStream_t st = s->st = ctx->stream;
    SFM_TRY(s->Z.need((size_t)ncell));
    SFM_HIP_TRY(hipMemcpyAsync(s->Z.p, chm, sizeof(float) * (size_t)ncell, hipMemcpyHostToDevice, st));
    int kept = 0;
    SFM_TRY(delineate(ctx, s->k, Scan{scan_ctx, s}, s->Z.p, De, Dn, p, 0.0f, 0.0f, Points(), res, kept));
    if (labels) SFM_HIP_TRY(hipMemcpyAsync(labels, s->k.labels.p, sizeof(int) * (size_t)ncell, hipMemcpyDeviceToHost, st));
    if (smooth) SFM_HIP_TRY(hipMemcpyAsync(smooth, s->k.Hfin, sizeof(float) * (size_t)ncell, hipMemcpyDeviceToHost, st));
    SFM_TRY(fetch_tops(st, s->k, kept, cap, tops));
    SFM_HIP_TRY(hipStreamSynchronize(st));
  }
  *out = mirror<sfmhip_crowns_result>(res);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_crowns(sfmhip_cloud* c, const sfmhip_crowns_opts* opts, int32_t* tree_of, int cap, sfmhip_crown_top* tops,
                                   sfmhip_crowns_result* out) {
  if (!c || !opts || !out || cap < 0) return SFMHIP_ERR_ARG;
  CrnState* s = sfmgrid::stage<CrnState>(c);
  s->has_call = false;
  s->ncell = 0;
  for (double& m : s->k.ms) m = 0;
  sfmterrain::LastCall lc;
  if (!sfmterrain::last_call(c, lc)) return SFMHIP_ERR_ARG;
  Prep p;
  if (!prepare(mirror<Opts>(*opts), lc.c, p)) return SFMHIP_ERR_ARG;
  Result res;
  empty_result(res, lc.c, lc.d.e_min, lc.d.n_min, lc.d.De, lc.d.Dn);
  const int ncell = lc.d.De * lc.d.Dn, n = lc.n;
  if (ncell == 0 || !lc.chm) {  // the terrain call selected nothing
    if (tree_of) std::fill(tree_of, tree_of + std::max(n, 0), -1);
    s->has_call = true;
    *out = mirror<sfmhip_crowns_result>(res);
    return SFMHIP_OK;
  }
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  SFM_TRY(s->tree_of.need((size_t)std::max(n, 1)));
  Points pts;
  pts.enh = lc.enh, pts.hag = lc.hag, pts.n = n, pts.tree_of = s->tree_of.p, pts.d = lc.d;
  int kept = 0;
  SFM_TRY(delineate(c->ctx, s->k, Scan{scan_cloud, c}, lc.chm, lc.d.De, lc.d.Dn, p, lc.d.e_min, lc.d.n_min, pts, res, kept));
  if (tree_of && n > 0) SFM_HIP_TRY(hipMemcpyAsync(tree_of, s->tree_of.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
  SFM_TRY(fetch_tops(st, s->k, kept, cap, tops));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  s->ncell = ncell;
  s->has_call = true;
  *out = mirror<sfmhip_crowns_result>(res);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_crowns_raster(sfmhip_cloud* c, float* smooth, int32_t* labels) {
  if (!c) return SFMHIP_ERR_ARG;
  const CrnState* s = sfmgrid::stage<CrnState>(c);
  if (!s->has_call) return SFMHIP_ERR_ARG;
  if (s->ncell == 0) return SFMHIP_OK;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  if (smooth) SFM_HIP_TRY(hipMemcpyAsync(smooth, s->k.Hfin, sizeof(float) * (size_t)s->ncell, hipMemcpyDeviceToHost, st));
  if (labels) SFM_HIP_TRY(hipMemcpyAsync(labels, s->k.labels.p, sizeof(int) * (size_t)s->ncell, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_crowns_last_timing(sfmhip_cloud* c, double ms6[6]) {
  if (!c || !ms6) return SFMHIP_ERR_ARG;
  const CrnState* s = sfmgrid::stage<CrnState>(c);
  for (int i = 0; i < 6; ++i) ms6[i] = s->k.ms[i];
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_crowns_last_rounds(sfmhip_cloud* c, int32_t rounds2[2]) {
  if (!c || !rounds2) return SFMHIP_ERR_ARG;
  const CrnState* s = sfmgrid::stage<CrnState>(c);
  rounds2[0] = s->k.rounds_up, rounds2[1] = s->k.rounds_parent;
  return SFMHIP_OK;
}
