// register.hip -- two clouds meet: the nearest target point of every source point, ONE ICP loop
// around it behind the four looping entries (sfmhip_cloud_register, its batch, sfmhip_cloud_register_icp, its batch), and the two
// calls that keep the result on the device (transform, concat).  The rules are register.h's and register_icp.h's, which the CPU
// test stubs compile too.
//
// The loop (run_loop) and its iteration (launch_iteration): the search, the rejectors, the sums, the update.  A call is a
// batch of n_init problems, the problem being grid dimension y: problem b owns record b, row b of idx / d2 / kept and slab b of
// the partials; a workgroup whose problem has stopped reads the stop flag and returns, so a stopped problem's row stays the
// pairs under its result.  The host reads the block of records once per iteration and leaves when all have stopped; no
// n-sized array crosses the bus inside the loop.  f-17's entries are the loop with metric 0 and no rejector (f-22 rule 7); what
// the entries keep to themselves is their rule 1, the struct they hand back and which of the state's three timing records the
// call fills.
//
// reg_nearest: a lane per source point; in a single call a source of at least SORT_MIN points is walked in the order of the
// target cells of its images under the call's first transform (reg_keys + the handle's cell_sort, once per call), so that the
// lanes of a wave walk the same rows; results do not depend on the order.  The point is moved by the current transform (read
// from the loop's record on the device), its cell in the TARGET's k-NN grid is cell_of clamped to the grid, and the rings grow
// as in cloud_knn with one best slot.  block_bound stays a lower bound for a point outside the grid's box: it only counts faces
// that have cells beyond them, the clamped cell is the border cell on every axis on which the point is outside, so the face the
// point is beyond is never counted, and the distance to every counted face is taken from the point's own coordinate.  The
// slack adds the point's magnitude, since a source point can lie far from the box the grid's knn_abs_eps was sized for.
//
// The rejectors (f-22 rules 3 - 5) run only when one is active: the plane metric (a target row without a plane), one_to_one or
// trim < 1.  Then the search tracks nothing, the rejectors write a row of kept pairs and raise "changed" themselves, and the sums
// read that row.  Without one the stage is skipped, launches and timing bracket alike: the search tracks "changed" on the idx
// row, the sums read idx, and idx is what the caller gets.  icp_survive: rule 3 and, with one_to_one, an unsigned 64-bit atomicMin
// of (bits(d2) << 32 | i) into the target's slot; icp_unique: a source stays when its slot names it (a loser keeps its target as
// -(j + 2), so icp_keep can clear the slot by a plain store: the slots are all "empty" again after every iteration).  The trim's
// tau: a radix select over the float's bits, four digits of 8, a 256-bin integer histogram per digit (LDS atomics, then one
// global atomicAdd per occupied bin: exact whatever the order) and one wave that finds the digit.  icp_keep writes the kept row,
// raises "changed" and records tau.
//
// The sums: 256 source points per workgroup through block_tree (reg_sums1 / reg_sums2, metric 0) or its unrolled form
// (icp_plane_sums, metric 1); reg_means, reg_update and icp_plane_update (one wave each) fold the partials in ascending block order,
// a lane per sum (fold_partials); lane 0 then takes the step's decision (loop_step / plane_loop_step) and writes the next
// transform.  No spins, no hand-offs between workgroups, no float atomics: the "pairs changed" flag is a plain store of 1.
#include "common.h"
#include "cloud.h"
#include "cloud_grid.h"
#include "block_sum.h"
#include "register_icp.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace sfmgrid;
using sfmreg::Loop;
using sfmreg::N1;
using sfmreg::N2;
using sfmreg::Opts;
using sfmreg::Result;
using sfmreg::Transform;

namespace {

constexpr int SUM_BLOCK = sfmsum::CHUNK;  // rule 4's block: 256 source points, one workgroup
constexpr int NEAR_BLOCK = 128;
constexpr int SORT_MIN = 8192;  // sources of at least this many points are searched in the order of the target's cells

struct DevLoop {  // the loop's record on the device
  Loop L;
  int32_t changed, pad;
  double s1[N1], mu_p[3], mu_m[3];
};

struct Sel {  // the trim's select of one problem
  uint32_t prefix, k, n;
  float tau;
};
struct Centre {
  double c[3];
};
struct Timing {  // host-clock ms of a call's stages (search, rejectors, sums, update) and the iterations of its longest problem
  double ms[4] = {0, 0, 0, 0};
  int iterations = 0;
};

struct RegState {  // the one state of the loop, on the TARGET handle, freed with it
  static constexpr sfmgrid::Stage slot = sfmgrid::REGISTER;
  Grow<int> idx, kin, kout, vin, order;
  Grow<float> d2;
  Grow<double> part1, part2;
  Grow<DevLoop> rec;
  // f-22's, each sized only by a call that asks for its feature: the rejectors' rows, one_to_one's slots, the trim's select, the
  // plane metric's partials and normals
  Grow<int> cand, kept;
  Grow<sfmreg::IcpExtra> extra;
  Grow<unsigned long long> slots;
  Grow<uint32_t> hist;
  Grow<Sel> sel;
  Grow<double> part;
  Grow<float> normals;
  Timing single, batch, icp;  // of the last sfmhip_cloud_register, of the last _batch, of the last _icp / _icp_batch
};

// lane k < Q: sum k of the n_blocks partials in ascending block order into s[k]; every lane may read s afterwards
template <int Q>
__device__ __forceinline__ void fold_partials(const double* part, int n_blocks, double* s) {
  const int k = threadIdx.x;
  if (k < Q) {
    double a = 0.0;
    for (int b = 0; b < n_blocks; ++b) a = a + part[(size_t)b * Q + k];
    s[k] = a;
  }
  __syncthreads();
}
// lane k < Q stores its workgroup's partial of sum k from the four wave sums the block's tree left in sh, by the tree's own
// pairing: what block_tree hands every lane as v[k], read where it lies (picking v[k] by the lane would index the register array)
template <int Q>
__device__ __forceinline__ void store_partial(const double (*sh)[4], double* part) {
  const int k = threadIdx.x;
  if (k < Q) part[(size_t)blockIdx.x * Q + k] = (sh[k][0] + sh[k][1]) + (sh[k][2] + sh[k][3]);
}

__device__ __forceinline__ void scan_best(const GridDev& g, int row, int xa, int xb, const float4& q, float& bd, int& bi) {
  int s, e;
  row_span(g, row, xa, xb, &s, &e);
  for (int j = s; j < e; ++j) {
    const float4 t = g.pts[j];
    const float dd = sfmcloud::dist2(q.x, q.y, q.z, t.x, t.y, t.z);
    const int ti = __float_as_int(t.w);
    if (sfmcloud::knn_less(dd, ti, bd, bi)) bd = dd, bi = ti;
  }
}

// the target cell of every source point's image (a point without one: `invalid`, behind every cell) and its index: what
// the handle's cell_sort turns into the order reg_nearest walks the source in, so that the lanes of a wave walk the same rows
__global__ void reg_keys(GridDev g, const float* src, int n_src, const Transform* Tp, int invalid, int* keys, int* vals) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_src) return;
  const Transform T = *Tp;
  float q[3];
  int key = invalid;
  if (sfmreg::move(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], q))
    key = (cell_of((double)q[2], g.o[2], g.cell, g.D[2]) * g.D[1] + cell_of((double)q[1], g.o[1], g.cell, g.D[1])) * g.D[0] +
          cell_of((double)q[0], g.o[0], g.cell, g.D[0]);
  keys[i] = key;
  vals[i] = i;
}

// rules 2 + 3 for problem blockIdx.y.  order: NULL, or the source index of every lane (results do not depend on it).  rec: the
// records, one per problem; the transform is the record's (the loop's, or the one sfmhip_cloud_nearest uploaded into it), and
// a problem whose record says "stopped" is left as it is.  row: the length of a problem's row of idx / d2.  exact: search
// until the nearest is known also beyond md2 (sfmhip_cloud_nearest: a rejected pair keeps its d2); else a lane with nothing
// within md2 in reach leaves once the bound exceeds max_dist.  track: raise the record's "changed" when an index differs from
// the row's old entry.
__global__ __launch_bounds__(NEAR_BLOCK) void reg_nearest(GridDev g, double abs_eps, const float* src, int n_src, const int* order,
                                                         DevLoop* rec, size_t row, float md2, int exact, int* idx, float* d2, int track) {
  const int l = blockIdx.x * NEAR_BLOCK + threadIdx.x;
  rec += blockIdx.y;
  if (l >= n_src || rec->L.stop) return;
  idx += row * blockIdx.y, d2 += row * blockIdx.y;
  int32_t* changed = track ? &rec->changed : nullptr;
  const int i = order ? order[l] : l;
  const Transform T = rec->L.T;
  float qv[3];
  const bool ok = sfmreg::move(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], qv);
  float bd = sfmcloud::bits_f(0x7F800000u);
  int bi = INT_MAX;
  if (ok && g.n_valid > 0) {
    const float4 q = make_float4(qv[0], qv[1], qv[2], 0.0f);
    const int c[3] = {cell_of((double)q.x, g.o[0], g.cell, g.D[0]), cell_of((double)q.y, g.o[1], g.cell, g.D[1]),
                      cell_of((double)q.z, g.o[2], g.cell, g.D[2])};
    const double eps = abs_eps + 1e-12 * ((fabs((double)q.x) + fabs((double)q.y)) + fabs((double)q.z));
    for (int R = 0;; ++R) {
      for (int z = max(c[2] - R, 0); z <= min(c[2] + R, g.D[2] - 1); ++z)
        for (int y = max(c[1] - R, 0); y <= min(c[1] + R, g.D[1] - 1); ++y) {
          const int row = (z * g.D[1] + y) * g.D[0];
          if (abs(z - c[2]) == R || abs(y - c[1]) == R) {
            scan_best(g, row, max(c[0] - R, 0), min(c[0] + R, g.D[0] - 1), q, bd, bi);
          } else {
            if (c[0] - R >= 0) scan_best(g, row, c[0] - R, c[0] - R, q, bd, bi);
            if (c[0] + R <= g.D[0] - 1) scan_best(g, row, c[0] + R, c[0] + R, q, bd, bi);
          }
        }
      const double b = block_bound(g, q, c, R);
      if (b == INFINITY) break;  // the block covers the grid
      const double bs = b * (1.0 - 1.0 / 65536.0) - eps;
      if (bs > 0.0) {
        if (bi != INT_MAX && bs * bs > (double)bd) break;  // every unsearched point is strictly farther than the best
        if (!exact && bs * bs > (double)md2) break;        // ... or than max_dist
      }
    }
  }
  const bool got = bi != INT_MAX;
  const int out = got && sfmreg::keep(bd, md2) ? bi : -1;
  if (changed && idx[i] != out) *changed = 1;
  idx[i] = out;
  d2[i] = got ? bd : sfmcloud::bits_f(0x7F800000u);
}

__device__ __forceinline__ bool load_pair(const float* src, const float* tgt, const int* idx, int i, int n_src, float p[3], float m[3]) {
  bool paired = false;
  for (int a = 0; a < 3; ++a) p[a] = m[a] = 0.0f;
  if (i < n_src) {
    const int j = idx[i];
    paired = j >= 0;
    for (int a = 0; a < 3; ++a) p[a] = src[3 * (size_t)i + a];
    if (paired)
      for (int a = 0; a < 3; ++a) m[a] = tgt[3 * (size_t)j + a];
  }
  return paired;
}

__global__ __launch_bounds__(SUM_BLOCK) void reg_sums1(const float* src, const float* tgt, const int* idx, int n_src, const DevLoop* rec,
                                                      size_t row, double* part) {
  __shared__ double sh[N1][4];
  if (rec[blockIdx.y].L.stop) return;  // (uniform over the workgroup)
  idx += row * blockIdx.y, part += (size_t)gridDim.x * N1 * blockIdx.y;
  const int i = blockIdx.x * SUM_BLOCK + threadIdx.x;
  float p[3], m[3];
  const bool paired = load_pair(src, tgt, idx, i, n_src, p, m);
  double v[N1];
  sfmreg::terms1(paired, p, m, v);
  sfmsum::block_tree<N1>(v, sh);
  store_partial<N1>(sh, part);
}

// the partials of pass 1 in ascending block order, a lane per sum; then the means
__global__ __launch_bounds__(64) void reg_means(const double* part, int n_blocks, DevLoop* rec) {
  rec += blockIdx.x, part += (size_t)n_blocks * N1 * blockIdx.x;
  if (rec->L.stop) return;
  fold_partials<N1>(part, n_blocks, rec->s1);
  if (threadIdx.x == 0) sfmreg::means(rec->s1, rec->mu_p, rec->mu_m);
}

__global__ __launch_bounds__(SUM_BLOCK) void reg_sums2(const float* src, const float* tgt, const int* idx, const float* d2, int n_src,
                                                      const DevLoop* rec, size_t row, double* part) {
  __shared__ double sh[N2][4];
  rec += blockIdx.y;
  if (rec->L.stop) return;  // (uniform over the workgroup)
  idx += row * blockIdx.y, d2 += row * blockIdx.y, part += (size_t)gridDim.x * N2 * blockIdx.y;
  const int i = blockIdx.x * SUM_BLOCK + threadIdx.x;
  float p[3], m[3];
  const bool paired = load_pair(src, tgt, idx, i, n_src, p, m);
  double mu_p[3], mu_m[3];
  for (int a = 0; a < 3; ++a) mu_p[a] = rec->mu_p[a], mu_m[a] = rec->mu_m[a];
  double v[N2];
  sfmreg::terms2(paired, p, m, paired ? d2[i] : 0.0f, mu_p, mu_m, v);
  sfmsum::block_tree<N2>(v, sh);
  store_partial<N2>(sh, part);
}

// pass 2's partials folded as pass 1's, then rule 6's step on lane 0: the stop decision or the next transform
__global__ __launch_bounds__(64) void reg_update(const double* part, int n_blocks, Opts o, DevLoop* rec) {
  __shared__ double s2[N2];
  rec += blockIdx.x, part += (size_t)n_blocks * N2 * blockIdx.x;
  if (rec->L.stop) return;
  fold_partials<N2>(part, n_blocks, s2);
  if (threadIdx.x == 0) {
    double t2[N2];
    for (int q = 0; q < N2; ++q) t2[q] = s2[q];
    sfmreg::loop_step(rec->L, o, rec->changed != 0, rec->s1, t2);
    rec->changed = 0;
  }
}

__global__ void reg_transform(const float* xyz, int n, Transform T, float* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * (size_t)i], y = xyz[3 * (size_t)i + 1], z = xyz[3 * (size_t)i + 2];
  float q[3];
  sfmreg::move(T, x, y, z, q);
  const bool f = sfmcloud::finite3(x, y, z);  // rule 8: a non-finite point stays as it is
  out[3 * (size_t)i] = f ? q[0] : x;
  out[3 * (size_t)i + 1] = f ? q[1] : y;
  out[3 * (size_t)i + 2] = f ? q[2] : z;
}

int prepare(sfmhip_cloud* tgt, sfmhip_cloud* src, RegState** state, int n_init = 1) {
  SFM_HIP_TRY(hipSetDevice(tgt->ctx->device));
  RegState* s = stage<RegState>(tgt);
  const size_t n1 = (size_t)std::max(src->n, 1), nb = blocks(n1, SUM_BLOCK), B = (size_t)n_init;
  SFM_TRY(s->idx.need(B * n1));
  SFM_TRY(s->d2.need(B * n1));
  SFM_TRY(s->part1.need(B * nb * N1));
  SFM_TRY(s->part2.need(B * nb * N2));
  SFM_TRY(s->rec.need(B));
  if (tgt->n_valid > 0) SFM_TRY(knn_grid(tgt));
  *state = s;
  return SFMHIP_OK;
}

// the source's order by target cell under the transform at d_T (once per call: the loop moves the points little); *order
// stays NULL for a small source or a target without a finite point
int sort_source(sfmhip_cloud* tgt, sfmhip_cloud* src, RegState* s, const Transform* d_T, const int** order) {
  *order = nullptr;
  const int n = src->n;
  if (n < SORT_MIN || tgt->n_valid == 0) return SFMHIP_OK;
  SFM_TRY(s->kin.need(n));
  SFM_TRY(s->kout.need(n));
  SFM_TRY(s->vin.need(n));
  SFM_TRY(s->order.need(n));
  const long long ncell = tgt->kg.ncell;
  hipLaunchKernelGGL(reg_keys, dim3(blocks(n, 256)), dim3(256), 0, tgt->ctx->stream, tgt->kg.dev(tgt->n_valid), src->xyz, n, d_T, (int)ncell,
                     s->kin.p, s->vin.p);
  SFM_HIP_TRY(hipGetLastError());
  SFM_TRY(cell_sort(tgt, ncell, s->kin.p, s->kout.p, s->vin.p, s->order.p, n));
  *order = s->order.p;
  return SFMHIP_OK;
}

void launch_nearest(sfmhip_cloud* tgt, sfmhip_cloud* src, RegState* s, const int* order, float md2, bool exact, bool track, int n_init = 1) {
  if (src->n == 0) return;
  GridDev g = tgt->kg.dev(tgt->n_valid);  // (never dereferenced without a finite target point)
  const double eps = tgt->n_valid > 0 ? knn_abs_eps(tgt) : 0.0;
  hipLaunchKernelGGL(reg_nearest, dim3(blocks(src->n, NEAR_BLOCK), n_init), dim3(NEAR_BLOCK), 0, tgt->ctx->stream, g, eps, src->xyz, src->n,
                     order, s->rec.p, (size_t)src->n, md2, exact ? 1 : 0, s->idx.p, s->d2.p, track ? 1 : 0);
}

// ---------------------------------------------------------------- f-22: the rejectors and the point-to-plane step
__global__ __launch_bounds__(256) void icp_survive(const int* idx, const float* d2, const float* normals, int stride, int metric, int one_to_one,
                                                   int n_src, int n_tgt, const DevLoop* rec, size_t row, int* cand, unsigned long long* slot) {
  if (rec[blockIdx.y].L.stop) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_src) return;
  idx += row * blockIdx.y, d2 += row * blockIdx.y, cand += row * blockIdx.y;
  int j = idx[i];
  if (j >= 0 && metric == sfmreg::METRIC_PLANE) {
    const float* n = normals + (size_t)stride * j;
    if (!sfmreg::has_plane(n[0], n[1], n[2])) j = -1;
  }
  cand[i] = j;
  if (one_to_one && j >= 0) atomicMin(&slot[(size_t)n_tgt * blockIdx.y + j], (unsigned long long)sfmreg::slot_of(d2[i], i));
}

__global__ __launch_bounds__(256) void icp_unique(int n_src, int n_tgt, const DevLoop* rec, size_t row, int* cand, const unsigned long long* slot) {
  if (rec[blockIdx.y].L.stop) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_src) return;
  cand += row * blockIdx.y;
  const int j = cand[i];
  if (j >= 0 && sfmreg::slot_source(slot[(size_t)n_tgt * blockIdx.y + j]) != i) cand[i] = sfmreg::lost(j);
}

// digit `pass` (0: the top 8 bits) of the survivors whose higher digits equal the select's prefix
__global__ __launch_bounds__(256) void icp_hist(const int* cand, const float* d2, int n_src, const DevLoop* rec, size_t row, const Sel* sel, int pass,
                                                uint32_t* hist) {
  __shared__ uint32_t bins[256];
  if (rec[blockIdx.y].L.stop) return;  // (uniform over the workgroup)
  cand += row * blockIdx.y, d2 += row * blockIdx.y, hist += ((size_t)blockIdx.y * 4 + pass) * 256;
  bins[threadIdx.x] = 0;
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_src && cand[i] >= 0) {
    const uint32_t b = sfmreg::d2_bits(d2[i]);
    const int low = 32 - 8 * pass;  // the bits below the digits already fixed
    const bool match = pass == 0 || (b >> low) == (sel[blockIdx.y].prefix >> low);
    if (match) atomicAdd(&bins[(b >> (24 - 8 * pass)) & 255u], 1u);
  }
  __syncthreads();
  if (bins[threadIdx.x]) atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}

// one wave per problem: the bin in which the k-th smallest lies; lane l holds bins 4 l .. 4 l + 3
__global__ __launch_bounds__(64) void icp_pick(const uint32_t* hist, int pass, double trim, const DevLoop* rec, Sel* sel) {
  if (rec[blockIdx.x].L.stop) return;
  hist += ((size_t)blockIdx.x * 4 + pass) * 256;
  sel += blockIdx.x;
  const int l = threadIdx.x;
  uint32_t c[4], sum = 0;
  for (int q = 0; q < 4; ++q) c[q] = hist[4 * l + q], sum += c[q];
  uint32_t incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t up = __shfl_up(incl, off);
    if (l >= off) incl += up;
  }
  const uint32_t total = __shfl(incl, 63);
  const uint32_t n = pass == 0 ? total : sel->n;
  if (n == 0) {  // rule 5 without a survivor: nothing to trim
    if (pass == 0 && l == 0) sel->prefix = 0, sel->k = 0, sel->n = 0, sel->tau = sfmreg::inf_f();
    return;
  }
  const uint32_t k = pass == 0 ? sfmreg::trim_count(trim, n) : sel->k;
  const uint32_t prefix = pass == 0 ? 0u : sel->prefix;
  uint32_t cum = incl - sum;
  if (cum < k && k <= incl) {  // (one lane: 1 <= k <= total)
    int digit = 4 * l + 3;
    bool found = false;
    for (int q = 0; q < 4; ++q) {
      if (found) continue;
      if (k <= cum + c[q]) digit = 4 * l + q, found = true;
      else cum += c[q];
    }
    const uint32_t p = prefix | ((uint32_t)digit << (24 - 8 * pass));
    sel->prefix = p, sel->k = k - cum, sel->n = n;
    if (pass == 3) sel->tau = sfmcloud::bits_f(p);
  }
}

// rule 5's cut and rule 6's row: kept[i] is the pair of source i or -1; a slot that was written goes back to "empty"
__global__ __launch_bounds__(256) void icp_keep(const int* cand, const float* d2, int n_src, int n_tgt, DevLoop* rec, size_t row, const Sel* sel,
                                                int one_to_one, unsigned long long* slot, int* kept, sfmreg::IcpExtra* extra) {
  rec += blockIdx.y;
  if (rec->L.stop) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_src) return;
  cand += row * blockIdx.y, d2 += row * blockIdx.y, kept += row * blockIdx.y;
  const float tau = sel ? sel[blockIdx.y].tau : sfmreg::inf_f();
  const int c = cand[i];
  const int out = c >= 0 && d2[i] <= tau ? c : -1;
  if (kept[i] != out) rec->changed = 1;
  kept[i] = out;
  if (one_to_one) {
    const int j = c >= 0 ? c : c <= -2 ? sfmreg::lost_target(c) : -1;
    if (j >= 0) slot[(size_t)n_tgt * blockIdx.y + j] = sfmreg::SLOT_EMPTY;
  }
  if (i == 0) extra[blockIdx.y].trim_d2 = (double)tau;
}

// rule 8's one pass: 256 source points per workgroup, NP sums through block_tree
__global__ __launch_bounds__(SUM_BLOCK) void icp_plane_sums(const float* src, const float* tgt, const float* normals, int stride, const int* kept,
                                                           const float* d2, int n_src, const DevLoop* rec, size_t row, Centre ctr, int with_scale,
                                                           double* part) {
  constexpr int NP = sfmreg::NP;
  __shared__ double sh[NP][4];
  rec += blockIdx.y;
  if (rec->L.stop) return;  // (uniform over the workgroup)
  kept += row * blockIdx.y, d2 += row * blockIdx.y, part += (size_t)gridDim.x * NP * blockIdx.y;
  const int i = blockIdx.x * SUM_BLOCK + threadIdx.x;
  float q[3] = {0.0f, 0.0f, 0.0f}, m[3] = {0.0f, 0.0f, 0.0f}, n[3] = {0.0f, 0.0f, 0.0f}, dd = 0.0f;
  bool on = false;
  if (i < n_src) {
    const int j = kept[i];
    on = j >= 0;
    if (on) {
      const Transform T = rec->L.T;
      sfmreg::move(T, src[3 * (size_t)i], src[3 * (size_t)i + 1], src[3 * (size_t)i + 2], q);
      for (int a = 0; a < 3; ++a) m[a] = tgt[3 * (size_t)j + a], n[a] = normals[(size_t)stride * j + a];
      dd = d2[i];
    }
  }
  double v[NP];
  sfmreg::plane_terms(on, q, m, n, dd, ctr.c, with_scale, v);
  // block_sum.h's block_tree, unrolled (NP sums stay in registers): the same butterfly, the same pairing
#pragma unroll
  for (int k = 0; k < NP; ++k) {
    double x = v[k];
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_xor(x, off);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  store_partial<NP>(sh, part);
}

// the partials in ascending block order, a lane per sum; then rule 9's step on lane 0
__global__ __launch_bounds__(64) void icp_plane_update(const double* part, int n_blocks, sfmreg::IcpOpts o, Centre ctr, DevLoop* rec,
                                                       sfmreg::IcpExtra* extra) {
  constexpr int NP = sfmreg::NP;
  __shared__ double s[NP];
  rec += blockIdx.x, part += (size_t)n_blocks * NP * blockIdx.x;
  if (rec->L.stop) return;
  fold_partials<NP>(part, n_blocks, s);
  if (threadIdx.x == 0) {
    double t[NP];
    for (int q = 0; q < NP; ++q) t[q] = s[q];
    sfmreg::plane_loop_step(rec->L, extra[blockIdx.x], o, ctr.c, t);
    rec->changed = 0;
  }
}

// one iteration for n_init problems: the search, the rejectors when one is active (else skipped, and the search tracks the idx
// row itself), the sums and the update of the metric.  t (nullable): host-clock ms added to search / rejectors / sums / update, a
// stream synchronisation after every stage that ran; else the launches only
int launch_iteration(sfmhip_cloud* tgt, sfmhip_cloud* src, RegState* s, const int* order, const sfmreg::IcpOpts& o, float md2, const Centre& ctr,
                     bool reject, int n_init, double* t) {
  hipStream_t st = tgt->ctx->stream;
  const int n = src->n, nb = (int)blocks(n, SUM_BLOCK), nt = tgt->n;
  const size_t row = (size_t)n;
  DevLoop* rec = s->rec.p;
  const int* pairs = reject ? s->kept.p : s->idx.p;  // the row the sums read
  const bool trim = o.trim < 1.0;
  double t0 = 0, t1 = 0, t2 = 0, t3 = 0;
  if (t) t0 = sfm_now_ms();
  launch_nearest(tgt, src, s, order, md2, false, !reject, n_init);
  SFM_HIP_TRY(hipGetLastError());
  if (t) {
    SFM_HIP_TRY(hipStreamSynchronize(st));
    t2 = t1 = sfm_now_ms();
  }
  if (reject) {
    if (nb > 0) {
      const dim3 grid(nb, n_init);
      hipLaunchKernelGGL(icp_survive, grid, dim3(256), 0, st, s->idx.p, s->d2.p, s->normals.p, o.normal_stride, o.metric, o.one_to_one, n, nt, rec,
                         row, s->cand.p, s->slots.p);
      if (o.one_to_one) hipLaunchKernelGGL(icp_unique, grid, dim3(256), 0, st, n, nt, rec, row, s->cand.p, s->slots.p);
      if (trim) {
        SFM_HIP_TRY(hipMemsetAsync(s->hist.p, 0, sizeof(uint32_t) * 1024 * (size_t)n_init, st));
        for (int pass = 0; pass < 4; ++pass) {
          hipLaunchKernelGGL(icp_hist, grid, dim3(256), 0, st, s->cand.p, s->d2.p, n, rec, row, s->sel.p, pass, s->hist.p);
          hipLaunchKernelGGL(icp_pick, dim3(n_init), dim3(64), 0, st, s->hist.p, pass, o.trim, rec, s->sel.p);
        }
      }
      hipLaunchKernelGGL(icp_keep, grid, dim3(256), 0, st, s->cand.p, s->d2.p, n, nt, rec, row, trim ? s->sel.p : nullptr, o.one_to_one, s->slots.p,
                         s->kept.p, s->extra.p);
    }
    SFM_HIP_TRY(hipGetLastError());
    if (t) {
      SFM_HIP_TRY(hipStreamSynchronize(st));
      t2 = sfm_now_ms();
    }
  }
  if (o.metric == sfmreg::METRIC_POINT) {
    if (nb > 0) hipLaunchKernelGGL(reg_sums1, dim3(nb, n_init), dim3(SUM_BLOCK), 0, st, src->xyz, tgt->xyz, pairs, n, rec, row, s->part1.p);
    hipLaunchKernelGGL(reg_means, dim3(n_init), dim3(64), 0, st, s->part1.p, nb, rec);
    if (nb > 0) hipLaunchKernelGGL(reg_sums2, dim3(nb, n_init), dim3(SUM_BLOCK), 0, st, src->xyz, tgt->xyz, pairs, s->d2.p, n, rec, row, s->part2.p);
  } else if (nb > 0) {
    hipLaunchKernelGGL(icp_plane_sums, dim3(nb, n_init), dim3(SUM_BLOCK), 0, st, src->xyz, tgt->xyz, s->normals.p, o.normal_stride, pairs, s->d2.p, n,
                       rec, row, ctr, o.with_scale, s->part.p);
  }
  SFM_HIP_TRY(hipGetLastError());
  if (t) {
    SFM_HIP_TRY(hipStreamSynchronize(st));
    t3 = sfm_now_ms();
  }
  if (o.metric == sfmreg::METRIC_POINT) hipLaunchKernelGGL(reg_update, dim3(n_init), dim3(64), 0, st, s->part2.p, nb, sfmreg::point_opts(o), rec);
  else hipLaunchKernelGGL(icp_plane_update, dim3(n_init), dim3(64), 0, st, s->part.p, nb, o, ctr, rec, s->extra.p);
  SFM_HIP_TRY(hipGetLastError());
  if (t) t[0] += t1 - t0, t[1] += t2 - t1, t[2] += t3 - t2, t[3] -= t3;  // (the caller adds the clock after the record's read)
  return SFMHIP_OK;
}

struct Sink {  // where a call's outcome goes
  Timing RegState::*clock;           // which of the state's timing records the call fills
  int32_t* idx;                      // n_init rows of the pairs under the results (nullable)
  std::vector<sfmreg::IcpResult> res;  // one per start
};

// the one loop: n_init starts in lock step (cell_order: the source walked in the order of the target's cells under the first
// start -- the single calls; a batch would need a sort per start, and results do not depend on it).  The entries have applied
// their rule 1
int run_loop(sfmhip_cloud* tgt, sfmhip_cloud* src, const float* normals, const sfmreg::IcpOpts& o, const Transform* inits, int n_init,
             bool cell_order, Sink& sink) {
  RegState* s = nullptr;
  SFM_TRY(prepare(tgt, src, &s, n_init));
  hipStream_t st = tgt->ctx->stream;
  const bool timing = tgt->ctx->timing;
  const int n = src->n;
  const size_t n1 = (size_t)std::max(n, 1), nt1 = (size_t)std::max(tgt->n, 1), B = (size_t)n_init, nb = blocks(n1, SUM_BLOCK);
  const bool plane = o.metric == sfmreg::METRIC_PLANE, trim = o.trim < 1.0, reject = plane || trim || o.one_to_one != 0;
  if (reject) {
    SFM_TRY(s->cand.need(B * n1));
    SFM_TRY(s->kept.need(B * n1));
    SFM_TRY(s->extra.need(B));
  }
  if (o.one_to_one) {
    SFM_TRY(s->slots.need(B * nt1));
    SFM_HIP_TRY(hipMemsetAsync(s->slots.p, 0xFF, sizeof(unsigned long long) * B * nt1, st));
  }
  if (trim) {
    SFM_TRY(s->hist.need(B * 1024));
    SFM_TRY(s->sel.need(B));
  }
  if (plane) {
    SFM_TRY(s->part.need(B * nb * sfmreg::NP));
    SFM_TRY(s->normals.need(nt1 * (size_t)o.normal_stride));
    if (tgt->n > 0)  // rule 3: once per call
      SFM_HIP_TRY(hipMemcpyAsync(s->normals.p, normals, sizeof(float) * (size_t)tgt->n * o.normal_stride, hipMemcpyHostToDevice, st));
  }
  Centre ctr;
  sfmreg::box_centre(tgt->n_valid, tgt->lo, tgt->hi, ctr.c);
  const float md2 = sfmreg::max_d2(o.max_dist);
  Timing& clock = s->*sink.clock;
  clock = Timing();
  std::vector<DevLoop> h(B);
  std::vector<sfmreg::IcpExtra> ex(B);
  memset(h.data(), 0, sizeof(DevLoop) * B);
  for (size_t b = 0; b < B; ++b) sfmreg::loop_init(h[b].L, inits[b]), ex[b].plane_mse = sfmreg::qnan_d(), ex[b].trim_d2 = sfmreg::inf_d();
  DevLoop* rec = s->rec.p;
  int* pairs = reject ? s->kept.p : s->idx.p;  // the row under the results
  SFM_HIP_TRY(hipMemcpyAsync(rec, h.data(), sizeof(DevLoop) * B, hipMemcpyHostToDevice, st));
  if (reject) SFM_HIP_TRY(hipMemcpyAsync(s->extra.p, ex.data(), sizeof(sfmreg::IcpExtra) * B, hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(pairs, 0xFE, sizeof(int) * B * n1, st));  // (no index: C_0 differs from it)
  const int* order = nullptr;
  if (cell_order) {
    const double ts = timing ? sfm_now_ms() : 0.0;
    SFM_TRY(sort_source(tgt, src, s, &rec->L.T, &order));
    if (timing) {
      SFM_HIP_TRY(hipStreamSynchronize(st));
      clock.ms[0] = sfm_now_ms() - ts;  // (the source's cell order counts as search)
    }
  }
  for (int round = 0;; ++round) {
    SFM_TRY(launch_iteration(tgt, src, s, order, o, md2, ctr, reject, n_init, timing ? clock.ms : nullptr));
    SFM_HIP_TRY(hipMemcpyAsync(h.data(), rec, sizeof(DevLoop) * B, hipMemcpyDeviceToHost, st));  // the block of records, once
    SFM_HIP_TRY(hipStreamSynchronize(st));
    if (timing) clock.ms[3] += sfm_now_ms();
    bool all = true;
    for (size_t b = 0; b < B; ++b) {
      if (h[b].L.k < 0 || h[b].L.k > o.max_iters) return SFMHIP_ERR_STATE;
      all = all && h[b].L.stop;
    }
    if (all) break;
    if (round >= o.max_iters) return SFMHIP_ERR_STATE;  // (a problem stops at k == max_iters at the latest)
  }
  if (reject) SFM_HIP_TRY(hipMemcpyAsync(ex.data(), s->extra.p, sizeof(sfmreg::IcpExtra) * B, hipMemcpyDeviceToHost, st));
  if (sink.idx && n > 0)  // (n > 0: the rows are n apart on the device too)
    SFM_HIP_TRY(hipMemcpyAsync(sink.idx, pairs, sizeof(int) * B * (size_t)n, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  sink.res.resize(B);
  for (size_t b = 0; b < B; ++b) {
    sink.res[b] = sfmreg::icp_result(h[b].L.res, ex[b]);
    clock.iterations = std::max(clock.iterations, (int)h[b].L.res.iterations);
  }
  return SFMHIP_OK;
}

int report(sfmhip_cloud* tgt, Timing RegState::*clock, bool rejectors, double* ms, int32_t* iterations) {
  if (!tgt || !ms) return SFMHIP_ERR_ARG;
  const Timing& t = stage<RegState>(tgt)->*clock;
  for (int i = 0; i < 4; ++i)
    if (rejectors || i != 1) *ms++ = t.ms[i];  // (f-17's calls report three stages: they run no rejector)
  if (iterations) *iterations = t.iterations;
  return SFMHIP_OK;
}

}  // namespace

extern "C" void sfmhip_icp_default_opts(sfmhip_icp_opts* o) {
  if (o) *o = mirror<sfmhip_icp_opts>(sfmreg::default_icp_opts());
}

extern "C" int sfmhip_cloud_register_icp(sfmhip_cloud* tgt, sfmhip_cloud* src, const float* target_normals, const sfmhip_icp_opts* opts,
                                         const sfmhip_transform* init, sfmhip_icp_result* out, int32_t* idx) {
  if (!tgt || !src || !out || tgt->ctx != src->ctx) return SFMHIP_ERR_ARG;
  const sfmreg::IcpOpts o = opts ? mirror<sfmreg::IcpOpts>(*opts) : sfmreg::default_icp_opts();
  const Transform T0 = init ? mirror<Transform>(*init) : sfmreg::identity();
  if (!sfmreg::valid_icp_batch(o, target_normals != nullptr, &T0, 1)) return SFMHIP_ERR_ARG;
  Sink sink{&RegState::icp, idx};
  SFM_TRY(run_loop(tgt, src, target_normals, o, &T0, 1, true, sink));
  *out = mirror<sfmhip_icp_result>(sink.res[0]);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_register_icp_batch(sfmhip_cloud* tgt, sfmhip_cloud* src, const float* target_normals, const sfmhip_icp_opts* opts,
                                               const sfmhip_transform* inits, int n_init, sfmhip_icp_result* out, int32_t* idx) {
  if (!tgt || !src || !out || !inits || tgt->ctx != src->ctx) return SFMHIP_ERR_ARG;
  const sfmreg::IcpOpts o = opts ? mirror<sfmreg::IcpOpts>(*opts) : sfmreg::default_icp_opts();
  static_assert(sizeof(sfmhip_transform) == sizeof(Transform), "the C ABI mirrors register.h");
  if (!sfmreg::valid_icp_batch(o, target_normals != nullptr, (const Transform*)inits, n_init)) return SFMHIP_ERR_ARG;
  Sink sink{&RegState::icp, idx};
  SFM_TRY(run_loop(tgt, src, target_normals, o, (const Transform*)inits, n_init, false, sink));
  for (int b = 0; b < n_init; ++b) out[b] = mirror<sfmhip_icp_result>(sink.res[b]);
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_register_icp_last_timing(sfmhip_cloud* tgt, double ms4[4], int32_t* iterations) {
  return report(tgt, &RegState::icp, true, ms4, iterations);
}

extern "C" void sfmhip_register_default_opts(sfmhip_register_opts* o) {
  if (o) *o = mirror<sfmhip_register_opts>(sfmreg::default_opts());
}

extern "C" int sfmhip_cloud_nearest(sfmhip_cloud* tgt, sfmhip_cloud* src, const sfmhip_transform* T, double max_dist, int32_t* idx, float* d2) {
  if (!tgt || !src || tgt->ctx != src->ctx || !sfmreg::valid_max_dist(max_dist) || (src->n > 0 && (!idx || !d2))) return SFMHIP_ERR_ARG;
  const Transform T0 = T ? mirror<Transform>(*T) : sfmreg::identity();
  if (!sfmreg::valid_transform(T0)) return SFMHIP_ERR_ARG;
  if (src->n == 0) return SFMHIP_OK;
  RegState* s = nullptr;
  SFM_TRY(prepare(tgt, src, &s));
  hipStream_t st = tgt->ctx->stream;
  Loop L;
  sfmreg::loop_init(L, T0);
  SFM_HIP_TRY(hipMemcpyAsync(&s->rec.p->L, &L, sizeof L, hipMemcpyHostToDevice, st));
  const int* order = nullptr;
  SFM_TRY(sort_source(tgt, src, s, &s->rec.p->L.T, &order));
  launch_nearest(tgt, src, s, order, sfmreg::max_d2(max_dist), true, false);
  SFM_HIP_TRY(hipGetLastError());
  SFM_HIP_TRY(hipMemcpyAsync(idx, s->idx.p, sizeof(int) * (size_t)src->n, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(d2, s->d2.p, sizeof(float) * (size_t)src->n, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  return SFMHIP_OK;
}

// f-17's and f-18's entries: the loop with metric 0 and no rejector (sfmreg::icp_opts), its result narrowed to theirs
extern "C" int sfmhip_cloud_register(sfmhip_cloud* tgt, sfmhip_cloud* src, const sfmhip_register_opts* opts, const sfmhip_transform* init,
                                     sfmhip_register_result* out, int32_t* idx) {
  if (!tgt || !src || !out || tgt->ctx != src->ctx) return SFMHIP_ERR_ARG;
  const Opts o = opts ? mirror<Opts>(*opts) : sfmreg::default_opts();
  const Transform T0 = init ? mirror<Transform>(*init) : sfmreg::identity();
  if (!sfmreg::valid_opts(o) || !sfmreg::valid_transform(T0)) return SFMHIP_ERR_ARG;
  Sink sink{&RegState::single, idx};
  SFM_TRY(run_loop(tgt, src, nullptr, sfmreg::icp_opts(o), &T0, 1, true, sink));
  *out = mirror<sfmhip_register_result>(sfmreg::point_result(sink.res[0]));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_register_batch(sfmhip_cloud* tgt, sfmhip_cloud* src, const sfmhip_register_opts* opts, const sfmhip_transform* inits,
                                           int n_init, sfmhip_register_result* out, int32_t* idx) {
  if (!tgt || !src || !out || !inits || tgt->ctx != src->ctx) return SFMHIP_ERR_ARG;
  const Opts o = opts ? mirror<Opts>(*opts) : sfmreg::default_opts();
  static_assert(sizeof(sfmhip_transform) == sizeof(Transform), "the C ABI mirrors register.h");
  if (!sfmreg::valid_batch(o, (const Transform*)inits, n_init)) return SFMHIP_ERR_ARG;
  Sink sink{&RegState::batch, idx};
  SFM_TRY(run_loop(tgt, src, nullptr, sfmreg::icp_opts(o), (const Transform*)inits, n_init, false, sink));
  for (int b = 0; b < n_init; ++b) out[b] = mirror<sfmhip_register_result>(sfmreg::point_result(sink.res[b]));
  return SFMHIP_OK;
}

extern "C" int sfmhip_cloud_transform(sfmhip_cloud* c, const sfmhip_transform* T, sfmhip_cloud** out) {
  if (!c || !T || !out) return SFMHIP_ERR_ARG;
  const Transform T0 = mirror<Transform>(*T);
  if (!sfmreg::valid_transform(T0)) return SFMHIP_ERR_ARG;
  *out = nullptr;
  SFM_HIP_TRY(hipSetDevice(c->ctx->device));
  hipStream_t st = c->ctx->stream;
  float* d = nullptr;
  SFM_TRY(sfm_dev_alloc(&d, (size_t)3 * std::max(c->n, 1)));
  if (c->n > 0) {
    hipLaunchKernelGGL(reg_transform, dim3(blocks(c->n, 256)), dim3(256), 0, st, c->xyz, c->n, T0, d);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
      hipFree(d);
      return SFMHIP_ERR_HIP;
    }
  }
  return adopt_device(c->ctx, d, c->n, out);
}

extern "C" int sfmhip_cloud_concat(sfmhip_cloud* a, sfmhip_cloud* b, sfmhip_cloud** out) {
  if (!a || !b || !out || a->ctx != b->ctx) return SFMHIP_ERR_ARG;
  if ((long long)a->n + b->n > INT_MAX) return SFMHIP_ERR_UNSUPPORTED;
  *out = nullptr;
  SFM_HIP_TRY(hipSetDevice(a->ctx->device));
  hipStream_t st = a->ctx->stream;
  const int n = a->n + b->n;
  float* d = nullptr;
  SFM_TRY(sfm_dev_alloc(&d, (size_t)3 * std::max(n, 1)));
  hipError_t e = hipSuccess;
  if (a->n > 0) e = hipMemcpyAsync(d, a->xyz, sizeof(float) * 3 * (size_t)a->n, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess && b->n > 0) e = hipMemcpyAsync(d + 3 * (size_t)a->n, b->xyz, sizeof(float) * 3 * (size_t)b->n, hipMemcpyDeviceToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) {
    g_sfmhip_last_hip_error = (int)e;
    hipFree(d);
    return SFMHIP_ERR_HIP;
  }
  return adopt_device(a->ctx, d, n, out);
}

extern "C" int sfmhip_cloud_register_last_timing(sfmhip_cloud* tgt, double ms3[3], int32_t* iterations) {
  return report(tgt, &RegState::single, false, ms3, iterations);
}

extern "C" int sfmhip_cloud_register_batch_last_timing(sfmhip_cloud* tgt, double ms3[3], int32_t* iterations) {
  return report(tgt, &RegState::batch, false, ms3, iterations);
}
