// pose.hip -- the pose step of baseReconstruction (getCameraPose, reference src/Sfm.cpp:713-789) on gfx950: OpenCV 3.4.1's
// recoverPose(E, p1, p2, R, t, focal, pp, mask) for a batch of pairs, and findEssentialMat followed by it with E and the
// RANSAC mask never leaving the device.
//
// Two kernels.  pose_candidates: one thread per match, a workgroup per tile of 256 matches of one pair; every lane
// decomposes the pair's E (the same operations in every lane of the wave: no LDS broadcast), normalises its match,
// triangulates it under the four candidate poses (four 4 x 4 DLTs, f64) and stores a 4-bit code; the tile's counts go
// into counts[pair][4] through one integer atomicAdd per wave and candidate (integers: the order of the adds does not
// matter).  pose_select: a workgroup per pair applies recoverPose's selection rule and writes R, t, the count and the
// output mask from the codes.  The arithmetic is pose.h's, which the CPU test stub compiles too.
#include "common.h"
#include "essential_dev.h"
#include "pose.h"
#include <algorithm>
#include <vector>

namespace {

constexpr int TILE = 256;

struct PoseArgs {
  const int* off;                 // n_pairs + 1
  const int2* tiles;              // (pair, first match of the tile)
  const double2* xy1;             // pixels, as given
  const double2* xy2;
  const double* E;                // 9 per pair
  const unsigned char* has;       // nullable: 0 = the pair has no model (essential_pose)
  const unsigned char* mask_in;   // nullable
  double f, ppx, ppy, dist_thr;
  int* counts;                    // 4 per pair, zeroed before pose_candidates
  unsigned char* codes;           // 1 per match
  double* R;                      // 9 per pair
  double* t;                      // 3 per pair
  int* n_good;                    // 1 per pair
  unsigned char* mask_out;        // 1 per match
  int* flags;                     // 1
};

__global__ __launch_bounds__(TILE) void pose_candidates(PoseArgs a) {
  const int2 tl = a.tiles[blockIdx.x];
  const int p = tl.x;
  if (a.has && a.has[p] == 0) return;  // (uniform over the workgroup)
  const int o = a.off[p], n = a.off[p + 1] - o;
  const int i = tl.y + (int)threadIdx.x;
  const bool live = i < n;
  double E[9], R1[9], R2[9], t[3], P[4][12];
#pragma unroll
  for (int k = 0; k < 9; ++k) E[k] = a.E[(size_t)p * 9 + k];
  sfmpose::decompose_essential(E, R1, R2, t);
#pragma unroll
  for (int c = 0; c < 4; ++c) sfmpose::candidate(R1, R2, t, c, P[c]);
  const double2 u = live ? a.xy1[(size_t)o + i] : make_double2(0, 0);
  const double2 v = live ? a.xy2[(size_t)o + i] : make_double2(0, 0);
  unsigned bits = sfmpose::candidate_bits(P, u.x, u.y, v.x, v.y, a.f, a.ppx, a.ppy, a.dist_thr);
  if (!live || (a.mask_in && !a.mask_in[(size_t)o + i])) bits = 0;
  if (live) a.codes[(size_t)o + i] = (unsigned char)bits;
  const int c0 = __popcll(__ballot(bits & 1)), c1 = __popcll(__ballot(bits & 2)), c2 = __popcll(__ballot(bits & 4)),
            c3 = __popcll(__ballot(bits & 8));
  const int lane = threadIdx.x & 63;
  const int mine = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : c3;
  if (lane < 4 && mine) atomicAdd(&a.counts[4 * p + lane], mine);
}

__global__ __launch_bounds__(TILE) void pose_select(PoseArgs a) {
  const int p = blockIdx.x;
  const int o = a.off[p], n = a.off[p + 1] - o;
  if (a.has && a.has[p] == 0) {  // no model: n_good -1, R and t zero, empty mask
    if (threadIdx.x < 9) a.R[(size_t)p * 9 + threadIdx.x] = 0;
    if (threadIdx.x < 3) a.t[(size_t)p * 3 + threadIdx.x] = 0;
    if (threadIdx.x == 0) a.n_good[p] = -1;
    for (int i = threadIdx.x; i < n; i += TILE) a.mask_out[(size_t)o + i] = 0;
    return;
  }
  const int g[4] = {a.counts[4 * p], a.counts[4 * p + 1], a.counts[4 * p + 2], a.counts[4 * p + 3]};
  const int sel = sfmpose::select_candidate(g);
  if (threadIdx.x < 64) {  // (one wave decomposes)
    double E[9], R1[9], R2[9], t[3];
    for (int k = 0; k < 9; ++k) E[k] = a.E[(size_t)p * 9 + k];
    const int fl = sfmpose::decompose_essential(E, R1, R2, t);
    if (threadIdx.x == 0) {
      const double* R = (sel & 1) ? R2 : R1;
      for (int k = 0; k < 9; ++k) a.R[(size_t)p * 9 + k] = R[k];
      for (int k = 0; k < 3; ++k) a.t[(size_t)p * 3 + k] = (sel & 2) ? -t[k] : t[k];
      a.n_good[p] = g[sel];
      if (fl) atomicOr(a.flags, fl);
    }
  }
  // bitwise_and(mask, mask1): the input byte where the candidate passes (255 without an input mask), else 0
  for (int i = threadIdx.x; i < n; i += TILE) {
    const size_t k = (size_t)o + i;
    a.mask_out[k] = ((a.codes[k] >> sel) & 1) ? (a.mask_in ? a.mask_in[k] : (unsigned char)255) : (unsigned char)0;
  }
}

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// One slab for what the two kernels need beyond the inputs already on the device: the tile list, the counts, the
// codes, the outputs and the flags word, and (explicit-E entry) the uploaded inputs.  in_* < 0: that input is not
// uploaded.  Launches both kernels and downloads the outputs; synchronises.
int run_pose(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, PoseArgs a, const double* h_left, const double* h_right,
             const double* h_E, const uint8_t* h_mask_in, double* R, double* t, int32_t* n_good, uint8_t* mask_out) {
  hipStream_t st = ctx->stream;
  const size_t total = (size_t)offsets[n_pairs];
  std::vector<int2> tiles;
  for (int p = 0; p < n_pairs; ++p)
    for (int s = 0; s < offsets[p + 1] - offsets[p]; s += TILE) tiles.push_back(int2{p, s});
  const bool up_pts = h_left != nullptr, up_E = h_E != nullptr, up_mask = h_mask_in != nullptr;
  size_t off_b = 0;
  auto take = [&](size_t bytes) {
    const size_t at = off_b;
    off_b += align256(bytes ? bytes : 1);
    return at;
  };
  const size_t o_tiles = take(sizeof(int2) * tiles.size()), o_counts = take(sizeof(int) * 4 * n_pairs),
               o_codes = take(total), o_R = take(sizeof(double) * 9 * n_pairs), o_t = take(sizeof(double) * 3 * n_pairs),
               o_ng = take(sizeof(int) * n_pairs), o_mask = take(total), o_flags = take(sizeof(int)),
               o_off = a.off ? 0 : take(sizeof(int) * (n_pairs + 1)), o_l = up_pts ? take(16 * total) : 0,
               o_r = up_pts ? take(16 * total) : 0, o_E = up_E ? take(sizeof(double) * 9 * n_pairs) : 0,
               o_min = up_mask ? take(total) : 0;
  DevBufs bufs;
  unsigned char* d = nullptr;
  SFM_TRY(bufs.alloc(&d, off_b));
  a.tiles = (const int2*)(d + o_tiles);
  a.counts = (int*)(d + o_counts);
  a.codes = d + o_codes;
  a.R = (double*)(d + o_R);
  a.t = (double*)(d + o_t);
  a.n_good = (int*)(d + o_ng);
  a.mask_out = d + o_mask;
  a.flags = (int*)(d + o_flags);
  if (!a.off) {
    SFM_HIP_TRY(hipMemcpyAsync(d + o_off, offsets, sizeof(int) * (n_pairs + 1), hipMemcpyHostToDevice, st));
    a.off = (const int*)(d + o_off);
  }
  if (up_pts && total) {
    SFM_HIP_TRY(hipMemcpyAsync(d + o_l, h_left, 16 * total, hipMemcpyHostToDevice, st));
    SFM_HIP_TRY(hipMemcpyAsync(d + o_r, h_right, 16 * total, hipMemcpyHostToDevice, st));
    a.xy1 = (const double2*)(d + o_l);
    a.xy2 = (const double2*)(d + o_r);
  }
  if (up_E) {
    SFM_HIP_TRY(hipMemcpyAsync(d + o_E, h_E, sizeof(double) * 9 * n_pairs, hipMemcpyHostToDevice, st));
    a.E = (const double*)(d + o_E);
  }
  if (up_mask && total) {
    SFM_HIP_TRY(hipMemcpyAsync(d + o_min, h_mask_in, total, hipMemcpyHostToDevice, st));
    a.mask_in = d + o_min;
  }
  if (!tiles.empty())
    SFM_HIP_TRY(hipMemcpyAsync(d + o_tiles, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice, st));
  SFM_HIP_TRY(hipMemsetAsync(d + o_counts, 0, sizeof(int) * 4 * n_pairs, st));
  SFM_HIP_TRY(hipMemsetAsync(d + o_flags, 0, sizeof(int), st));
  if (!tiles.empty()) hipLaunchKernelGGL(pose_candidates, dim3((unsigned)tiles.size()), dim3(TILE), 0, st, a);
  hipLaunchKernelGGL(pose_select, dim3((unsigned)n_pairs), dim3(TILE), 0, st, a);
  SFM_HIP_TRY(hipGetLastError());
  SFM_HIP_TRY(hipMemcpyAsync(R, d + o_R, sizeof(double) * 9 * n_pairs, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(t, d + o_t, sizeof(double) * 3 * n_pairs, hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipMemcpyAsync(n_good, d + o_ng, sizeof(int) * n_pairs, hipMemcpyDeviceToHost, st));
  if (mask_out && total) SFM_HIP_TRY(hipMemcpyAsync(mask_out, d + o_mask, total, hipMemcpyDeviceToHost, st));
  int flags = 0;
  SFM_HIP_TRY(hipMemcpyAsync(&flags, d + o_flags, sizeof(int), hipMemcpyDeviceToHost, st));
  SFM_HIP_TRY(hipStreamSynchronize(st));
  ctx->pose_flags = flags;
  return SFMHIP_OK;
}

bool offsets_ok(int n_pairs, const int32_t* offsets) {
  if (offsets[0] < 0) return false;
  for (int p = 0; p < n_pairs; ++p)
    if (offsets[p + 1] < offsets[p]) return false;
  return true;
}

}  // namespace

extern "C" int sfmhip_recover_pose(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy,
                                   const double* right_xy, const double* E, double focal, double ppx, double ppy,
                                   double distance_thresh, const uint8_t* mask_in, double* R, double* t, int32_t* n_good,
                                   uint8_t* mask_out) {
  if (!ctx || n_pairs < 0 || !offsets || !E || !R || !t || !n_good) return SFMHIP_ERR_ARG;
  if (n_pairs == 0) return SFMHIP_OK;
  if (!offsets_ok(n_pairs, offsets)) return SFMHIP_ERR_ARG;
  const long long total = offsets[n_pairs];
  if (total > 0 && (!left_xy || !right_xy)) return SFMHIP_ERR_ARG;
  SFM_HIP_TRY(hipSetDevice(ctx->device));
  ctx->pose_flags = 0;
  PoseArgs a = {};
  a.f = focal;
  a.ppx = ppx;
  a.ppy = ppy;
  a.dist_thr = distance_thresh;
  return run_pose(ctx, n_pairs, offsets, a, total ? left_xy : nullptr, total ? right_xy : nullptr, E, mask_in, R, t, n_good,
                  mask_out);
}

extern "C" int sfmhip_essential_pose(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy,
                                     const double* right_xy, double fx, double fy, double cx, double cy, double prob,
                                     double threshold, double* E, int32_t* inliers, double* R, double* t, int32_t* n_good,
                                     uint8_t* mask) {
  if (!ctx || n_pairs < 0 || !offsets || !E || !inliers || !R || !t || !n_good || !(prob > 0 && prob < 1)) return SFMHIP_ERR_ARG;
  if (n_pairs == 0) return SFMHIP_OK;
  if (!offsets_ok(n_pairs, offsets)) return SFMHIP_ERR_ARG;
  const long long total = offsets[n_pairs];
  if (total > 0 && (!left_xy || !right_xy)) return SFMHIP_ERR_ARG;
  ctx->pose_flags = 0;
  EssentialDev dev;
  SFM_TRY(sfm_essential_ransac(ctx, n_pairs, offsets, left_xy, right_xy, fx, fy, cx, cy, prob, threshold, inliers, nullptr, true,
                               dev));
  SFM_HIP_TRY(hipMemcpyAsync(E, dev.d_bestE, sizeof(double) * 9 * n_pairs, hipMemcpyDeviceToHost, ctx->stream));
  PoseArgs a = {};
  a.off = dev.d_off;
  a.xy1 = (const double2*)dev.d_left;
  a.xy2 = (const double2*)dev.d_right;
  a.E = dev.d_bestE;
  a.has = dev.d_has;
  a.mask_in = dev.d_mask;
  a.f = fx;  // recoverPose(E, ..., fx, (cx, cy), mask): fx serves both axes (src/Sfm.cpp:750-755)
  a.ppx = cx;
  a.ppy = cy;
  a.dist_thr = 50;
  return run_pose(ctx, n_pairs, offsets, a, nullptr, nullptr, nullptr, nullptr, R, t, n_good, mask);
}

extern "C" int sfmhip_pose_last_flags(sfmhip_ctx* ctx) { return ctx ? ctx->pose_flags : 0; }
