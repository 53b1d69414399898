// common.h -- context object and error plumbing shared by the HIP translation units.
#pragma once
#include <chrono>
#include <cstdlib>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>
#include "../../include/sfmhip.h"

extern thread_local int g_sfmhip_last_hip_error;

#define SFM_HIP_TRY(expr)                                                              \
  do {                                                                                 \
    hipError_t e__ = (expr);                                                           \
    if (e__ != hipSuccess) {                                                           \
      g_sfmhip_last_hip_error = (int)e__;                                              \
      fprintf(stderr, "[sfmhip] %s:%d %s -> %s\n", __FILE__, __LINE__, #expr,          \
              hipGetErrorString(e__));                                                 \
      return SFMHIP_ERR_HIP;                                                           \
    }                                                                                  \
  } while (0)

#define SFM_TRY(expr)            \
  do {                           \
    int rc__ = (expr);           \
    if (rc__ != SFMHIP_OK) return rc__; \
  } while (0)

struct sfmhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  bool timing = false;  // record hipEvents between the stages of a run (sfmhip_set_timing)
  int n_cu = 0;
  // reusable pinned + device scratch for the one-shot host-pointer entry points
  void* pinned = nullptr;
  size_t pinned_bytes = 0;
  // two grow-only device blocks for entry points that would otherwise hipMalloc / hipFree per call (sift.hip)
  void* dev_scratch[2] = {nullptr, nullptr};
  size_t dev_scratch_bytes[2] = {0, 0};
  // worker contexts (own stream + scratch) of the batched entry points (sfmhip_sift_batch): created on demand, freed
  // with the context
  std::vector<sfmhip_ctx*> workers;
  int score_flags = 0;  // OR of the five-point samples' flags of the last sfmhip_score_essential call (score.hip)
  int pose_flags = 0;   // OR of the decompositions' flags of the last pose call (pose.hip, sfmhip_pose_last_flags)
  int pnp_flags = 0;    // OR of the EPnP solves' flags of the last PnP call (pnp.hip, sfmhip_pnp_last_flags)
  double pnp_ms[3] = {0, 0, 0};  // solver / scoring / refit kernel time of the last sfmhip_pnp_ransac call (timing on)
  double undistort_ms[2] = {0, 0};  // map / gather kernel time of the last sfmhip_image_undistort call (timing on)
  // sfmhip_ba_solve (ba.hip): where the last call's time went, and the problem it keeps for a next call of the same structure
  sfmhip_ba_solve_profile ba_profile = {};
  void* ba_cache = nullptr;
  void (*ba_cache_free)(void*) = nullptr;
  // ... and the memory its problems live in: ONE grow-only device block that every problem of the one-shot entry point is carved
  // from (a problem is 60-odd hipMallocs and as many hipFrees otherwise: 6.4 ms of a 33 ms call at cfg4), and one pinned block
  // for the records the device writes to the host
  void* ba_arena = nullptr;
  size_t ba_arena_bytes = 0, ba_arena_need = 0;  // need: what the last problem took in all (the next call grows the block to it)
  void* ba_pinned = nullptr;
  size_t ba_pinned_bytes = 0;
  void* ba_host_scratch = nullptr;  // (and the host vectors of its set-ups: ba.hip, BaHostScratch)
  void (*ba_host_scratch_free)(void*) = nullptr;
  void* crowns_state = nullptr;  // the device state of sfmhip_chm_crowns, the raster entry of crowns.hip (grow-only, freed with the context)
  void (*crowns_state_free)(void*) = nullptr;
};

int sfm_ctx_pinned(sfmhip_ctx* ctx, size_t bytes, void** out);
// block `which` (0 or 1) of at least `bytes` bytes; its contents do not survive a growing call.  The caller's work on
// it is ordered by the context's stream (the entry points that use it end with a stream synchronisation).
int sfm_ctx_dev_scratch(sfmhip_ctx* ctx, int which, size_t bytes, void** out);

template <typename T>
static inline int sfm_dev_alloc(T** p, size_t n) {
  void* v = nullptr;
  hipError_t e = hipMalloc(&v, (n ? n : 1) * sizeof(T));
  if (e != hipSuccess) {
    g_sfmhip_last_hip_error = (int)e;
    return SFMHIP_ERR_ALLOC;
  }
  // SFMHIP_POISON=1 (tests): fresh device memory holds 0xFF bytes (NaN as float / double, -1 as int) instead of
  // whatever the driver hands out -- a kernel that reads before it writes shows up as NaN, not as a rare flake
  const bool poison = getenv("SFMHIP_POISON") != nullptr;
  if (poison) {
    // (the fill runs on the null stream: it must be over before a kernel on one of the library's own streams touches the
    // buffer -- an allocation made between two launches, like the front tree's second reduced-system buffer, raced with it)
    hipMemset(v, 0xFF, (n ? n : 1) * sizeof(T));
    hipDeviceSynchronize();
  }
  *p = (T*)v;
  return SFMHIP_OK;
}

struct DevBufs {  // device memory of one call (or one object), freed with it
  std::vector<void*> p;
  DevBufs() = default;
  DevBufs(const DevBufs&) = delete;
  DevBufs& operator=(const DevBufs&) = delete;
  ~DevBufs() {
    for (void* q : p) hipFree(q);
  }
  template <typename T>
  int alloc(T** out, size_t n) {
    const int rc = sfm_dev_alloc(out, n);
    if (rc == SFMHIP_OK) p.push_back((void*)*out);
    return rc;
  }
};

// rocPRIM's exclusive plus-scan of n ints on `st`, defined once (context.hip).  The caller owns the temporary storage:
// sfm_scan_bytes says how much n needs, sfm_exclusive_scan runs on a block of at least that.  With `total` it also
// returns out[n - 1] + in[n - 1] (two async 4-byte copies and one stream synchronisation), so n >= 1 there: every
// caller returns early on an empty input.
int sfm_scan_bytes(size_t n, hipStream_t st, size_t* bytes);
int sfm_exclusive_scan(void* tmp, size_t tmp_bytes, const int* in, int* out, size_t n, hipStream_t st, long long* total);

// The lens-distortion resampling of undistort.hip for the callers inside the library (mvs.hip): launches on
// `st`, no synchronisation, device pointers throughout.  map: rows x cols entries (sfmund::Packed), padded to a multiple of 4.
namespace sfmund {
struct Packed;
}
size_t sfm_undistort_map_entries(int rows, int cols);
int sfm_undistort_map(hipStream_t st, int rows, int cols, const double* K9, const double* dist5, sfmund::Packed* map, uint8_t* valid);
int sfm_undistort_apply(hipStream_t st, int n, int rows, int cols, int ch, const uint8_t* src, uint8_t* dst, const sfmund::Packed* map);
int sfm_undistort_level_mask(hipStream_t st, int rows, int cols, int level, const uint8_t* valid0, uint8_t* out);
int sfm_undistort_seam(hipStream_t st, int rows, int cols, int window, const uint8_t* valid, int32_t* idx, float* depth, float* score);

// The ratio-test lists of a match plan's last run where they lie in HBM (match.hip), for tracks.hip: pair p's matches are
// q[p * stride + k], t[p * stride + k] with k < counts[p]; pairs, counts, q and t are device pointers, n_rows is the host's
// row count per image.  Valid until the plan's next run or set_pairs; work on them is ordered by the context's stream.
struct sfm_matchplan_lists {
  sfmhip_ctx* ctx;
  int n_images, n_pairs, stride;
  const int* n_rows;
  const int *pairs, *counts, *q, *t;
};
int sfm_matchplan_device_lists(sfmhip_matchplan* pl, sfm_matchplan_lists* out);
// The same view of a verified match set (verify.hip): its own lists, valid as long as the handle.
int sfm_verified_device_lists(const sfmhip_verified* v, sfm_matchplan_lists* out);

static inline double sfm_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
