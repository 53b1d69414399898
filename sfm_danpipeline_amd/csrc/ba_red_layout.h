// ba_red_layout.h -- the layout of the reduced-system buffer of the bundle adjustment (BaDev::red in ba.hip), in doubles:
//
//   [ S ld*ld | g ld | F^T b ld | dc ld | SC scalars | RANK_SLOTS, one per rank | red2 RED2_N | X ld*ld ]
//
// S: the reduced camera matrix (upper triangle, row-major); g: its right-hand side; F^T b: the unreduced gradient of the camera
// columns; dc: their squared column norms; the scalars: [0] the cost's sum of squares, [1] |points|^2, [2] failed point blocks,
// [3] the gradient maximum; a rank's slot: its own gradient maximum; red2: the step evaluation's scalars and the reduced solve's
// status; X: the identity that rides through the dense factorisation (L^-T after it).  Several ranks all-reduce [S .. rank slots);
// a linearisation zeroes everything but X, and the scalars .. red2 go to the host in one copy.
//
// Every offset depends on ld alone.  No HIP runtime: the host, the kernels and the set-up (ba_setup.h, plain g++) read it here.
#pragma once
#include <cstddef>

#ifdef __HIPCC__
#define REDL_HD __host__ __device__ __forceinline__
#else
#define REDL_HD inline
#endif

namespace redl {

constexpr int SC = 16;          // scalar slots behind dc
constexpr int RANK_SLOTS = 64;  // the most ranks of a sharded problem
// red2: [0..4) the four totals (candidate cost, model cost change, |step|^2, |candidate|^2) that step_finish leaves -- the sums
// of the workgroups' slots in BaDev::step_part, added in a fixed order; [0, RED2_SUM_N) is what several ranks all-reduce --
// | RED2_TMP (a scratch double) | RED2_INFO (an int: the reduced solve's status) | pad.
constexpr int RED2_SUM_N = 8, RED2_TMP = RED2_SUM_N, RED2_INFO = RED2_SUM_N + 1, RED2_N = RED2_SUM_N + 8;
// red2[RED2_TIMEOUT]: 1 when a bounded spin of this rank's reduced solve or step evaluation ran out; summed over the ranks by the
// step evaluation's all-reduce, so that EVERY rank stops and repeats the solve (a rank-local stop would leave its peers waiting
// in an all-reduce the stopped rank never issues)
constexpr int RED2_TIMEOUT = 4;
// the reduced solve's status word (RED2_INFO): > 0 a pivot was not positive; -1 a hand-off of the reduced solve never arrived
// (the front tree then runs level by level); -2 a slot of the step evaluation's sums never arrived (no fallback: SFMHIP_ERR_TIMEOUT)
constexpr int INFO_FINISHER_TIMEOUT = -2;

REDL_HD size_t S(int) { return 0; }
REDL_HD size_t g(int ld) { return (size_t)ld * ld; }
REDL_HD size_t gF(int ld) { return (size_t)ld * ld + ld; }
REDL_HD size_t dc(int ld) { return (size_t)ld * ld + 2 * ld; }
REDL_HD size_t sc(int ld) { return (size_t)ld * ld + 3 * ld; }
// the same four as pointers into a buffer.  Not `red + dc(ld)`: the kernels have always formed (red + ld * ld) + 2 * ld, two additions
// that the compiler keeps apart, and their code is to stay what it is
template <typename T> REDL_HD T* g(T* red, int ld) { return red + (size_t)ld * ld; }
template <typename T> REDL_HD T* gF(T* red, int ld) { return red + (size_t)ld * ld + ld; }
template <typename T> REDL_HD T* dc(T* red, int ld) { return red + (size_t)ld * ld + 2 * ld; }
template <typename T> REDL_HD T* sc(T* red, int ld) { return red + (size_t)ld * ld + 3 * ld; }
REDL_HD size_t rank_slot(int ld, int r) { return sc(ld) + SC + r; }
REDL_HD size_t red2(int ld) { return sc(ld) + SC + RANK_SLOTS; }
REDL_HD size_t info(int ld) { return red2(ld) + RED2_INFO; }
REDL_HD size_t X(int ld) { return red2(ld) + RED2_N; }

REDL_HD size_t count(int ld) { return X(ld) + (size_t)ld * ld; }
REDL_HD size_t count_without_X(int ld) { return X(ld); }  // what a linearisation zeroes, and the spare workgroups of a solve
// the part behind S that several ranks sum: g | F^T b | dc | scalars | the ranks' slots in use
REDL_HD size_t allreduce_tail(int ld, int world) { return 3 * (size_t)ld + SC + world; }
// the all-reduce payload: the packed upper triangle of S and the tail with every rank's slot
REDL_HD size_t packed_count(int ld) { return (size_t)ld * (ld + 1) / 2 + allreduce_tail(ld, RANK_SLOTS); }
// the window ba_publish copies to the host: scalars | rank slots | red2
constexpr int host_scalars_n() { return SC + RANK_SLOTS + RED2_N; }

static_assert((SC + RANK_SLOTS + RED2_N) % 2 == 0, "count_without_X() is zeroed as double2 (ld is a multiple of 64)");
static_assert(host_scalars_n() <= 256, "ba_publish copies one double per thread");

}  // namespace redl
