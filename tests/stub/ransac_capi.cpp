// ransac_capi.cpp -- a C surface over csrc/ransac_host.h and csrc/score_host.h for tests/test_ransac_replay_cpu.py (built with
// g++ -O2 -std=c++17 -ffp-contract=off): ransac_replay under each of its three uses (essential matrix, homography, PnP) with
// a backend that answers from tables instead of solving, RANSACUpdateNumIters, and the homography's sample stream.
#include <cstdint>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/ransac_host.h"
#include "../../sfm_danpipeline_amd/csrc/score_host.h"

namespace {

using namespace sfmransac;

enum { ESSENTIAL = 0, HOMOGRAPHY = 1, PNP = 2 };
enum { ERR_SAMPLES = 71, ERR_KEEP = 72 };  // the sample table is not the view's next rows / a keep names a slot of another view

// row i of a view is {i, i, ...}: the backend reads the absolute iteration of a slot off the sample table.  From
// dead_at[view] on (>= 0) the rows are -1, as when getSubset gives up.
struct ScriptedSamples {
  int mp;
  const int32_t* dead_at;  // nullable
  std::vector<int> buf;
  const int* rows(int view, int /*count*/, int first, int n) {
    buf.assign((size_t)mp * n, 0);
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < mp; ++k) buf[(size_t)i * mp + k] = dead_at && dead_at[view] >= 0 && first + i >= dead_at[view] ? -1 : first + i;
    return buf.data();
  }
};

// answers from nm[view][iteration], cnt[view][iteration][m], flags[view][iteration] (n_iters iterations per view; past them
// no model).  With the real per-count sampler (check_stream) the iteration of a slot is counted instead -- a view that is
// still active has consumed every chunk it was given -- and the rows must be that count's stream at those iterations.
struct ScriptedBackend {
  int mp, M, n_iters;
  const int32_t *nm, *cnt, *flags;
  bool check_stream;
  std::vector<int> next;               // per view: iterations handed out so far (check_stream)
  std::map<int, SampleStream> ref;     // per count: the stream a view of that count must be given (check_stream)
  struct SlotId { int view, iter; };
  std::vector<SlotId> last;            // who each slot of the LAST chunk was
  std::vector<int32_t> kept_it, kept_m;  // per view: the model kept last (-1: none)
  int run_chunk(const std::vector<Job>& jobs, int chunk, const std::vector<int>& samples, std::vector<int>& ok, std::vector<int>& counts) {
    last.assign(ok.size(), SlotId{-1, -1});
    for (size_t j = 0; j < jobs.size(); ++j) {
      const Job& jb = jobs[j];
      for (int it = 0; it < chunk; ++it) {
        const size_t slot = j * chunk + it;
        const int* row = samples.data() + ((size_t)jb.samp + it) * mp;
        int i;
        if (jb.count == mp) {  // the view is its one sample: rows 0 .. mp - 1
          for (int k = 0; k < mp; ++k)
            if (row[k] != k) return ERR_SAMPLES;
          i = 0;
        } else if (check_stream) {
          i = next[jb.view] + it;
          SampleStream& ss = ref[jb.count];
          ss.extend(jb.count, i + 1);
          for (int k = 0; k < mp; ++k)
            if (row[k] != ss.idx[(size_t)i * 5 + k]) return ERR_SAMPLES;
        } else {
          i = row[0];
        }
        ok[slot] = 0;
        for (int m = 0; m < M; ++m) counts[slot * M + m] = 0;
        if (i < 0 || i >= n_iters) continue;  // a dead row (homog_solve gives no model) or past the tables
        last[slot] = SlotId{jb.view, i};
        const size_t e = (size_t)jb.view * n_iters + i;
        ok[slot] = nm[e] | (flags[e] << 8);
        for (int m = 0; m < M; ++m) counts[slot * M + m] = cnt[e * M + m];
      }
      if (check_stream) next[jb.view] += chunk;
    }
    return 0;
  }
  int keep_best(const std::vector<Keep>& keeps) {
    std::vector<char> seen(kept_it.size(), 0);
    for (const Keep& k : keeps) {
      const SlotId id = last[(size_t)(k.slot / M)];
      if (id.view != k.view || seen[k.view]) return ERR_KEEP;  // (at most one keep per view per chunk)
      seen[k.view] = 1;
      kept_it[k.view] = id.iter;
      kept_m[k.view] = k.slot % M;
    }
    return 0;
  }
};

}  // namespace

extern "C" {

int ransac_update_num_iters_c(double p, double ep, int model_points, int max_iters) {
  return ransac_update_num_iters(p, ep, model_points, max_iters);
}

// ransac_replay as `policy` calls it, over views of n_corr[view] correspondences (offsets are their running sum).
// real_sampler: the per-count sample streams of the essential-matrix and PnP uses instead of the scripted rows.
// Per view: best, iter, status, the kept (iteration, m) (-1, -1: none); flags_any: the OR over every view.
int ransac_scripted(int policy, int n_views, const int32_t* n_corr, int n_iters, const int32_t* nm, const int32_t* cnt,
                    const int32_t* flags, const int32_t* dead_at, double confidence, int max_iters, int real_sampler, int32_t* best,
                    int32_t* iter, int32_t* status, int32_t* kept_it, int32_t* kept_m, int32_t* flags_any) {
  const int mp = policy == HOMOGRAPHY ? 4 : 5, M = policy == ESSENTIAL ? 10 : 1;
  const int limit = policy == ESSENTIAL ? 1000 : policy == HOMOGRAPHY ? std::max(max_iters, 1) : std::max(max_iters, 0);
  std::vector<int32_t> offsets((size_t)n_views + 1, 0);
  for (int v = 0; v < n_views; ++v) offsets[v + 1] = offsets[v] + n_corr[v];
  ScriptedBackend be{mp, M, n_iters, nm, cnt, flags, real_sampler != 0};
  be.next.assign((size_t)n_views, 0);
  be.kept_it.assign((size_t)n_views, -1);
  be.kept_m.assign((size_t)n_views, -1);
  std::vector<ViewState> vs;
  int fl = 0, rc;
  if (real_sampler) {
    CountSamples draw;
    rc = ransac_replay(be, draw, mp, M, n_views, offsets.data(), confidence, limit, vs, fl);
  } else {
    ScriptedSamples draw{mp, policy == HOMOGRAPHY ? dead_at : nullptr};
    rc = ransac_replay(be, draw, mp, M, n_views, offsets.data(), confidence, limit, vs, fl);
  }
  if (rc) return rc;
  for (int v = 0; v < n_views; ++v) {
    best[v] = vs[v].best;
    iter[v] = vs[v].iter;
    status[v] = vs[v].status;
    kept_it[v] = be.kept_it[v];
    kept_m[v] = be.kept_m[v];
  }
  *flags_any = fl;
  return 0;
}

int ransac_has_code(int status, int count, int model_points) { return has_code(status, count, model_points); }

// the first n rows (4 indices each; -1: the stream is dead) of the homography's sample stream over `count` float point pairs
void homography_samples(int count, const float* m1, const float* m2, int n, int32_t* out) {
  HSampleStream ss;
  ss.extend(m1, m2, count, n);
  for (int i = 0; i < 4 * n; ++i) out[i] = ss.idx[i];
}

}  // extern "C"
