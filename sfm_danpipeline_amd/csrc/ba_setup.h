// ba_setup.h -- host-side set-up of a bundle-adjustment problem: the observations grouped by point, the points grouped by
// camera list ("signature") into runs, the runs cut into the pieces of ba_eliminate_mfma, the gather lists of its slab
// epilogue, the camera co-visibility graph, and the pair path's camera-major lists.  sfmhip_ba_create (ba.hip) builds this,
// then allocates and uploads it.
//
// Pure host C++ (no HIP): tests/test_ba_setup.py compiles it with g++ and checks the grouping, the chunks and the graph
// against a numpy restatement, once under AddressSanitizer / UBSan.
#pragma once
#include <algorithm>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>
#include <unistd.h>
#include "../../include/sfmhip.h"
#include "ba_red_layout.h"

namespace bsetup {

constexpr int FB_MAXN = 4096;  // sanity cap on the observations of one point (the pair path has no structural limit)
constexpr int SHORT_RUN = 12;  // runs of at most this many points go to the pair path
// a chunk's slab: [Gram block, MFMA layout, NT x 256 <= 2560 | F^T F sums 36 x FP | Jf^2, Jf r, r^2 | gmax | nfail]
constexpr int ELIM_SLAB_FF = 2560, ELIM_SLAB = 2944;
constexpr int FP = 10;  // slots per row of the F^T F accumulators in LDS (the MFMA path takes signatures of n <= 10 cameras)

// the layouts of HIP's int2 / int4 (ba.hip asserts it): the lists below go to the device in one copy each
struct I2 {
  int x, y;
};
struct I4 {
  int x, y, z, w;
};

struct Chunk {
  int sig_off;  // offset into sig_cams
  int n;        // observations per point in this signature
  int p0;       // first sorted point
  int cnt;      // points in the chunk
};

// threads of a pass over n items: one below 20 000 items, else `cap` -- 0: the machine's, at most 16
inline int host_threads(int n, int cap = 0) {
  if (n < 20000) return 1;
  if (cap > 0) return cap;
  const unsigned hw = std::thread::hardware_concurrency();
  return (int)std::max(1u, std::min(16u, hw ? hw : 1u));
}
// The host threads of the set-up's passes: a pool that lives as long as the process (starting and joining sixteen threads is
// 0.4-0.5 ms, and a set-up has five such passes).  One job at a time; a caller that finds the pool busy (another host thread is
// setting a problem up) or that is itself running a job of the pool (a nested pass) starts threads of its own.
class HostPool {
 public:
  static HostPool& get() {
    static HostPool* p = new HostPool();  // (never destroyed: its threads wait on a condition variable until the process ends)
    return *p;
  }
  // f(t) for t in [0, nth): the caller is t = 0.  Returns false when the pool is taken (nothing has run).  An exception out of
  // f(0) leaves run() only once the workers are done with f.
  bool run(int nth, const std::function<void(int)>& f) {
    if (in_pool_ || getpid() != pid_) return false;  // (a forked child has this object but none of its threads: it starts its own)
    std::unique_lock<std::mutex> job_lock(job_m_, std::try_to_lock);
    if (!job_lock.owns_lock()) return false;
    {
      std::lock_guard<std::mutex> lk(m_);
      while ((int)workers_.size() < nth - 1) {
        const int id = (int)workers_.size() + 1;
        workers_.emplace_back([this, id]() { work(id); });
        workers_.back().detach();
      }
      f_ = &f;
      nth_ = nth;
      pending_ = nth - 1;
      ++gen_;
    }
    cv_.notify_all();
    struct Join {  // (declared first: runs last, after in_pool_ is cleared)
      HostPool* p;
      ~Join() {
        std::unique_lock<std::mutex> lk(p->m_);
        p->done_.wait(lk, [this]() { return p->pending_ == 0; });
        p->f_ = nullptr;
      }
    } join{this};
    struct InPool {
      InPool() { in_pool_ = true; }
      ~InPool() { in_pool_ = false; }
    } mark;
    f(0);
    return true;
  }

 private:
  void work(int id) {
    in_pool_ = true;
    unsigned seen = 0;
    for (;;) {
      const std::function<void(int)>* f = nullptr;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&]() { return gen_ != seen; });
        seen = gen_;
        if (id < nth_) f = f_;
      }
      if (!f) continue;
      (*f)(id);
      {
        std::lock_guard<std::mutex> lk(m_);
        if (--pending_ == 0) done_.notify_all();
      }
    }
  }
  static inline thread_local bool in_pool_ = false;  // this thread runs a job of the pool (a worker, or a caller inside f(0))
  const pid_t pid_ = getpid();
  std::mutex job_m_, m_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  const std::function<void(int)>* f_ = nullptr;
  int nth_ = 0, pending_ = 0;
  unsigned gen_ = 0;
};

// fn(t, lo, hi): thread t of nth takes [lo, hi)
template <typename F>
inline void host_parallel_for_t(int n, int nth, F fn) {
  if (nth <= 1) {
    fn(0, 0, n);
    return;
  }
  const std::function<void(int)> job = [&](int t) {
    const int lo = (int)((long long)n * t / nth), hi = (int)((long long)n * (t + 1) / nth);
    fn(t, lo, hi);
  };
  if (HostPool::get().run(nth, job)) return;
  std::vector<std::thread> th;
  for (int t = 0; t < nth; ++t) th.emplace_back([&job, t]() { job(t); });
  for (auto& x : th) x.join();
}
// fn(lo, hi) over [0, n) on host_threads(n, cap) threads
template <typename F>
inline void host_parallel_for(int n, F fn, int cap = 0) {
  host_parallel_for_t(n, host_threads(n, cap), [&](int, int lo, int hi) { fn(lo, hi); });
}

struct Setup;
// Host memory kept between set-ups by a caller that makes many (sfmhip_ba_solve: 50 MB of vectors at cfg4, whose fresh pages cost
// 3-4 ms on the way in and as much on the way out).  The five large arrays of the result borrow their storage from here.
struct Scratch {
  std::vector<int> cnt, slot, scam, run_of, order, optr, ocam, table, obs_src, cxy_src;
  std::vector<uint64_t> sig_hash;
  inline void swap_kept(Setup& s);  // lends the storage to s, or takes it back
};

struct Input {
  int n_cam = 0, n_pt = 0, n_obs = 0;
  const int32_t* obs_cam = nullptr;  // n_obs each
  const int32_t* obs_pt = nullptr;
  const double* obs_xy = nullptr;  // 2 n_obs
  int ld = 0;                      // row stride of S (6 n_cam + 1 rounded up)
  int n_cu = 1;                    // compute units of the device
  bool deterministic = true;       // the slab epilogue (run-to-run identical sums) rather than atomics
  int short_pieces = 512;          // the most short runs that become pieces of the elimination (0: none)
  int threads = 0;                 // threads of the passes over >= 20 000 items (0: the machine's, at most 16)
  std::function<void(const char*)> lap;  // called behind every stage with its name (profiling), or empty
};

struct Setup {
  int np = 0, no = 0;                       // points with observations, their observations
  std::vector<int> order;                   // sorted point -> input point
  std::vector<int> optr;                    // np + 1: a sorted point's first observation
  std::vector<int> ocam;                    // no: a sorted observation's camera
  std::vector<int> obs_src;                 // no: sorted observation -> input observation
  std::vector<unsigned char> cam_used;      // n_cam: the camera has an observation
  // the elimination's pieces: ids[NB - 1] the chunks of NB column blocks, large first; bs_desc 16 ints per chunk, large first
  std::vector<Chunk> chunks;
  std::vector<int> ids[8], sig_cams, bs_desc;
  // the slab epilogue (deterministic only): destination lists [0] full linearisation, [1] norms only; the row lists
  bool elim_deterministic = true;
  std::vector<int> gth_ptr[2], gth_dest[2], grow_colmap;
  std::vector<unsigned> gth_src[2];
  std::vector<I4> grow_hdr, grow_head, grow_over;
  int grow_waves = 0, grow_accw = 0;
  std::vector<unsigned long long> adj;  // camera co-visibility, n_cam x ceil(n_cam / 64) bit rows (empty past 4096 cameras)
  // the pair path: its points (sorted index, ascending), their observations camera-major, the camera pairs
  std::vector<int> fb, pp_obase, cptr, cpt, cxy_src, pair_ptr;
  std::vector<I2> cslot, pair_cams, pair_ent;
  std::vector<double> cxy;
  int cam_split = 1;
};

inline void Scratch::swap_kept(Setup& s) {
  order.swap(s.order);
  optr.swap(s.optr);
  ocam.swap(s.ocam);
  obs_src.swap(s.obs_src);
  cxy_src.swap(s.cxy_src);
}

// Fills `out`, a fresh Setup but for the five arrays it may have borrowed from a Scratch (whose capacity is reused).
// SFMHIP_OK, SFMHIP_ERR_ARG (an observation's camera or point out of range), SFMHIP_ERR_UNSUPPORTED (more than FB_MAXN
// observations of one point)
inline int build(const Input& in, Scratch& hs, Setup& out) {
  const int n_cam = in.n_cam, n_pt = in.n_pt, n_obs = in.n_obs;
  const int32_t *obs_cam = in.obs_cam, *obs_pt = in.obs_pt;
  const double* obs_xy = in.obs_xy;
  auto lap_ = [&](const char* what) {
    if (in.lap) in.lap(what);
  };
  auto threads = [&](int n) { return host_threads(n, in.threads); };
  // (one pass: the range check, and whether the observations already come grouped by point -- the order the reference adds
  // residual blocks in, src/BundleAdjustment.cpp:83-110 -- in which case the counting sort's scatter below is the identity)
  bool grouped = true;
  {
    int bad = 0;
    for (int o = 0; o < n_obs; ++o) {
      bad |= (obs_cam[o] < 0) | (obs_cam[o] >= n_cam) | (obs_pt[o] < 0) | (obs_pt[o] >= n_pt);
      grouped &= o == 0 || obs_pt[o - 1] <= obs_pt[o];
    }
    if (bad) return SFMHIP_ERR_ARG;
  }
  // ---- group observations by point, ascending camera inside a point (std::map order of
  //      Point3D::idxImage, reference src/BundleAdjustment.cpp:87)
  std::vector<int>& cnt = hs.cnt;
  cnt.assign((size_t)n_pt + 1, 0);
  for (int o = 0; o < n_obs; ++o) cnt[obs_pt[o] + 1]++;
  for (int p = 0; p < n_pt; ++p) cnt[p + 1] += cnt[p];
  std::vector<int>& slot = hs.slot;
  slot.resize(n_obs);
  if (grouped) {
    host_parallel_for(n_obs, [&](int lo, int hi) {
      for (int o = lo; o < hi; ++o) slot[o] = o;
    }, in.threads);
  } else {
    std::vector<int> fill(n_pt, 0);
    for (int o = 0; o < n_obs; ++o) slot[cnt[obs_pt[o]] + fill[obs_pt[o]]++] = o;
  }
  // per point (a few host threads: every pass over a million observations is a cache-miss chain on
  // one core): stable insertion sort -- a point has a handful of observations --, then the point's
  // ascending camera list, flat, and a hash of it: the signature grouping below compares
  // (length, hash) first and walks the lists only on equal hashes
  std::vector<int>& scam = hs.scam;
  scam.resize(n_obs);
  std::vector<uint64_t>& sig_hash = hs.sig_hash;
  sig_hash.assign(n_pt, 0);
  host_parallel_for(n_pt, [&](int plo, int phi) {
    for (int p = plo; p < phi; ++p) {
      for (int i = cnt[p] + 1; i < cnt[p + 1]; ++i) {
        const int v = slot[i], cv = obs_cam[v];
        int j = i - 1;
        for (; j >= cnt[p] && obs_cam[slot[j]] > cv; --j) slot[j + 1] = slot[j];
        slot[j + 1] = v;
      }
      uint64_t h = 1469598103934665603ull;
      for (int k = cnt[p]; k < cnt[p + 1]; ++k) {
        scam[k] = obs_cam[slot[k]];
        h = (h ^ (uint64_t)(uint32_t)scam[k]) * 1099511628211ull;
      }
      sig_hash[p] = h;
    }
  }, in.threads);
  lap_("group by point");
  // ---- group the points that have observations by signature (their ascending camera list): a
  //      hash table assigns run ids in order of first appearance, a counting sort makes the runs
  //      contiguous (stable: ascending point index inside a run)
  auto sig_equal = [&](int x, int y) {  // x, y: input point indices
    const int nx = cnt[x + 1] - cnt[x];
    if (nx != cnt[y + 1] - cnt[y] || sig_hash[x] != sig_hash[y]) return false;
    for (int k = 0; k < nx; ++k)
      if (scam[cnt[x] + k] != scam[cnt[y] + k]) return false;
    return true;
  };
  // (round 6: the three passes run on the host threads.  Every thread groups the points of ITS block with a table of its own --
  // local run ids in the block's order of first appearance --, the blocks' runs then meet one table in block order, which IS the
  // points' order of first appearance, and the counting sort scatters block by block from per-block start positions: the same
  // run ids, the same order as one thread produces, whatever the number of threads -- tests/test_ba_setup.py)
  std::vector<int>& run_of = hs.run_of;
  run_of.resize(n_pt);
  std::vector<int> run_rep, run_cnt;
  const int sig_threads = threads(n_pt);
  std::vector<std::vector<int>> loc_rep((size_t)sig_threads), loc_cnt((size_t)sig_threads);
  auto probe = [&](int* table, size_t cap, std::vector<int>& rep, int p) -> int {  // the run of point p among `rep`, entered when new
    size_t slot_i = (size_t)(sig_hash[p] ^ (sig_hash[p] >> 29)) & (cap - 1);
    for (;; slot_i = (slot_i + 1) & (cap - 1)) {
      const int r = table[slot_i];
      if (r < 0) {
        table[slot_i] = (int)rep.size();
        rep.push_back(p);
        return (int)rep.size() - 1;
      }
      if (sig_equal(rep[r], p)) return r;
    }
  };
  {
    const size_t blk = ((size_t)n_pt + sig_threads - 1) / sig_threads;
    size_t cap = 64;
    while (cap < 2 * blk + 16) cap <<= 1;
    std::vector<int>& table = hs.table;  // open addressing: run id, keyed by the signature hash; a slice per thread
    table.resize(cap * (size_t)sig_threads);
    std::vector<char> too_many((size_t)sig_threads, 0);
    host_parallel_for_t(n_pt, sig_threads, [&](int t, int lo, int hi) {
      int* tab = table.data() + cap * (size_t)t;
      std::fill(tab, tab + cap, -1);
      for (int p = lo; p < hi; ++p) {
        const int n = cnt[p + 1] - cnt[p];
        if (n > FB_MAXN) {
          too_many[t] = 1;
          return;
        }
        run_of[p] = n == 0 ? -1 : probe(tab, cap, loc_rep[t], p);
      }
    });
    for (char c : too_many)
      if (c) return SFMHIP_ERR_UNSUPPORTED;  // more than FB_MAXN observations of one point
    // the blocks' runs, block by block in their local order, into one table: global run ids in the points' order of first appearance
    size_t total = 0;
    for (const auto& r : loc_rep) total += r.size();
    size_t gcap = 64;
    while (gcap < 2 * total + 16) gcap <<= 1;
    std::vector<int> gtab(gcap, -1);
    for (int t = 0; t < sig_threads; ++t)
      for (int& lp : loc_rep[t]) lp = probe(gtab.data(), gcap, run_rep, lp);  // (the block's representative -> the global run)
    // global ids for the points, and every block's count per run
    const size_t R = run_rep.size();
    host_parallel_for_t(n_pt, sig_threads, [&](int t, int lo, int hi) {
      std::vector<int>& c = loc_cnt[t];
      c.assign(R, 0);
      const int* l2g = loc_rep[t].data();
      for (int p = lo; p < hi; ++p)
        if (run_of[p] >= 0) ++c[run_of[p] = l2g[run_of[p]]];
    });
    run_cnt.assign(R, 0);
    for (int t = 0; t < sig_threads; ++t)
      for (size_t r = 0; r < R; ++r) run_cnt[r] += loc_cnt[t][r];
  }
  lap_("  sig: hash table");
  std::vector<int> run_start(run_rep.size() + 1, 0);
  for (size_t r = 0; r < run_rep.size(); ++r) run_start[r + 1] = run_start[r] + run_cnt[r];
  std::vector<int>& order = out.order;
  order.resize(run_start.back());
  {
    // block t starts run r behind the points of the blocks before it (loc_cnt becomes the blocks' write positions)
    for (size_t r = 0; r < run_rep.size(); ++r) {
      int at = run_start[r];
      for (int t = 0; t < sig_threads; ++t) {
        const int c = loc_cnt[t][r];
        loc_cnt[t][r] = at;
        at += c;
      }
    }
    host_parallel_for_t(n_pt, sig_threads, [&](int t, int lo, int hi) {
      int* at = loc_cnt[t].data();
      for (int p = lo; p < hi; ++p)
        if (run_of[p] >= 0) order[at[run_of[p]]++] = p;
    });
  }
  lap_("  sig: counting sort");
  const int np = out.np = (int)order.size();
  std::vector<int>& optr = out.optr;
  optr.resize((size_t)np + 1);
  {
    // prefix sums of the sorted points' observation counts: block sums first, then every block from its own start
    const int nth = threads(np);
    std::vector<long long> bsum((size_t)nth + 1, 0);
    host_parallel_for_t(np, nth, [&](int t, int lo, int hi) {
      long long sacc = 0;
      for (int sp = lo; sp < hi; ++sp) sacc += cnt[order[sp] + 1] - cnt[order[sp]];
      bsum[t + 1] = sacc;
    });
    for (int t = 0; t < nth; ++t) bsum[t + 1] += bsum[t];
    host_parallel_for_t(np, nth, [&](int t, int lo, int hi) {
      int at = (int)bsum[t];
      for (int sp = lo; sp < hi; ++sp) {
        optr[sp] = at;
        at += cnt[order[sp] + 1] - cnt[order[sp]];
      }
    });
    optr[np] = (int)bsum[nth];
  }
  out.no = optr[np];
  std::vector<int>& ocam = out.ocam;
  ocam.resize(out.no);
  out.obs_src.resize(out.no);
  out.cam_used.assign(n_cam, 0);
  lap_("  sig: optr + resizes");
  // the gather of a million observations is a cache-miss chain on one core: split it over a few (each marks the cameras it
  // meets in a list of its own; the lists are merged behind the threads)
  {
    const int nth = threads(np);
    std::vector<std::vector<unsigned char>> used((size_t)nth, std::vector<unsigned char>(n_cam, 0));
    host_parallel_for_t(np, nth, [&](int t, int lo, int hi) {
      unsigned char* mine = used[t].data();
      for (int sp = lo; sp < hi; ++sp) {
        const int p = order[sp];
        int w = optr[sp];
        for (int k = cnt[p]; k < cnt[p + 1]; ++k, ++w) {
          const int o = slot[k];
          out.obs_src[w] = o;
          ocam[w] = obs_cam[o];
          if (!mine[ocam[w]]) mine[ocam[w]] = 1;  // (written once: the threads' lists are neighbours in memory, and a store per
                                                  //  observation to a line another thread's list shares kept that line travelling)
          // (the coordinates are put in this order on the device: ba_permute_xy)
        }
      }
    });
    for (const auto& u : used)
      for (int c = 0; c < n_cam; ++c) out.cam_used[c] |= u[c];
  }
  lap_("signature sort + csr");
  // ---- chunks: runs of equal signature with strictly ascending cameras, n <= 10 -> MFMA path,
  //      classed by the width of the local Gram matrix: NB = ceil((6n+2)/16) column blocks
  std::vector<Chunk>& chunks = out.chunks;
  std::vector<int>* ids = out.ids;
  std::vector<int>&sig_cams = out.sig_cams, &fb = out.fb;
  // points per workgroup: 2 workgroups of 4 waves are resident per CU (register-bound), so the launch runs in
  // rounds of 512 workgroups; a wave takes 4 points per iteration (~3.7 us at n = 10) and a fixed ~7 iterations'
  // worth of prologue, reductions and scatter (s_memtime stamps, scripts/elim_stamps.py).  Pick the run length
  // that minimises rounds x (iterations per wave + fixed).  Measured at cfg4 (round 2, stage
  // time per LM iteration): 400 workgroups of 4 waves 100 us; 800 of 2 waves 106 us; 200 of 8 waves 150 us (not a
  // matter of the two waves of a SIMD running in step: starting waves 4..7 up to 8 k cycles late changes nothing,
  // 148-151 us); 800 of 4 waves (2 rounds) 136 us.
  int target = 64;
  const std::vector<int>& gstart = run_start;  // first sorted point of every run, + np
  {
    std::vector<int> gsz;
    for (size_t gi = 0; gi + 1 < gstart.size(); ++gi)
      if (gstart[gi + 1] - gstart[gi] > SHORT_RUN) gsz.push_back(gstart[gi + 1] - gstart[gi]);
    double best = 1e300;
    for (int t = 32; t <= 1024; t += 4) {
      long long w = 0;
      for (int g : gsz) w += (g + t - 1) / t;
      // (a workgroup's iteration takes 4 waves x 6 points with ten lanes per point; its iterations are a third longer than the
      // 4 x 4 of sixteen lanes per point, so the fixed part counts for 5.5 of them where it counted for 7)
      const int ppi = 24;
      const double cost = (double)((w + 511) / 512) * ((double)((t + ppi - 1) / ppi) + 5.5);
      if (cost < best) {
        best = cost;
        target = t;
      }
    }
  }
  // One round of workgroups: when the runs cut at `target` leave resident slots empty (cfg4: 400 workgroups on 512
  // slots, so 112 CUs hold one workgroup and idle half the launch while 144 hold two), the largest pieces are cut
  // once more until the slots are full, and the launch lists the large pieces first: the dispatcher deals the first
  // n_cu workgroups one per CU, so every CU ends up with a large and a small piece or two small ones.  The busiest
  // SIMD then has 250 + 167 points instead of 500.
  const int slots = 2 * std::max(in.n_cu, 1);  // (resident workgroups per CU)
  std::vector<int> parts_of(gstart.size(), 0);
  {
    long long w = 0;
    for (size_t gi = 0; gi + 1 < gstart.size(); ++gi) {
      const int g = gstart[gi + 1] - gstart[gi];
      if (g > SHORT_RUN) w += (parts_of[gi] = (g + target - 1) / target);
    }
    if (w > slots / 2 && w < slots) {
      // (a max-heap on the current piece size; a piece of fewer than 64 points is not worth another workgroup)
      std::vector<std::pair<double, size_t>> heap;
      for (size_t gi = 0; gi + 1 < gstart.size(); ++gi)
        if (parts_of[gi]) heap.push_back({(double)(gstart[gi + 1] - gstart[gi]) / parts_of[gi], gi});
      std::make_heap(heap.begin(), heap.end());
      while (w < slots && !heap.empty()) {
        std::pop_heap(heap.begin(), heap.end());
        const size_t gi = heap.back().second;
        heap.pop_back();
        const int g = gstart[gi + 1] - gstart[gi];
        if (g / (parts_of[gi] + 1) < 64) continue;
        ++parts_of[gi];
        ++w;
        heap.push_back({(double)g / parts_of[gi], gi});
        std::push_heap(heap.begin(), heap.end());
      }
    }
  }
  // Short runs: the pair path sums per camera pair instead of per run, which is what a camera list shared by a dozen points
  // wants -- when there are thousands of such lists.  The path itself costs four launches behind the elimination (33 us of a
  // 220 us iteration at cfg4, measured with ONE such point), so while nothing else needs it (no ragged, unsorted or > 10-camera
  // point) and the short runs are few, each becomes a small piece of the elimination: a workgroup among 512
  // (in.short_pieces = the most short runs that are turned into pieces, 0: none; scripts/gpu_short_runs_ab.py)
  bool short_as_pieces = false;
  {
    int n_short = 0;
    bool pair_path_needed = false;
    for (size_t gi = 0; gi + 1 < gstart.size() && !pair_path_needed; ++gi) {
      const int sp = gstart[gi], n = optr[sp + 1] - optr[sp];
      bool strict = true;
      for (int k = 1; k < n; ++k) strict = strict && ocam[optr[sp] + k - 1] < ocam[optr[sp] + k];
      if (!(n <= 10 && strict)) pair_path_needed = true;
      else if (gstart[gi + 1] - sp <= SHORT_RUN) ++n_short;
    }
    short_as_pieces = !pair_path_needed && n_short > 0 && n_short <= in.short_pieces;
  }
  for (size_t gi = 0; gi + 1 < gstart.size(); ++gi) {
    const int sp = gstart[gi], e = gstart[gi + 1];
    const int n = optr[sp + 1] - optr[sp];
    bool strict = true;
    for (int k = 1; k < n; ++k) strict = strict && ocam[optr[sp] + k - 1] < ocam[optr[sp] + k];
    if (n <= 10 && strict) {
      const int so = (int)sig_cams.size();
      for (int k = 0; k < n; ++k) sig_cams.push_back(ocam[optr[sp] + k]);
      const int nb = (6 * n + 2 + 15) / 16;
      if (e - sp <= SHORT_RUN && !short_as_pieces) {
        sig_cams.resize(so);  // (a camera list shared by few points: the pair path, per-pair instead of per-run sums)
        for (int q = sp; q < e; ++q) fb.push_back(q);
      } else {
        const int parts = std::max(parts_of[gi], 1);
        for (int q = 0; q < parts; ++q) {
          const int lo = sp + (int)((long long)(e - sp) * q / parts), hi = sp + (int)((long long)(e - sp) * (q + 1) / parts);
          ids[nb - 1].push_back((int)chunks.size());
          chunks.push_back(Chunk{so, n, lo, hi - lo});
        }
      }
    } else {
      for (int q = sp; q < e; ++q) fb.push_back(q);
    }
  }
  for (int l = 0; l < 8; ++l)  // large pieces first (stable: equal sizes keep the point order)
    std::stable_sort(ids[l].begin(), ids[l].end(), [&](int a, int c) { return chunks[a].cnt > chunks[c].cnt; });
  if (!chunks.empty()) {
    // the chunks' descriptors for ba_backsub_runs, large first: n, first point, points, first observation, the cameras
    std::vector<int> all(chunks.size());
    for (size_t i = 0; i < all.size(); ++i) all[i] = (int)i;
    std::stable_sort(all.begin(), all.end(), [&](int a, int c) { return chunks[a].cnt > chunks[c].cnt; });
    out.bs_desc.assign(16 * all.size(), 0);
    for (size_t i = 0; i < all.size(); ++i) {
      const Chunk& c = chunks[all[i]];
      int* r = &out.bs_desc[16 * i];
      r[0] = c.n, r[1] = c.p0, r[2] = c.cnt, r[3] = optr[c.p0];
      for (int k = 0; k < c.n && k < 10; ++k) r[4 + k] = sig_cams[c.sig_off + k];
    }
  }
  lap_("chunks");
  // ---- the gather lists of the slab epilogue (ba_gather_slabs): for every destination in `red` the slab entries that
  // add to it, in chunk order; list 0 for a full linearisation, list 1 for the norms-only mode (diagonal only)
  std::vector<int>*gth_ptr = out.gth_ptr, *gth_dest = out.gth_dest, grow_ptr, grow_id, &grow_colmap = out.grow_colmap;
  std::vector<unsigned>* gth_src = out.gth_src;
  std::vector<I4> grow_src, &grow_hdr = out.grow_hdr, &grow_head = out.grow_head, &grow_over = out.grow_over;
  out.elim_deterministic = in.deterministic;
  if (out.elim_deterministic && chunks.size() * (size_t)ELIM_SLAB >= ((size_t)1 << 31)) {
    // the gather lists address a slab entry with 31 bits (bit 31 carries the sign): past ~740 000 chunks the elimination goes
    // back to the atomic epilogue -- said out loud, because the sums are then no longer the same bit patterns run after run
    fprintf(stderr, "sfmhip_ba: %zu chunks exceed the slab epilogue's 31-bit offsets; atomic epilogue (not run-to-run identical)\n",
            chunks.size());
    out.elim_deterministic = false;
  }
  if (out.elim_deterministic && !chunks.empty()) {
    const int ld = in.ld, fo = 6 * n_cam;
    const long long o_g = (long long)redl::g(ld), o_gF = (long long)redl::gF(ld), o_dc = (long long)redl::dc(ld), o_sc = (long long)redl::sc(ld);
    std::vector<std::pair<long long, unsigned>> ent[2];  // (destination, source | sign)
    // rows of S by their own kernel role while a wave's accumulator fits the default LDS limit (until round 6 the accumulator was
    // a whole row, ld entries zeroed and scanned whatever the row held: at 640 cameras that outweighed what the row-wise reads
    // save, and rows of more than 3072 columns went through the per-destination lists -- scripts/gpu_gather_bits.py: 640 cameras
    // 3305 -> 3619 it/s, 1000: 2805 -> 3267, the same bits as the whole-row form wherever that ran).
    // (round 6: a row's accumulator holds only the columns the row can have -- the cameras that share a run with the row's camera,
    // the focal column, g's / the diagonal's / F^T b's entries --, not all ld of them: a wave zeroed and scanned ld entries whatever
    // the row held, which is what kept rows of 640 cameras and more on the per-destination lists)
    // per camera: the cameras of the runs it is in, ascending (tl_flat[tl_off[c] .. tl_off[c + 1])): a bit row per camera first
    std::vector<int> tl_off(n_cam + 1, 0), tl_flat;
    {
      const int wpr_ = (n_cam + 63) / 64;
      std::vector<unsigned long long> bits((size_t)n_cam * wpr_, 0ull);
      std::vector<char> seen_sig(sig_cams.size() + 1, 0);
      for (const Chunk& ch : chunks) {
        if (seen_sig[ch.sig_off]) continue;
        seen_sig[ch.sig_off] = 1;
        for (int a = 0; a < ch.n; ++a) {
          unsigned long long* row = bits.data() + (size_t)sig_cams[ch.sig_off + a] * wpr_;
          for (int c2 = 0; c2 < ch.n; ++c2) row[sig_cams[ch.sig_off + c2] >> 6] |= 1ull << (sig_cams[ch.sig_off + c2] & 63);
        }
      }
      for (int c = 0; c < n_cam; ++c) {
        for (int w = 0; w < wpr_; ++w)
          for (unsigned long long m = bits[(size_t)c * wpr_ + w]; m; m &= m - 1) tl_flat.push_back(64 * w + __builtin_ctzll(m));
        tl_off[c + 1] = (int)tl_flat.size();
      }
    }
    size_t accw = 64;  // a wave's accumulator: 6 entries per camera of the longest list + 4, in whole 64s
    for (int c = 0; c < n_cam; ++c) accw = std::max(accw, (6 * (size_t)(tl_off[c + 1] - tl_off[c]) + 4 + 63) / 64 * 64);
    const bool use_rows = accw * 8 <= 65536;
    out.grow_waves = accw * 8 * 4 <= 65536 ? 4 : accw * 8 * 2 <= 65536 ? 2 : 1;
    out.grow_accw = (int)accw;
    if (use_rows) {
      std::vector<int> cntr((size_t)fo + 1, 0);
      for (const Chunk& ch : chunks)
        for (int sl = 0; sl < ch.n; ++sl)
          for (int i = 0; i < 6; ++i) ++cntr[(size_t)6 * sig_cams[ch.sig_off + sl] + i + 1];
      for (int r = 0; r < fo; ++r) cntr[r + 1] += cntr[r];
      grow_src.resize((size_t)cntr[fo]);
      std::vector<int> pos(cntr.begin(), cntr.end() - 1);
      // the cameras' lists, each behind its length: a row's header points at its camera's
      std::vector<int> clist_of(n_cam, 0);
      for (int c = 0; c < n_cam; ++c) {
        if (tl_off[c + 1] == tl_off[c]) continue;
        grow_colmap.push_back(tl_off[c + 1] - tl_off[c]);
        clist_of[c] = (int)grow_colmap.size();
        grow_colmap.insert(grow_colmap.end(), tl_flat.begin() + tl_off[c], tl_flat.begin() + tl_off[c + 1]);
      }
      // (signature = offset of its camera list, the row's camera's place in it) -> offset of the column map (64 ints)
      std::vector<int> cmap_of(sig_cams.size() + 1, -1);
      for (size_t c = 0; c < chunks.size(); ++c) {  // chunk order inside every row
        const Chunk& ch = chunks[c];
        const int n = ch.n, NBc = (6 * n + 2 + 15) / 16;
        for (int sl = 0; sl < n; ++sl) {
          int& cm = cmap_of[ch.sig_off + sl];
          if (cm < 0) {
            // local column lc < 6 n of the signature -> its place in the accumulator of a row of camera sig[sl]: 6 * (the rank of
            // camera sig[lc / 6] in that camera's list) + lc % 6; behind the nT = 6 * |list| columns of S: the focal column, g's
            // entry, the diagonal's and F^T b's (ba_gather_rows)
            cm = (int)grow_colmap.size();
            const int row_cam = sig_cams[ch.sig_off + sl];
            const int* tl = tl_flat.data() + tl_off[row_cam];
            const int nT = 6 * (tl_off[row_cam + 1] - tl_off[row_cam]);
            grow_colmap.resize((size_t)cm + 64);
            int* o = grow_colmap.data() + cm;
            for (int a = 0, t = 0; a < n; ++a) {  // (both lists ascend: one walk gives every camera's rank)
              while (tl[t] != sig_cams[ch.sig_off + a]) ++t;
              for (int i = 0; i < 6; ++i) o[6 * a + i] = 6 * t + i;
            }
            for (int lc = 6 * n; lc < 62; ++lc) o[lc] = lc == 6 * n ? nT : nT + 1;
            o[62] = nT + 2, o[63] = nT + 3;
          }
          for (int i = 0; i < 6; ++i) {
            const int lr = 6 * sl + i, ti = lr >> 4;
            const int t0 = ti * NBc - ti * (ti - 1) / 2;  // tile (ti, ti)
            const int roff = (t0 * 4 + ((lr & 15) >> 2)) * 64 + (lr & 3) * 16 - 256 * ti;
            const int dcr = (i * 6 - i * (i - 1) / 2) * FP + sl, gfr = (27 + i) * FP + sl;
            grow_src[(size_t)pos[(size_t)6 * sig_cams[ch.sig_off + sl] + i]++] =
                I4{(int)(unsigned)(c * (size_t)ELIM_SLAB), lr | (n << 8) | (roff << 16), cm, dcr | (gfr << 16)};
          }
        }
      }
      for (int r = 0; r < fo; ++r)
        if (cntr[r + 1] > cntr[r]) {
          grow_ptr.push_back(cntr[r]);
          grow_id.push_back(r);
        }
      grow_ptr.push_back(cntr[fo]);
      // a row's first 32 records in a table of their own (fixed stride), the rest in one overflow list
      for (size_t r = 0; r < grow_id.size(); ++r) {
        const int k0 = grow_ptr[r], cnt = grow_ptr[r + 1] - k0;
        grow_hdr.push_back(I4{grow_id[r], cnt, (int)grow_over.size(), clist_of[grow_id[r] / 6]});
        for (int k = 0; k < 32; ++k) grow_head.push_back(k < cnt ? grow_src[(size_t)k0 + k] : I4{0, 0, 0, 0});
        for (int k = 32; k < cnt; ++k) grow_over.push_back(grow_src[(size_t)k0 + k]);
      }
      if (grow_over.empty()) grow_over.push_back(I4{0, 0, 0, 0});
    }
    const long long GMAX = -1;                            // (sorts first; the kernel takes the rank's slot as an argument)
    for (size_t c = 0; c < chunks.size(); ++c) {
      const Chunk& ch = chunks[c];
      const int n = ch.n, NBc = (6 * n + 2 + 15) / 16, NTc = NBc * (NBc + 1) / 2;
      const int* cams = sig_cams.data() + ch.sig_off;
      const unsigned base = (unsigned)(c * (size_t)ELIM_SLAB);
      auto gidx = [&](int l) { return l < 6 * n ? 6 * cams[l / 6] + l % 6 : l == 6 * n ? fo : l == 6 * n + 1 ? -2 : -1; };
      // (ba_gather_rows: the cameras' rows from the row lists above, the focal row chunk by chunk -- nothing of the Gram block
      // goes through the destination lists then, and walking its NTc * 256 entries per chunk was half of this stage's time)
      for (int idx = 0; !use_rows && idx < NTc * 256; ++idx) {  // the Gram block, as the kernel lays it out
        int t = idx >> 8, ti = 0;
        while (t >= NBc - ti) {
          t -= NBc - ti;
          ++ti;
        }
        const int tj = ti + t, gg = (idx >> 6) & 3, ln = idx & 63;
        const int lr = 16 * ti + (ln >> 4) + 4 * gg, lc = 16 * tj + (ln & 15);
        const int gr = gidx(lr), gc = gidx(lc);
        if (gr < 0 || lr > lc || gc == -1) continue;
        ent[0].push_back({gc >= 0 ? (long long)gr * ld + gc : o_g + gr, (base + idx) | 0x80000000u});  // S -= Gram (F^T F folded in)
      }
      for (int e = 0; e < 33; ++e)
        for (int slot = 0; slot < n; ++slot) {
          const unsigned sidx = base + ELIM_SLAB_FF + e * FP + slot;
          const int r0 = 6 * cams[slot];
          if (e < 21) {
            int i = 0, rem = e;
            while (rem >= 6 - i) {
              rem -= 6 - i;
              ++i;
            }
            if (rem == 0) {
              if (!use_rows) ent[0].push_back({o_dc + r0 + i, sidx});
              ent[1].push_back({o_dc + r0 + i, sidx});
            }
          } else if (e >= 27) {
            if (!use_rows) ent[0].push_back({o_gF + r0 + e - 27, sidx});
          }
        }
      const unsigned tail = base + ELIM_SLAB_FF + 36 * FP;
      ent[1].push_back({o_dc + fo, tail});
      if (!use_rows) {
        ent[0].push_back({o_dc + fo, tail});
        ent[0].push_back({o_gF + fo, tail + 1});
        ent[0].push_back({o_sc + 0, tail + 2});
        ent[0].push_back({GMAX, tail + 3});
        ent[0].push_back({o_sc + 2, tail + 4});
      }
    }
    for (int m = 0; m < 2; ++m) {
      const size_t range = redl::red2(ld) + 2;   // destinations + the GMAX key shifted to 0
      if (ent[m].size() * 16 < range) {
        // few entries for the range (the row lists carry S: what is left are the diagonal's entries): a stable sort of the
        // entries instead of three passes over ld^2 counters (cfg4: 31 k entries, 1.5 M destinations)
        std::stable_sort(ent[m].begin(), ent[m].end(), [](const std::pair<long long, unsigned>& a, const std::pair<long long, unsigned>& c) { return a.first < c.first; });
        gth_src[m].resize(ent[m].size());
        for (size_t k = 0; k < ent[m].size(); ++k) {
          gth_src[m][k] = ent[m][k].second;
          if (k == 0 || ent[m][k].first != ent[m][k - 1].first) {
            gth_ptr[m].push_back((int)k);
            gth_dest[m].push_back((int)ent[m][k].first);
          }
        }
        gth_ptr[m].push_back((int)ent[m].size());
        continue;
      }
      // counting sort by destination (stable: a destination's sources stay in chunk order)
      std::vector<int> cnt(range + 1, 0);
      for (const auto& e : ent[m]) ++cnt[(size_t)(e.first + 1) + 1];
      for (size_t k = 0; k < range; ++k) cnt[k + 1] += cnt[k];
      gth_src[m].resize(ent[m].size());
      {
        std::vector<int> pos(cnt.begin(), cnt.end() - 1);
        for (const auto& e : ent[m]) gth_src[m][(size_t)pos[(size_t)(e.first + 1)]++] = e.second;
      }
      for (size_t k = 0; k < range; ++k)
        if (cnt[k + 1] > cnt[k]) {
          gth_ptr[m].push_back(cnt[k]);
          gth_dest[m].push_back((int)((long long)k - 1));
        }
      gth_ptr[m].push_back((int)ent[m].size());
    }
  }
  lap_("gather lists");
  // ---- camera co-visibility (one bit row per camera) for the dissection of the reduced system
  if (n_cam <= 4096) {  // (from one camera on: a small system is one front)
    const int wpr = (n_cam + 63) / 64;
    out.adj.assign((size_t)n_cam * wpr, 0ull);
    auto add_clique = [&](const int* cs, int n) {
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) out.adj[(size_t)cs[i] * wpr + (cs[j] >> 6)] |= 1ull << (cs[j] & 63);
    };
    std::vector<char> is_fb(np, 0);
    for (int q : fb) is_fb[q] = 1;
    for (size_t gi = 0; gi + 1 < gstart.size(); ++gi) {
      const int sp = gstart[gi];
      if (!is_fb[sp]) add_clique(&ocam[optr[sp]], optr[sp + 1] - optr[sp]);  // one signature per run
    }
    for (int q : fb) add_clique(&ocam[optr[q]], optr[q + 1] - optr[q]);
    lap_("camera graph");
  }
  // ---- the pair path's lists (ba_pp_points / ba_pp_pairs / ba_cam_blocks): its points in ascending sorted order, a
  //      row of T per observation, the camera-major list of those observations, and per camera pair that a point
  //      sees together the (row of a, row of b) entries
  std::sort(fb.begin(), fb.end());
  std::vector<int>&cptr = out.cptr, &cpt = out.cpt, &pp_obase = out.pp_obase, &pair_ptr = out.pair_ptr;
  std::vector<I2>&cslot = out.cslot, &pair_cams = out.pair_cams, &pair_ent = out.pair_ent;
  std::vector<double>& cxy = out.cxy;
  cptr.assign(n_cam + 1, 0);
  pp_obase.assign(fb.size() + 1, 0);
  pair_ptr.assign(1, 0);
  {
    for (size_t i = 0; i < fb.size(); ++i) pp_obase[i + 1] = pp_obase[i] + (optr[fb[i] + 1] - optr[fb[i]]);
    const size_t nfo = (size_t)pp_obase[fb.size()];
    cpt.resize(nfo);
    cslot.resize(nfo);
    cxy.resize(2 * nfo);
    out.cxy_src.resize(nfo);
    for (int sp : fb)
      for (int k = optr[sp]; k < optr[sp + 1]; ++k) cptr[ocam[k] + 1]++;
    for (int c = 0; c < n_cam; ++c) cptr[c + 1] += cptr[c];
    std::vector<int> fill(cptr.begin(), cptr.end() - 1);
    struct PE {
      long long key;
      int a, b;
    };
    std::vector<PE> pes;
    for (size_t i = 0; i < fb.size(); ++i) {  // ascending sorted point index: the order inside a camera is the stable one
      const int sp = fb[i], k0 = optr[sp], n = optr[sp + 1] - k0;
      for (int o = 0; o < n; ++o) {
        const int dst = fill[ocam[k0 + o]]++;
        cpt[dst] = sp;
        cslot[dst] = I2{pp_obase[i] + o, (int)i};
        out.cxy_src[dst] = k0 + o;
        cxy[2 * (size_t)dst] = obs_xy[2 * (size_t)out.obs_src[k0 + o]];
        cxy[2 * (size_t)dst + 1] = obs_xy[2 * (size_t)out.obs_src[k0 + o] + 1];
        for (int o2 = o + 1; o2 < n; ++o2) {
          int ca = ocam[k0 + o], cb = ocam[k0 + o2], ra = pp_obase[i] + o, rb = pp_obase[i] + o2;
          if (ca > cb) std::swap(ca, cb), std::swap(ra, rb);
          pes.push_back(PE{(long long)ca * n_cam + cb, ra, rb});
        }
      }
    }
    std::sort(pes.begin(), pes.end(), [](const PE& x, const PE& y) { return x.key != y.key ? x.key < y.key : (x.a != y.a ? x.a < y.a : x.b < y.b); });
    for (size_t e = 0; e < pes.size(); ++e) {
      if (e == 0 || pes[e].key != pes[e - 1].key) {
        if (e) pair_ptr.push_back((int)e);
        pair_cams.push_back(I2{(int)(pes[e].key / n_cam), (int)(pes[e].key % n_cam)});
      }
      pair_ent.push_back(I2{pes[e].a, pes[e].b});
    }
    if (!pes.empty()) pair_ptr.push_back((int)pes.size());
    // (a workgroup per (camera, slice): ~1024 entries each, so that the 69-value block reduction is paid once per four
    // entries of a thread: 57 -> 25 us at 200 cameras x 1000 observations)
    out.cam_split = (int)std::max<size_t>(1, std::min<size_t>(64, nfo / (size_t)std::max(n_cam, 1) / 1024));
  }
  lap_("camera-major copy");
  return SFMHIP_OK;
}

}  // namespace bsetup
