// ransac_host.h -- the host half of OpenCV 3.4.1's RANSACPointSetRegistrator (calib3d/ptsetreg.cpp) that the essential-matrix,
// homography and PnP RANSACs share: cv::RNG as run() seeds it, getSubset's distinct-index draw of five indices,
// RANSACUpdateNumIters, and run()'s loop itself, replayed in chunks of iterations over a backend (ransac_replay: score.hip
// and pnp.hip launch kernels for it, the CPU test stubs loop or answer from tables).  Host code only.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <map>
#include <vector>

namespace sfmransac {

struct CvRng {
  unsigned long long state = 0xFFFFFFFFFFFFFFFFull;  // RNG rng((uint64)-1)
  unsigned next() {
    state = (unsigned long long)(unsigned)state * 4164903690U + (unsigned)(state >> 32);
    return (unsigned)state;
  }
  int uniform(int a, int b) { return a == b ? a : (int)(next() % (unsigned)(b - a) + a); }
};
struct SampleStream {  // the samples of one match count, generated on demand
  CvRng rng;
  std::vector<int> idx;  // 5 per iteration
  void extend(int count, int n_iters) {
    while ((int)idx.size() < 5 * n_iters) {
      int s[5];
      for (int i = 0; i < 5;) {
        const int v = rng.uniform(0, count);
        int j = 0;
        for (; j < i; ++j)
          if (s[j] == v) break;
        if (j < i) continue;  // drawn before: again
        s[i++] = v;
      }
      idx.insert(idx.end(), s, s + 5);
    }
  }
};
// the sampler of the essential-matrix and PnP RANSACs: a sample depends on the correspondence count alone, so every view
// of a count reads the same stream
struct CountSamples {
  std::map<int, SampleStream> streams;
  const int* rows(int /*view*/, int count, int first, int n) {
    SampleStream& ss = streams[count];
    ss.extend(count, first + n);
    return ss.idx.data() + 5 * (size_t)first;
  }
};
// cv::RANSACUpdateNumIters (calib3d/ptsetreg.cpp), with the host libm as the reference runs it
inline int ransac_update_num_iters(double p, double ep, int model_points, int max_iters) {
  p = std::max(p, 0.0);
  p = std::min(p, 1.0);
  ep = std::max(ep, 0.0);
  ep = std::min(ep, 1.0);
  double num = std::max(1.0 - p, DBL_MIN);
  double denom = 1.0 - std::pow(1.0 - ep, model_points);
  if (denom < DBL_MIN) return 0;
  num = std::log(num);
  denom = std::log(denom);
  return denom >= 0 || -num >= max_iters * (-denom) ? max_iters : (int)std::nearbyint(num / denom);  // cvRound
}

struct ViewState {
  int count, niters, iter, best, best_it;
  bool done;
  int status;  // 1: a model; 0: none; -1: fewer than the model's points
};
struct Job {  // one active view of a chunk (the kernels read it too)
  int view;
  int off;    // first correspondence of the view in the point arrays
  int count;  // correspondences
  int samp;   // first row of its sample table (one row of model points per iteration) for this chunk
};
struct Keep {  // model `slot` (sample slot * models per sample + model) of the last chunk becomes view `view`'s best
  int slot, view;
};
// what the mask kernels read: 0 no model (mask 0), 1 a RANSAC model, 2 exactly the model's points (every one an inlier)
inline unsigned char has_code(int status, int count, int model_points) { return status == 1 ? (count == model_points ? 2 : 1) : 0; }

// RANSACPointSetRegistrator::run per view, in chunks of iterations (32, then doubling up to 256).  mp = points per sample,
// M = the most models a sample gives, limit = the iteration limit every view starts from.  draw.rows(view, count, first, n)
// = n sample rows (mp indices each) of a view from its iteration `first`; a row of -1 says getSubset gave up there, which
// ends the view's loop at that iteration.  The backend solves and scores every (view, iteration) sample of a chunk --
// be.run_chunk(jobs, chunk, samples, ok, counts) fills ok[slot] = models | flags << 8 and counts[slot * M + m] = the
// inliers of model m, slot = job * chunk + iteration -- and keeps the models named by be.keep_best(keeps) before the next
// chunk overwrites them.  The rule: the models of a sample in order, a model replaces the best when its count exceeds
// max(best, mp - 1); the limit is then RANSACUpdateNumIters(confidence, (count - good) / count, mp, limit), and slots past
// a limit that dropped inside the chunk are not looked at.  A view of exactly mp correspondences is its one sample (every
// point an inlier when it gives a model).  Returns the backend's first non-zero status.
template <class Backend, class Sampler>
int ransac_replay(Backend& be, Sampler& draw, int mp, int M, int n_views, const int32_t* offsets, double confidence, int limit,
                  std::vector<ViewState>& vs, int& flags_any) {
  vs.resize((size_t)n_views);
  for (int v = 0; v < n_views; ++v) {
    ViewState& s = vs[v];
    s.count = offsets[v + 1] - offsets[v];
    s.niters = limit;
    s.iter = 0;
    s.best = 0;
    s.best_it = -1;
    s.status = s.count < mp ? -1 : 0;
    s.done = s.count < mp || (s.count > mp && s.niters == 0);
  }
  std::vector<Job> jobs;
  std::vector<int> samples, ok, counts;
  std::vector<Keep> keeps;
  int chunk = 32;
  for (;;) {
    jobs.clear();
    samples.clear();
    for (int v = 0; v < n_views; ++v) {
      const ViewState& s = vs[v];
      if (s.done) continue;
      jobs.push_back(Job{v, offsets[v], s.count, (int)(samples.size() / mp)});
      if (s.count == mp) {
        for (int it = 0; it < chunk; ++it)
          for (int k = 0; k < mp; ++k) samples.push_back(k);
      } else {
        const int* r = draw.rows(v, s.count, s.iter, chunk);
        samples.insert(samples.end(), r, r + (size_t)mp * chunk);
      }
    }
    if (jobs.empty()) break;
    const size_t slots = jobs.size() * (size_t)chunk;
    ok.resize(slots);
    counts.resize(slots * M);
    const int rc = be.run_chunk(jobs, chunk, samples, ok, counts);
    if (rc) return rc;
    keeps.clear();
    for (size_t j = 0; j < jobs.size(); ++j) {
      ViewState& s = vs[jobs[j].view];
      if (s.count == mp) {
        const size_t slot = j * chunk;
        flags_any |= ok[slot] >> 8;
        if ((ok[slot] & 0xff) > 0) {
          s.best = mp;
          s.status = 1;
          keeps.push_back(Keep{(int)(slot * M), jobs[j].view});
        }
        s.done = true;
        continue;
      }
      long long keep = -1;  // the last model of this chunk that raised the best count
      for (int it = 0; it < chunk && s.iter < s.niters; ++it, ++s.iter) {
        const size_t slot = j * chunk + it;
        if (samples[((size_t)jobs[j].samp + it) * mp] < 0) {  // getSubset failed: run() leaves the loop (iter 0: no model at all)
          s.niters = s.iter;
          break;
        }
        flags_any |= ok[slot] >> 8;
        for (int m = 0; m < (ok[slot] & 0xff); ++m) {
          const int good = counts[slot * M + m];
          if (good > std::max(s.best, mp - 1)) {
            s.best = good;
            s.best_it = s.iter;
            s.status = 1;
            keep = (long long)(slot * M + m);
            s.niters = ransac_update_num_iters(confidence, (double)(s.count - good) / s.count, mp, s.niters);
          }
        }
      }
      if (keep >= 0) keeps.push_back(Keep{(int)keep, jobs[j].view});
      if (s.iter >= s.niters) s.done = true;
    }
    if (!keeps.empty()) {
      const int rk = be.keep_best(keeps);
      if (rk) return rk;
    }
    chunk = std::min(2 * chunk, 256);
  }
  return 0;
}

}  // namespace sfmransac
