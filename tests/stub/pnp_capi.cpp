// pnp_capi.cpp -- a C surface over csrc/pnp.h for tests/test_pnp_cpu.py and tests/test_gpu_pnp.py (built with g++ -O2
// -ffp-contract=off): sfmhip_pnp_ransac and sfmhip_pnp_epnp the way pnp.hip's kernels compute them, from the same header,
// on one CPU thread.  The RANSAC loop is the header's ransac_replay with a backend that loops where the device launches.
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/pnp.h"

namespace {

using namespace sfmpnp;

// the fixed-order sum (pnp.h) by one thread for any number of points
struct ReduceTree {
  std::vector<double> part;
  template <int K, class F>
  void run(int n, F f, Mem<1> w) {
    part.assign((size_t)SLOTS * K, 0.0);
    double t[K];
    for (int i = 0; i < n; ++i) {
      f(i, t);
      for (int k = 0; k < K; ++k) part[(size_t)(i % SLOTS) * K + k] += t[k];
    }
    for (int g = 0; g < SLOTS / 64; ++g)
      for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; ++l)
          for (int k = 0; k < K; ++k) part[(size_t)(g * 64 + l) * K + k] += part[(size_t)(g * 64 + l + off) * K + k];
    for (int k = 0; k < K; ++k)
      w[W_ACC + k] = (part[k] + part[(size_t)64 * K + k]) + (part[(size_t)128 * K + k] + part[(size_t)192 * K + k]);
  }
};

struct ListPoints {  // explicit f64 points, optionally through an index list
  int n;
  const double* xyz;
  const double* uv;
  const int* idx;
  void get(int i, double* p, double* q) const {
    const int k = idx ? idx[i] : i;
    for (int j = 0; j < 3; ++j) p[j] = xyz[3 * (size_t)k + j];
    q[0] = uv[2 * (size_t)k];
    q[1] = uv[2 * (size_t)k + 1];
  }
};

int epnp_list(int n, const double* xyz, const double* uv, const int* idx, double* R, double* t) {
  std::vector<double> work(WORK_DOUBLES, 0.0);
  ListPoints pts{n, xyz, uv, idx};
  ReduceTree red;
  for (int k = 0; k < 9; ++k) R[k] = 0;
  for (int k = 0; k < 3; ++k) t[k] = 0;
  return epnp_solve<1>(pts, red, Mem<1>{work.data()}, R, t);
}

struct CpuBackend {
  const float* xyz;
  const float* xy;
  const double* K;
  const double* dist;
  const float* thr2;  // per view
  std::vector<double> models;       // 6 per slot of the last chunk
  std::vector<double> best;         // 6 per view
  std::vector<double> work = std::vector<double>(WORK_DOUBLES, 0.0);
  int run_chunk(const std::vector<Job>& jobs, int chunk, const std::vector<int>& samples, std::vector<int>& ok, std::vector<int>& counts) {
    models.assign(ok.size() * 6, 0.0);
    for (size_t j = 0; j < jobs.size(); ++j)
      for (int it = 0; it < chunk; ++it) {
        const size_t slot = j * chunk + it;
        const int* s = samples.data() + ((size_t)jobs[j].samp + it) * 5;
        float P3[5][3], P2[5][2];
        for (int k = 0; k < 5; ++k) {
          const size_t m = (size_t)jobs[j].off + s[k];
          for (int c = 0; c < 3; ++c) P3[k][c] = xyz[3 * m + c];
          for (int c = 0; c < 2; ++c) P2[k][c] = xy[2 * m + c];
        }
        ok[slot] = solve_sample<1>(P3, P2, K, dist, Mem<1>{work.data()}, &models[slot * 6]);
        int cnt = 0;
        if (ok[slot] & 0xff) {
          double P[12];
          pose_matrix(&models[slot * 6], &models[slot * 6 + 3], P);
          for (int i = 0; i < jobs[j].count; ++i) {
            const size_t m = (size_t)jobs[j].off + i;
            cnt += reproj_err2(P, K, dist, xyz[3 * m], xyz[3 * m + 1], xyz[3 * m + 2], xy[2 * m], xy[2 * m + 1]) <= thr2[jobs[j].view];
          }
        }
        counts[slot] = cnt;
      }
    return 0;
  }
  int keep_best(const std::vector<Keep>& keeps) {
    for (const Keep& k : keeps) std::memcpy(&best[(size_t)k.view * 6], &models[(size_t)k.slot * 6], 6 * sizeof(double));
    return 0;
  }
};

}  // namespace

extern "C" {

void pnp_sincos(double x, double* sc) { sincos_restated(x, sc[0], sc[1]); }
double pnp_acos(double x) { return acos_restated(x); }
void pnp_rodrigues_to_matrix(const double* rv, double* R) { rodrigues_to_matrix(rv, R); }
int pnp_rodrigues_to_vector(const double* R, double* rv) { return rodrigues_to_vector(R, rv); }

// the first n_iters samples (5 indices each) that a view of `count` correspondences draws
void pnp_samples(int count, int n_iters, int32_t* out) {
  sfmransac::SampleStream ss;
  ss.extend(count, n_iters);
  for (int i = 0; i < 5 * n_iters; ++i) out[i] = ss.idx[i];
}

// one sample's model (rvec, tvec) from five float correspondences; returns models | flags << 8
int pnp_sample(const float* xyz5, const float* xy5, const double* K, const double* dist, double* model) {
  std::vector<double> work(WORK_DOUBLES, 0.0);
  float P3[5][3], P2[5][2];
  for (int k = 0; k < 5; ++k) {
    for (int c = 0; c < 3; ++c) P3[k][c] = xyz5[3 * k + c];
    for (int c = 0; c < 2; ++c) P2[k][c] = xy5[2 * k + c];
  }
  return solve_sample<1>(P3, P2, K, dist, Mem<1>{work.data()}, model);
}

// the inliers of a model over n float correspondences (mask nullable)
int pnp_count(int n, const float* xyz, const float* xy, const double* K, const double* dist, const double* model, double thr,
              uint8_t* mask) {
  double P[12];
  pose_matrix(model, model + 3, P);
  const float t = (float)(thr * thr);
  int cnt = 0;
  for (int i = 0; i < n; ++i) {
    const bool in = reproj_err2(P, K, dist, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], xy[2 * i], xy[2 * i + 1]) <= t;
    cnt += in;
    if (mask) mask[i] = in;
  }
  return cnt;
}

// sfmhip_pnp_epnp's twin; flags: OR over the problems
int pnp_epnp(int n_problems, const int32_t* offsets, const double* xyz, const double* xy_normalised, double* R, double* t, int32_t* flags) {
  int fl = 0;
  for (int p = 0; p < n_problems; ++p) {
    const int o = offsets[p], n = offsets[p + 1] - o;
    if (n < MODEL_POINTS) return -2;
    fl |= epnp_list(n, xyz + 3 * (size_t)o, xy_normalised + 2 * (size_t)o, nullptr, R + 9 * (size_t)p, t + 3 * (size_t)p);
  }
  *flags = fl;
  return 0;
}

// sfmhip_pnp_ransac's twin (nullable outputs as there); flags: what sfmhip_pnp_last_flags would report
int pnp_ransac(int n_views, const int32_t* offsets, const double* xyz, const double* xy, const double* K, const double* dist,
               const double* thresholds, double confidence, int max_iters, int32_t* status, double* rvec, double* tvec,
               double* rvec_ransac, double* tvec_ransac, double* rvec_refit, double* tvec_refit, int32_t* inliers, uint8_t* mask,
               int32_t* iterations, int32_t* flags) {
  const size_t total = (size_t)offsets[n_views];
  std::vector<float> fxyz(3 * total + 1), fxy(2 * total + 1), thr2((size_t)n_views);
  for (size_t i = 0; i < 3 * total; ++i) fxyz[i] = (float)xyz[i];
  for (size_t i = 0; i < 2 * total; ++i) fxy[i] = (float)xy[i];
  for (int v = 0; v < n_views; ++v) thr2[v] = (float)(thresholds[v] * thresholds[v]);
  CpuBackend be{fxyz.data(), fxy.data(), K, dist, thr2.data()};
  be.best.assign((size_t)n_views * 6, 0.0);
  std::vector<ViewState> vs;
  int fl = 0;
  ransac_replay(be, n_views, offsets, confidence, max_iters, vs, fl);
  for (int v = 0; v < n_views; ++v) {
    const int o = offsets[v], n = offsets[v + 1] - o;
    const double* m = &be.best[(size_t)v * 6];
    status[v] = vs[v].status;
    inliers[v] = vs[v].best;
    if (iterations) iterations[v] = vs[v].iter;
    double refit[6] = {0, 0, 0, 0, 0, 0};
    std::vector<uint8_t> mk((size_t)n, 0);
    if (vs[v].status == 1) {
      if (n == MODEL_POINTS) {
        std::fill(mk.begin(), mk.end(), 1);
      } else {
        double P[12];
        pose_matrix(m, m + 3, P);
        for (int i = 0; i < n; ++i) {
          const size_t k = (size_t)o + i;
          mk[i] = reproj_err2(P, K, dist, fxyz[3 * k], fxyz[3 * k + 1], fxyz[3 * k + 2], fxy[2 * k], fxy[2 * k + 1]) <= thr2[v];
        }
      }
      // the refit: EPnP on the inliers, the float points taken back to f64, undistortPoints in f64
      std::vector<int> idx;
      std::vector<double> pw(3 * (size_t)n), uv(2 * (size_t)n);
      for (int i = 0; i < n; ++i) {
        const size_t k = (size_t)o + i;
        if (mk[i]) idx.push_back(i);
        for (int c = 0; c < 3; ++c) pw[3 * (size_t)i + c] = (double)fxyz[3 * k + c];
        sfmcam::undistort_point(K, dist, (double)fxy[2 * k], (double)fxy[2 * k + 1], uv[2 * (size_t)i], uv[2 * (size_t)i + 1]);
      }
      double R[9], t[3];
      const int rf = epnp_list((int)idx.size(), pw.data(), uv.data(), idx.data(), R, t);
      fl |= rf;
      if (!(rf & FLAG_RANK_DEFICIENT)) {
        fl |= rodrigues_to_vector(R, refit);
        for (int k = 0; k < 3; ++k) refit[3 + k] = t[k];
      }
    }
    for (int k = 0; k < 3; ++k) {
      rvec[3 * v + k] = m[k];
      tvec[3 * v + k] = m[3 + k];
      if (rvec_ransac) rvec_ransac[3 * v + k] = m[k];
      if (tvec_ransac) tvec_ransac[3 * v + k] = m[3 + k];
      if (rvec_refit) rvec_refit[3 * v + k] = refit[k];
      if (tvec_refit) tvec_refit[3 * v + k] = refit[3 + k];
    }
    if (mask)
      for (int i = 0; i < n; ++i) mask[(size_t)o + i] = mk[i];
  }
  *flags = fl;
  return 0;
}

}  // extern "C"
