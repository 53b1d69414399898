// C entry points over csrc/ba_setup.h for tests/test_ba_setup.py (host only, no HIP): the set-up of a problem, its arrays by
// name, and the host pool's nested and throwing passes.  Built with -DBSETUP_MAIN it is a program that runs one set-up read
// from a file and both pool passes (the test's sanitizer build).
#include "../../sfm_danpipeline_amd/csrc/ba_setup.h"
#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>

extern "C" void* bsetup_run(int n_cam, int n_pt, int n_obs, const int32_t* obs_cam, const int32_t* obs_pt, const double* obs_xy,
                            int ld, int n_cu, int deterministic, int short_pieces, int threads, int* status) {
  bsetup::Input in;
  in.n_cam = n_cam, in.n_pt = n_pt, in.n_obs = n_obs;
  in.obs_cam = obs_cam, in.obs_pt = obs_pt, in.obs_xy = obs_xy;
  in.ld = ld, in.n_cu = n_cu, in.deterministic = deterministic != 0, in.short_pieces = short_pieces, in.threads = threads;
  bsetup::Scratch scratch;
  auto* s = new bsetup::Setup();
  *status = bsetup::build(in, scratch, *s);
  return s;
}

extern "C" void bsetup_free(void* h) { delete (bsetup::Setup*)h; }

extern "C" int bsetup_scalar(void* h, const char* name) {
  const bsetup::Setup& s = *(const bsetup::Setup*)h;
  const std::string n = name;
  if (n == "np") return s.np;
  if (n == "no") return s.no;
  if (n == "cam_split") return s.cam_split;
  if (n == "grow_waves") return s.grow_waves;
  if (n == "grow_accw") return s.grow_accw;
  if (n == "elim_deterministic") return s.elim_deterministic;
  return -1;
}

// the array `name` (ids0..ids7, gth_ptr0/1, ...): its data, *count elements of *elem_bytes bytes; *elem_bytes stays as it was
// when the name is unknown
extern "C" const void* bsetup_array(void* h, const char* name, long long* count, int* elem_bytes) {
  const bsetup::Setup& s = *(const bsetup::Setup*)h;
  const std::string n = name;
  auto ret = [&](const auto& v) -> const void* {
    *count = (long long)v.size();
    *elem_bytes = (int)sizeof(v[0]);
    return v.data();
  };
  if (n == "order") return ret(s.order);
  if (n == "optr") return ret(s.optr);
  if (n == "ocam") return ret(s.ocam);
  if (n == "obs_src") return ret(s.obs_src);
  if (n == "cam_used") return ret(s.cam_used);
  if (n == "chunks") return ret(s.chunks);
  if (n.size() == 4 && n.compare(0, 3, "ids") == 0 && n[3] >= '0' && n[3] < '8') return ret(s.ids[n[3] - '0']);
  if (n == "sig_cams") return ret(s.sig_cams);
  if (n == "bs_desc") return ret(s.bs_desc);
  if (n == "gth_ptr0" || n == "gth_ptr1") return ret(s.gth_ptr[n.back() - '0']);
  if (n == "gth_dest0" || n == "gth_dest1") return ret(s.gth_dest[n.back() - '0']);
  if (n == "gth_src0" || n == "gth_src1") return ret(s.gth_src[n.back() - '0']);
  if (n == "grow_colmap") return ret(s.grow_colmap);
  if (n == "grow_hdr") return ret(s.grow_hdr);
  if (n == "grow_head") return ret(s.grow_head);
  if (n == "grow_over") return ret(s.grow_over);
  if (n == "adj") return ret(s.adj);
  if (n == "fb") return ret(s.fb);
  if (n == "pp_obase") return ret(s.pp_obase);
  if (n == "cptr") return ret(s.cptr);
  if (n == "cpt") return ret(s.cpt);
  if (n == "cxy_src") return ret(s.cxy_src);
  if (n == "pair_ptr") return ret(s.pair_ptr);
  if (n == "cslot") return ret(s.cslot);
  if (n == "pair_cams") return ret(s.pair_cams);
  if (n == "pair_ent") return ret(s.pair_ent);
  if (n == "cxy") return ret(s.cxy);
  return nullptr;
}

// a pass of nth threads over `outer` items whose every item runs a pass of its own over `inner` items: hits[i * inner + j]
// counts the visits of (i, j)
extern "C" void bsetup_pool_nested(int outer, int inner, int nth, int* hits) {
  bsetup::host_parallel_for_t(outer, nth, [&](int, int lo, int hi) {
    for (int i = lo; i < hi; ++i)
      bsetup::host_parallel_for_t(inner, nth, [&](int, int lo2, int hi2) {
        for (int j = lo2; j < hi2; ++j) ++hits[(size_t)i * inner + j];
      });
  });
}

// a pass whose thread 0 throws at once while the other threads sleep 50 ms and then mark their items: 1 when the exception
// arrived, and by then done[] holds every item of threads 1..nth-1
extern "C" int bsetup_pool_throw(int n, int nth, int* done) {
  try {
    bsetup::host_parallel_for_t(n, nth, [&](int t, int lo, int hi) {
      if (t == 0) throw std::runtime_error("thread 0");
      std::this_thread::sleep_for(std::chrono::milliseconds(50));
      for (int j = lo; j < hi; ++j) done[j] = 1;
    });
  } catch (const std::runtime_error&) {
    return 1;
  }
  return 0;
}

#ifdef BSETUP_MAIN
// bsetup_asan <file>: int32 header [n_cam, n_pt, n_obs, ld, n_cu, threads], obs_cam, obs_pt (int32), obs_xy (f64); prints the
// set-up's sizes, then runs both pool passes
#include <cstdio>
#include <vector>
int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  int hd[6];
  if (fread(hd, sizeof(int), 6, f) != 6) return 2;
  const int n_obs = hd[2];
  std::vector<int32_t> oc(n_obs), op(n_obs);
  std::vector<double> xy(2 * (size_t)n_obs);
  if (fread(oc.data(), 4, n_obs, f) != (size_t)n_obs || fread(op.data(), 4, n_obs, f) != (size_t)n_obs ||
      fread(xy.data(), 8, 2 * (size_t)n_obs, f) != 2 * (size_t)n_obs)
    return 2;
  fclose(f);
  int status = 0;
  void* h = bsetup_run(hd[0], hd[1], n_obs, oc.data(), op.data(), xy.data(), hd[3], hd[4], 1, 512, hd[5], &status);
  const bsetup::Setup& s = *(const bsetup::Setup*)h;
  printf("status %d np %d no %d chunks %zu fb %zu pairs %zu gth %zu %zu rows %zu\n", status, s.np, s.no, s.chunks.size(),
         s.fb.size(), s.pair_cams.size(), s.gth_src[0].size(), s.gth_src[1].size(), s.grow_hdr.size());
  bsetup_free(h);
  std::vector<int> hits(64 * 50, 0), done(40000, 0);
  bsetup_pool_nested(64, 50, 4, hits.data());
  int bad = 0;
  for (int x : hits) bad += x != 1;
  const int thrown = bsetup_pool_throw(40000, 4, done.data());
  for (int j = 10000; j < 40000; ++j) bad += done[j] != 1;
  printf("pool nested+throw %s\n", bad == 0 && thrown == 1 ? "ok" : "BAD");
  return 0;
}
#endif
