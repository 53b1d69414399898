// pose_capi.cpp -- a C surface over csrc/pose.h for tests/test_pose_cpu.py (built with g++ -O2 -ffp-contract=off) and, with
// -DPOSE_MAIN, a driver that runs one pair from a file under the sanitizers.  recoverPose for ONE pair, the way
// pose.hip's two kernels compute it, from the same header.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../sfm_danpipeline_amd/csrc/pose.h"

extern "C" {

int pose_decompose(const double* E, double* R1, double* R2, double* t) { return sfmpose::decompose_essential(E, R1, R2, t); }

void pose_normalize(double u, double v, double f, double ppx, double ppy, double* xy) { sfmpose::normalize(u, v, f, ppx, ppy, xy[0], xy[1]); }

// returns the chosen candidate (0..3); counts[4]: the four counts; flags: decompose_essential's
int pose_recover(int n, const double* xy1, const double* xy2, const double* E, double f, double ppx, double ppy, double dist_thr,
                 const uint8_t* mask_in, double* R, double* t, int32_t* n_good, uint8_t* mask_out, int32_t* counts, int32_t* flags) {
  double R1[9], R2[9], tt[3], P[4][12];
  *flags = sfmpose::decompose_essential(E, R1, R2, tt);
  for (int c = 0; c < 4; ++c) sfmpose::candidate(R1, R2, tt, c, P[c]);
  std::vector<unsigned char> codes((size_t)n);
  int g[4] = {0, 0, 0, 0};
  for (int i = 0; i < n; ++i) {
    unsigned bits = sfmpose::candidate_bits(P, xy1[2 * i], xy1[2 * i + 1], xy2[2 * i], xy2[2 * i + 1], f, ppx, ppy, dist_thr);
    if (mask_in && !mask_in[i]) bits = 0;
    codes[i] = (unsigned char)bits;
    for (int c = 0; c < 4; ++c) g[c] += (bits >> c) & 1;
  }
  const int sel = sfmpose::select_candidate(g);
  for (int k = 0; k < 9; ++k) R[k] = (sel & 1) ? R2[k] : R1[k];
  for (int k = 0; k < 3; ++k) t[k] = (sel & 2) ? -tt[k] : tt[k];
  *n_good = g[sel];
  for (int c = 0; c < 4; ++c) counts[c] = g[c];
  if (mask_out)
    for (int i = 0; i < n; ++i) mask_out[i] = ((codes[i] >> sel) & 1) ? (mask_in ? mask_in[i] : (uint8_t)255) : (uint8_t)0;
  return sel;
}

double pose_fullpivlu_det(const double* R) { return sfmpose::fullpivlu_det3(R); }
int pose_coherent_det(double det) { return sfmpose::coherent_det(det) ? 1 : 0; }
int pose_check_rotation(const double* R) { return sfmpose::coherent_det(sfmpose::fullpivlu_det3(R)) ? 1 : 0; }

}  // extern "C"

#ifdef POSE_MAIN
// in.bin: i32 n, i32 has_mask, f64 f, ppx, ppy, dist, f64 E[9], n x f64 xy1[2], n x f64 xy2[2], (has_mask) n x u8 mask.
// stdout: "sel <s> n_good <g> counts <c0> <c1> <c2> <c3> flags <f>", then R and t as 12 hex words
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* fi = fopen(argv[1], "rb");
  if (!fi) return 2;
  int32_t hdr[2];
  double par[4], E[9];
  if (fread(hdr, 4, 2, fi) != 2 || fread(par, 8, 4, fi) != 4 || fread(E, 8, 9, fi) != 9) return 2;
  const int n = hdr[0];
  std::vector<double> a(2 * (size_t)n), b(2 * (size_t)n);
  std::vector<uint8_t> m((size_t)n), out((size_t)n);
  if (fread(a.data(), 8, a.size(), fi) != a.size() || fread(b.data(), 8, b.size(), fi) != b.size()) return 2;
  if (hdr[1] && fread(m.data(), 1, m.size(), fi) != m.size()) return 2;
  fclose(fi);
  double R[9], t[3];
  int32_t ng = 0, counts[4], flags = 0;
  const int sel = pose_recover(n, a.data(), b.data(), E, par[0], par[1], par[2], par[3], hdr[1] ? m.data() : nullptr, R, t, &ng,
                               out.data(), counts, &flags);
  std::printf("sel %d n_good %d counts %d %d %d %d flags %d\n", sel, ng, counts[0], counts[1], counts[2], counts[3], flags);
  for (int k = 0; k < 12; ++k) {
    const double v = k < 9 ? R[k] : t[k - 9];
    uint64_t u;
    std::memcpy(&u, &v, 8);
    std::printf("%016llx\n", (unsigned long long)u);
  }
  return 0;
}
#endif
