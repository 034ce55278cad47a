// exp_overlap_check.cpp -- the kissvec sub-column generator under exponential (icld 4) and exponential-random (icld 5) overlap
// on the CPU, no device: kiss_mask_column_exp (one sequential stream per column) and kiss_mask_jump_exp with kiss_build_jumps
// (what a thread of kiss_mask_exp_kernel runs) of climt_amd/csrc/rrtmg_sw_device.h and rrtmg_kiss_host.h.  A stand-alone
// program for the host sanitizers (the HIP headers are only read for their host-side definitions of __host__ / __device__):
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       tools/exp_overlap_check.cpp -o exp_overlap_check
//   ./exp_overlap_check ncol nlay nsub icld changeSeed in.bin out.bin
//
// in.bin : play, cldfr, alpha -- three [nlay][ncol] arrays of doubles, one after the other
// out.bin: the mask words of the jump-ahead form, uint64 [nsub][nw][ncol], nw = ceil(nlay / 64)
// The program checks that the sequential form and the jump-ahead form agree in every word, that neither raised an error code
// and that the guard words around both masks are intact; exit status 0 and "ok" when everything holds.
// tests/test_exp_overlap.py compares out.bin with a numpy statement of the definition in include/rrtmg_hip.h.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../climt_amd/csrc/rrtmg_kiss_host.h"
#include "../climt_amd/csrc/rrtmg_sw_device.h"
#include "check_common.h"

using namespace rrtmg;

constexpr size_t kWordGuard = 16;
constexpr uint64_t kWordPoison = 0xa5a5a5a5a5a5a5a5ull;

int main(int argc, char **argv) {
  if (argc != 8) { fprintf(stderr, "usage: %s ncol nlay nsub icld changeSeed in.bin out.bin\n", argv[0]); return 2; }
  const int ncol = atoi(argv[1]), nlay = atoi(argv[2]), nsub = atoi(argv[3]), icld = atoi(argv[4]), seed = atoi(argv[5]);
  CHECK(ncol > 0 && nlay >= 4 && nlay <= 256 && nsub > 0 && (icld == 4 || icld == 5) && seed >= 0);
  const size_t nl = (size_t)ncol * nlay;
  const int nw = (nlay + 63) / 64;
  std::vector<double> in(3 * nl);
  FILE *f = fopen(argv[6], "rb");
  CHECK(f != nullptr);
  CHECK(fread(in.data(), sizeof(double), in.size(), f) == in.size());
  fclose(f);
  const double *play = in.data(), *cldfr = play + nl, *alpha = cldfr + nl;

  const size_t words = (size_t)nsub * nw * ncol;
  std::vector<uint64_t> seq(words + 2 * kWordGuard, kWordPoison), jmp(words + 2 * kWordGuard, kWordPoison);
  int err_seq = 0, err_jmp = 0;
  for (int c = 0; c < ncol; ++c) kiss_mask_column_exp(ncol, nlay, nsub, icld, seed, play, cldfr, alpha, seq.data() + kWordGuard, nw, &err_seq, c);
  std::vector<uint32_t> jumps;
  kiss_build_jumps(nsub, nlay, icld, seed, jumps);
  CHECK(jumps.size() == (size_t)nsub * kKissJumpWords);
  for (int g = 0; g < nsub; ++g) CHECK(jumps[(size_t)g * kKissJumpWords] == (uint32_t)seed + (uint32_t)g * 2u * (uint32_t)nlay);
  // (the order of a launch: the sub-column index fastest within a tile of 64 columns)
  for (int c = 0; c < ncol; ++c)
    for (int g = 0; g < nsub; ++g) kiss_mask_jump_exp(ncol, nlay, icld, play, cldfr, alpha, jmp.data() + kWordGuard, nw, &err_jmp, jumps.data(), c, g);
  CHECK(err_seq == 0 && err_jmp == 0);
  for (size_t g = 0; g < kWordGuard; ++g) CHECK(seq[g] == kWordPoison && seq[kWordGuard + words + g] == kWordPoison && jmp[g] == kWordPoison && jmp[kWordGuard + words + g] == kWordPoison);
  size_t differ = 0;
  for (size_t i = 0; i < words; ++i) differ += seq[kWordGuard + i] != jmp[kWordGuard + i];
  if (differ) { fprintf(stderr, "sequential and jump-ahead masks differ in %zu of %zu words\n", differ, words); return 1; }
  // no bit above the last layer
  if (nlay % 64)
    for (int g = 0; g < nsub; ++g)
      for (int c = 0; c < ncol; ++c) CHECK((jmp[kWordGuard + ((size_t)g * nw + nw - 1) * ncol + c] >> (nlay % 64)) == 0);
  f = fopen(argv[7], "wb");
  CHECK(f != nullptr);
  CHECK(fwrite(jmp.data() + kWordGuard, sizeof(uint64_t), words, f) == words);
  fclose(f);
  printf("ok (%d x %d x %d, icld %d, seed %d)\n", ncol, nlay, nsub, icld, seed);
  return 0;
}
