// solve_map_check.cpp -- the launch-order rule of the solve kernels (climt_amd/csrc/rrtmg_solve_map.h) on the CPU, no device: a
// stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/solve_map_check.cpp -o solve_map_check && ./solve_map_check
//
// For the (wavefronts per workgroup, groups per block) pairs the kernels are built with -- 16 x 8 (sw_solve_all_kernel), 8 x 16
// (sw_solve_cloudy_kernel, and sw_solve_cloudy_allsky_kernel as built by default), 12 x 11 (the all-sky kernel under
// RRTMG_ALLSKY_WAVES=12; =16 is 16 x 8 again) and 4 x 8 (the longwave) -- for 32 and 38 work items, and for every tile count
// of the variant from 0 to three blocks and a workgroup more, and the largest chunk's 2048, over the whole launch the drivers
// size for a chunk that also holds tiles of the other variant:
//   * the q-th workgroup of the dispatch order is the q-th entry of the order the header's comment promises, written out
//     here as three nested loops: blocks in order, in a block sched positions slowest and tile groups fastest, the last block
//     holding the remaining groups;
//   * so every (group, sched position) with work is produced exactly once (counted), by the FIRST ngrp x nitem workgroups of
//     the launch, and no other workgroup has work;
//   * first + W never exceeds the list padded to whole groups, and first itself is an entry that exists.
// Then the first 40 mappings of one partial block (4 x 8, 38 items, 21 tiles: six groups) and the 16 around the end of the full
// block of 45 tiles (twelve groups: q = 296 .. 311), one "q first k" per line, for tests/test_night_pack.py to hold against the list written from the formulas the kernels carried before the rule was shared.
// Exit status 0 and a last line "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../climt_amd/csrc/rrtmg_solve_map.h"

using namespace rrtmg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s (W %d GPB %d nitem %d nmine %d q %d)\n", __FILE__, __LINE__, #cond, W, GPB, nitem, nmine, q); exit(1); } } while (0)

// nmine: the variant's tiles; launched: the workgroups of the launch
template <int W, int GPB>
static void check_case(int nmine, int nitem, int launched) {
  const int ngrp = (nmine + W - 1) / W, nfull = ngrp / GPB, rem = ngrp - nfull * GPB;
  int q = 0;
  std::vector<int> seen((size_t)ngrp * nitem, 0);
  for (int b = 0; b <= nfull; ++b) {
    const int groups = b < nfull ? GPB : rem;
    for (int k = 0; k < nitem; ++k)
      for (int g = 0; g < groups; ++g, ++q) {
        CHECK(q < launched);
        const SolveWork m = solve_map<W, GPB>(q, nmine, nitem);
        const int grp = b * GPB + g;
        CHECK(m.work && m.first == grp * W && m.k == k);
        CHECK(m.first >= 0 && m.first < nmine && m.first + W <= ngrp * W);
        CHECK(++seen[(size_t)grp * nitem + k] == 1);
      }
  }
  CHECK(q == ngrp * nitem);
  for (int s : seen) CHECK(s == 1);
  for (; q < launched; ++q) CHECK(!(solve_map<W, GPB>(q, nmine, nitem).work));
}

// sw: the launch of sw_fluxes_impl, ceil(ntile / W) x nitem workgroups; lw: that of lw_fluxes_impl, whole blocks of GPB
template <int W, int GPB>
static void check_pair(bool lw) {
  for (int nitem : {32, 38}) {
    std::vector<int> counts;
    for (int n = 0; n <= 3 * W * GPB + W + 1; ++n) counts.push_back(n);
    counts.push_back(2048);
    for (int nmine : counts)
      for (int other : {0, 1, W * GPB + 3}) {      // tiles of the other variant in the chunk
        const int ntile = nmine + other > 2048 ? 2048 : nmine + other;
        const int launched = lw ? (ntile + W * GPB - 1) / (W * GPB) * GPB * nitem : (ntile + W - 1) / W * nitem;
        check_case<W, GPB>(nmine, nitem, launched);
      }
  }
}

int main() {
  check_pair<16, 8>(false);
  check_pair<8, 16>(false);
  check_pair<12, 11>(false);
  check_pair<4, 8>(true);
  for (int q = 0; q < 40; ++q) {
    const SolveWork m = solve_map<4, 8>(q, 21, 38);
    if (!m.work) { fprintf(stderr, "q %d: no work\n", q); return 1; }
    printf("%d %d %d\n", q, m.first, m.k);
  }
  for (int q = 296; q < 312; ++q) {
    const SolveWork m = solve_map<4, 8>(q, 45, 38);
    if (!m.work) { fprintf(stderr, "q %d: no work\n", q); return 1; }
    printf("%d %d %d\n", q, m.first, m.k);
  }
  puts("ok");
  return 0;
}
