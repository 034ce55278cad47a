// permute_check.cpp -- the host-checkable part of the column-permutation engine (climt_amd/csrc/rrtmg_permute.h: the slot rule,
// the head, the table builder) on the CPU, no device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/permute_check.cpp -o permute_check && ./permute_check
//
// map(): what permute_class_kernel, permute_scan_kernel and permute_map_kernel compute, stated serially with the header's own
// permute_head, permute_slot and permute_replica.  Checked on small flag vectors under both policies: the map is a bijection
// between the caller's columns and the non-replica slots, stable within each kind, and every replica names the right column;
// under the pack's policy it is climt_amd.night.packed_order, whose results for the fields of tests/test_night_pack.py are
// written out below by hand.  Then the table builder: depth split, flush at overflow, the entry counts the constants assume.
// Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../climt_amd/csrc/rrtmg_permute.h"
#include "check_common.h"

using namespace rrtmg;

struct Map { PermuteHead h; std::vector<int> src, dst; };

// flagB[col] != 0: the column is of kind B
static Map map(const std::vector<int> &flagB, bool both_live) {
  const int n = (int)flagB.size(), ntile = (n + 63) / 64, npad = (ntile + 1) * 64;
  std::vector<int> base(ntile);
  int nB = 0, lastA = -1, lastB = -1;
  for (int c = 0; c < n; ++c) {
    if (c % 64 == 0) base[c / 64] = nB;
    if (flagB[c]) { ++nB; lastB = c; } else lastA = c;
  }
  Map m{permute_head(n - nB, lastA, lastB, npad, both_live), std::vector<int>(npad, -9), std::vector<int>(npad, -9)};
  for (int slot = 0; slot < npad; ++slot) {      // the slot side first: a mapped slot written here would show below
    const int r = permute_replica(slot, m.h, n, both_live);
    if (r != kPermuteMapped) { m.src[slot] = r; m.dst[slot] = -1; }
  }
  for (int t = 0; t < ntile; ++t) {
    int before[2] = {0, 0};
    for (int c = t * 64; c < n && c < (t + 1) * 64; ++c) {
      const bool b = flagB[c] != 0;
      const int slot = permute_slot(b, before[b]++, t, base[t], m.h);
      CHECK(slot >= 0 && slot < npad);
      CHECK(m.src[slot] == -9 && m.dst[slot] == -9);      // no replica slot, and no second column
      m.src[slot] = c; m.dst[slot] = c;
    }
  }
  return m;
}

static void check_layout(const std::vector<int> &flagB, bool both_live) {
  const int n = (int)flagB.size(), npad = ((n + 63) / 64 + 1) * 64;
  const Map m = map(flagB, both_live);
  std::vector<int> A, B;
  for (int c = 0; c < n; ++c) (flagB[c] ? B : A).push_back(c);
  const int nA = (int)A.size(), nB = (int)B.size(), nApad = (nA + 63) / 64 * 64;
  CHECK(m.h.nA == nA && m.h.nApad == nApad && m.h.live == (both_live ? npad : nApad));
  CHECK(m.h.lastA == (nA ? A.back() : -1) && m.h.lastB == (nB ? B.back() : -1));
  CHECK(nApad + nB <= npad - 1);
  for (int s = 0; s < npad; ++s) {
    CHECK(m.src[s] != -9 && m.dst[s] != -9);      // every slot is written
    if (s < nA) CHECK(m.src[s] == A[s] && m.dst[s] == A[s]);
    else if (s < nApad) CHECK(m.src[s] == A.back() && m.dst[s] == -1);
    else if (s < nApad + nB) CHECK(m.src[s] == B[s - nApad] && m.dst[s] == B[s - nApad]);
    else CHECK(m.dst[s] == -1 && m.src[s] == (!both_live ? -1 : nB ? B.back() : A.back()));
    if (both_live) CHECK(m.src[s] >= 0 && m.src[s] < n);      // the sort's gathers read every slot's column
  }
}

static std::vector<int> pattern(int n, int mode, unsigned seed) {
  std::vector<int> f(n);
  for (int c = 0; c < n; ++c) {
    seed = seed * 1664525u + 1013904223u;
    f[c] = mode == 0 ? 0 : mode == 1 ? 1 : mode == 2 ? (int)((seed >> 16) & 1u) : mode == 3 ? (c % 3 == 0) : (c >= n / 2);
  }
  return f;
}

// night.packed_order on coszen given as "is night" flags: (src, dst) slot by slot
static void check_packed(const std::vector<int> &night, const std::vector<int> &src, const std::vector<int> &dst) {
  const Map m = map(night, false);
  CHECK(m.src == src && m.dst == dst);
}
static void fill(std::vector<int> &v, int lo, int hi, int value) { for (int i = lo; i < hi; ++i) v[i] = value; }

int main() {
  // ---- the slot rule, both policies ----------------------------------------------------------------------------------------
  for (int both = 0; both < 2; ++both) {
    for (int n : {1, 63, 64, 65, 127, 128, 130, 191, 192, 500})
      for (int mode = 0; mode < 5; ++mode) check_layout(pattern(n, mode, 7u * n + mode), both != 0);
    // nA a multiple of 64 (no replica slot behind the A block), in tiles that are all mixed, N not a multiple of 64
    std::vector<int> f(191, 1);
    for (int k = 0; k < 64; ++k) f[3 * k - k / 2] = 0;
    check_layout(f, both != 0);
    f.assign(130, 1); fill(f, 0, 128, 0);      // nA = 128 = two whole tiles, the B columns in the ragged third
    check_layout(f, both != 0);
    f.assign(130, 0); f[77] = 1; check_layout(f, both != 0);      // exactly one B column
    f.assign(130, 1); f[129] = 0; check_layout(f, both != 0);     // exactly one A column, the last of the grid
    f.assign(128, 1); fill(f, 32, 96, 0); check_layout(f, both != 0);      // 64 A columns across a tile boundary
  }
  // ---- the pack's policy against climt_amd.night.packed_order (tests/test_night_pack.py pins these by hand) ---------------
  {   // 130 columns, day columns 5, 70, 129
    std::vector<int> night(130, 1), src(256, -1), dst(256, -1);
    night[5] = night[70] = night[129] = 0;
    src[0] = dst[0] = 5; src[1] = dst[1] = 70; src[2] = dst[2] = 129;
    fill(src, 3, 64, 129);
    int s = 64;
    for (int c = 0; c < 130; ++c) if (night[c]) { src[s] = c; dst[s] = c; ++s; }
    CHECK(s == 191);
    check_packed(night, src, dst);
  }
  {   // 200 columns, every third one day but 0, 3, 6: 64 day columns, the first night column directly behind them
    std::vector<int> night(200), src(320, -1), dst(320, -1);
    for (int c = 0; c < 200; ++c) night[c] = !(c % 3 == 0 && c > 6);
    int s = 0;
    for (int c = 0; c < 200; ++c) if (!night[c]) { src[s] = c; dst[s] = c; ++s; }
    CHECK(s == 64);
    for (int c = 0; c < 200; ++c) if (night[c]) { src[s] = c; dst[s] = c; ++s; }
    CHECK(s == 200 && src[64] == 0);
    check_packed(night, src, dst);
  }
  {   // 100 columns all night; all day
    std::vector<int> night(100, 1), src(192, -1), dst(192, -1);
    for (int c = 0; c < 100; ++c) src[c] = dst[c] = c;
    check_packed(night, src, dst);
    night.assign(100, 0);
    fill(src, 100, 128, 99);
    check_packed(night, src, dst);
  }
  {   // coszen 0.3, -0.0, NaN, 0.0, -1.0, 5e-324, NaN: night = coszen <= 0, NaN is day
    const double nan = __builtin_nan(""), cz[7] = {0.3, -0.0, nan, 0.0, -1.0, 5.0e-324, nan};
    std::vector<int> night(7), src(128, -1), dst(128, -1);
    for (int c = 0; c < 7; ++c) night[c] = cz[c] <= 0.0;
    const int day[4] = {0, 2, 5, 6}, dark[3] = {1, 3, 4};
    for (int k = 0; k < 4; ++k) src[k] = dst[k] = day[k];
    fill(src, 4, 64, 6);
    for (int k = 0; k < 3; ++k) src[64 + k] = dst[64 + k] = dark[k];
    check_packed(night, src, dst);
  }
  // ---- the table builder -----------------------------------------------------------------------------------------------------
  {
    std::vector<double> in(1), out(1);      // (addresses only: nothing is dereferenced)
    PermuteTable t{};
    int n = 0, flushes = 0;
    auto flush = [&]() { ++flushes; n = 0; };
    // nlay = 6: depth 7.  7 rows: one entry; 6: one; 16 (emis): 7 + 7 + 2; 96 (tauaer, 16 x nlay): 13 x 7 + 5
    const int depth = 7;
    const size_t N = 130, Np = 256;
    permute_table_add(t, n, depth, in.data(), out.data(), 7, 0, N, Np, flush);
    CHECK(n == 1 && t.e[0].rows == 7 && t.e[0].aux == 0 && t.e[0].in == in.data() && t.e[0].out == out.data());
    permute_table_add(t, n, depth, in.data(), out.data(), 6, 1, N, Np, flush);
    CHECK(n == 2 && t.e[1].rows == 6 && t.e[1].aux == 1);
    permute_table_add(t, n, depth, in.data(), out.data(), 16, 0, N, Np, flush);
    CHECK(n == 5 && t.e[2].rows == 7 && t.e[3].rows == 7 && t.e[4].rows == 2);
    CHECK(t.e[3].in == in.data() + 7 * N && t.e[3].out == out.data() + 7 * Np && t.e[4].in == in.data() + 14 * N && t.e[4].out == out.data() + 14 * Np);
    permute_table_add(t, n, depth, in.data(), out.data(), 96, 0, N, Np, flush);
    CHECK(n == 5 + 14 && t.e[18].rows == 5 && flushes == 0 && permute_entries(96, depth) == 14);
    // overflow: the table is flushed exactly when it is full, and the array goes on in the emptied table
    n = kPermuteMaxEntries - 2;
    permute_table_add(t, n, depth, in.data(), out.data(), 5 * depth, 0, N, Np, flush);
    CHECK(flushes == 1 && n == 3 && t.e[0].in == in.data() + 2 * depth * N && t.e[2].rows == depth);
    n = kPermuteMaxEntries - 1;
    permute_table_add(t, n, depth, in.data(), out.data(), 1, 0, N, Np, flush);
    CHECK(flushes == 1 && n == kPermuteMaxEntries);      // full, not yet flushed: the flush belongs to the next entry
    permute_table_add(t, n, depth, in.data(), out.data(), 1, 0, N, Np, flush);
    CHECK(flushes == 2 && n == 1);
    // what the constants assume: a call's outputs fit ONE scatter table at every depth -- the shortwave's 6 outputs, 8
    // components and 6 band members of 14 x (nlay + 1) or 14 x 2 rows; the longwave's sorted call has 8 outputs
    for (int nlay = 1; nlay <= 256; ++nlay)
      for (int levels = 0; levels < 2; ++levels) {
        const int d = nlay + 1;
        const int total = 4 * permute_entries(nlay + 1, d) + 2 * permute_entries(nlay, d) + 8 * permute_entries(nlay + 1, d) +
                          6 * permute_entries((size_t)14 * (levels ? 2 : nlay + 1), d);
        CHECK(total <= kPermuteMaxEntries && total <= 98);
      }
    CHECK(sizeof(PermuteEntry) == 24 && sizeof(PermuteTable) == 24 * (size_t)kPermuteMaxEntries && sizeof(PermuteTable) + 40 <= 4096);
    CHECK(kPermuteMaxElemEntries >= 5 && sizeof(PermuteHead) == 24);
  }
  puts("ok");
  return 0;
}
