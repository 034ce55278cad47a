// call_arrays_check.cpp -- prints the array tables of a call (climt_amd/csrc/rrtmg_call_arrays.h), one line per array, on the
// CPU: no device, no GPU call.  A stand-alone program for tests/test_call_arrays.py and the host sanitizers.  The header names
// members of the kernels' structs, so the compiler is hipcc, host side only:
//
//   hipcc --offload-arch=gfx950 --offload-host-only -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/call_arrays_check.cpp -o call_arrays_check && ./call_arrays_check
//
// Line: <spectrum> <in|out> <struct> <member> <buffer name> <staging name or -> <extent> <k> <group> <flags>
// It also walks every row with the loops' own extent functions on a 130 x 6 grid and checks each count against the formula
// written out by hand here.  Exit status 0 and a last line "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../climt_amd/csrc/rrtmg_call_arrays.h"
#include "check_common.h"

using namespace rrtmg;

static const char *ext_name(Ext e) {
  static const char *const n[] = {"[nlay][N]", "[nlay+1][N]", "[N]", "[k][N]", "[k*nlay][N]", "[k*nrow][N]", "[nlay][N][k]"};
  return n[(int)e];
}
static std::string group_name(unsigned need) {
  static const char *const n[] = {"clouds", "subcols", "iaer10", "iaer6", "band_albedo_dir", "band_albedo_dif", "broadband_dir", "broadband_dif", "clear_sky", "idrv", "components", "bands"};
  std::string s;
  for (int b = 0; b < 12; ++b)
    if (need & (1u << b)) s += (s.empty() ? "" : "+") + std::string(n[b]);
  return s.empty() ? "always" : s;
}
static size_t by_hand(Ext e, size_t k, size_t N, size_t L, size_t nrow) {
  switch (e) {
    case Ext::Lay: return L * N;
    case Ext::Lev: return (L + 1) * N;
    case Ext::Col: return N;
    case Ext::KCol: return k * N;
    case Ext::KLay: return k * L * N;
    case Ext::KBandLev: return k * nrow * N;
    case Ext::LayColK: return L * N * k;
  }
  return 0;
}
template <class Row>
static void check_extent(const Row &e) {
  for (size_t nrow : {(size_t)2, (size_t)7}) {
    const GridShape g{130, 6, nrow};
    CHECK(ext_count(e.ext, e.k, g) == by_hand(e.ext, (size_t)e.k, 130, 6, nrow));
    // the permutation's rows x columns (x elements of a band-fastest array) are the same elements
    CHECK(ext_rows(e.ext, e.k, g) * 130 * (e.ext == Ext::LayColK ? (size_t)e.k : 1) == ext_count(e.ext, e.k, g));
  }
  CHECK(e.k >= 1 && e.name && e.name[0]);
}
template <class In, size_t n>
static void print_inputs(const char *spectrum, const In (&t)[n]) {
  for (const In &e : t) {
    check_extent(e);
    CHECK(e.m != nullptr && e.dev != nullptr);
    printf("%s in %s %s %s - %s %d %s %s\n", spectrum, e.strct, e.member, e.name, ext_name(e.ext), e.k, group_name(e.need).c_str(), e.whole ? "whole" : "-");
  }
}
template <class Out, size_t n>
static void print_outputs(const char *spectrum, const Out (&t)[n]) {
  for (const Out &e : t) {
    check_extent(e);
    CHECK(e.m != nullptr && e.dev != nullptr && e.wname && e.wname[0]);
    printf("%s out %s %s %s %s %s %d %s %s\n", spectrum, e.strct, e.member, e.name, e.wname, ext_name(e.ext), e.k, group_name(e.need).c_str(), e.required ? "required" : "-");
  }
}

int main() {
  print_inputs("sw", kSwIn); print_outputs("sw", kSwOut);
  print_inputs("lw", kLwIn); print_outputs("lw", kLwOut);
  // the predicates: what a plain clear-sky call and a call with everything on read
  rrtmg_sw_args a{}; rrtmg_sw_surface s{}; rrtmg_sw_components c{}; rrtmg_sw_band_fluxes b{};
  CHECK(sw_call_reads(&a, nullptr, nullptr, nullptr, true) == (kBroadDir | kBroadDif | kClear));
  a.icld = 7; a.mcica = 1; a.iaer = 10; s.albdir = (const double *)&a;
  CHECK(sw_call_reads(&a, &s, &c, &b, false) == (kClouds | kSubcols | kAer10 | kBandDir | kBroadDif | kComp | kBands));
  a.iaer = 6; a.mcica = 0;
  CHECK(sw_call_reads(&a, nullptr, nullptr, nullptr, true) == (kClouds | kAer6 | kBroadDir | kBroadDif | kClear));
  rrtmg_lw_args l{}; rrtmg_lw_band_fluxes lb{};
  CHECK(lw_call_reads(&l, nullptr, true) == kClear);
  l.icld = -1; l.mcica = 1; l.idrv = 1;
  CHECK(lw_call_reads(&l, &lb, false) == (kClouds | kSubcols | kDrv | kBands));
  // the side-by-side copy keeps every struct, and an absent one is all NULL
  const SwStructs x(&a, &s, nullptr, nullptr);
  CHECK(x.icld == 7 && x.albdir == s.albdir && x.dirdflx == nullptr && x.dndirc == nullptr);
  printf("ok\n");
  return 0;
}
