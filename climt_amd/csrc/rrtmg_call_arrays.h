// rrtmg_call_arrays.h -- THE list of a call's grid arrays, one table of inputs and one of outputs per spectrum (host code only).
// Every path that enumerates the caller's arrays walks these tables (the loops are in rrtmg_call.h): the drivers' HostInputs
// registration, output binding and output copies; the gathers and the scatter of a permuted call (rrtmg_permute.h); the widen
// and narrow tables of the float32 boundary (rrtmg_precision.h).  A row states once: the member of the public struct, the
// name of its work buffers behind every prefix ("sw.in.", "sw.sort.", "sw.pack.", "sw.f32."; outputs: also the name of the
// driver's own staging buffer behind "sw.w."), the member of the driver's bound struct, the extent, and the group that decides
// whether the call reads it at all.  Order: the driver's registration order (inputs), the public struct's (outputs).
// A new grid array is one row here (tests/test_call_arrays.py compares the tables with include/rrtmg_hip.h).
#pragma once
#include <cstddef>

#include "../../include/rrtmg_hip.h"
#include "rrtmg_lw_device.h"
#include "rrtmg_sw_device.h"

namespace rrtmg {

// ---- extent: [rows][N] as the permutation sees it, rows * N elements as HostInputs and the float32 boundary do --------------------
enum class Ext { Lay, Lev, Col, KCol, KLay, KBandLev, LayColK };
// Lay [nlay][N]; Lev [nlay+1][N]; Col [N]; KCol [k][N]; KLay [k*nlay][N]; KBandLev [k*nrow][N], nrow = nlay + 1 or the 2 boundary
// levels (rrtmg_*_band_fluxes::levels); LayColK band-fastest [nlay][N][k]: nlay rows of k elements per column (gather_elem)
struct GridShape { size_t N, L, band_rows; };
// band_levels: rrtmg_*_band_fluxes::levels of the call, 0 where no band fluxes are requested
inline GridShape grid_shape(int ncol, int nlay, int band_levels) { return {(size_t)ncol, (size_t)nlay, band_levels ? (size_t)2 : (size_t)nlay + 1}; }
constexpr size_t ext_rows(Ext e, int k, const GridShape &g) {
  return e == Ext::Lay || e == Ext::LayColK ? g.L : e == Ext::Lev ? g.L + 1 : e == Ext::Col ? 1 : e == Ext::KCol ? (size_t)k : e == Ext::KLay ? k * g.L : k * g.band_rows;
}
constexpr size_t ext_count(Ext e, int k, const GridShape &g) { return ext_rows(e, k, g) * g.N * (e == Ext::LayColK ? (size_t)k : 1); }

// ---- groups: a row is read where every bit of its `need` is set in what {sw,lw}_call_reads answers ------------------------------
enum : unsigned {
  kClouds = 1, kSubcols = 2,         // clouds; clouds and McICA (the caller's sub-columns, where given)
  kAer10 = 4, kAer6 = 8,             // iaer == 10; iaer == 6
  kBandDir = 16, kBandDif = 32,      // the per-band albedo (direct, diffuse) is given ...
  kBroadDir = 64, kBroadDif = 128,   // ... or not: the broadband pair is not shadowed
  kClear = 256, kDrv = 512,          // clear-sky outputs on; idrv
  kComp = 1024, kBands = 2048,       // components requested; band fluxes requested
};
constexpr bool array_is_read(unsigned need, unsigned on) { return (need & ~on) == 0; }

// the structs of a call side by side: a member pointer of any of them is a member pointer of this one
struct SwStructs : rrtmg_sw_args, rrtmg_sw_surface, rrtmg_sw_components, rrtmg_sw_band_fluxes {
  SwStructs(const rrtmg_sw_args *a, const rrtmg_sw_surface *s, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b)
      : rrtmg_sw_args(*a), rrtmg_sw_surface(s ? *s : rrtmg_sw_surface{}), rrtmg_sw_components(c ? *c : rrtmg_sw_components{}), rrtmg_sw_band_fluxes(b ? *b : rrtmg_sw_band_fluxes{}) {}
};
struct LwStructs : rrtmg_lw_args, rrtmg_lw_band_fluxes {
  LwStructs(const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *b) : rrtmg_lw_args(*a), rrtmg_lw_band_fluxes(b ? *b : rrtmg_lw_band_fluxes{}) {}
};
// ... and what a driver binds them to: the kernels' struct, the optional outputs' structs, and the two inputs no kernel struct holds
struct CallLocals { const double *ecaer, *cldfmcl; };
struct SwBound : SwDev, SwCompOut, SwBandOut, CallLocals {};
struct LwBound : LwDev, LwBandOut, CallLocals {};

template <class All, class Bound>
struct InArray { const char *strct, *member; const double *All::*m; const char *name; const double *Bound::*dev; Ext ext; int k; unsigned need; bool whole = false; };
// wname: the driver's staging buffer of a host-pointer call; required: NULL is refused where the group is on (else: not requested)
template <class All, class Bound>
struct OutArray { const char *strct, *member; double *All::*m; const char *name, *wname; double *Bound::*dev; Ext ext; int k; unsigned need; bool required; };
#define RRTMG_M(S, F) #S, #F, &S::F

// ---- shortwave -------------------------------------------------------------------------------------------------------------------
// (tlev and tsfc of rrtmg_sw_args are absent: the shortwave reads neither)
// whole: the pack fills every slot -- coszen: the night kernels decide from it; ecaer: sw_aer_kernel runs over the whole grid
constexpr InArray<SwStructs, SwBound> kSwIn[] = {
    {RRTMG_M(rrtmg_sw_args, play), "play", &SwDev::play, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_sw_args, plev), "plev", &SwDev::plev, Ext::Lev, 1, 0},
    {RRTMG_M(rrtmg_sw_args, tlay), "tlay", &SwDev::tlay, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_sw_args, h2ovmr), "h2o", &SwDev::h2o, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_sw_args, o3vmr), "o3", &SwDev::o3, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_sw_args, co2vmr), "co2", &SwDev::co2, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_sw_args, ch4vmr), "ch4", &SwDev::ch4, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_sw_args, n2ovmr), "n2o", &SwDev::n2o, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_sw_args, o2vmr), "o2", &SwDev::o2, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_sw_args, asdir), "asdir", &SwDev::asdir, Ext::Col, 1, kBroadDir},
    {RRTMG_M(rrtmg_sw_args, aldir), "aldir", &SwDev::aldir, Ext::Col, 1, kBroadDir}, {RRTMG_M(rrtmg_sw_args, asdif), "asdif", &SwDev::asdif, Ext::Col, 1, kBroadDif},
    {RRTMG_M(rrtmg_sw_args, aldif), "aldif", &SwDev::aldif, Ext::Col, 1, kBroadDif}, {RRTMG_M(rrtmg_sw_surface, albdir), "albdir", &SwDev::albdir, Ext::KCol, kSwNBand, kBandDir},
    {RRTMG_M(rrtmg_sw_surface, albdif), "albdif", &SwDev::albdif, Ext::KCol, kSwNBand, kBandDif}, {RRTMG_M(rrtmg_sw_args, coszen), "coszen", &SwDev::coszen, Ext::Col, 1, 0, true},
    {RRTMG_M(rrtmg_sw_args, cldfr), "cldfr", &SwDev::cldfr, Ext::Lay, 1, kClouds}, {RRTMG_M(rrtmg_sw_args, ssacld), "ssacld", &SwDev::ssacld, Ext::LayColK, kSwNBand, kClouds},
    {RRTMG_M(rrtmg_sw_args, asmcld), "asmcld", &SwDev::asmcld, Ext::LayColK, kSwNBand, kClouds}, {RRTMG_M(rrtmg_sw_args, fsfcld), "fsfcld", &SwDev::fsfcld, Ext::LayColK, kSwNBand, kClouds},
    {RRTMG_M(rrtmg_sw_args, cicewp), "cicewp", &SwDev::cicewp, Ext::Lay, 1, kClouds}, {RRTMG_M(rrtmg_sw_args, cliqwp), "cliqwp", &SwDev::cliqwp, Ext::Lay, 1, kClouds},
    {RRTMG_M(rrtmg_sw_args, reice), "reice", &SwDev::reice, Ext::Lay, 1, kClouds}, {RRTMG_M(rrtmg_sw_args, reliq), "reliq", &SwDev::reliq, Ext::Lay, 1, kClouds},
    {RRTMG_M(rrtmg_sw_args, taucld), "taucld", &SwDev::taucld, Ext::LayColK, kSwNBand, kClouds}, {RRTMG_M(rrtmg_sw_args, tauaer), "tauaer", &SwDev::tauaer, Ext::KLay, kSwNBand, kAer10},
    {RRTMG_M(rrtmg_sw_args, ssaaer), "ssaaer", &SwDev::ssaaer, Ext::KLay, kSwNBand, kAer10}, {RRTMG_M(rrtmg_sw_args, asmaer), "asmaer", &SwDev::asmaer, Ext::KLay, kSwNBand, kAer10},
    {RRTMG_M(rrtmg_sw_args, ecaer), "ecaer", &CallLocals::ecaer, Ext::KLay, 6, kAer6, true}, {RRTMG_M(rrtmg_sw_args, cldfmcl), "cldfmcl", &CallLocals::cldfmcl, Ext::LayColK, kSwNGpt, kSubcols},
};
constexpr OutArray<SwStructs, SwBound> kSwOut[] = {
    {RRTMG_M(rrtmg_sw_args, swuflx), "o0", "o.uflx", &SwDev::swuflx, Ext::Lev, 1, 0, true}, {RRTMG_M(rrtmg_sw_args, swdflx), "o1", "o.dflx", &SwDev::swdflx, Ext::Lev, 1, 0, true},
    {RRTMG_M(rrtmg_sw_args, swhr), "o2", "o.hr", &SwDev::swhr, Ext::Lay, 1, 0, true}, {RRTMG_M(rrtmg_sw_args, swuflxc), "o3", "o.uflxc", &SwDev::swuflxc, Ext::Lev, 1, kClear, true},
    {RRTMG_M(rrtmg_sw_args, swdflxc), "o4", "o.dflxc", &SwDev::swdflxc, Ext::Lev, 1, kClear, true}, {RRTMG_M(rrtmg_sw_args, swhrc), "o5", "o.hrc", &SwDev::swhrc, Ext::Lay, 1, kClear, true},
    {RRTMG_M(rrtmg_sw_components, dirdflx), "c0", "o.dirdflx", &SwCompOut::dirdflx, Ext::Lev, 1, kComp}, {RRTMG_M(rrtmg_sw_components, difdflx), "c1", "o.difdflx", &SwCompOut::difdflx, Ext::Lev, 1, kComp},
    {RRTMG_M(rrtmg_sw_components, dirdnuv), "c2", "o.dirdnuv", &SwCompOut::dirdnuv, Ext::Lev, 1, kComp}, {RRTMG_M(rrtmg_sw_components, difdnuv), "c3", "o.difdnuv", &SwCompOut::difdnuv, Ext::Lev, 1, kComp},
    {RRTMG_M(rrtmg_sw_components, dirdnir), "c4", "o.dirdnir", &SwCompOut::dirdnir, Ext::Lev, 1, kComp}, {RRTMG_M(rrtmg_sw_components, difdnir), "c5", "o.difdnir", &SwCompOut::difdnir, Ext::Lev, 1, kComp},
    {RRTMG_M(rrtmg_sw_components, dirdflxc), "c6", "o.dirdflxc", &SwCompOut::dirdflxc, Ext::Lev, 1, kComp}, {RRTMG_M(rrtmg_sw_components, difdflxc), "c7", "o.difdflxc", &SwCompOut::difdflxc, Ext::Lev, 1, kComp},
    {RRTMG_M(rrtmg_sw_band_fluxes, up), "b0", "ob.up", &SwBandOut::up, Ext::KBandLev, kSwNBand, kBands}, {RRTMG_M(rrtmg_sw_band_fluxes, dn), "b1", "ob.dn", &SwBandOut::dn, Ext::KBandLev, kSwNBand, kBands},
    {RRTMG_M(rrtmg_sw_band_fluxes, upc), "b2", "ob.upc", &SwBandOut::upc, Ext::KBandLev, kSwNBand, kBands}, {RRTMG_M(rrtmg_sw_band_fluxes, dnc), "b3", "ob.dnc", &SwBandOut::dnc, Ext::KBandLev, kSwNBand, kBands},
    {RRTMG_M(rrtmg_sw_band_fluxes, dndir), "b4", "ob.dndir", &SwBandOut::dndir, Ext::KBandLev, kSwNBand, kBands}, {RRTMG_M(rrtmg_sw_band_fluxes, dndirc), "b5", "ob.dndirc", &SwBandOut::dndirc, Ext::KBandLev, kSwNBand, kBands},
};
// What a shortwave call reads and writes.  THE place where icld and iaer are normalised for the tables: every icld but 0 is a
// cloud rule (outside 0..3: 2, or 4 / 5 with rank correlations set -- call_overlap); every iaer but 6 and 10 is 0.
inline unsigned sw_call_reads(const rrtmg_sw_args *a, const rrtmg_sw_surface *sp, const rrtmg_sw_components *cp, const rrtmg_sw_band_fluxes *bp, bool clear_sky) {
  const bool clouds = a->icld != 0;
  return (clouds ? kClouds : 0) | (clouds && a->mcica ? kSubcols : 0) | (a->iaer == 10 ? kAer10 : 0) | (a->iaer == 6 ? kAer6 : 0) |
         (sp && sp->albdir ? kBandDir : kBroadDir) | (sp && sp->albdif ? kBandDif : kBroadDif) | (clear_sky ? kClear : 0) | (cp ? kComp : 0) | (bp ? kBands : 0);
}

// ---- longwave --------------------------------------------------------------------------------------------------------------------
constexpr InArray<LwStructs, LwBound> kLwIn[] = {
    {RRTMG_M(rrtmg_lw_args, play), "play", &LwDev::play, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, plev), "plev", &LwDev::plev, Ext::Lev, 1, 0},
    {RRTMG_M(rrtmg_lw_args, tlay), "tlay", &LwDev::tlay, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, tlev), "tlev", &LwDev::tlev, Ext::Lev, 1, 0},
    {RRTMG_M(rrtmg_lw_args, tsfc), "tsfc", &LwDev::tsfc, Ext::Col, 1, 0}, {RRTMG_M(rrtmg_lw_args, h2ovmr), "h2o", &LwDev::h2o, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_lw_args, o3vmr), "o3", &LwDev::o3, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, co2vmr), "co2", &LwDev::co2, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_lw_args, ch4vmr), "ch4", &LwDev::ch4, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, n2ovmr), "n2o", &LwDev::n2o, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_lw_args, o2vmr), "o2", &LwDev::o2, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, cfc11vmr), "cfc11", &LwDev::cfc11, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_lw_args, cfc12vmr), "cfc12", &LwDev::cfc12, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, cfc22vmr), "cfc22", &LwDev::cfc22, Ext::Lay, 1, 0},
    {RRTMG_M(rrtmg_lw_args, ccl4vmr), "ccl4", &LwDev::ccl4, Ext::Lay, 1, 0}, {RRTMG_M(rrtmg_lw_args, emis), "emis", &LwDev::emis, Ext::KCol, kLwNBand, 0},
    {RRTMG_M(rrtmg_lw_args, cldfr), "cldfr", &LwDev::cldfr, Ext::Lay, 1, kClouds}, {RRTMG_M(rrtmg_lw_args, taucld), "taucld", &LwDev::taucld, Ext::LayColK, kLwNBand, kClouds},
    {RRTMG_M(rrtmg_lw_args, cicewp), "cicewp", &LwDev::cicewp, Ext::Lay, 1, kClouds}, {RRTMG_M(rrtmg_lw_args, cliqwp), "cliqwp", &LwDev::cliqwp, Ext::Lay, 1, kClouds},
    {RRTMG_M(rrtmg_lw_args, reice), "reice", &LwDev::reice, Ext::Lay, 1, kClouds}, {RRTMG_M(rrtmg_lw_args, reliq), "reliq", &LwDev::reliq, Ext::Lay, 1, kClouds},
    {RRTMG_M(rrtmg_lw_args, tauaer), "tauaer", &LwDev::tauaer, Ext::KLay, kLwNBand, 0}, {RRTMG_M(rrtmg_lw_args, cldfmcl), "cldfmcl", &CallLocals::cldfmcl, Ext::LayColK, kLwNGpt, kSubcols},
};
// (duflx_dt / duflxc_dt: not `required` here -- a NULL one is refused with a message of its own, lw_check_drv)
constexpr OutArray<LwStructs, LwBound> kLwOut[] = {
    {RRTMG_M(rrtmg_lw_args, uflx), "o0", "o.uflx", &LwDev::uflx, Ext::Lev, 1, 0, true}, {RRTMG_M(rrtmg_lw_args, dflx), "o1", "o.dflx", &LwDev::dflx, Ext::Lev, 1, 0, true},
    {RRTMG_M(rrtmg_lw_args, hr), "o2", "o.hr", &LwDev::hr, Ext::Lay, 1, 0, true}, {RRTMG_M(rrtmg_lw_args, uflxc), "o3", "o.uflxc", &LwDev::uflxc, Ext::Lev, 1, kClear, true},
    {RRTMG_M(rrtmg_lw_args, dflxc), "o4", "o.dflxc", &LwDev::dflxc, Ext::Lev, 1, kClear, true}, {RRTMG_M(rrtmg_lw_args, hrc), "o5", "o.hrc", &LwDev::hrc, Ext::Lay, 1, kClear, true},
    {RRTMG_M(rrtmg_lw_args, duflx_dt), "o6", "o.du", &LwDev::duflx_dt, Ext::Lev, 1, kDrv}, {RRTMG_M(rrtmg_lw_args, duflxc_dt), "o7", "o.duc", &LwDev::duflxc_dt, Ext::Lev, 1, kDrv | kClear},
    {RRTMG_M(rrtmg_lw_band_fluxes, up), "b0", "ob.up", &LwBandOut::up, Ext::KBandLev, kLwNBand, kBands}, {RRTMG_M(rrtmg_lw_band_fluxes, dn), "b1", "ob.dn", &LwBandOut::dn, Ext::KBandLev, kLwNBand, kBands},
    {RRTMG_M(rrtmg_lw_band_fluxes, upc), "b2", "ob.upc", &LwBandOut::upc, Ext::KBandLev, kLwNBand, kBands}, {RRTMG_M(rrtmg_lw_band_fluxes, dnc), "b3", "ob.dnc", &LwBandOut::dnc, Ext::KBandLev, kLwNBand, kBands},
};
// (the longwave reads no aerosol switch: tauaer is read where it is given)
inline unsigned lw_call_reads(const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *bp, bool clear_sky) {
  const bool clouds = a->icld != 0;
  return (clouds ? kClouds : 0) | (clouds && a->mcica ? kSubcols : 0) | (clear_sky ? kClear : 0) | (a->idrv ? kDrv : 0) | (bp ? kBands : 0);
}
#undef RRTMG_M

template <class T, size_t n> constexpr int table_size(const T (&)[n]) { return (int)n; }

}  // namespace rrtmg
