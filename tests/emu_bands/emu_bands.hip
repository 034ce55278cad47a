// TEST INFRASTRUCTURE ONLY -- host emulation of the band fluxes (rrtmg_hip_sw_fluxes_bands, rrtmg_hip_lw_fluxes_bands).
//
// Runs the __host__ __device__ per-thread functions of climt_amd/csrc/rrtmg_{sw,lw}_device.h on the CPU: the solve with
// the sinks of the device path, the broadband integration, and the band integration (sw_band_level / lw_band_level) with
// the thread-to-row mapping of the band kernels, so that the per-band sums are checked against the reference without a GPU.
// The set-up of the two drivers follows tests/emu_components/emu_sw_components.hip and tests/emu/emu_lw.hip.  Built into
// tests/_emu_bands/librrtmg_emu_bands.so by tests/emu_bands/build.sh; never loaded by the product.
// Supported: what those two support (shortwave: clear sky, overcast, McICA with a given mask, iaer 0 / 10).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../climt_amd/csrc/rrtmg_lw_device.h"
#include "../../climt_amd/csrc/rrtmg_lw_host.h"
#include "../../climt_amd/csrc/rrtmg_sw_device.h"
#include "../../climt_amd/csrc/rrtmg_sw_host.h"
#include "../../include/rrtmg_hip.h"

using namespace rrtmg;

namespace rrtmg {
void mt_mask_host(int ncol, int nlay, int nsub, int icld, int seed, const double *cldfr, std::vector<uint64_t> &mask, int nw, int col0 = 0, int ncol_total = 0);
}

extern "C" int emu_sw_bands(const rrtmg_sw_args *a, const rrtmg_sw_band_fluxes *bp, const char *blob_path, double cpdair,
                            const double *consts, char *errbuf, int errlen) {
  auto fail = [&](int code, const std::string &m) { if (errbuf) { strncpy(errbuf, m.c_str(), errlen - 1); errbuf[errlen - 1] = 0; } return code; };
  Blob blob;
  std::string err;
  if (!blob.load(blob_path, err)) return fail(3, err);
  TableSet ts;
  Constants k{};
  k.pi = consts[0]; k.grav = consts[1]; k.planck = consts[2]; k.boltz = consts[3]; k.clight = consts[4];
  k.avogad = consts[5]; k.alosmt = consts[6]; k.gascon = consts[7]; k.sbcnst = consts[8]; k.secdy = consts[9];
  if (!build_tables(blob, "sw", cpdair, k.grav, k.secdy, ts, err)) return fail(3, err);
  SwTab T{};
  if (!build_sw_tab(ts, T, err)) return fail(3, err);
  T.t = ts.flat.data();
  const int N = a->ncol, L = a->nlay;
  const size_t nl = (size_t)N * L, nl1 = (size_t)N * (L + 1);
  SwDev d{};
  d.ncol = N; d.nlay = L; d.icld = a->icld; d.iaer = a->iaer;
  if (d.icld < 0 || d.icld > 3) d.icld = 2;
  if (d.iaer != 0 && d.iaer != 6 && d.iaer != 10) d.iaer = 0;
  if (d.iaer == 6) return fail(4, "emu_sw_bands: iaer 6 is not emulated here");
  d.inflag = a->inflgsw; d.iceflag = a->iceflgsw; d.liqflag = a->liqflgsw; d.mcica = a->mcica ? 1 : 0;
  if (d.icld >= 1 && d.mcica && !a->cldfmcl) return fail(4, "emu_sw_bands: McICA needs the sub-column mask (cldfmcl)");
  d.k = k;
  std::vector<double> svar_col;
  const long omg = ts.off("sw/sol/mgavgcyc"), osb = ts.off("sw/sol/sbavgcyc");
  int rc = sw_scalar_setup(d, N, a->isolvar, a->adjes, a->dyofyr, a->scon, a->solcycfrac, a->bndsolvar, a->indsolvar,
                           omg >= 0 ? ts.flat.data() + omg : nullptr, osb >= 0 ? ts.flat.data() + osb : nullptr, svar_col, err);
  if (!svar_col.empty()) d.svar_col = svar_col.data();
  if (rc) return fail(rc, err);
  d.play = a->play; d.plev = a->plev; d.tlay = a->tlay; d.h2o = a->h2ovmr; d.o3 = a->o3vmr; d.co2 = a->co2vmr;
  d.ch4 = a->ch4vmr; d.n2o = a->n2ovmr; d.o2 = a->o2vmr; d.asdir = a->asdir; d.asdif = a->asdif; d.aldir = a->aldir;
  d.aldif = a->aldif; d.coszen = a->coszen;
  if (d.icld >= 1) {
    d.cldfr = a->cldfr; d.taucld = a->taucld; d.ssacld = a->ssacld; d.asmcld = a->asmcld; d.fsfcld = a->fsfcld;
    d.cicewp = a->cicewp; d.cliqwp = a->cliqwp; d.reice = a->reice; d.reliq = a->reliq;
  }
  if (d.iaer == 10) { d.tauaer = a->tauaer; d.ssaaer = a->ssaaer; d.asmaer = a->asmaer; }
  std::vector<std::vector<double>> keep;
  auto wd = [&](size_t n) { keep.emplace_back(n, 0.0); return keep.back().data(); };
  d.prep = wd(sw_prep_size(N, L)); d.pdp = wd(nl); d.cossza = wd(N);
  std::vector<int32_t> laytrop(N), laysolfr((size_t)N * kSwNBand), anycld(N);
  d.laytrop = laytrop.data(); d.laysolfr = laysolfr.data(); d.anycld = anycld.data();
  if (d.icld >= 1) { d.ctau = wd(nl * kSwNBand); d.cssa = wd(nl * kSwNBand); d.casm = wd(nl * kSwNBand); }
  d.nw = (L + 63) / 64;
  d.col0 = 0; d.pcols = N;
  d.part = wd((size_t)kSwNSlot * 4 * nl1);
  double *partdir = wd((size_t)kSwNSlot * 2 * nl1);
  d.swuflx = a->swuflx; d.swdflx = a->swdflx; d.swhr = a->swhr; d.swuflxc = a->swuflxc; d.swdflxc = a->swdflxc; d.swhrc = a->swhrc;
  int errflag = 0;
  d.err = &errflag;
  for (int c = 0; c < N; ++c) { for (int l = 0; l < L; ++l) sw_prep_layer(d, T, c, l); sw_prep_column(d, T, c); }
  std::vector<uint64_t> mask;
  if (d.icld >= 1) {
    for (int lay = 0; lay < L; ++lay) for (int c = 0; c < N; ++c) sw_cloud_layer(d, T, c, lay);
    if (d.mcica) {
      mask.assign((size_t)kSwNGpt * d.nw * N, 0);
      for (int g = 0; g < kSwNGpt; ++g) for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c)
        if (a->cldfmcl[((size_t)l * N + c) * kSwNGpt + g] > 1.e-12) mask[((size_t)g * d.nw + (l >> 6)) * N + c] |= 1ull << (l & 63);
      d.mask = mask.data();
    }
  }
  // the solve: the clear-sky variant for cloud-free columns, as the device picks it per tile (here: per column)
  std::vector<double> scr((size_t)F_NTOT * L * 4);
  for (int col = 0; col < N; ++col) {
    const bool cld = d.anycld[col] != 0;
    for (int i = 0; i < T.nitem; ++i) {
      SwPartDirSink sink = sw_part_dir_sink(d, partdir, i, col);
      if (cld) sw_solve_item<true>(d, T, T.t + T.exp_tbl, T.item[i], col, scr.data(), 1, sink);
      else sw_solve_item<false>(d, T, T.t + T.exp_tbl, T.item[i], col, scr.data(), 1, sink);
    }
  }
  for (int lev = 0; lev <= L; ++lev) for (int c = 0; c < N; ++c) sw_flux_level(d, T, c, lev, d.anycld[c] != 0);
  for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) sw_heat_layer(d, T, c, l);
  // the band integration, as sw_bandflux_kernel maps its threads: every interface level, or the two boundary levels
  const SwBandOut o{bp->up, bp->dn, bp->upc, bp->dnc, bp->dndir, bp->dndirc};
  const int nrow = bp->levels ? 2 : L + 1;
  for (int row = 0; row < nrow; ++row)
    for (int c = 0; c < N; ++c) sw_band_level(d, T, partdir, o, c, bp->levels ? (row ? L : 0) : row, row, nrow, d.anycld[c] != 0);
  if (errflag) return fail(errflag, "device-side error flag " + std::to_string(errflag));
  return 0;
}

// the clear-sky variant for cloud-free columns, as the device picks it per tile
static bool emu_lw_cloudy(const LwDev &d, int col) {
  bool cld = false;
  if (d.icld >= 1 && d.cldfr) for (int l = 0; l < d.nlay; ++l) cld = cld || d.cldfr[(size_t)l * d.ncol + col] > 0.0;
  return cld;
}
static void emu_lw_solve(const LwDev &d, const LwTab &T) {
  std::vector<double> scr((size_t)LF_N * d.nlay * 4);
  for (int slot = 0; slot < T.nitem; ++slot)
    for (int col = 0; col < d.ncol; ++col) {
      LwPartSink sink = lw_part_sink(d, slot, col);
      const bool cld = emu_lw_cloudy(d, col);
      if (cld && !d.mcica && d.icld >= 2) lw_solve_item<true, true>(d, T, T.item[slot], col, scr.data(), 1, sink);
      else if (cld) lw_solve_item<true, false>(d, T, T.item[slot], col, scr.data(), 1, sink);
      else lw_solve_item<false, false>(d, T, T.item[slot], col, scr.data(), 1, sink);
    }
}

extern "C" int emu_lw_bands(const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *bp, const char *blob_path, double cpdair, const double *consts, char *errbuf, int errlen) {
  auto fail = [&](int code, const std::string &m) { if (errbuf) { strncpy(errbuf, m.c_str(), errlen - 1); errbuf[errlen - 1] = 0; } return code; };
  Blob blob;
  std::string err;
  if (!blob.load(blob_path, err)) return fail(3, err);
  TableSet ts;
  Constants k{};
  k.pi = consts[0]; k.grav = consts[1]; k.planck = consts[2]; k.boltz = consts[3]; k.clight = consts[4];
  k.avogad = consts[5]; k.alosmt = consts[6]; k.gascon = consts[7]; k.sbcnst = consts[8]; k.secdy = consts[9];
  if (!build_tables(blob, "lw", cpdair, k.grav, k.secdy, ts, err)) return fail(3, err);
  LwTab T{};
  if (!build_lw_tab(ts, T, err)) return fail(3, err);
  T.t = ts.flat.data();
  const int N = a->ncol, L = a->nlay;
  const size_t nl = (size_t)N * L, nl1 = (size_t)N * (L + 1);
  LwDev d{};
  d.ncol = N; d.nlay = L; d.icld = a->icld;
  if (d.icld < 0 || d.icld > 3) d.icld = 2;
  d.idrv = a->idrv ? 1 : 0;
  d.inflag = a->inflglw; d.iceflag = a->iceflglw; d.liqflag = a->liqflglw; d.mcica = a->mcica ? 1 : 0;
  d.k = k;
  d.fluxfac = (2.0 * asin(1.0)) * 2.e4;
  d.play = a->play; d.plev = a->plev; d.tlay = a->tlay; d.tlev = a->tlev; d.tsfc = a->tsfc; d.h2o = a->h2ovmr; d.o3 = a->o3vmr;
  d.co2 = a->co2vmr; d.ch4 = a->ch4vmr; d.n2o = a->n2ovmr; d.o2 = a->o2vmr; d.cfc11 = a->cfc11vmr; d.cfc12 = a->cfc12vmr;
  d.cfc22 = a->cfc22vmr; d.ccl4 = a->ccl4vmr; d.emis = a->emis; d.tauaer = a->tauaer;
  std::vector<double> tlev_host;
  if (!d.tlev) {   // interface temperatures not given: the interpolation the library does on the device (util.py:89-142)
    tlev_host.resize(nl1);
    for (int c = 0; c < N; ++c) {
      tlev_host[c] = d.tsfc[c];
      tlev_host[(size_t)L * N + c] = d.tlay[(size_t)(L - 1) * N + c];
      for (int lev = 1; lev < L; ++lev) {
        const double lp1 = log(d.play[(size_t)lev * N + c]), lp0 = log(d.play[(size_t)(lev - 1) * N + c]);
        const double w = (log(d.plev[(size_t)lev * N + c]) - lp1) / (lp0 - lp1);
        const double m1 = d.tlay[(size_t)lev * N + c], m0 = d.tlay[(size_t)(lev - 1) * N + c];
        tlev_host[(size_t)lev * N + c] = m1 - w * (m1 - m0);
      }
    }
    d.tlev = tlev_host.data();
  }
  const bool clouds = d.icld >= 1;
  if (clouds) { d.cldfr = a->cldfr; d.taucld = a->taucld; d.cicewp = a->cicewp; d.cliqwp = a->cliqwp; d.reice = a->reice; d.reliq = a->reliq; }
  std::vector<std::vector<double>> keep;
  auto wd = [&](size_t n) { keep.emplace_back(n, 0.0); return keep.back().data(); };
  d.prep = wd(lw_prep_size(N, L)); d.secdiff = wd((size_t)N * 16);
  std::vector<int32_t> laytrop(N), ncb(N, 1);
  d.laytrop = laytrop.data(); d.ncbands = ncb.data();
  if (clouds) d.ctau = wd(nl * 16);
  d.nw = (L + 63) / 64;
  std::vector<uint64_t> mask, anym;
  const int nk = d.idrv ? 6 : 4;
  d.col0 = 0; d.pcols = N;
  d.part = wd((size_t)kLwNGpt * nk * nl1);
  d.uflx = a->uflx; d.dflx = a->dflx; d.hr = a->hr; d.uflxc = a->uflxc; d.dflxc = a->dflxc; d.hrc = a->hrc;
  d.duflx_dt = a->duflx_dt; d.duflxc_dt = a->duflxc_dt;
  int errflag = 0;
  d.err = &errflag;
  for (int c = 0; c < N; ++c) { for (int l = 0; l < L; ++l) lw_prep_layer(d, T, c, l); lw_prep_column(d, T, c); }
  if (clouds) {
    if (!d.mcica) {
      for (int c = 0; c < N; ++c) lw_cloud_column(d, T, c);
      if (d.icld >= 2) { d.mr = wd(lw_mr_size(N, L)); for (int c = 0; c < N; ++c) lw_mr_column(d, c); }
    } else {
      for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) lw_cloudmc_layer(d, T, c, l);
      mask.assign((size_t)kLwNGpt * d.nw * N, 0);
      anym.assign((size_t)d.nw * N, 0);
      d.mask = mask.data(); d.anymask = anym.data();
      if (a->cldfmcl) {
        for (int g = 0; g < kLwNGpt; ++g) for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c)
          if (a->cldfmcl[((size_t)l * N + c) * kLwNGpt + g] > 1.e-12) mask[((size_t)g * d.nw + (l >> 6)) * N + c] |= 1ull << (l & 63);
      } else if (a->irng == 0) {
        for (int c = 0; c < N; ++c) kiss_mask_column(N, L, kLwNGpt, d.icld, a->permuteseed, d.play, d.cldfr, d.mask, d.nw, d.err, c);
      } else {
        mt_mask_host(N, L, kLwNGpt, d.icld, a->permuteseed, a->cldfr, mask, d.nw, a->shard_col0, a->shard_ncol);
        d.mask = mask.data();
      }
      for (int c = 0; c < N; ++c) lw_anymask_column(d, c);
    }
  }
  emu_lw_solve(d, T);
  for (int lev = 0; lev <= L; ++lev) for (int c = 0; c < N; ++c) lw_flux_level(d, T, c, lev, T.nitem, emu_lw_cloudy(d, c));
  for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) lw_heat_layer(d, T, c, l);
  // the band integration, as lw_bandflux_kernel maps its threads: every interface level, or the two boundary levels
  const LwBandOut o{bp->up, bp->dn, bp->upc, bp->dnc};
  const int nrow = bp->levels ? 2 : L + 1;
  for (int row = 0; row < nrow; ++row)
    for (int c = 0; c < N; ++c) lw_band_level(d, T, o, c, bp->levels ? (row ? L : 0) : row, row, nrow, emu_lw_cloudy(d, c));
  if (errflag) return fail(errflag, "device-side error flag " + std::to_string(errflag));
  return 0;
}
