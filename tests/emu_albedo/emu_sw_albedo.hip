// TEST INFRASTRUCTURE ONLY -- host emulation of the shortwave with the surface albedo by band (rrtmg_hip_sw_fluxes_surface).
//
// Runs the __host__ __device__ per-thread functions of climt_amd/csrc/rrtmg_sw_device.h on the CPU with SwDev::albdir /
// albdif set the way sw_fluxes_run sets them, so that the per-band albedo load of sw_solve_thread, its fallback to the band
// rule and the band fluxes it shapes are checked against the reference without a GPU.  The driver is the shortwave one of
// tests/emu_bands/emu_bands.hip plus the surface struct; bp may be NULL (no band fluxes).  Built into
// tests/_emu_albedo/librrtmg_emu_albedo.so by tests/emu_albedo/build.sh; never loaded by the product.
// Supported: clear sky, overcast, McICA with a given mask, iaer 0 / 10.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../climt_amd/csrc/rrtmg_sw_device.h"
#include "../../climt_amd/csrc/rrtmg_sw_host.h"
#include "../../include/rrtmg_hip.h"

using namespace rrtmg;

extern "C" int emu_sw_surface(const rrtmg_sw_args *a, const rrtmg_sw_surface *sf, const rrtmg_sw_band_fluxes *bp, const char *blob_path,
                              double cpdair, const double *consts, char *errbuf, int errlen) {
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
  if (d.iaer == 6) return fail(4, "emu_sw_surface: iaer 6 is not emulated here");
  d.inflag = a->inflgsw; d.iceflag = a->iceflgsw; d.liqflag = a->liqflgsw; d.mcica = a->mcica ? 1 : 0;
  if (d.icld >= 1 && d.mcica && !a->cldfmcl) return fail(4, "emu_sw_surface: McICA needs the sub-column mask (cldfmcl)");
  d.k = k;
  std::vector<double> svar_col;
  const long omg = ts.off("sw/sol/mgavgcyc"), osb = ts.off("sw/sol/sbavgcyc");
  int rc = sw_scalar_setup(d, N, a->isolvar, a->adjes, a->dyofyr, a->scon, a->solcycfrac, a->bndsolvar, a->indsolvar,
                           omg >= 0 ? ts.flat.data() + omg : nullptr, osb >= 0 ? ts.flat.data() + osb : nullptr, svar_col, err);
  if (!svar_col.empty()) d.svar_col = svar_col.data();
  if (rc) return fail(rc, err);
  d.play = a->play; d.plev = a->plev; d.tlay = a->tlay; d.h2o = a->h2ovmr; d.o3 = a->o3vmr; d.co2 = a->co2vmr;
  d.ch4 = a->ch4vmr; d.n2o = a->n2ovmr; d.o2 = a->o2vmr; d.coszen = a->coszen;
  // the surface albedo as sw_fluxes_run sets it up: a broadband pair is read only where its per-band array is not given
  if (sf && (size_t)sf->struct_size != sizeof(rrtmg_sw_surface)) return fail(RRTMG_ERR_ARG, "rrtmg_sw_surface: struct_size");
  const bool bdir = sf && sf->albdir, bdif = sf && sf->albdif;
  if (!bdir) { d.asdir = a->asdir; d.aldir = a->aldir; if (!d.asdir || !d.aldir) return fail(RRTMG_ERR_ARG, "required array 'asdir' / 'aldir' is NULL"); }
  if (!bdif) { d.asdif = a->asdif; d.aldif = a->aldif; if (!d.asdif || !d.aldif) return fail(RRTMG_ERR_ARG, "required array 'asdif' / 'aldif' is NULL"); }
  if (bdir) d.albdir = sf->albdir;
  if (bdif) d.albdif = sf->albdif;
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
  if (!bp) return errflag ? fail(errflag, "device-side error flag " + std::to_string(errflag)) : 0;
  // the band integration, as sw_bandflux_kernel maps its threads: every interface level, or the two boundary levels
  const SwBandOut o{bp->up, bp->dn, bp->upc, bp->dnc, bp->dndir, bp->dndirc};
  const int nrow = bp->levels ? 2 : L + 1;
  for (int row = 0; row < nrow; ++row)
    for (int c = 0; c < N; ++c) sw_band_level(d, T, partdir, o, c, bp->levels ? (row ? L : 0) : row, row, nrow, d.anycld[c] != 0);
  if (errflag) return fail(errflag, "device-side error flag " + std::to_string(errflag));
  return 0;
}
