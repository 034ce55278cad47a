// TEST INFRASTRUCTURE ONLY -- host emulation of the shortwave device functions WITHOUT the clear-sky outputs
// (rrtmg_hip_set_sw_clear_sky(ctx, 0)): sw_fluxes_impl's sequence with the clear-sky outputs off, thread by thread on the CPU,
// on the very __host__ __device__ functions the gfx950 kernels run.  A column with cloud goes through sw_solve_item in the ONE
// mode (sw_solve_cloudy_allsky_kernel), a cloud-free one through the clear-sky variant as ever; the integration is
// sw_flux_level_allsky / sw_heat_layer_allsky, the arithmetic of sw_fluxheat_allsky_kernel.  swuflxc, swdflxc and swhrc of the
// argument struct are not looked at.  Set-up (tables, preparation, cloud optics, McICA mask): as tests/emu/emu_sw.hip, without
// its optional structs.  Built into tests/_emu_allsky/librrtmg_emu_allsky.so by tests/emu_allsky/build.sh; never loaded by the
// product.
#include <cstring>
#include <string>
#include <vector>

#include "../../climt_amd/csrc/rrtmg_sw_device.h"
#include "../../climt_amd/csrc/rrtmg_sw_host.h"
#include "../../climt_amd/csrc/rrtmg_kiss_host.h"
#include "../../include/rrtmg_hip.h"

using namespace rrtmg;

namespace rrtmg {
void mt_mask_host(int ncol, int nlay, int nsub, int icld, int seed, const double *cldfr, std::vector<uint64_t> &mask, int nw, int col0 = 0, int ncol_total = 0);
}

extern "C" int emu_sw_fluxes_allsky(const rrtmg_sw_args *a, const char *blob_path, double cpdair, const double *consts, char *errbuf, int errlen) {
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
  if (d.iaer != 0 && d.iaer != 10) return fail(RRTMG_ERR_ARG, "emu_sw_fluxes_allsky: iaer 0 or 10");
  d.inflag = a->inflgsw; d.iceflag = a->iceflgsw; d.liqflag = a->liqflgsw; d.mcica = a->mcica ? 1 : 0;
  d.k = k;
  std::vector<double> svar_col;
  const long omg = ts.off("sw/sol/mgavgcyc"), osb = ts.off("sw/sol/sbavgcyc");
  const int rc = sw_scalar_setup(d, a->ncol, a->isolvar, a->adjes, a->dyofyr, a->scon, a->solcycfrac, a->bndsolvar, a->indsolvar,
                                 omg >= 0 ? ts.flat.data() + omg : nullptr, osb >= 0 ? ts.flat.data() + osb : nullptr, svar_col, err,
                                 a->shard_col0, a->shard_ncol);
  if (!svar_col.empty()) d.svar_col = svar_col.data();
  if (rc) return fail(rc, err);
  d.play = a->play; d.plev = a->plev; d.tlay = a->tlay; d.h2o = a->h2ovmr; d.o3 = a->o3vmr; d.co2 = a->co2vmr;
  d.ch4 = a->ch4vmr; d.n2o = a->n2ovmr; d.o2 = a->o2vmr; d.coszen = a->coszen;
  d.asdir = a->asdir; d.aldir = a->aldir; d.asdif = a->asdif; d.aldif = a->aldif;
  if (!d.asdir || !d.aldir || !d.asdif || !d.aldif) return fail(RRTMG_ERR_ARG, "required albedo array is NULL");
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
  std::vector<uint64_t> mask;
  d.col0 = 0; d.pcols = N;
  d.part = wd((size_t)kSwNSlot * 4 * nl1);
  d.swuflx = a->swuflx; d.swdflx = a->swdflx; d.swhr = a->swhr;   // (the three clear-sky members stay nullptr, as in sw_fluxes_impl)
  if (!d.swuflx || !d.swdflx || !d.swhr) return fail(RRTMG_ERR_ARG, "output array is NULL");
  int errflag = 0;
  d.err = &errflag;
  for (int c = 0; c < N; ++c) { for (int l = 0; l < L; ++l) sw_prep_layer(d, T, c, l); sw_prep_column(d, T, c); }
  if (d.icld >= 1) {
    for (int lay = 0; lay < L; ++lay) for (int c = 0; c < N; ++c) sw_cloud_layer(d, T, c, lay);
    if (d.mcica) {
      mask.assign((size_t)kSwNGpt * d.nw * N, 0);
      d.mask = mask.data();
      if (a->cldfmcl) {
        for (int g = 0; g < kSwNGpt; ++g) for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c)
          if (a->cldfmcl[((size_t)l * N + c) * kSwNGpt + g] > 1.e-12) mask[((size_t)g * d.nw + (l >> 6)) * N + c] |= 1ull << (l & 63);
      } else if (a->irng == 0) {
        for (int c = 0; c < N; ++c) kiss_mask_column(N, L, kSwNGpt, d.icld, a->permuteseed, d.play, d.cldfr, d.mask, d.nw, d.err, c);
      } else {
        mt_mask_host(N, L, kSwNGpt, d.icld, a->permuteseed, a->cldfr, mask, d.nw, a->shard_col0, a->shard_ncol);
        d.mask = mask.data();
      }
    }
  }
  // the solve, one column at a time: the ONE mode where the device picks sw_solve_cloudy_allsky_kernel (per tile there, per column
  // here); only the F_RUP / F_RUPD rows of the slab are touched: the other half is poisoned and must stay so
  std::vector<double> scr((size_t)F_NTOT * L * 4);
  const double poison = -7.0e300;
  for (int col = 0; col < N; ++col)
    for (int i = 0; i < T.nitem; ++i) {
      SwPartSink sink = sw_part_sink(d, i, col);
      if (d.anycld[col] != 0) {
        for (double &v : scr) v = poison;
        sw_solve_item<true, false, true>(d, T, T.t + T.exp_tbl, T.item[i], col, scr.data(), 1, sink);
        const int g = item_g(T.item[i]);
        for (int l = 0; l < L; ++l)
          for (int f = F_NCLR; f < F_NTOT; ++f)
            for (int q = 0; q < g; ++q)
              if (scr[((size_t)l * F_NTOT + f) * g + q] != poison) return fail(RRTMG_ERR_ARG, "all-sky-only mode wrote a clear-sky scratch row");
      } else {
        sw_solve_item<false>(d, T, T.t + T.exp_tbl, T.item[i], col, scr.data(), 1, sink);
      }
    }
  for (int lev = 0; lev <= L; ++lev) for (int c = 0; c < N; ++c) sw_flux_level_allsky(d, T, c, lev);
  for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) sw_heat_layer_allsky(d, T, c, l);
  if (errflag) return fail(errflag, "device-side error flag " + std::to_string(errflag));
  return 0;
}
