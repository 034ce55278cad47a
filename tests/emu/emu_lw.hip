// TEST INFRASTRUCTURE ONLY -- host emulation of the longwave DEVICE functions (see emu_sw.hip).
#include <cmath>
#include <string>
#include <vector>

#include "../../climt_amd/csrc/rrtmg_lw_device.h"
#include "../../climt_amd/csrc/rrtmg_lw_host.h"
#include "../../include/rrtmg_hip.h"
#include "emu_common.h"

using namespace rrtmg;

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
// The solve without the clear-sky outputs: a column with cloud through the ONE mode (lw_solve_all_allsky_kernel<true, MR>), a
// cloud-free one through the cloud-free variant as ever, both into LwPartSinkAllsky's planes.  What the mode does not own is
// poisoned and checked.  `part` has the DEFAULT layout's size (4 planes per item, 6 with idrv), of which the mode owns the first
// nitem x 2 (3): everything behind them -- where the clear-sky planes of the default layout would start -- must stay as it was,
// and so must the scratch slab (room for 4 g-points per (layer, row)) behind the LF_N x L x G doubles of an item of G g-points.
// -> what went wrong, or nullptr
static const char *emu_lw_solve_allsky(LwDev &d, const LwTab &T, std::vector<double> &part) {
  const double poison = -7.0e300;
  const size_t nl1 = (size_t)d.ncol * (d.nlay + 1);
  const size_t part_full = (size_t)T.nitem * (d.idrv ? 6 : 4) * nl1, part_own = (size_t)T.nitem * lw_allsky_planes(d) * nl1;
  part.assign(part_full, poison);
  d.part = part.data();
  std::vector<double> scr((size_t)LF_N * d.nlay * 4);
  const bool maxrand = !d.mcica && d.icld >= 2;
  for (int slot = 0; slot < T.nitem; ++slot)
    for (int col = 0; col < d.ncol; ++col) {
      LwPartSinkAllsky sink = lw_part_sink_allsky(d, slot, col);
      for (double &v : scr) v = poison;
      const bool cld = emu_lw_cloudy(d, col);
      if (cld && maxrand) lw_solve_item<true, true, false, true>(d, T, T.item[slot], col, scr.data(), 1, sink);
      else if (cld) lw_solve_item<true, false, false, true>(d, T, T.item[slot], col, scr.data(), 1, sink);
      else lw_solve_item<false, false>(d, T, T.item[slot], col, scr.data(), 1, sink);
      const int g = (T.item[slot] >> 16) & 0xf;
      for (size_t i = (size_t)LF_N * d.nlay * g; i < scr.size(); ++i)
        if (scr[i] != poison) return "all-sky-only mode wrote scratch behind its item's rows";
    }
  for (size_t i = 0; i < part_own; ++i)
    if (part[i] == poison) return "all-sky-only mode left a total plane unwritten";
  for (size_t i = part_own; i < part_full; ++i)
    if (part[i] != poison) return "all-sky-only mode wrote a partial plane behind its own";
  return nullptr;
}

// bp: the band fluxes requested (rrtmg_hip_lw_fluxes_bands), or NULL.  clear_sky = 0: the call after
// rrtmg_hip_set_lw_clear_sky(ctx, 0) -- uflxc, dflxc, hrc and duflxc_dt are not looked at, bp->upc and bp->dnc are refused.
extern "C" int emu_lw_fluxes(const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *bp, int clear_sky, const char *blob_path, double cpdair, const double *consts,
                             char *errbuf, int errlen) {
  const EmuFail fail{errbuf, errlen};
  if (!clear_sky && bp && (bp->upc || bp->dnc)) return fail(RRTMG_ERR_ARG, "longwave band fluxes upc / dnc need the clear-sky stream");
  std::string err;
  TableSet ts;
  Constants k;
  if (!emu_tables(blob_path, "lw", cpdair, consts, ts, k, err)) return fail(3, err);
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
  std::vector<double> part_allsky;
  if (clear_sky) d.part = wd((size_t)kLwNGpt * nk * nl1);   // (else: emu_lw_solve_allsky's)
  d.uflx = a->uflx; d.dflx = a->dflx; d.hr = a->hr; d.duflx_dt = a->duflx_dt;
  if (clear_sky) { d.uflxc = a->uflxc; d.dflxc = a->dflxc; d.hrc = a->hrc; d.duflxc_dt = a->duflxc_dt; }   // (else they stay nullptr, as in lw_fluxes_impl)
  else if (!d.uflx || !d.dflx || !d.hr || (d.idrv && !d.duflx_dt)) return fail(RRTMG_ERR_ARG, "output array is NULL");
  int errflag = 0;
  d.err = &errflag;
  for (int c = 0; c < N; ++c) { for (int l = 0; l < L; ++l) lw_prep_layer(d, T, c, l); lw_prep_column(d, T, c); }
  if (clouds) {
    if (!d.mcica) {
      for (int c = 0; c < N; ++c) lw_cloud_column(d, T, c);
      if (d.icld >= 2) { d.mr = wd(lw_mr_size(N, L)); for (int c = 0; c < N; ++c) lw_mr_column(d, c); }
    } else {
      for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) lw_cloudmc_layer(d, T, c, l);
      anym.assign((size_t)d.nw * N, 0);
      d.anymask = anym.data();
      d.mask = emu_mcica_mask(a, kLwNGpt, d.icld, d.nw, d.err, mask);
      for (int c = 0; c < N; ++c) lw_anymask_column(d, c);
    }
  }
  if (!clear_sky) {   // the arithmetic of lw_solve_all_allsky_kernel and lw_fluxheat_allsky_kernel
    if (const char *what = emu_lw_solve_allsky(d, T, part_allsky)) return fail(RRTMG_ERR_ARG, what);
    for (int lev = 0; lev <= L; ++lev) for (int c = 0; c < N; ++c) lw_flux_level_allsky(d, T, c, lev, T.nitem);
    for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) lw_heat_layer_allsky(d, T, c, l);
  } else {
    emu_lw_solve(d, T);
    for (int lev = 0; lev <= L; ++lev) for (int c = 0; c < N; ++c) lw_flux_level(d, T, c, lev, T.nitem, emu_lw_cloudy(d, c));
    for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) lw_heat_layer(d, T, c, l);
  }
  if (bp) {   // as lw_bandflux[_allsky]_kernel maps its threads: every interface level, or the two boundary levels
    const LwBandOut o{bp->up, bp->dn, bp->upc, bp->dnc};
    const int nrow = bp->levels ? 2 : L + 1;
    for (int row = 0; row < nrow; ++row)
      for (int c = 0; c < N; ++c) {
        const int lev = bp->levels ? (row ? L : 0) : row;
        if (clear_sky) lw_band_level(d, T, o, c, lev, row, nrow, emu_lw_cloudy(d, c));
        else lw_band_level_allsky(d, T, o, c, lev, row, nrow);
      }
  }
  if (errflag) return fail(errflag, "device-side error flag " + std::to_string(errflag));
  return 0;
}

// stage check: taug / fracs of every (layer, g-point) of ONE column through lw_prep_column + lw_taug<>
template <int BAND>
static void emu_taug_band(const LwDev &d, const LwTab &T, double *taug, double *fracs) {
  const int L = d.nlay;
  for (int ig = 0; ig < T.b[BAND - 1].ng; ig += 2)
    for (int l = 0; l < L; ++l) {
      LwLayerIn s;
      lw_load_layer(d, 0, l, s);
      V<2> fr;
      const V<2> tg = lw_taug<BAND, 2>(T, s, (l + 1) <= d.laytrop[0], ig, fr);
      for (int j = 0; j < 2; ++j) {
        taug[(size_t)(T.b[BAND - 1].gs + ig + j) * L + l] = tg[j];    // Fortran (nlay, ngpt) order
        fracs[(size_t)(T.b[BAND - 1].gs + ig + j) * L + l] = fr[j];
      }
    }
}

extern "C" int emu_lw_taumol(const rrtmg_lw_args *a, const char *blob_path, double cpdair, const double *consts, double *taug, double *fracs) {
  std::string err;
  TableSet ts;
  Constants k;
  if (!emu_tables(blob_path, "lw", cpdair, consts, ts, k, err)) return 3;
  LwTab T{};
  if (!build_lw_tab(ts, T, err)) return 3;
  T.t = ts.flat.data();
  const int L = a->nlay;
  LwDev d{};
  d.ncol = 1; d.nlay = L; d.k = k;
  d.play = a->play; d.plev = a->plev; d.tlay = a->tlay; d.tlev = a->tlev; d.tsfc = a->tsfc; d.h2o = a->h2ovmr; d.o3 = a->o3vmr;
  d.co2 = a->co2vmr; d.ch4 = a->ch4vmr; d.n2o = a->n2ovmr; d.o2 = a->o2vmr; d.cfc11 = a->cfc11vmr; d.cfc12 = a->cfc12vmr;
  d.cfc22 = a->cfc22vmr; d.ccl4 = a->ccl4vmr; d.emis = a->emis;
  std::vector<std::vector<double>> keep;
  auto wd = [&](size_t n) { keep.emplace_back(n, 0.0); return keep.back().data(); };
  d.prep = wd(lw_prep_size(1, L)); d.secdiff = wd(16);
  std::vector<int32_t> laytrop(1);
  d.laytrop = laytrop.data();
  int errflag = 0;
  d.err = &errflag;
  for (int l = 0; l < L; ++l) lw_prep_layer(d, T, 0, l);
  lw_prep_column(d, T, 0);
  emu_taug_band<1>(d, T, taug, fracs); emu_taug_band<2>(d, T, taug, fracs); emu_taug_band<3>(d, T, taug, fracs); emu_taug_band<4>(d, T, taug, fracs);
  emu_taug_band<5>(d, T, taug, fracs); emu_taug_band<6>(d, T, taug, fracs); emu_taug_band<7>(d, T, taug, fracs); emu_taug_band<8>(d, T, taug, fracs);
  emu_taug_band<9>(d, T, taug, fracs); emu_taug_band<10>(d, T, taug, fracs); emu_taug_band<11>(d, T, taug, fracs); emu_taug_band<12>(d, T, taug, fracs);
  emu_taug_band<13>(d, T, taug, fracs); emu_taug_band<14>(d, T, taug, fracs); emu_taug_band<15>(d, T, taug, fracs); emu_taug_band<16>(d, T, taug, fracs);
  return laytrop[0];
}

// reduced table read-back for the reduction tests: builds tables on the host only
extern "C" long emu_get_table(const char *which, const char *blob_path, double cpdair, const char *name, double *out, long cap) {
  Blob blob;
  std::string err;
  if (!blob.load(blob_path, err)) return -3;
  TableSet ts;
  if (!build_tables(blob, which, cpdair, 9.80665, 86400.0, ts, err)) return -3;
  auto it = ts.reg.find(name);
  if (it == ts.reg.end()) return -1;
  if (out) { if (cap < it->second.n) return -2; memcpy(out, ts.flat.data() + it->second.off, (size_t)it->second.n * 8); }
  return it->second.n;
}
