// TEST INFRASTRUCTURE ONLY -- host emulation of the longwave device functions WITHOUT the clear-sky outputs
// (rrtmg_hip_set_lw_clear_sky(ctx, 0)): lw_fluxes_impl's sequence with the clear-sky outputs off, thread by thread on the CPU,
// on the very __host__ __device__ functions the gfx950 kernels run.  A column with cloud goes through lw_solve_item in the ONE
// mode (lw_solve_all_allsky_kernel<true, MR>), a cloud-free one through the cloud-free variant as ever, both into
// LwPartSinkAllsky's planes; the integration is lw_flux_level_allsky / lw_heat_layer_allsky, the arithmetic of
// lw_fluxheat_allsky_kernel.  uflxc, dflxc, hrc and duflxc_dt of the argument struct are not looked at.  Set-up (tables,
// preparation, cloud optics, McICA mask): as tests/emu/emu_lw.hip, without its band struct.  What the mode does not own is
// poisoned and checked: the partial-plane buffer has the DEFAULT layout's size, and everything behind the planes of the compact
// layout -- where the clear-sky planes of the default layout would start -- must stay as it was; so must the scratch slab behind
// the item's own g-points.  Built into tests/_emu_lw_allsky/librrtmg_emu_lw_allsky.so by tests/emu_lw_allsky/build.sh; never
// loaded by the product.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../climt_amd/csrc/rrtmg_lw_device.h"
#include "../../climt_amd/csrc/rrtmg_lw_host.h"
#include "../../climt_amd/csrc/rrtmg_sw_device.h"
#include "../../include/rrtmg_hip.h"

using namespace rrtmg;

namespace rrtmg {
void mt_mask_host(int ncol, int nlay, int nsub, int icld, int seed, const double *cldfr, std::vector<uint64_t> &mask, int nw, int col0 = 0, int ncol_total = 0);
}

static bool emu_lw_cloudy(const LwDev &d, int col) {
  bool cld = false;
  if (d.icld >= 1 && d.cldfr) for (int l = 0; l < d.nlay; ++l) cld = cld || d.cldfr[(size_t)l * d.ncol + col] > 0.0;
  return cld;
}

extern "C" int emu_lw_fluxes_allsky(const rrtmg_lw_args *a, const char *blob_path, double cpdair, const double *consts, char *errbuf, int errlen) {
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
  d.col0 = 0; d.pcols = N;
  // the partial planes: the size of the default layout (4 planes per item, 6 with idrv), of which the mode owns the first
  // nitem x 2 (3); the rest is poisoned
  const double poison = -7.0e300;
  const size_t part_full = (size_t)T.nitem * (d.idrv ? 6 : 4) * nl1, part_own = (size_t)T.nitem * lw_allsky_planes(d) * nl1;
  std::vector<double> part(part_full, poison);
  d.part = part.data();
  d.uflx = a->uflx; d.dflx = a->dflx; d.hr = a->hr; d.duflx_dt = a->duflx_dt;   // (the clear-sky members stay nullptr, as in lw_fluxes_impl)
  if (!d.uflx || !d.dflx || !d.hr || (d.idrv && !d.duflx_dt)) return fail(RRTMG_ERR_ARG, "output array is NULL");
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
  // the solve, one column at a time; the scratch slab has room for 4 g-points per (layer, row): an item of G g-points owns the
  // first LF_N x L x G doubles
  std::vector<double> scr((size_t)LF_N * L * 4);
  const bool maxrand = !d.mcica && d.icld >= 2;
  for (int slot = 0; slot < T.nitem; ++slot)
    for (int col = 0; col < N; ++col) {
      LwPartSinkAllsky sink = lw_part_sink_allsky(d, slot, col);
      for (double &v : scr) v = poison;
      const bool cld = emu_lw_cloudy(d, col);
      if (cld && maxrand) lw_solve_item<true, true, false, true>(d, T, T.item[slot], col, scr.data(), 1, sink);
      else if (cld) lw_solve_item<true, false, false, true>(d, T, T.item[slot], col, scr.data(), 1, sink);
      else lw_solve_item<false, false>(d, T, T.item[slot], col, scr.data(), 1, sink);
      const int g = (T.item[slot] >> 16) & 0xf;
      for (size_t i = (size_t)LF_N * L * g; i < scr.size(); ++i)
        if (scr[i] != poison) return fail(RRTMG_ERR_ARG, "all-sky-only mode wrote scratch behind its item's rows");
    }
  for (size_t i = 0; i < part_own; ++i)
    if (part[i] == poison) return fail(RRTMG_ERR_ARG, "all-sky-only mode left a total plane unwritten");
  for (size_t i = part_own; i < part_full; ++i)
    if (part[i] != poison) return fail(RRTMG_ERR_ARG, "all-sky-only mode wrote a partial plane behind its own");
  for (int lev = 0; lev <= L; ++lev) for (int c = 0; c < N; ++c) lw_flux_level_allsky(d, T, c, lev, T.nitem);
  for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c) lw_heat_layer_allsky(d, T, c, l);
  if (errflag) return fail(errflag, "device-side error flag " + std::to_string(errflag));
  return 0;
}
