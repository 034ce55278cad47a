// rrtmg_lw.hip -- longwave kernels and launch sequence (gfx950).
//
// Launch sequence of one rrtmg_hip_lw_fluxes call (all on the context's longwave stream):
//   kiss_mask_kernel / mask upload + lw_anymask_kernel (McICA, whole grid)
//   per column chunk (<= RRTMG_HIP_CHUNK_TILES tiles), so that a chunk's rows are still cached when its solve reads them:
//     lw_prep_fused_kernel <<<tiles, 16 waves>>>  inatm + setcoef per (column, layer), then the column part (laytrop,
//                          precipitable water -> secdiff, tile cloud flag) on what the layer part left in LDS; non-McICA cloudy
//                          tiles: cldprop and the rtrnmr overlap factors
//     lw_cloudmc_kernel    (McICA)                cldprmc band optics per (column, layer)
//     tile_lists_kernel    <<<1, 64>>>            the chunk's tiles by solve variant, compacted in tile order (LwDev::tlist)
//     lw_solve_all_kernel  one launch per variant (cloud-free / cloudy tiles): wavefront = tile(64 columns) x work item (4|2
//                          g-points of a band), workgroup = 4 tiles of one item sharing its k-distribution slice in LDS
//     lw_fluxheat_kernel   <<<(tiles, levels/15), 16 waves>>>  band / g-point integration per interface + heating rates
// With the clear-sky outputs off (rrtmg_hip_set_lw_clear_sky(0)): lw_solve_all_allsky_kernel in the place of lw_solve_all_kernel,
// lw_fluxheat_allsky_kernel in the place of lw_fluxheat_kernel, lw_bandflux_allsky_kernel in the place of lw_bandflux_kernel;
// uflxc, dflxc, hrc and duflxc_dt are neither formed nor copied, and the partial planes are half as many
// The host steps this call shares with the shortwave's (gate, checks, chunk plan and loop, mask choice, epilogue): rrtmg_call.h;
// the call's grid arrays -- what the driver, the sorted call and the float32 boundary register, gather and copy: the tables
// kLwIn / kLwOut of rrtmg_call_arrays.h
#include "rrtmg_call.h"
#include "rrtmg_lw_device.h"
#include "rrtmg_lw_host.h"
#include "rrtmg_solve_map.h"

namespace rrtmg {

// Preparation in ONE launch (see sw_prep_fused_kernel): phase 1 the layer part, layers strided over the 16 waves; phase 2
// wave 0: the column scan (laytrop, precipitable water -> diffusivity angles) on the rows just written, and the tile's
// cloud flag; phase 3, cloudy tiles only: cldprop / the rtrnmr overlap factors (one wave each, sequential in the layers as
// the reference); with McICA the cldprmc band optics stay a launch of their own (see sw_prep_fused_kernel).
constexpr int kPrepWaves = 16;
constexpr int kLwKeepLayers = 104;   // 104 x 3 x 64 doubles = 156 KB of the 160 KB a gfx950 workgroup can have
static_assert(kLwKeepLayers * 3 * 64 * sizeof(double) + 1024 <= 160 * 1024, "lw_prep_fused_kernel: LDS budget of gfx950");
__global__ void __launch_bounds__(64 * kPrepWaves) lw_prep_fused_kernel(LwDev d, LwTab T, int clouds, int maxrand, int keep_layers, int tile0) {
  const int tile = tile0 + blockIdx.x;   // (launched per column chunk, see sw_prep_fused_kernel)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = tile * 64 + lane;
  const bool act = col < d.ncol;
  __shared__ int sh_cld;
  // what the column scan reads back from the layer part -- [layer][coldry | h2o | lower flag][lane] -- in DYNAMIC LDS sized by
  // the launch for the grid's layer count (92 KB at 60 layers: a second workgroup, or a longwave solve workgroup, still fits
  // the CU); grids deeper than kLwKeepLayers get none (keep_layers = 0) and re-read the slab
  extern __shared__ __attribute__((aligned(16))) double sh_keep[];
  __shared__ int sh_any[kPrepWaves];
  const bool keep = keep_layers > 0;
  bool cld = false;
  if (act)
    for (int l = w; l < d.nlay; l += kPrepWaves) {
      lw_prep_layer(d, T, col, l, keep ? sh_keep + (3 * l) * 64 + lane : nullptr, 64);
      if (d.icld >= 1 && d.cldfr) cld = cld || d.cldfr[(long)l * d.ncol + col] > 0.0;
    }
  {
    const unsigned long long any = __ballot(cld);
    if (lane == 0) sh_any[w] = any != 0ull;
  }
  __syncthreads();
  if (w == 0) {
    if (act) lw_prep_column(d, T, col, keep ? sh_keep + lane : nullptr, 64);
    if (lane == 0) {
      int any = 0;
      for (int k = 0; k < kPrepWaves; ++k) any |= sh_any[k];
      d.tile_cld[tile] = any; sh_cld = any;
      if (any) atomicAdd(d.ncloudy, 1);
    }
  }
  if (!clouds) return;
  __syncthreads();
  if (!sh_cld || !act) return;
  if (w == 0) lw_cloud_column(d, T, col);
  if (w == kPrepWaves - 1 && maxrand) lw_mr_column(d, col);
}

__global__ void __launch_bounds__(64) lw_cloudmc_kernel(LwDev d, LwTab T, int tile0) {
  const int tile = tile0 + blockIdx.x;
  if (!d.tile_cld[tile]) return;
  const int col = tile * 64 + threadIdx.x;
  if (col < d.ncol) lw_cloudmc_layer(d, T, col, blockIdx.y);
}
__global__ void __launch_bounds__(64) lw_anymask_kernel(LwDev d) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  if (col < d.ncol) lw_anymask_column(d, col);
}

// All 140 g-points in ONE launch.  Wavefront = 64 columns of one tile x one work item (4 or 2 consecutive g-points
// of a band, LwTab::item).  The thread carries the item's g-points through both sweeps: the layer state, the species
// mixtures (specparm/js/fs of the major, minor and Planck mixtures, adjusted columns), the Planck functions and the
// cloud optics -- more than half of the per-g-point work of rtrnmc+taumol -- are evaluated once per item.  The item's
// band-weighted radiances are summed in registers: part[item][k][level][column].
// Workgroup = kLwWgWaves wavefronts = the same item for kLwWgWaves consecutive tiles, sharing ONE copy of the item's
// k-distribution slice in LDS: columns ig0..ig0+G-1 of the band's table slab, [nrows][G], <= 66 KB, two workgroups per
// CU.  Every absorption-coefficient / Planck-fraction row a lane needs is then a 16/32-byte LDS read at a per-lane
// row (bank conflicts only) instead of a per-lane gather through the vector L1, whose return path (64 B/clk/CU) the
// ~30 row gathers per layer saturated: with the rows through the scalar cache (an ablation) the kernel ran 23 %
// faster, which bounded what staging could win.
// Launch order: blocks of kLwGroupBlocks workgroups = kLwTileGroup tiles (rrtmg_solve_map.h) -- the block's prep rows stay
// L2-resident while its items run.  Speed only, never correctness.
constexpr int kLwWgWaves = 4;
constexpr int kLwTileGroup = 32;
constexpr int kLwGroupBlocks = kLwTileGroup / kLwWgWaves;
static_assert(kLwTileGroup % kLwWgWaves == 0, "tile group must be a whole number of workgroups");
// Two variants are launched back to back (see sw_solve_all_kernel): CLD = false for the cloud-free tiles.
// MR = true: non-McICA maximum/random overlap (rtrnmr).
// (lw_solve_all_allsky_kernel below carries a copy of this kernel's body: routed through a shared body with the sink made by a
//  lambda, all three instantiations came out with the same number of instructions in another order -- rung C of the acceptance
//  ladder, docs/EXPERIMENTS.md -- so a change to the staging or the addressing here is made there too)
template <bool CLD, bool MR>
__global__ void __launch_bounds__(64 * kLwWgWaves) __attribute__((amdgpu_waves_per_eu(2))) lw_solve_all_kernel(LwDev d, LwTab T, int tile0, int ntile) {   // tiles tile0 .. tile0 + ntile - 1 (one column chunk)
  const int nmine = d.tcnt[CLD ? 1 : 0];
  const SolveWork m = solve_map<kLwWgWaves, kLwGroupBlocks>(blockIdx.x, nmine, T.nitem);
  if (!m.work) return;
  const int first = m.first, k = m.k;
  RRTMG_PROFILE_ONLY_ITEM(d, k)
  const int slot = T.sched[k], item = T.item[slot];
  const int g = (item >> 16) & 0xf, ig0 = (item >> 8) & 0xff;
  constexpr bool kLdsK = true;
  __shared__ __attribute__((aligned(16))) double sh_k[kLwSlabMaxRows * 4];   // rows are read 16 bytes at a time
  {
    const LwBandTab &B = T.b[item & 0xff];
    const double *src = T.t + B.slab + ig0;
    const int ng = B.ng, sh = g == 4 ? 2 : 1, n = B.nrows << sh;
    for (int i = threadIdx.x; i < n; i += 64 * kLwWgWaves) sh_k[i] = src[(long)(i >> sh) * ng + (i & (g - 1))];
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (first + wave >= nmine) return;
  const int ctile = d.tlist[(CLD ? d.tcap : 0) + first + wave], tile = tile0 + ctile;
  const int lane = threadIdx.x & 63;
  const int col = tile * 64 + lane;
  if (col >= d.ncol) return;
  double *scr = d.scratch + ((long)ctile * kLwNGpt + ((item >> 20) & 0xff)) * (long)LF_N * d.nlay * 64 + lane * 2;
  LwPartSink sink = lw_part_sink(d, slot, col);
  lw_solve_item<CLD, MR, kLdsK>(d, T, item, col, scr, 64, sink, sh_k);
}

// band integration AND heating rates in one launch (see sw_fluxheat_kernel)
constexpr int kFluxLev = 15;   // 16 waves per workgroup: the halo level is 1 in 16 of the partial-plane reads
// CLEAR = false: without the clear-sky half -- LwPartSinkAllsky's planes in EVERY tile; uflxc, dflxc, hrc and duflxc_dt are
// never dereferenced
template <bool CLEAR>
__device__ __forceinline__ void lw_fluxheat_body(const LwDev &d, const LwTab &T, int tile0) {
  // (the call's last launch leaves the preparation kernels' cloudy-tile count where the host will look for it, and clears it)
  if (d.hint_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { *d.hint_out = *d.ncloudy; *d.ncloudy = 0; }
  const int tile = tile0 + blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int col = tile * 64 + lane, lev = blockIdx.y * kFluxLev + j;
  __shared__ double net[kFluxLev + 1][64], netc[CLEAR ? kFluxLev + 1 : 1][64];
  const bool act = col < d.ncol && lev <= d.nlay;
  if (act) {
    double f[6];   // up, down, clear-sky up, clear-sky down, d(up)/dTs, clear-sky d(up)/dTs; without the clear-sky half: up, down, d(up)/dTs
    if (CLEAR) lw_flux_sums(d, col, lev, T.nitem, d.tile_cld[tile] != 0, f);
    else lw_flux_sums_allsky(d, col, lev, T.nitem, f);
    if (j < kFluxLev || lev == d.nlay) {
      const long o = (long)lev * d.ncol + col;
      d.uflx[o] = f[0]; d.dflx[o] = f[1];
      if (CLEAR) { d.uflxc[o] = f[2]; d.dflxc[o] = f[3]; }
      if (d.idrv) {
        d.duflx_dt[o] = f[CLEAR ? 4 : 2];
        if (CLEAR) d.duflxc_dt[o] = f[5];
      }
    }
    net[j][lane] = f[0] - f[1];
    if (CLEAR) netc[j][lane] = f[2] - f[3];
  }
  __syncthreads();
  if (col < d.ncol && j < kFluxLev && lev < d.nlay) {
    const long o0 = (long)lev * d.ncol + col;
    const double dp = d.plev[o0] - d.plev[o0 + d.ncol];
    d.hr[o0] = T.heatfac * (net[j][lane] - net[j + 1][lane]) / dp;
    if (CLEAR) d.hrc[o0] = T.heatfac * (netc[j][lane] - netc[j + 1][lane]) / dp;
  }
}
__global__ void __launch_bounds__(64 * (kFluxLev + 1)) lw_fluxheat_kernel(LwDev d, LwTab T, int tile0) { lw_fluxheat_body<true>(d, T, tile0); }

// Band fluxes (rrtmg_hip_lw_fluxes_bands), launched per column chunk behind lw_fluxheat_kernel: one thread per (column,
// level), lane = column, the per-band sums of lw_band_level (see sw_bandflux_kernel).  levels = 0: every interface level;
// 1: a workgroup of two waves, row 0 = surface, row 1 = top.  ALLSKY: on LwPartSinkAllsky's planes, the members up and dn (upc,
// dnc: refused by the driver)
constexpr int kBandLev = 4;
template <bool ALLSKY>
__device__ __forceinline__ void lw_bandflux_body(const LwDev &d, const LwTab &T, int tile0, const LwBandOut &o, int levels) {
  const int tile = tile0 + blockIdx.x, col = tile * 64 + (threadIdx.x & 63), row = blockIdx.y * kBandLev + (threadIdx.x >> 6);
  const int lev = levels ? (row ? d.nlay : 0) : row;
  if (col >= d.ncol || row > (levels ? 1 : d.nlay)) return;
  if (ALLSKY) lw_band_level_allsky(d, T, o, col, lev, row, levels ? 2 : d.nlay + 1);
  else lw_band_level(d, T, o, col, lev, row, levels ? 2 : d.nlay + 1, d.tile_cld[tile] != 0);
}
__global__ void __launch_bounds__(64 * kBandLev) lw_bandflux_kernel(LwDev d, LwTab T, int tile0, LwBandOut o, int levels) { lw_bandflux_body<false>(d, T, tile0, o, levels); }

// ---- No clear-sky outputs (rrtmg_hip_set_lw_clear_sky(0); opt-in) ----------------------------------------------------------------
// Kernels of their own, launched INSTEAD of lw_solve_all_kernel, lw_fluxheat_kernel and lw_bandflux_kernel when the clear-sky
// outputs are off: with them on the launch sequence and every kernel in it are those of a library without the option
// (tools/isa_compare.py, profiles/isa_compare_lw_allsky_only.txt).  The partial planes are LwPartSinkAllsky's: up and down (and
// d(up)/dTs with idrv) per item, in every tile.  CLD = true: lw_solve_thread's ONE mode, the total-sky stream alone.  CLD = false:
// the cloud-free tiles run the device functions they always ran -- lw_solve_thread<.., CLD = false> has no second stream -- and
// differ from lw_solve_all_kernel<false, false> in where the sink stores.  Tile lists, launch order, LDS staging and
// amdgpu_waves_per_eu: lw_solve_all_kernel's.
template <bool CLD, bool MR>
__global__ void __launch_bounds__(64 * kLwWgWaves) __attribute__((amdgpu_waves_per_eu(2))) lw_solve_all_allsky_kernel(LwDev d, LwTab T, int tile0, int ntile) {
  const int nmine = d.tcnt[CLD ? 1 : 0];
  const SolveWork m = solve_map<kLwWgWaves, kLwGroupBlocks>(blockIdx.x, nmine, T.nitem);
  if (!m.work) return;   // workgroup-uniform exit before the slice is staged
  const int first = m.first, k = m.k;
  RRTMG_PROFILE_ONLY_ITEM(d, k)
  const int slot = T.sched[k], item = T.item[slot];
  const int g = (item >> 16) & 0xf, ig0 = (item >> 8) & 0xff;
  __shared__ __attribute__((aligned(16))) double sh_k[kLwSlabMaxRows * 4];   // rows are read 16 bytes at a time
  {
    const LwBandTab &B = T.b[item & 0xff];
    const double *src = T.t + B.slab + ig0;
    const int ng = B.ng, sh = g == 4 ? 2 : 1, n = B.nrows << sh;
    for (int i = threadIdx.x; i < n; i += 64 * kLwWgWaves) sh_k[i] = src[(long)(i >> sh) * ng + (i & (g - 1))];
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (first + wave >= nmine) return;
  const int ctile = d.tlist[(CLD ? d.tcap : 0) + first + wave], tile = tile0 + ctile;
  const int lane = threadIdx.x & 63;
  const int col = tile * 64 + lane;
  if (col >= d.ncol) return;
  double *scr = d.scratch + ((long)ctile * kLwNGpt + ((item >> 20) & 0xff)) * (long)LF_N * d.nlay * 64 + lane * 2;
  LwPartSinkAllsky sink = lw_part_sink_allsky(d, slot, col);
  lw_solve_item<CLD, MR, true, CLD>(d, T, item, col, scr, 64, sink, sh_k);
}
__global__ void __launch_bounds__(64 * (kFluxLev + 1)) lw_fluxheat_allsky_kernel(LwDev d, LwTab T, int tile0) { lw_fluxheat_body<false>(d, T, tile0); }
__global__ void __launch_bounds__(64 * kBandLev) lw_bandflux_allsky_kernel(LwDev d, LwTab T, int tile0, LwBandOut o, int levels) { lw_bandflux_body<true>(d, T, tile0, o, levels); }

void free_lw_desc(rrtmg_ctx *ctx) {
  delete (LwTab *)ctx->lw_desc;
  ctx->lw_desc = nullptr;
}

int lw_init_impl(rrtmg_ctx *ctx, double cpdair, const char *blob_path) {
  if (!ctx->have_constants) return ctx->fail(RRTMG_ERR_NOT_INITIALISED, "set_constants must be called before lw_init");
  std::string path = blob_path ? std::string(blob_path) : default_blob_path("lw");
  Blob blob;
  std::string err;
  if (!blob.load(path, err)) return ctx->fail(RRTMG_ERR_TABLES, "%s", err.c_str());
  ctx->lw_ts = TableSet();
  if (!build_tables(blob, "lw", cpdair, ctx->k.grav, ctx->k.secdy, ctx->lw_ts, err)) return ctx->fail(RRTMG_ERR_TABLES, "%s", err.c_str());
  LwTab *T = ctx->lw_desc ? (LwTab *)ctx->lw_desc : new LwTab();
  ctx->lw_desc = T;
  if (!build_lw_tab(ctx->lw_ts, *T, err)) return ctx->fail(RRTMG_ERR_TABLES, "%s", err.c_str());
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  if (ctx->lw_tab_dev) (void)hipFree(ctx->lw_tab_dev);
  ctx->lw_tab_dev = nullptr;
  RRTMG_HIP_CHECK(ctx, hipMalloc((void **)&ctx->lw_tab_dev, ctx->lw_ts.flat.size() * sizeof(double)));
  RRTMG_HIP_CHECK(ctx, hipMemcpy(ctx->lw_tab_dev, ctx->lw_ts.flat.data(), ctx->lw_ts.flat.size() * sizeof(double), hipMemcpyHostToDevice));
  T->t = ctx->lw_tab_dev;
  ctx->lw_ready = true;
  return RRTMG_OK;
}

// the outputs a call must be given: the standard ones, and with idrv the derivative(s)
static int lw_check_outputs(rrtmg_ctx *ctx, unsigned on, const LwStructs &x) {
  if (int rc = check_outputs(ctx, kLwOut, on, x)) return rc;
  const bool clr = on & kClear;
  if ((on & kDrv) && (!x.duflx_dt || (clr && !x.duflxc_dt))) return ctx->fail(RRTMG_ERR_ARG, clr ? "idrv=1 needs duflx_dt/duflxc_dt" : "idrv=1 needs duflx_dt");
  return RRTMG_OK;
}
// the call on an internal copy of its inputs, cloud-free columns first (rrtmg_permute.h; see sw_permuted_call): what the driver
// reads (kLwIn under lw_call_reads; the gate has icld != 0), the optional arrays where they are given
static int lw_sorted_call(rrtmg_ctx *ctx, const rrtmg_lw_args *a) {
  if (int rc = ctx_prepare_device(ctx)) return rc;
  const CallSite c{ctx, 1, call_stream(ctx, 1, 1)};
  // (clear-sky outputs off: the four are absent from the scatter table, and from the inner call)
  LwStructs b(a, nullptr);
  const unsigned on = lw_call_reads(a, nullptr, ctx->lw_clear_sky);
  if (int rc = lw_check_outputs(ctx, on, b)) return rc;
  ColumnPermute pm(ctx, c.s, kInnerSorted, a->ncol, a->nlay, "lw.sort.");
  if (!pm.prepare(a->cldfr)) return ctx->status;
  b.ncol = pm.Np; b.shard_col0 = 0; b.shard_ncol = 0;
  const GridShape g = grid_shape(a->ncol, a->nlay, 0);
  permute_inputs(pm, kLwIn, on, b, g);
  // exponential overlap: the rank correlations are one more [nlay][N] input of the mask step
  if (call_overlap_exp(ctx, 1, a) && !a->cldfmcl) ctx->alpha_inner[1] = pm.gather("alpha", ctx->alpha[1].dev, g.L);
  if (!pm.ok) { ctx->alpha_inner[1] = nullptr; return ctx->status; }
  pm.flush_gather();
  permute_outputs(pm, kLwOut, on, b, g);
  if (!pm.ok) { ctx->alpha_inner[1] = nullptr; return ctx->status; }
  return permuted_tail(c, pm, [&]() { return lw_fluxes_impl(ctx, &b); });
}

// bp: the band fluxes requested (at least one member set, levels 0 or 1), or nullptr for the plain call.  A call with bands
// is never sorted: its outputs would need a scatter of their own.
// the clear-sky band members of a call without the clear-sky stream: refused before anything is enqueued
static int lw_refuse_clear_bands(rrtmg_ctx *ctx, const rrtmg_lw_band_fluxes *bp) {
  if (ctx->lw_clear_sky || !bp || (!bp->upc && !bp->dnc)) return RRTMG_OK;
  return ctx->fail(RRTMG_ERR_ARG, "longwave band fluxes upc / dnc need the clear-sky stream: rrtmg_hip_set_lw_clear_sky(ctx, 0) is in force (set it to 1 for this call, or request up / dn only)");
}

int lw_fluxes_impl(rrtmg_ctx *ctx, const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *bp) {
  const bool clr = ctx->lw_clear_sky;   // rrtmg_hip_set_lw_clear_sky: false = uflxc, dflxc, hrc and duflxc_dt are neither formed nor read from `a`
  if (int orc = call_overlap_check(ctx, 1, a)) return orc;
  if (call_is_sorted(ctx, 1, a, bp != nullptr)) return lw_sorted_call(ctx, a);
  int rc = call_begin(ctx, 1, a);
  if (rc) return rc;
  if ((rc = lw_refuse_clear_bands(ctx, bp))) return rc;   // (a call with bands is never sorted; nothing is enqueued yet)
  const CallSite c{ctx, 1, call_stream(ctx, 1, a->memspace)}; hipStream_t s = c.s;
  const int N = a->ncol, L = a->nlay;
  const size_t nl = (size_t)N * L, nl1 = (size_t)N * (L + 1);
  const LwTab &T = *(LwTab *)ctx->lw_desc;
  LwBound bound{};   // the kernels' struct and what else the array tables bind (rrtmg_call_arrays.h)
  LwDev &d = bound;
  d.ncol = N; d.nlay = L;
  const double *alpha = nullptr;
  d.icld = call_overlap(ctx, 1, a, alpha);    // (outside 0..3: 2, rrtmg_lw_rad.nomcica.f90:436; 4, 5 with rank correlations set)
  d.idrv = a->idrv ? 1 : 0;
  d.inflag = a->inflglw; d.iceflag = a->iceflglw; d.liqflag = a->liqflglw; d.mcica = a->mcica ? 1 : 0;
  d.k = ctx->k;
  RRTMG_PROFILE_READ_ONLY_ITEM(d)
  d.fluxfac = (2.0 * asin(1.0)) * 2.e4;       // rrtmg_lw_rad.nomcica.f90:420-421
  const bool maxrand = !d.mcica && d.icld >= 2;   // rtrnmr (rrtmg_lw_rad.nomcica.f90:527-544)
  if (d.mcica && d.icld >= 1 && d.inflag == 1) return ctx->fail(RRTMG_ERR_INFLAG1_MCICA, "longwave: %s", status_message(RRTMG_ERR_INFLAG1_MCICA));   // rrtmg_lw_cldprmc.f90:172

  // ---- inputs (rrtmg_host_inputs.h: uniform arrays are filled on the device, all-zero band arrays are absent) ----------------
  bool ok = true;
  const double ps = a->pressure_scale, ws = a->water_path_scale;
  HostInputs hi(ctx, s, "lw.in.", a->memspace, call_share(ctx), 1, ctx->f32);
  const LwStructs x(a, bp);
  const unsigned on = lw_call_reads(a, bp, clr);
  const GridShape g = grid_shape(N, L, bp ? bp->levels : 0);
  const bool clouds = on & kClouds;
  // (taucld given directly -- inflag 0 -- is used as it is; otherwise zeros mean there is none to add, as for tauaer)
  const InRule optional{false};
  const InRuleFor<LwBound> rules[] = {
      {&LwDev::play, {true, InPolicy::Plain, ps}}, {&LwDev::plev, {true, InPolicy::Plain, ps}}, {&LwDev::h2o, {true, InPolicy::Plain, a->h2o_mul, a->h2o_div}},
      {&LwDev::tlev, optional}, {&LwDev::cfc11, optional}, {&LwDev::cfc12, optional}, {&LwDev::cfc22, optional}, {&LwDev::ccl4, optional},
      {&LwDev::taucld, {d.inflag == 0, d.inflag == 0 ? InPolicy::Plain : InPolicy::ZeroAbsent}},
      {&LwDev::cicewp, {d.inflag >= 1, InPolicy::Plain, ws}}, {&LwDev::cliqwp, {d.inflag >= 1, InPolicy::Plain, ws}}, {&LwDev::reice, {d.inflag == 2}}, {&LwDev::reliq, {d.inflag == 2}},
      {&LwDev::tauaer, {false, InPolicy::ZeroAbsent}}, {&CallLocals::cldfmcl, optional}};   // (the sub-columns: where given)
  register_inputs(hi, kLwIn, on, x, bound, g, rules);
  if (!hi.finish()) return ctx->status;

  auto wd = [&](const char *name, size_t n) -> double * { double *p = (double *)ctx->buf(std::string("lw.w.") + name, n * sizeof(double)); if (!p) ok = false; return p; };
  d.prep = wd("prep", lw_prep_size(N, L));
  d.secdiff = wd("secdiff", (size_t)N * 16);
  d.laytrop = (int32_t *)ctx->buf("lw.w.laytrop", (size_t)N * 4);
  d.ncbands = (int32_t *)ctx->buf("lw.w.ncbands", (size_t)N * 4);
  d.tile_cld = (int32_t *)ctx->buf("lw.w.tilecld", (size_t)((N + 63) / 64) * 4);
  d.ncloudy = ctx->ncloudy_dev + 1;
  if (maxrand) d.mr = wd("mr", lw_mr_size(N, L));
  if (!d.laytrop || !d.ncbands || !d.tile_cld) ok = false;
  if (clouds) d.ctau = wd("ctau", nl * 16);
  d.nw = (L + 63) / 64;
  if (clouds && d.mcica) {
    d.mask = (uint64_t *)ctx->buf("lw.w.mask", (size_t)kLwNGpt * d.nw * N * 8);
    d.anymask = (uint64_t *)ctx->buf("lw.w.anymask", (size_t)d.nw * N * 8);
    if (!d.mask || !d.anymask) ok = false;
  }
  const int ntile = (N + 63) / 64;
  const int nk = clr ? (d.idrv ? 6 : 4) : lw_allsky_planes(d);   // partial planes per item (LwPartSink | LwPartSinkAllsky)
  const int hint_cloudy = call_hint_cloudy(ctx, 1, ntile, L);
  const int ctile = plan_call_chunks(ctx, 1, d, clouds, hint_cloudy, (size_t)kLwNGpt * LF_N * L * 64 * sizeof(double));   // tiles per solve chunk
  if (!d.tlist) ok = false;
  d.scratch = wd("scratch", (size_t)ctile * kLwNGpt * LF_N * L * 64);
  d.part = wd("part", (size_t)T.nitem * nk * (L + 1) * ctile * 64);
  if ((rc = lw_check_outputs(ctx, on, x))) return rc;
  // the outputs: the standard ones (with idrv: the derivatives), the band fluxes [16][nrow][ncol] where requested
  // (clear-sky outputs off: d.uflxc, d.dflxc, d.hrc and d.duflxc_dt stay nullptr -- no kernel of that path dereferences them)
  OutCopy oc[table_size(kLwOut)];
  const int nout = bind_outputs(kLwOut, on, x, bound, g, a->memspace, wd, oc);
  const LwBandOut &bo = bound;
  if (!ok) return ctx->status;
#ifdef RRTMG_PROFILE
  d.phase = (unsigned long long *)ctx->buf("lw.w.phase", 16 * 8);
  if (!d.phase) return ctx->status;
  RRTMG_HIP_CHECK(ctx, hipMemsetAsync(d.phase, 0, 16 * 8, s));
#endif
  if ((rc = call_own_flag(c, a->memspace, d))) return rc;

  const dim3 gcol(ntile), blk(64);
  if (!d.tlev) {
    // no interface temperatures given: log-pressure interpolation of the layer temperatures on the device, as climt's
    // host does before the call when calculate_interface_temperature is set (lw/component.py:378-384, util.py:89-142)
    double *tl = wd("tlev", nl1);
    if (!ok) return ctx->status;
    launch_interface_values(s, N, L, d.tlay, d.tsfc, d.play, d.plev, tl);
    d.tlev = tl;
  }
  // (more than 64 KB of dynamic LDS has to be allowed per kernel once; if the runtime refuses, the scan re-reads the slab)
  const bool big_lds = ctx->allow_dynamic_lds(0, (const void *)lw_prep_fused_kernel, kLwKeepLayers * 3 * 64 * (int)sizeof(double));
  const int keep_layers = (L <= kLwKeepLayers && (big_lds || (size_t)L * 3 * 64 * sizeof(double) <= 64 * 1024)) ? L : 0;
  if (clouds && d.mcica && (rc = mcica_mask_launch(c, kLwNGpt, d, a, bound.cldfmcl, nullptr, nullptr, alpha))) return rc;
  if (clouds && d.mcica) hipLaunchKernelGGL(lw_anymask_kernel, gcol, blk, 0, s, d);
  // preparation, solve and band integration, one column chunk at a time (see sw_fluxes_impl)
  const dim3 lwwg(64 * kLwWgWaves);
  auto lwgrid = [&](int nt) { return dim3((nt + kLwTileGroup - 1) / kLwTileGroup * kLwGroupBlocks * T.nitem); };
  run_chunks(c, d, clouds, hint_cloudy,
    [&](int t0, int nt) {
      hipLaunchKernelGGL(lw_prep_fused_kernel, dim3(nt), dim3(64 * kPrepWaves), (size_t)keep_layers * 3 * 64 * sizeof(double), s, d, T,
                         clouds && !d.mcica ? 1 : 0, maxrand ? 1 : 0, keep_layers, t0);
      if (clouds && d.mcica) hipLaunchKernelGGL(lw_cloudmc_kernel, dim3(nt, L), blk, 0, s, d, T, t0);
      hipLaunchKernelGGL(tile_lists_kernel, dim3(1), blk, 0, s, d.tile_cld + t0, nt, (int32_t *)d.tlist, (int32_t *)d.tcnt, d.tcap);
    },
    [&](int t0, int nt) {
      if (!clr) hipLaunchKernelGGL((lw_solve_all_allsky_kernel<false, false>), lwgrid(nt), lwwg, 0, s, d, T, t0, nt);
      else hipLaunchKernelGGL((lw_solve_all_kernel<false, false>), lwgrid(nt), lwwg, 0, s, d, T, t0, nt);
    },
    [&](int t0, int nt) {
      if (!clr && maxrand) hipLaunchKernelGGL((lw_solve_all_allsky_kernel<true, true>), lwgrid(nt), lwwg, 0, s, d, T, t0, nt);
      else if (!clr) hipLaunchKernelGGL((lw_solve_all_allsky_kernel<true, false>), lwgrid(nt), lwwg, 0, s, d, T, t0, nt);
      else if (maxrand) hipLaunchKernelGGL((lw_solve_all_kernel<true, true>), lwgrid(nt), lwwg, 0, s, d, T, t0, nt);
      else hipLaunchKernelGGL((lw_solve_all_kernel<true, false>), lwgrid(nt), lwwg, 0, s, d, T, t0, nt);
    },
    [&](int t0, int nt) {
      const auto flux_k = clr ? lw_fluxheat_kernel : lw_fluxheat_allsky_kernel;
      const auto band_k = clr ? lw_bandflux_kernel : lw_bandflux_allsky_kernel;
      hipLaunchKernelGGL(flux_k, dim3(nt, (L + kFluxLev) / kFluxLev), dim3(64 * (kFluxLev + 1)), 0, s, d, T, t0);
      if (bp && bp->levels) hipLaunchKernelGGL(band_k, dim3(nt, 1), dim3(64 * 2), 0, s, d, T, t0, bo, 1);
      else if (bp) hipLaunchKernelGGL(band_k, dim3(nt, (L + kBandLev) / kBandLev), dim3(64 * kBandLev), 0, s, d, T, t0, bo, 0);
    });
#ifdef RRTMG_PROFILE
  {
    unsigned long long ph[16];
    RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
    RRTMG_HIP_CHECK(ctx, hipMemcpy(ph, d.phase, sizeof ph, hipMemcpyDeviceToHost));
    static const char *nm[8] = {"setup", "prep rows", "taumol", "planck+rows", "lookups+recurrence", "stores", "surface+up sweep", "-"};
    const double w = ph[8] ? (double)ph[8] : 1.0;
    fprintf(stderr, "lw phases (s_memtime ticks per wave-item, %llu waves, %d layers):", ph[8], L);
    for (int k = 0; k < 7; ++k) fprintf(stderr, " %s %.0f;", nm[k], ph[k] / w);
    fprintf(stderr, "\n  per layer of the downward sweep:");
    for (int k = 1; k <= 5; ++k) fprintf(stderr, " %s %.0f", nm[k], ph[k] / w / L);
    fprintf(stderr, "; up sweep per layer %.0f\n", ph[6] / w / L);
  }
#endif
  // the inner call of a sorted one stops here, enqueued: permuted_tail scatters behind it and runs the epilogue
  if (ctx->inner != kInnerNone) { RRTMG_HIP_CHECK(ctx, hipGetLastError()); return RRTMG_OK; }
  return call_finish(c, a->memspace, oc, nout, d.err);   // the requested band fluxes behind the same synchronise
}

// Both spectra of one host state (rrtmg_hip_radiation_fluxes): the argument checks of both before anything is enqueued, then
// the two drivers, each with its one body, under joint_run (rrtmg_call.h).
int radiation_fluxes_impl(rrtmg_ctx *ctx, const rrtmg_sw_args *sw, const rrtmg_sw_surface *sf, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b,
                          const rrtmg_lw_args *lw, const rrtmg_lw_band_fluxes *lb) {
  if (int rc = call_begin(ctx, 0, sw)) return rc;
  if (int rc = call_begin(ctx, 1, lw)) return rc;
  if (int rc = lw_refuse_clear_bands(ctx, lb)) return rc;
  return joint_run(ctx, [=]() { return sw_fluxes_impl(ctx, sw, sf, c, b); }, [=]() { return lw_fluxes_impl(ctx, lw, lb); });
}

// rrtmg_hip_lw_fluxes_f32 (rrtmg_precision.h; see sw_fluxes_f32_impl): host pointers run the ordinary driver with ctx->f32 set;
// device pointers get ONE widen launch for what the driver reads, the ordinary call on the fp64 copies, ONE narrow launch.
int lw_fluxes_f32_impl(rrtmg_ctx *ctx, const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *bp) {
  if (a->memspace != 1) {
    ctx->f32 = true;
    const int rc = lw_fluxes_impl(ctx, a, bp);
    ctx->f32 = false;
    return rc;
  }
  // (the sorted call has never checked the shard arguments: lw_sorted_call)
  if (int rc = call_is_sorted(ctx, 1, a, bp != nullptr) ? ctx_prepare_device(ctx) : call_begin(ctx, 1, a)) return rc;
  if (int rc = lw_refuse_clear_bands(ctx, bp)) return rc;
  const CallSite c{ctx, 1, call_stream(ctx, 1, 1)};
  BoundaryF32 bf(ctx, c.s, "lw.f32.");
  LwStructs b(a, bp);
  const unsigned on = lw_call_reads(a, bp, ctx->lw_clear_sky);
  const GridShape g = grid_shape(a->ncol, a->nlay, bp ? bp->levels : 0);
  boundary_inputs(bf, kLwIn, on, b, g);
  // (clear-sky outputs off: whatever the four point to is ignored -- absent from the narrow table, and from the inner call)
  boundary_outputs(bf, kLwOut, on, b, g);
  if (!bf.ok) return ctx->status;
  return boundary_f32_tail(c, bf, [&]() { return lw_fluxes_impl(ctx, &b, bp ? &b : nullptr); });
}

}  // namespace rrtmg
