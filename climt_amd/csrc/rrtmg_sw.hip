// rrtmg_sw.hip -- shortwave kernels and launch sequence (gfx950).
//
// Launch sequence of one rrtmg_hip_sw_fluxes call (all on the context's shortwave stream):
//   sw_aer_kernel       (iaer == 6)              ECMWF aerosol mixing per (column, layer)
//   kiss_mask_kernel / mask upload (McICA)       sub-column cloud mask
//   per column chunk (<= RRTMG_HIP_CHUNK_TILES tiles), so that a chunk's rows are still cached when its solve reads them:
//     sw_prep_fused_kernel <<<tiles, 16 waves>>>  inatm_sw + setcoef_sw per (column, layer), then the column part from the
//                         index words in LDS (laytrop, cloud flag, solar-source layer per band); non-McICA cloudy tiles: the
//                         band cloud optics
//     sw_cloud_kernel     (McICA)                 band cloud optics per (column, layer)
//     tile_lists_kernel   <<<1, 64>>>             the chunk's tiles by solve variant, compacted in tile order (SwDev::tlist)
//     sw_solve_all_kernel<false> (cloud-free tiles) + sw_solve_cloudy_kernel (cloudy tiles): wavefront = tile(64 columns) x work
//                         item (4|2 g-points of a band), workgroup = 16 | 8 tiles of one item sharing its tables in LDS;
//                         a workgroup's tiles are consecutive entries of ITS variant's list, so all of its wavefronts have
//                         work wherever cloud-free and cloudy tiles interleave (every fourth tile cloud-free: 6 of 8 and
//                         4 of 16 wavefronts otherwise, in workgroups that hold a whole CU either way)
//     sw_fluxheat_kernel  <<<(tiles, levels/15), 16 waves>>>  g-point sum per interface + heating rates
//   With components requested (rrtmg_hip_sw_fluxes_components): the solve variants sw_solve_all_dir_kernel<false> and
//   sw_solve_cloudy_dir_kernel instead, which also write the direct-beam partial planes, and sw_components_kernel
//   <<<(tiles, levels/4), 4 waves>>> behind sw_fluxheat_kernel: direct / diffuse, UV-visible / near-IR sums per interface
//   With band fluxes requested (rrtmg_hip_sw_fluxes_bands): sw_bandflux_kernel <<<(tiles, levels/4), 4 waves>>> (or the two
//   boundary levels only) behind them, and the *_dir solve variants where a direct-beam member is set
//   With the surface albedo by band (rrtmg_hip_sw_fluxes_surface): the same launches; the solve reads its two albedos from
//   the caller's [band][column] rows (SwDev::albdir / albdif) instead of the four broadband arrays
//   With the night-column skip on (rrtmg_hip_set_sw_night_skip): sw_kiss_mask_night_kernel, sw_prep_fused_night_kernel,
//   sw_cloud_night_kernel, sw_tile_lists_night_kernel and sw_{fluxheat,components,bandflux}_night_kernel in the places of their
//   namesakes; the solve kernels are the same and find a night tile in neither of their lists
//   A permuted call (rrtmg_permute.h) -- with the column sort on (rrtmg_hip_set_column_sort), or with the day-column pack on
//   (rrtmg_hip_set_sw_night_pack): then with the night kernels -- runs the sequence above on an internal copy, around it:
//   permute_class_kernel, permute_scan_kernel, permute_map_kernel, permute_gather_kernel (+ permute_gather_elem_kernel for
//   band-fastest cloud arrays) in front, permute_scatter_kernel behind
//   With the clear-sky outputs off (rrtmg_hip_set_sw_clear_sky(0)): sw_solve_cloudy_allsky_kernel in the place of
//   sw_solve_cloudy_kernel and sw_fluxheat_allsky_kernel<night> in the place of sw_fluxheat[_night]_kernel; swuflxc, swdflxc and
//   swhrc are neither formed nor copied
// The host steps this call shares with the longwave's (gate, checks, chunk plan and loop, mask choice, epilogue): rrtmg_call.h;
// the call's grid arrays -- what the driver, the permuted call and the float32 boundary register, gather and copy: the tables
// kSwIn / kSwOut of rrtmg_call_arrays.h
#include "rrtmg_call.h"
#include "rrtmg_sw_device.h"
#include "rrtmg_sw_host.h"
#include "rrtmg_solve_map.h"

namespace rrtmg {

// Preparation in ONE launch (round 1: three kernels): a workgroup = one 64-column tile, 16 wavefronts.  Phase 1: wave w prepares layers w, w+16, ...; phase 2, behind a barrier: wave b runs
// band b's column bookkeeping on the rows just written (L2-hot) and wave 0 sets the tile's cloud flag; phase 3, in cloudy
// tiles of a non-McICA call: the band cloud optics, again layers strided over the waves (with McICA, where most tiles are
// cloudy, the optics stay a launch of their own over (tile, layer): one workgroup per tile was measured 5 % slower on the
// whole McICA step).  Same per-thread functions, same results.
constexpr int kPrepWaves = 16;
__global__ void __launch_bounds__(64 * kPrepWaves) sw_prep_fused_kernel(SwDev d, SwTab T, int clouds, int tile0) {
  const int tile = tile0 + blockIdx.x;   // (launched per column chunk, right before the chunk's solve: its rows are still cached)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = tile * 64 + lane;
  const bool act = col < d.ncol;
  __shared__ int sh_cld;
  extern __shared__ int sh_idx[];    // the tile's packed index words [layer][lane] (dynamic LDS, nlay x 64 ints): the 14 band scans of phase 2 read them here
  if (act)
    for (int l = w; l < d.nlay; l += kPrepWaves) sh_idx[l * 64 + lane] = sw_prep_layer(d, T, col, l);
  __syncthreads();
  if (act)
    for (int b = w; b < kSwNBand; b += kPrepWaves) sw_prep_column(d, T, col, b, b + 1, sh_idx + lane, 64);
  if (w == 0) {
    const unsigned long long any = __ballot(act && d.anycld[col] != 0);
    if (lane == 0) { d.tile_cld[tile] = any != 0ull; sh_cld = any != 0ull; if (any) atomicAdd(d.ncloudy, 1); }
  }
  if (!clouds) return;
  __syncthreads();
  if (!sh_cld || !act) return;
  for (int l = w; l < d.nlay; l += kPrepWaves) sw_cloud_layer(d, T, col, l);
}

// The band cloud optics of the cloudy tiles (flag 1; 0 = cloud-free: the clear-sky solve variant never reads the optics).
// NIGHT: the flag may be 2, a night tile, which has none either.
template <bool NIGHT>
__device__ __forceinline__ void sw_cloud_body(const SwDev &d, const SwTab &T, int tile0) {
  const int tile = tile0 + blockIdx.x;
  if (NIGHT ? d.tile_cld[tile] != 1 : !d.tile_cld[tile]) return;
  const int col = tile * 64 + threadIdx.x;
  const int lay = blockIdx.y;
  if (col < d.ncol) sw_cloud_layer(d, T, col, lay);
}
__global__ void __launch_bounds__(64) sw_cloud_kernel(SwDev d, SwTab T, int tile0) { sw_cloud_body<false>(d, T, tile0); }

// ECMWF aerosol mixing (iaer = 6), rrtmg_sw_rad.nomcica.f90:693-727 -> per-band tau/ssa/asm
__global__ void __launch_bounds__(64) sw_aer_kernel(SwDev d, SwTab T, const double *ecaer, double *ta, double *om, double *as) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  const int lay = blockIdx.y;
  if (col >= d.ncol) return;
  const int L = d.nlay, N = d.ncol;
  const double *t = T.t;
  for (int ib = 0; ib < kSwNBand; ++ib) {
    double ztaua = 0.0, zasya = 0.0, zomga = 0.0;
    for (int ia = 0; ia < 6; ++ia) {
      const double e = ecaer[((long)ia * L + lay) * N + col];
      const double rt = t[T.rsrtaua + ib + kSwNBand * ia], rp = t[T.rsrpiza + ib + kSwNBand * ia], ra = t[T.rsrasya + ib + kSwNBand * ia];
      ztaua = ztaua + rt * e;
      zomga = zomga + rt * e * rp;
      zasya = zasya + rt * e * rp * ra;
    }
    if (ztaua == 0.0) {
      ztaua = 0.0; zasya = 0.0; zomga = 1.0;
    } else {
      if (zomga != 0.0) zasya = zasya / zomga;
      if (ztaua != 0.0) zomga = zomga / ztaua;
    }
    const long o = ((long)ib * L + lay) * N + col;
    ta[o] = ztaua; om[o] = zomga; as[o] = zasya;
  }
}

// All 112 g-points in ONE launch.  Wavefront = 64 columns of one tile x one work item (4 or 2 consecutive g-points
// of a band, SwTab::item): the thread carries the item's g-points through both sweeps, so the layer state, species
// mixtures and interpolation weights are evaluated once per item; the item's weighted fluxes are summed in
// registers: part[item][k][level][column].
// Workgroup = 16 wavefronts = the same item for 16 consecutive tiles (equal run times), one workgroup per CU,
// sharing in LDS (a) ONE copy of the 10001-entry transmittance table (80 KB): its lookups are per-lane random and
// cost a tag lookup per lane in the vector L1, but only bank conflicts in LDS; (b) the item's k-distribution slice,
// columns ig0..ig0+G-1 of the band's table slab, [nrows][G] (<= 58 KB): every absorption-coefficient row a lane
// needs is a 32-byte LDS read instead of a per-lane gather through the vector L1's 64 B/clk return path
// (measured: -6 % kernel time; with the rows through the scalar cache, an ablation, -10 % was the bound).
// Launch order: items heaviest first (SwTab::sched), tile groups fastest.  Speed only, never correctness.
constexpr int kSwWgWaves = 16;
constexpr int kSwGroupsPerBlock = 8;    // x 16 tiles = 128 tiles per block of the launch order
constexpr int kExpTblN = 10001;
// the item's slice of its band's table slab -> LDS: columns ig0 .. ig0+G-1, [nrows][G] (see SwBandTab)
__device__ __forceinline__ void sw_stage_slice(const SwTab &T, int item, double *sh_k, int nthreads) {
  const SwBandTab &B = T.b[item_band(item)];
  const int g = item_g(item);
  const double *src = T.t + B.slab + item_ig0(item);
  const int ng = B.ng, sh = g == 4 ? 2 : 1, n = B.nrows << sh;
  for (int i = threadIdx.x; i < n; i += nthreads) sh_k[i] = src[(long)(i >> sh) * ng + (i & (g - 1))];
}
// Two kernels are launched back to back: sw_solve_all_kernel<false> handles the cloud-free tiles with the cloud code compiled
// out (CLD = false: no spills, chunks of 4 g-points), sw_solve_cloudy_kernel the tiles flagged by the preparation kernel.
// The body of sw_solve_all_kernel and sw_solve_all_dir_kernel: make_sink(slot, col) -> the flux sink of the lane.
template <bool CLD, class MakeSink>
__device__ __forceinline__ void sw_solve_all_body(const SwDev &d, const SwTab &T, int tile0, MakeSink make_sink) {
  const int nmine = d.tcnt[CLD ? 1 : 0];   // this variant's tiles, compacted (SwDev::tlist)
  const SolveWork m = solve_map<kSwWgWaves, kSwGroupsPerBlock>(blockIdx.x, nmine, T.nitem);
  if (!m.work) return;   // workgroup-uniform exit before the tables are staged
  const int first = m.first, k = m.k;
  __shared__ double sh_exp[kExpTblN];
  for (int i = threadIdx.x; i < kExpTblN; i += 64 * kSwWgWaves) sh_exp[i] = T.t[T.exp_tbl + i];
  RRTMG_PROFILE_ONLY_ITEM(d, k)
  const int id = T.sched[k], item = T.item[id], slot = id;
  constexpr bool kLdsK = true;
  __shared__ __attribute__((aligned(16))) double sh_k[kSwSlabMaxRows * 4];   // rows are read 16 bytes at a time
  sw_stage_slice(T, item, sh_k, 64 * kSwWgWaves);
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (first + wave >= nmine) return;
  const int ctile = d.tlist[(CLD ? d.tcap : 0) + first + wave];   // tile within the chunk
  const int tile = tile0 + ctile;
  const int col = tile * 64 + (threadIdx.x & 63);
  if (col >= d.ncol) return;
  double *scr = d.scratch + ((long)ctile * kSwNGpt + item_iw0(item)) * (long)F_NTOT * d.nlay * 64 + (threadIdx.x & 63) * 2;
  auto sink = make_sink(slot, col);
  sw_solve_item<CLD, kLdsK>(d, T, sh_exp, item, col, scr, 64, sink, sh_k);
}
template <bool CLD>
__global__ void __launch_bounds__(64 * kSwWgWaves) __attribute__((amdgpu_waves_per_eu(4))) sw_solve_all_kernel(SwDev d, SwTab T, int tile0, int ntile) {   // tiles tile0 .. tile0 + ntile - 1 (one column chunk)
  sw_solve_all_body<CLD>(d, T, tile0, [&](int slot, int col) { return sw_part_sink(d, slot, col); });
}
// The components path (rrtmg_hip_sw_fluxes_components): the same, plus the direct-beam sums into partdir (SwPartDirSink).
template <bool CLD>
__global__ void __launch_bounds__(64 * kSwWgWaves) __attribute__((amdgpu_waves_per_eu(4))) sw_solve_all_dir_kernel(SwDev d, SwTab T, int tile0, int ntile, double *partdir) {
  sw_solve_all_body<CLD>(d, T, tile0, [&](int slot, int col) { return sw_part_dir_sink(d, partdir, slot, col); });
}


// The cloudy tiles (flagged by the preparation kernel): both sky streams per g-point.  They run the CLEAR kernel's item set
// -- chunks of 4 g-points, so the item-invariant work (layer state, species mixtures, weights, row indices) is paid once per
// 4 g-points, not per pair -- at 2 waves/SIMD: 238 VGPRs, no spills; 8-wave workgroups, one per CU, sharing the
// transmittance table and the chunk's slice in LDS.  Against the round-1 kernel (pairs, 170 VGPRs, 3 waves/SIMD, 12-wave
// workgroups): 1.91 -> 1.73 ms at 8192 columns.  The partial sums leave per chunk, the two pairs' sums added in the order the
// flux kernel added the pair slots of the round-1 kernel: bit-identical, half the partial-plane traffic.
constexpr int kC4Waves = 8;
constexpr int kC4GroupsPerBlock = 16;   // x 8 tiles = 128 tiles per block of the launch order
// (sw_solve_cloudy_body below is a copy of this kernel's body for sw_solve_cloudy_dir_kernel, and sw_solve_cloudy_allsky_kernel
//  carries another with its own workgroup shape: a change to the staging or the addressing here is made there too --
//  tests/test_sw_components.py and tests/test_allsky_only.py check that the bodies agree)
__global__ void __launch_bounds__(64 * kC4Waves) __attribute__((amdgpu_waves_per_eu(2, 2))) sw_solve_cloudy_kernel(SwDev d, SwTab T, int tile0, int ntile) {
  const int nmine = d.tcnt[1];   // the cloudy tiles, compacted (SwDev::tlist)
  const SolveWork m = solve_map<kC4Waves, kC4GroupsPerBlock>(blockIdx.x, nmine, T.nitem);
  if (!m.work) return;
  const int first = m.first, k = m.k;
  RRTMG_PROFILE_ONLY_ITEM(d, k)
  const int id = T.sched[k], item = T.item[id], slot = id;      // one slot per chunk
  __shared__ __attribute__((aligned(16))) double sh_k[kSwSlabMaxRows * 4];
  sw_stage_slice(T, item, sh_k, 64 * kC4Waves);
  __shared__ double sh_exp[kExpTblN];
  for (int i = threadIdx.x; i < kExpTblN; i += 64 * kC4Waves) sh_exp[i] = T.t[T.exp_tbl + i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (first + wave >= nmine) return;
  const int ctile = d.tlist[d.tcap + first + wave], tile = tile0 + ctile;
  const int lane = threadIdx.x & 63;
  const int col = tile * 64 + lane;
  if (col >= d.ncol) return;
  double *scr = d.scratch + ((long)ctile * kSwNGpt + item_iw0(item)) * (long)F_NTOT * d.nlay * 64 + lane * 2;
  SwPartSink sink = sw_part_sink(d, slot, col);
  sw_solve_item<true, true>(d, T, sh_exp, item, col, scr, 64, sink, sh_k);
}
// The body of sw_solve_cloudy_dir_kernel: sw_solve_cloudy_kernel's with the sink made by make_sink (see sw_solve_all_body).
// (sw_solve_cloudy_kernel keeps its own copy: routed through this template it comes out with the same number of instructions
// in another order and on other registers -- rung C of the acceptance ladder, docs/EXPERIMENTS.md -- and its ISA is what the
// profiles and resource figures refer to.)
template <class MakeSink>
__device__ __forceinline__ void sw_solve_cloudy_body(const SwDev &d, const SwTab &T, int tile0, MakeSink make_sink) {
  const int nmine = d.tcnt[1];   // the cloudy tiles, compacted (SwDev::tlist)
  const SolveWork m = solve_map<kC4Waves, kC4GroupsPerBlock>(blockIdx.x, nmine, T.nitem);
  if (!m.work) return;
  const int first = m.first, k = m.k;
  RRTMG_PROFILE_ONLY_ITEM(d, k)
  const int id = T.sched[k], item = T.item[id], slot = id;      // one slot per chunk
  __shared__ __attribute__((aligned(16))) double sh_k[kSwSlabMaxRows * 4];
  sw_stage_slice(T, item, sh_k, 64 * kC4Waves);
  __shared__ double sh_exp[kExpTblN];
  for (int i = threadIdx.x; i < kExpTblN; i += 64 * kC4Waves) sh_exp[i] = T.t[T.exp_tbl + i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (first + wave >= nmine) return;
  const int ctile = d.tlist[d.tcap + first + wave], tile = tile0 + ctile;
  const int lane = threadIdx.x & 63;
  const int col = tile * 64 + lane;
  if (col >= d.ncol) return;
  double *scr = d.scratch + ((long)ctile * kSwNGpt + item_iw0(item)) * (long)F_NTOT * d.nlay * 64 + lane * 2;
  auto sink = make_sink(slot, col);
  sw_solve_item<true, true>(d, T, sh_exp, item, col, scr, 64, sink, sh_k);
}
__global__ void __launch_bounds__(64 * kC4Waves) __attribute__((amdgpu_waves_per_eu(2, 2))) sw_solve_cloudy_dir_kernel(SwDev d, SwTab T, int tile0, int ntile, double *partdir) {
  sw_solve_cloudy_body(d, T, tile0, [&](int slot, int col) { return sw_part_dir_sink(d, partdir, slot, col); });
}

// Spectral integration AND heating rates in one launch: a workgroup = one tile x kFluxLev layers; wave j sums the partial
// planes of interface level l0 + j (the extra wave kFluxLev: the halo level on top, recomputed by the next workgroup, which
// owns and stores it), the net fluxes meet in LDS, waves j < kFluxLev form the layer's heating rates from levels j and j + 1
// -- the same differences of the same doubles as sw_heat_layer reads back from memory.
constexpr int kFluxLev = 15;   // 16 waves per workgroup: the halo level is 1 in 16 of the partial-plane reads
__global__ void __launch_bounds__(64 * (kFluxLev + 1)) sw_fluxheat_kernel(SwDev d, SwTab T, int tile0) {
  // (the call's last launch leaves the preparation kernels' cloudy-tile count where the host will look for it, and clears it)
  if (d.hint_out && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) { *d.hint_out = *d.ncloudy; *d.ncloudy = 0; }
  const int tile = tile0 + blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int col = tile * 64 + lane, lev = blockIdx.y * kFluxLev + j;
  __shared__ double net[kFluxLev + 1][64], netc[kFluxLev + 1][64];
  const bool act = col < d.ncol && lev <= d.nlay;
  if (act) {
    double fu, fd, cu, cd;
    sw_flux_sums(d, T, col, lev, d.tile_cld[tile] != 0, fu, fd, cu, cd);
    if (j < kFluxLev || lev == d.nlay) {
      const long o = (long)lev * d.ncol + col;
      d.swuflx[o] = fu; d.swdflx[o] = fd; d.swuflxc[o] = cu; d.swdflxc[o] = cd;
    }
    net[j][lane] = fd - fu; netc[j][lane] = cd - cu;
  }
  __syncthreads();
  if (col < d.ncol && j < kFluxLev && lev < d.nlay) {
    const long o0 = (long)lev * d.ncol + col;
    const double zdpgcp = T.heatfac / d.pdp[o0];
    d.swhrc[o0] = (netc[j + 1][lane] - netc[j][lane]) * zdpgcp;
    d.swhr[o0] = (net[j + 1][lane] - net[j][lane]) * zdpgcp;
  }
}

// Components (rrtmg_hip_sw_fluxes_components), launched per column chunk behind sw_fluxheat_kernel (part and partdir are per
// chunk): one thread per (column, interface level), the g-point sums of sw_components_level.  It reads the fd / cd partial
// planes once more after sw_fluxheat_kernel has (~4 GB at 131 072 x 60, most of the components' +6 % on the call): folding
// the components into sw_fluxheat_kernel's pass is where that cost would be recovered.
constexpr int kCompLev = 4;
__global__ void __launch_bounds__(64 * kCompLev) sw_components_kernel(SwDev d, SwTab T, int tile0, const double *partdir, SwCompOut o) {
  const int tile = tile0 + blockIdx.x, col = tile * 64 + (threadIdx.x & 63), lev = blockIdx.y * kCompLev + (threadIdx.x >> 6);
  if (col >= d.ncol || lev > d.nlay) return;
  sw_components_level(d, T, partdir, o, col, lev, d.tile_cld[tile] != 0);
}

// Band fluxes (rrtmg_hip_sw_fluxes_bands), launched per column chunk behind sw_fluxheat_kernel (and sw_components_kernel):
// one thread per (column, level), lane = column, the per-band sums of sw_band_level.  levels = 0: every interface level, row
// = level; 1: a workgroup of two waves, row 0 = surface, row 1 = top.  A streaming kernel: it reads the requested partial
// planes once more (see sw_components_kernel) and writes 14 rows per member.  NIGHT: +0.0 for a night column.
constexpr int kBandLev = 4;
template <bool NIGHT>
__device__ __forceinline__ void sw_bandflux_body(const SwDev &d, const SwTab &T, int tile0, const double *partdir, const SwBandOut &o, int levels) {
  const int tile = tile0 + blockIdx.x, col = tile * 64 + (threadIdx.x & 63), row = blockIdx.y * kBandLev + (threadIdx.x >> 6);
  const int lev = levels ? (row ? d.nlay : 0) : row;
  if (col >= d.ncol || row > (levels ? 1 : d.nlay)) return;
  const int nrow = levels ? 2 : d.nlay + 1;
  if (NIGHT && d.coszen[col] <= 0.0) {
    double *const m[6] = {o.up, o.dn, o.upc, o.dnc, o.dndir, o.dndirc};
    for (int band = 0; band < kSwNBand; ++band) {
      const long i = ((long)band * nrow + row) * d.ncol + col;
      for (int k = 0; k < 6; ++k)
        if (m[k]) m[k][i] = 0.0;
    }
    return;
  }
  sw_band_level(d, T, partdir, o, col, lev, row, nrow, d.tile_cld[tile] != 0);
}
__global__ void __launch_bounds__(64 * kBandLev) sw_bandflux_kernel(SwDev d, SwTab T, int tile0, const double *partdir, SwBandOut o, int levels) {
  sw_bandflux_body<false>(d, T, tile0, partdir, o, levels);
}

// ---- Night-column skip (rrtmg_hip_set_sw_night_skip; opt-in) -----------------------------------------------------------------
// Kernels of their own, launched INSTEAD of their namesakes when the option is on: with it off the launch sequence and every
// kernel in it are those of a library without the option (tools/isa_compare.py, profiles/isa_compare_night_skip.txt).
// A night column has coszen <= 0 as the caller passed it (SwDev::coszen, before the clamp of sw_prep_column; NaN compares
// false: day).  A night TILE -- every in-range column night -- gets SwDev::tile_cld = 2, a value that lands in neither list of
// sw_tile_lists_night_kernel: no solve workgroup has work for it, and nothing else of the preparation runs, so its prep rows,
// pdp, cloud optics, mask words and partial planes are never written NOR read.  The integration kernels decide per COLUMN from
// coszen alone (in a night tile every column takes that path): zeros for a night column, the default kernels' arithmetic for a
// day column.  Night columns of a mixed tile are prepared and solved in lockstep with their day neighbours, then zeroed.
// night_cnt: [night tiles, night columns] of the call so far (device; the call's last integration launch publishes and clears it)
constexpr int kTileNight = 2;
__global__ void __launch_bounds__(64 * kPrepWaves) sw_prep_fused_night_kernel(SwDev d, SwTab T, int clouds, int tile0, int32_t *night_cnt) {
  const int tile = tile0 + blockIdx.x, lane = threadIdx.x & 63, col = tile * 64 + lane;
  const bool act = col < d.ncol, dark = act && d.coszen[col] <= 0.0;
  // (each of the 16 wavefronts looks at the tile's 64 columns: the same two masks in all of them, the exit is workgroup-uniform)
  const unsigned long long mday = __ballot(act && !dark), mdark = __ballot(dark);
  if (threadIdx.x == 0 && mdark) atomicAdd(night_cnt + 1, __popcll(mdark));
  if (mday == 0ull) {
    if (threadIdx.x == 0) { d.tile_cld[tile] = kTileNight; atomicAdd(night_cnt, 1); }
    return;
  }
  // From here sw_prep_fused_kernel's body, a copy: that kernel routed through a shared body came out with other instructions
  // (rung C of the acceptance ladder, docs/EXPERIMENTS.md), and its ISA is to stay the one of a library without the option -- a
  // change to it is made here too (tests/test_night_skip.py checks that the two agree).
  const int w = threadIdx.x >> 6;
  __shared__ int sh_cld;
  extern __shared__ int sh_idx[];
  if (act)
    for (int l = w; l < d.nlay; l += kPrepWaves) sh_idx[l * 64 + lane] = sw_prep_layer(d, T, col, l);
  __syncthreads();
  if (act)
    for (int b = w; b < kSwNBand; b += kPrepWaves) sw_prep_column(d, T, col, b, b + 1, sh_idx + lane, 64);
  if (w == 0) {
    const unsigned long long any = __ballot(act && d.anycld[col] != 0);
    if (lane == 0) { d.tile_cld[tile] = any != 0ull; sh_cld = any != 0ull; if (any) atomicAdd(d.ncloudy, 1); }
  }
  if (!clouds) return;
  __syncthreads();
  if (!sh_cld || !act) return;
  for (int l = w; l < d.nlay; l += kPrepWaves) sw_cloud_layer(d, T, col, l);
}
__global__ void __launch_bounds__(64) sw_cloud_night_kernel(SwDev d, SwTab T, int tile0) { sw_cloud_body<true>(d, T, tile0); }
// tile_lists_kernel with a third flag value that lands in neither list (the longwave never produces it: its list kernel stays as it is)
__global__ void __launch_bounds__(64) sw_tile_lists_night_kernel(const int32_t *tile_cld, int ntile, int32_t *list, int32_t *cnt, int cap) {
  const int lane = threadIdx.x;
  if (ntile > cap) ntile = cap;
  int n0 = 0, n1 = 0;
  for (int t0 = 0; t0 < ntile; t0 += 64) {
    const int t = t0 + lane;
    const int flag = t < ntile ? tile_cld[t] : kTileNight;
    const unsigned long long m1 = __ballot(flag == 1), m0 = __ballot(flag == 0);
    const unsigned long long lower = (1ull << lane) - 1ull;
    if (flag == 1) list[cap + n1 + __popcll(m1 & lower)] = t;
    else if (flag == 0) list[n0 + __popcll(m0 & lower)] = t;
    n0 += __popcll(m0); n1 += __popcll(m1);
  }
  if (lane == 0) { cnt[0] = n0; cnt[1] = n1; }
}
// kiss_mask_kernel (a block = the 64 columns of a tile x one sub-column) that draws nothing for a night tile
__global__ void __launch_bounds__(64) sw_kiss_mask_night_kernel(int ncol, int nlay, int icld, const double *play, const double *cldfr, uint64_t *mask,
                                                                int nw, int *err, const uint32_t *jumps, const double *coszen) {
  const int col = blockIdx.y * 64 + threadIdx.x;
  const bool act = col < ncol;
  if (__ballot(act && !(coszen[col] <= 0.0)) == 0ull) return;
  if (act) kiss_mask_jump(ncol, nlay, icld, play, cldfr, mask, nw, err, jumps, col, blockIdx.x);
}
// ... and kiss_mask_exp_kernel's (exponential overlap, icld 4 and 5)
__global__ void __launch_bounds__(64) sw_kiss_mask_exp_night_kernel(int ncol, int nlay, int icld, const double *play, const double *cldfr, const double *alpha,
                                                                    uint64_t *mask, int nw, int *err, const uint32_t *jumps, const double *coszen) {
  const int col = blockIdx.y * 64 + threadIdx.x;
  const bool act = col < ncol;
  if (__ballot(act && !(coszen[col] <= 0.0)) == 0ull) return;
  if (act) kiss_mask_jump_exp(ncol, nlay, icld, play, cldfr, alpha, mask, nw, err, jumps, col, blockIdx.x);
}
// sw_fluxheat_kernel: a day column's sums, differences and stores are those of that kernel; a night column stores +0.0 and
// reads neither the partial planes nor pdp.  (A text of its own, like sw_components_night_kernel's and
// sw_fluxheat_allsky_kernel's: over one body<NIGHT, CLEAR> all of them, sw_fluxheat_kernel included, came out with their
// instructions in another order -- docs/EXPERIMENTS.md V)
__global__ void __launch_bounds__(64 * (kFluxLev + 1)) sw_fluxheat_night_kernel(SwDev d, SwTab T, int tile0, int32_t *night_cnt, int32_t *night_out) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    if (d.hint_out) { *d.hint_out = *d.ncloudy; *d.ncloudy = 0; }
    // (night_out: page-locked, set in the call's last launch like hint_out -- every preparation kernel of the call has finished)
    if (night_out) { night_out[0] = night_cnt[0]; night_out[1] = night_cnt[1]; night_cnt[0] = 0; night_cnt[1] = 0; }
  }
  const int tile = tile0 + blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int col = tile * 64 + lane, lev = blockIdx.y * kFluxLev + j;
  __shared__ double net[kFluxLev + 1][64], netc[kFluxLev + 1][64];
  const bool in = col < d.ncol && lev <= d.nlay;
  const bool dark = col < d.ncol && d.coszen[col] <= 0.0;
  if (in && !dark) {
    double fu, fd, cu, cd;
    sw_flux_sums(d, T, col, lev, d.tile_cld[tile] != 0, fu, fd, cu, cd);
    if (j < kFluxLev || lev == d.nlay) {
      const long o = (long)lev * d.ncol + col;
      d.swuflx[o] = fu; d.swdflx[o] = fd; d.swuflxc[o] = cu; d.swdflxc[o] = cd;
    }
    net[j][lane] = fd - fu; netc[j][lane] = cd - cu;
  } else if (in && (j < kFluxLev || lev == d.nlay)) {
    const long o = (long)lev * d.ncol + col;
    d.swuflx[o] = 0.0; d.swdflx[o] = 0.0; d.swuflxc[o] = 0.0; d.swdflxc[o] = 0.0;
  }
  __syncthreads();
  if (col < d.ncol && j < kFluxLev && lev < d.nlay) {
    const long o0 = (long)lev * d.ncol + col;
    if (dark) {
      d.swhrc[o0] = 0.0; d.swhr[o0] = 0.0;
    } else {
      const double zdpgcp = T.heatfac / d.pdp[o0];
      d.swhrc[o0] = (netc[j + 1][lane] - netc[j][lane]) * zdpgcp;
      d.swhr[o0] = (net[j + 1][lane] - net[j][lane]) * zdpgcp;
    }
  }
}
__global__ void __launch_bounds__(64 * kCompLev) sw_components_night_kernel(SwDev d, SwTab T, int tile0, const double *partdir, SwCompOut o) {
  const int tile = tile0 + blockIdx.x, col = tile * 64 + (threadIdx.x & 63), lev = blockIdx.y * kCompLev + (threadIdx.x >> 6);
  if (col >= d.ncol || lev > d.nlay) return;
  if (d.coszen[col] <= 0.0) {
    const long i = (long)lev * d.ncol + col;
    double *const m[8] = {o.dirdflx, o.difdflx, o.dirdnuv, o.difdnuv, o.dirdnir, o.difdnir, o.dirdflxc, o.difdflxc};
    for (int k = 0; k < 8; ++k)
      if (m[k]) m[k][i] = 0.0;
    return;
  }
  sw_components_level(d, T, partdir, o, col, lev, d.tile_cld[tile] != 0);
}
__global__ void __launch_bounds__(64 * kBandLev) sw_bandflux_night_kernel(SwDev d, SwTab T, int tile0, const double *partdir, SwBandOut o, int levels) {
  sw_bandflux_body<true>(d, T, tile0, partdir, o, levels);
}

// ---- No clear-sky outputs (rrtmg_hip_set_sw_clear_sky(0); opt-in) ----------------------------------------------------------------
// Kernels of their own, launched INSTEAD of sw_solve_cloudy_kernel and sw_fluxheat[_night]_kernel when the clear-sky outputs are
// off: with them on the launch sequence and every kernel in it are those of a library without the option (tools/isa_compare.py,
// profiles/isa_compare_allsky_only.txt).  The cloudy tiles run sw_solve_thread's ONE mode: the total-sky stream alone, two partial
// planes per slot like a cloud-free tile, the F_RUP / F_RUPD rows of the scratch slab.  Cloud-free tiles run sw_solve_all_kernel<false>
// as ever.  Tile list, launch order and LDS staging: sw_solve_cloudy_kernel's.  Workgroup shape: kAsWaves wavefronts at kAsWaves / 4 per
// SIMD (RRTMG_ALLSKY_WAVES, 8, 12 or 16: DESIGN.md 5 has them measured).
#ifndef RRTMG_ALLSKY_WAVES
#define RRTMG_ALLSKY_WAVES 8
#endif
constexpr int kAsWaves = RRTMG_ALLSKY_WAVES;
constexpr int kAsGroupsPerBlock = (128 + kAsWaves - 1) / kAsWaves;   // 128 tiles per block of the launch order (12 waves: 132)
static_assert(kAsWaves == 8 || kAsWaves == 12 || kAsWaves == 16, "RRTMG_ALLSKY_WAVES: 8 (2 waves per SIMD), 12 (3) or 16 (4)");
__global__ void __launch_bounds__(64 * kAsWaves) __attribute__((amdgpu_waves_per_eu(kAsWaves / 4, kAsWaves / 4))) sw_solve_cloudy_allsky_kernel(SwDev d, SwTab T, int tile0, int ntile) {
  const int nmine = d.tcnt[1];   // the cloudy tiles, compacted (SwDev::tlist)
  const SolveWork m = solve_map<kAsWaves, kAsGroupsPerBlock>(blockIdx.x, nmine, T.nitem);
  if (!m.work) return;
  const int first = m.first, k = m.k;
  RRTMG_PROFILE_ONLY_ITEM(d, k)
  const int id = T.sched[k], item = T.item[id], slot = id;      // one slot per chunk
  __shared__ __attribute__((aligned(16))) double sh_k[kSwSlabMaxRows * 4];
  sw_stage_slice(T, item, sh_k, 64 * kAsWaves);
  __shared__ double sh_exp[kExpTblN];
  for (int i = threadIdx.x; i < kExpTblN; i += 64 * kAsWaves) sh_exp[i] = T.t[T.exp_tbl + i];
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (first + wave >= nmine) return;
  const int ctile = d.tlist[d.tcap + first + wave], tile = tile0 + ctile;
  const int lane = threadIdx.x & 63;
  const int col = tile * 64 + lane;
  if (col >= d.ncol) return;
  double *scr = d.scratch + ((long)ctile * kSwNGpt + item_iw0(item)) * (long)F_NTOT * d.nlay * 64 + lane * 2;
  SwPartSink sink = sw_part_sink(d, slot, col);
  sw_solve_item<true, true, true>(d, T, sh_exp, item, col, scr, 64, sink, sh_k);
}
// sw_fluxheat_kernel without the clear-sky half: two planes per slot in EVERY tile (sw_flux_sums with cld = false), the sums,
// differences and stores of swuflx, swdflx and swhr as there.  NIGHT: sw_fluxheat_night_kernel's column rule and counts.
template <bool NIGHT>
__global__ void __launch_bounds__(64 * (kFluxLev + 1)) sw_fluxheat_allsky_kernel(SwDev d, SwTab T, int tile0, int32_t *night_cnt, int32_t *night_out) {
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    if (d.hint_out) { *d.hint_out = *d.ncloudy; *d.ncloudy = 0; }
    if (NIGHT && night_out) { night_out[0] = night_cnt[0]; night_out[1] = night_cnt[1]; night_cnt[0] = 0; night_cnt[1] = 0; }
  }
  const int tile = tile0 + blockIdx.x, lane = threadIdx.x & 63, j = threadIdx.x >> 6;
  const int col = tile * 64 + lane, lev = blockIdx.y * kFluxLev + j;
  __shared__ double net[kFluxLev + 1][64];
  const bool in = col < d.ncol && lev <= d.nlay;
  const bool dark = NIGHT && col < d.ncol && d.coszen[col] <= 0.0;
  if (in && !dark) {
    double fu, fd, cu, cd;
    sw_flux_sums(d, T, col, lev, false, fu, fd, cu, cd);
    if (j < kFluxLev || lev == d.nlay) {
      const long o = (long)lev * d.ncol + col;
      d.swuflx[o] = fu; d.swdflx[o] = fd;
    }
    net[j][lane] = fd - fu;
  } else if (in && (j < kFluxLev || lev == d.nlay)) {
    const long o = (long)lev * d.ncol + col;
    d.swuflx[o] = 0.0; d.swdflx[o] = 0.0;
  }
  __syncthreads();
  if (col < d.ncol && j < kFluxLev && lev < d.nlay) {
    const long o0 = (long)lev * d.ncol + col;
    if (dark) d.swhr[o0] = 0.0;
    else d.swhr[o0] = (net[j + 1][lane] - net[j][lane]) * (T.heatfac / d.pdp[o0]);
  }
}

void free_sw_desc(rrtmg_ctx *ctx) {
  delete (SwTab *)ctx->sw_desc;
  ctx->sw_desc = nullptr;
}

// stand-alone sub-column generator (host pointers): the mask is built on the device by either generator
int mcica_mask_impl(rrtmg_ctx *ctx, int which, int ncol, int nlay, int icld, int permuteseed, int irng,
                    const double *play, const double *cldfrac, double *cldfmcl) {
  if (ncol <= 0 || nlay <= 0 || !play || !cldfrac || !cldfmcl) return ctx->fail(RRTMG_ERR_ARG, "mcica_mask: bad argument");
  // (icld 4 and 5 -- exponential overlap -- exist while rank correlations are set for the spectrum: rrtmg_hip_set_mcica_overlap_alpha)
  const int w = which == 0 ? 0 : 1;
  const bool expo = (icld == 4 || icld == 5) && ctx->alpha[w].dev;
  if ((icld < 0 || icld > 3) && !expo) return ctx->fail(RRTMG_ERR_ICLD, "%s", status_message(RRTMG_ERR_ICLD));
  if (expo && (ctx->alpha[w].ncol != ncol || ctx->alpha[w].nlay != nlay))
    return ctx->fail(RRTMG_ERR_ARG, "mcica_mask: the rank correlations were set for %d x %d columns x layers, the call has %d x %d", ctx->alpha[w].ncol, ctx->alpha[w].nlay, ncol, nlay);
  const int nsub = which == 0 ? kSwNGpt : 140;
  const int nw = (nlay + 63) / 64;
  const size_t nl = (size_t)ncol * nlay;
  if (icld == 0) return RRTMG_OK;   // mcica_subcol_*: "if (icld.eq.0) return" -- outputs untouched
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  double *dp = (double *)ctx->buf("mm.play", nl * 8), *dc = (double *)ctx->buf("mm.cld", nl * 8);
  double *dm = (double *)ctx->buf("mm.out", nl * nsub * 8);
  uint64_t *mk = (uint64_t *)ctx->buf("mm.mask", (size_t)nsub * nw * ncol * 8);
  if (!dp || !dc || !dm || !mk) return ctx->status;
  RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(dp, play, nl * 8, hipMemcpyHostToDevice, s));
  RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(dc, cldfrac, nl * 8, hipMemcpyHostToDevice, s));
  RRTMG_HIP_CHECK(ctx, hipMemsetAsync(ctx->err_dev, 0, sizeof(int), s));
  const int ntile = (ncol + 63) / 64;
  const double *alpha = expo ? ctx->alpha[w].dev : nullptr;
  if (expo) RRTMG_HIP_CHECK(ctx, hipStreamWaitEvent(s, ctx->alpha_ev[w], 0));   // (a copy from device memory may be on the longwave's stream)
  if (irng != 0) {
    rc = mt_mask_device(ctx, w, ncol, nlay, nsub, icld, permuteseed, dc, mk, nw, 0, 0, s, alpha);
    if (rc) return rc;
  } else {
    const uint32_t *jumps = kiss_jumps_device(ctx, w, nsub, nlay, icld, permuteseed, s);
    if (!jumps) return ctx->status;
    if (expo) hipLaunchKernelGGL(kiss_mask_exp_kernel, dim3(nsub, ntile), dim3(64), 0, s, ncol, nlay, icld, dp, dc, alpha, mk, nw, ctx->err_dev, jumps);
    else hipLaunchKernelGGL(kiss_mask_kernel, dim3(nsub, ntile), dim3(64), 0, s, ncol, nlay, icld, dp, dc, mk, nw, ctx->err_dev, jumps);
  }
  hipLaunchKernelGGL(cldfmcl_from_mask_kernel, dim3(ntile, nsub), dim3(64), 0, s, ncol, nlay, nsub, mk, nw, dm);
  int herr = 0;
  RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(&herr, ctx->err_dev, sizeof(int), hipMemcpyDeviceToHost, s));
  RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(cldfmcl, dm, nl * nsub * 8, hipMemcpyDeviceToHost, s));
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  if (herr) return ctx->fail(herr, "mcica_mask: %s", status_message(herr));
  return RRTMG_OK;
}

int sw_init_impl(rrtmg_ctx *ctx, double cpdair, const char *blob_path) {
  if (!ctx->have_constants) return ctx->fail(RRTMG_ERR_NOT_INITIALISED, "set_constants must be called before sw_init");
  std::string path = blob_path ? std::string(blob_path) : default_blob_path("sw");
  Blob blob;
  std::string err;
  if (!blob.load(path, err)) return ctx->fail(RRTMG_ERR_TABLES, "%s", err.c_str());
  ctx->sw_ts = TableSet();
  if (!build_tables(blob, "sw", cpdair, ctx->k.grav, ctx->k.secdy, ctx->sw_ts, err)) return ctx->fail(RRTMG_ERR_TABLES, "%s", err.c_str());
  SwTab *T = ctx->sw_desc ? (SwTab *)ctx->sw_desc : new SwTab();
  ctx->sw_desc = T;
  if (!build_sw_tab(ctx->sw_ts, *T, err)) return ctx->fail(RRTMG_ERR_TABLES, "%s", err.c_str());
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  if (ctx->sw_tab_dev) (void)hipFree(ctx->sw_tab_dev);
  ctx->sw_tab_dev = nullptr;
  RRTMG_HIP_CHECK(ctx, hipMalloc((void **)&ctx->sw_tab_dev, ctx->sw_ts.flat.size() * sizeof(double)));
  RRTMG_HIP_CHECK(ctx, hipMemcpy(ctx->sw_tab_dev, ctx->sw_ts.flat.data(), ctx->sw_ts.flat.size() * sizeof(double), hipMemcpyHostToDevice));
  T->t = ctx->sw_tab_dev;
  ctx->sw_ready = true;
  return RRTMG_OK;
}

// cp: the components requested (at least one member set), or nullptr; bp: the band fluxes requested (at least one member
// set, levels 0 or 1), or nullptr; sp: the surface albedo by band (at least one member set), or nullptr; all nullptr: the
// plain call.  A call with components or bands is never sorted: its outputs would need a scatter of their own; nor is one with
// a surface struct: its rows would need a gather of their own; nor is a call with the night-column skip on: the sort would move
// night columns out of their tiles; nor is a call whose facular/sunspot amplitudes `indsolvar` differ from 1: the host rescales
// them once per column IN THE CALLER'S ORDER (sw_scalar_setup), so the multipliers are positional like the Mersenne twister's
// stream, and the inner call on the padded copy would hand each column another column's multipliers and rescale the caller's
// IN/OUT array once per padded slot.
static bool sw_amplitudes_differ_from_one(const rrtmg_sw_args *a) { return a && a->indsolvar && (a->indsolvar[0] != 1.0 || a->indsolvar[1] != 1.0); }
// The call runs packed (rrtmg_permute.h): opt-in, device pointers, at least two tiles, kissvec or no McICA, amplitudes indsolvar
// equal to 1 (the twister's stream and the rescaled amplitudes are positional), not half of a joint call and not an inner
// call itself.  Any other call with the option on runs as with the night-column skip on.
static bool sw_call_is_packed(const rrtmg_ctx *ctx, const rrtmg_sw_args *a) {
  return ctx->sw_night_pack && ctx->inner == kInnerNone && !ctx->joint && ctx->sw_ready && a && a->memspace == 1 && a->coszen && a->ncol > 64 &&
         a->nlay > 0 && a->nlay <= 256 && !(a->mcica && a->irng != 0) && !sw_amplitudes_differ_from_one(a);
}
// The permuted call, kind = sorted | packed: the column map from cldfr | coszen, ONE gather launch for the [rows][N] inputs (one
// more for the band-fastest cloud arrays where they are given), the ordinary driver on the copy of Np slots (packed: with the
// night kernels), ONE scatter launch for every requested output (packed: it also leaves the counts of
// rrtmg_hip_sw_night_last), then the epilogue the inner call left out.  Components, bands and the surface struct ride along
// where the gate lets them through (the sort's never does): their rows are entries of the same two tables.
static int sw_permuted_call(rrtmg_ctx *ctx, InnerCall kind, const rrtmg_sw_args *a, const rrtmg_sw_surface *sp, const rrtmg_sw_components *cp, const rrtmg_sw_band_fluxes *bp) {
  const bool packed = kind == kInnerPacked;
  // (the sorted call has never checked the shard arguments: its inner call, kissvec or no McICA, does not read them)
  if (int rc = packed ? call_begin(ctx, 0, a) : ctx_prepare_device(ctx)) return rc;
  const CallSite c{ctx, 0, call_stream(ctx, 0, 1)};
  // (clear-sky outputs off: the three are absent from the scatter table, and from the inner call)
  SwStructs b(a, sp, cp, bp);
  const unsigned on = sw_call_reads(a, sp, cp, bp, ctx->sw_clear_sky);
  if (int rc = check_outputs(ctx, kSwOut, on, b)) return rc;
  ColumnPermute pm(ctx, c.s, kind, a->ncol, a->nlay, packed ? "sw.pack." : "sw.sort.");
  if (!pm.prepare(packed ? a->coszen : a->cldfr)) return ctx->status;
  b.ncol = pm.Np; b.shard_col0 = 0; b.shard_ncol = 0;
  const GridShape g = grid_shape(a->ncol, a->nlay, bp ? bp->levels : 0);
  permute_inputs(pm, kSwIn, on, b, g);
  // exponential overlap: the rank correlations are one more [nlay][N] input of the mask step
  if (call_overlap_exp(ctx, 0, a) && !a->cldfmcl) ctx->alpha_inner[0] = pm.gather("alpha", ctx->alpha[0].dev, g.L);
  if (!pm.ok) { ctx->alpha_inner[0] = nullptr; return ctx->status; }
  pm.flush_gather();
  permute_outputs(pm, kSwOut, on, b, g);   // registered for the scatter in the order plain, components, bands
  if (!pm.ok) { ctx->alpha_inner[0] = nullptr; return ctx->status; }
  return permuted_tail(c, pm, [&]() {
    const int rc = sw_fluxes_impl(ctx, &b, sp ? &b : nullptr, cp ? &b : nullptr, bp ? &b : nullptr);
    if (!rc && packed) ctx->sw_pack_reported = true;
    return rc;
  }, packed ? (int32_t *)ctx->night_host() : nullptr);
}

int sw_fluxes_impl(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *sp, const rrtmg_sw_components *cp, const rrtmg_sw_band_fluxes *bp) {
  const bool clr = ctx->sw_clear_sky;   // rrtmg_hip_set_sw_clear_sky: false = swuflxc, swdflxc and swhrc are neither formed nor read from `a`
  if (!clr && (cp || bp)) return ctx->fail(RRTMG_ERR_ARG, "shortwave flux components and band fluxes need the clear-sky stream: rrtmg_hip_set_sw_clear_sky(ctx, 0) is in force (set it to 1 for this call)");
  if (int orc = call_overlap_check(ctx, 0, a)) return orc;
  if (sw_call_is_packed(ctx, a)) return sw_permuted_call(ctx, kInnerPacked, a, sp, cp, bp);
  if (call_is_sorted(ctx, 0, a, cp || bp || sp || ctx->sw_night_skip || ctx->sw_night_pack || sw_amplitudes_differ_from_one(a))) return sw_permuted_call(ctx, kInnerSorted, a, nullptr, nullptr, nullptr);
  int rc = call_begin(ctx, 0, a);
  if (rc) return rc;
  const CallSite c{ctx, 0, call_stream(ctx, 0, a->memspace)}; hipStream_t s = c.s;
  const int N = a->ncol, L = a->nlay;
  const size_t nl = (size_t)N * L;
  const SwTab &T = *(SwTab *)ctx->sw_desc;
  SwBound bound{};   // the kernels' struct and what else the array tables bind (rrtmg_call_arrays.h)
  SwDev &d = bound;
  d.ncol = N; d.nlay = L;
  d.iaer = a->iaer;
  const double *alpha = nullptr;
  d.icld = call_overlap(ctx, 0, a, alpha);                  // (outside 0..3: 2, rrtmg_sw_rad.nomcica.f90:563; 4, 5 with rank correlations set)
  if (d.iaer != 0 && d.iaer != 6 && d.iaer != 10) d.iaer = 0;
  d.inflag = a->inflgsw; d.iceflag = a->iceflgsw; d.liqflag = a->liqflgsw; d.mcica = a->mcica ? 1 : 0;
  d.k = ctx->k;
  RRTMG_PROFILE_READ_ONLY_ITEM(d)
  std::string err;
  std::vector<double> svar_col;
  {
    const long omg = ctx->sw_ts.off("sw/sol/mgavgcyc"), osb = ctx->sw_ts.off("sw/sol/sbavgcyc");
    rc = sw_scalar_setup(d, N, a->isolvar, a->adjes, a->dyofyr, a->scon, a->solcycfrac, a->bndsolvar, a->indsolvar,
                         omg >= 0 ? ctx->sw_ts.flat.data() + omg : nullptr, osb >= 0 ? ctx->sw_ts.flat.data() + osb : nullptr, svar_col, err,
                         a->shard_col0, a->shard_ncol);
  }
  if (rc) return ctx->fail(rc, "%s", err.c_str());
  if (d.icld >= 1 && d.inflag == 1 && d.mcica) return ctx->fail(RRTMG_ERR_INFLAG1_MCICA, "shortwave: %s", status_message(RRTMG_ERR_INFLAG1_MCICA));   // rrtmg_sw_cldprmc.f90:166
  if (d.icld >= 1 && d.inflag == 1) return ctx->fail(RRTMG_ERR_UNSUPPORTED, "inflgsw=1 has no shortwave implementation in RRTMG_SW (cldprop_sw handles 0 and 2)");

  // ---- inputs (rrtmg_host_inputs.h: uniform arrays are filled on the device, all-zero band arrays are absent) ----------------
  bool ok = true;
  const double ps = a->pressure_scale, ws = a->water_path_scale;
  HostInputs hi(ctx, s, "sw.in.", a->memspace, call_share(ctx), 0, ctx->f32);
  const SwStructs x(a, sp, cp, bp);
  const unsigned on = sw_call_reads(a, sp, cp, bp, clr);
  const GridShape g = grid_shape(N, L, bp ? bp->levels : 0);
  const bool clouds = on & kClouds, optics = d.inflag == 0, given = d.inflag == 2;
  // single-scattering albedo / asymmetry / forward fraction are read only where the optics are given directly -- under
  // inflag 2 they would multiply an optical depth below cldmin = 1e-20 at most -- so host copies are not uploaded then.
  // taucld stays live under inflag 2 (the tauctot gate of cldprop_sw); given directly -- inflag 0 -- it is used as it is.
  const InRule direct{optics, InPolicy::Plain, 0.0, 0.0, !(optics || a->memspace == 1)};
  const InRuleFor<SwBound> rules[] = {
      {&SwDev::play, {true, InPolicy::Plain, ps}}, {&SwDev::plev, {true, InPolicy::Plain, ps}}, {&SwDev::h2o, {true, InPolicy::Plain, a->h2o_mul, a->h2o_div}},
      {&SwDev::ssacld, direct}, {&SwDev::asmcld, direct}, {&SwDev::fsfcld, direct},
      {&SwDev::cicewp, {given, InPolicy::Plain, ws}}, {&SwDev::cliqwp, {given, InPolicy::Plain, ws}}, {&SwDev::reice, {given}}, {&SwDev::reliq, {given}},
      {&SwDev::taucld, {optics, optics ? InPolicy::Plain : InPolicy::ZeroAbsent}}, {&CallLocals::cldfmcl, {false}}};   // (the sub-columns: where given)
  register_inputs(hi, kSwIn, on, x, bound, g, rules);
  if (!hi.finish()) return ctx->status;

  // ---- work buffers -------------------------------------------------------------------------
  auto wd = [&](const char *name, size_t n) -> double * { double *p = (double *)ctx->buf(std::string("sw.w.") + name, n * sizeof(double)); if (!p) ok = false; return p; };
  d.prep = wd("prep", sw_prep_size(N, L));
  d.pdp = wd("pdp", nl); d.cossza = wd("cossza", N);
  d.laytrop = (int32_t *)ctx->buf("sw.w.laytrop", (size_t)N * 4);
  d.laysolfr = (int32_t *)ctx->buf("sw.w.laysolfr", (size_t)N * 4 * kSwNBand); d.anycld = (int32_t *)ctx->buf("sw.w.anycld", (size_t)N * 4);
  d.tile_cld = (int32_t *)ctx->buf("sw.w.tilecld", (size_t)((N + 63) / 64) * 4);
  d.ncloudy = ctx->ncloudy_dev;
  if (!d.laytrop || !d.laysolfr || !d.anycld || !d.tile_cld) ok = false;
  if (clouds) { d.ctau = wd("ctau", nl * kSwNBand); d.cssa = wd("cssa", nl * kSwNBand); d.casm = wd("casm", nl * kSwNBand); }
  d.nw = (L + 63) / 64;
  if (clouds && d.mcica) { d.mask = (uint64_t *)ctx->buf("sw.w.mask", (size_t)kSwNGpt * d.nw * N * 8); if (!d.mask) ok = false; }
  const int ntile = (N + 63) / 64;
  const int hint_cloudy = call_hint_cloudy(ctx, 0, ntile, L);
  const bool night = ctx->sw_night_skip || ctx->sw_night_pack;   // the *_night_kernel of every launch below that has one (the pack: on the packed copy, and as the skip where a call is not packed)
  // The count a call with the skip leaves is of the tiles that RAN cloudy: a night tile is of neither kind.  The chunk plan
  // follows the cloudy share of the tiles that were not night in that call (its night count: a hint like the other), scaled to
  // the grid: a grid keeps the plan it has without the skip, whichever way the previous call ran.
  int plan_cloudy = hint_cloudy;
  if (hint_cloudy >= 0 && ctx->sw_night_reported) {
    // (a packed call reports the night tiles of the caller's grid: its copy, this call's grid, has one more)
    const int nn = ctx->night_host()[0] + (ctx->inner == kInnerPacked && ctx->sw_pack_reported ? 1 : 0), run = ntile - nn;
    if (nn > 0 && run > 0 && hint_cloudy <= run) plan_cloudy = (int)((long)hint_cloudy * ntile / run);
  }
  // (work space per tile of a mixed grid's chunk: the scratch slab, and with components the direct-beam partial planes -- half
  //  again the size of `part`, about 4 GB more on a 2048-tile chunk at 60 layers)
  const bool need_dir = cp || (bp && (bp->dndir || bp->dndirc));   // the *_dir solve variants and their partdir planes
  const size_t tile_bytes = ((size_t)kSwNGpt * F_NTOT * L + (need_dir ? (size_t)kSwNSlot * 2 * (L + 1) : 0)) * 64 * sizeof(double);
  const int ctile = plan_call_chunks(ctx, 0, d, clouds, plan_cloudy, tile_bytes);   // tiles per solve chunk
  if (!d.tlist) ok = false;
  d.scratch = wd("scratch", (size_t)ctile * kSwNGpt * F_NTOT * L * 64);
  d.part = wd("part", (size_t)kSwNSlot * 4 * (L + 1) * ctile * 64);
  // components: the direct-beam partial planes [slot][2][nlay+1][pcols] (SwPartDirSink) and the outputs
  double *partdir = need_dir ? wd("partdir", (size_t)kSwNSlot * 2 * (L + 1) * ctile * 64) : nullptr;
  if (!svar_col.empty()) {   // per-column solar-variability multipliers (rare: facular/sunspot amplitudes != 1)
    double *p = wd("svarcol", svar_col.size());
    if (!ok) return ctx->status;
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(p, svar_col.data(), svar_col.size() * sizeof(double), hipMemcpyHostToDevice, s));
    RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));   // svar_col is a local
    d.svar_col = p;
  }
  // the outputs: the standard ones, the components [nlay+1][ncol], the band fluxes [14][nrow][ncol], each where requested
  // (clear-sky outputs off: d.swuflxc, d.swdflxc and d.swhrc stay nullptr -- no kernel of that path dereferences them)
  OutCopy oc[table_size(kSwOut)];
  const int nout = bind_outputs(kSwOut, on, x, bound, g, a->memspace, wd, oc);
  const SwCompOut &co = bound; const SwBandOut &bo = bound;
  if (!ok) return ctx->status;
  if ((rc = check_outputs(ctx, kSwOut, on, x)) || (rc = call_own_flag(c, a->memspace, d))) return rc;

  // ---- launches ---------------------------------------------------------------------------
  const dim3 gcl(ntile, L), blk(64);
  int32_t *const night_cnt = ctx->ncloudy_dev + 2;
  if (d.iaer == 6) {
    double *ta = wd("aer.tau", nl * kSwNBand), *om = wd("aer.ssa", nl * kSwNBand), *as = wd("aer.asm", nl * kSwNBand);
    if (!ok) return ctx->status;
    hipLaunchKernelGGL(sw_aer_kernel, gcl, blk, 0, s, d, T, bound.ecaer, ta, om, as);
    d.tauaer = ta; d.ssaaer = om; d.asmaer = as;
  }
  if (clouds && d.mcica && (rc = mcica_mask_launch(c, kSwNGpt, d, a, bound.cldfmcl, night ? sw_kiss_mask_night_kernel : nullptr, d.coszen, alpha, sw_kiss_mask_exp_night_kernel))) return rc;
  // preparation, solve and spectral integration, one column chunk at a time: the chunk's prep rows (58 MB at 8192 columns x
  // 60 layers) are read by its 32 work items while still in the L2s / the Infinity Cache, not streamed back from HBM after
  // the preparation of the whole grid (every solve launch of every chunk has its own event pair)
  // (Two chunks in flight at once -- even and odd chunks on two streams of the spectrum, each with its own work space -- were
  // built and measured in round 6: 131 072 clear-sky columns 23.2 -> 24.1-24.5 ms, config-5 shard 72.9-73.7 -> 74.1-74.9,
  // config-4 shard 5.83-5.94 -> 5.79-5.89: the other spectrum's solve already runs over a chunk's preparation and
  // integration, and two solves of one spectrum sharing the CUs take 1.7 x as long each.  docs/EXPERIMENTS.md E.)
  // Each launch stage's geometry once; with the night-column skip on, the *_night_kernel of every stage that has one
  const auto cloud_k = night ? sw_cloud_night_kernel : sw_cloud_kernel;
  const auto lists_k = night ? sw_tile_lists_night_kernel : tile_lists_kernel;
  const auto comp_k = night ? sw_components_night_kernel : sw_components_kernel;
  const auto band_k = night ? sw_bandflux_night_kernel : sw_bandflux_kernel;
  const dim3 bprep(64 * kPrepWaves), wg(64 * kSwWgWaves), bc(64 * kC4Waves), bas(64 * kAsWaves), bfl(64 * (kFluxLev + 1));
  const size_t lds_prep = (size_t)L * 64 * sizeof(int);
  const int prep_clouds = clouds && !d.mcica ? 1 : 0;
  run_chunks(c, d, clouds, hint_cloudy,
    [&](int t0, int nt) {
      if (night) hipLaunchKernelGGL(sw_prep_fused_night_kernel, dim3(nt), bprep, lds_prep, s, d, T, prep_clouds, t0, night_cnt);
      else hipLaunchKernelGGL(sw_prep_fused_kernel, dim3(nt), bprep, lds_prep, s, d, T, prep_clouds, t0);
      if (clouds && d.mcica) hipLaunchKernelGGL(cloud_k, dim3(nt, L), blk, 0, s, d, T, t0);
      hipLaunchKernelGGL(lists_k, dim3(1), blk, 0, s, d.tile_cld + t0, nt, (int32_t *)d.tlist, (int32_t *)d.tcnt, d.tcap);
    },
    [&](int t0, int nt) {
      const dim3 g((nt + kSwWgWaves - 1) / kSwWgWaves * T.nitem);
      if (partdir) hipLaunchKernelGGL(sw_solve_all_dir_kernel<false>, g, wg, 0, s, d, T, t0, nt, partdir);
      else hipLaunchKernelGGL(sw_solve_all_kernel<false>, g, wg, 0, s, d, T, t0, nt);
    },
    [&](int t0, int nt) {
      const dim3 gc((nt + kC4Waves - 1) / kC4Waves * T.nitem);
      if (!clr) hipLaunchKernelGGL(sw_solve_cloudy_allsky_kernel, dim3((nt + kAsWaves - 1) / kAsWaves * T.nitem), bas, 0, s, d, T, t0, nt);
      else if (partdir) hipLaunchKernelGGL(sw_solve_cloudy_dir_kernel, gc, bc, 0, s, d, T, t0, nt, partdir);
      else hipLaunchKernelGGL(sw_solve_cloudy_kernel, gc, bc, 0, s, d, T, t0, nt);
    },
    [&](int t0, int nt) {
      const dim3 gfl(nt, (L + kFluxLev) / kFluxLev);
      if (!clr && night) hipLaunchKernelGGL(sw_fluxheat_allsky_kernel<true>, gfl, bfl, 0, s, d, T, t0, night_cnt, d.hint_out ? (int32_t *)ctx->night_host() : nullptr);
      else if (!clr) hipLaunchKernelGGL(sw_fluxheat_allsky_kernel<false>, gfl, bfl, 0, s, d, T, t0, (int32_t *)nullptr, (int32_t *)nullptr);
      else if (night) hipLaunchKernelGGL(sw_fluxheat_night_kernel, gfl, bfl, 0, s, d, T, t0, night_cnt, d.hint_out ? (int32_t *)ctx->night_host() : nullptr);
      else hipLaunchKernelGGL(sw_fluxheat_kernel, gfl, bfl, 0, s, d, T, t0);
      if (cp) hipLaunchKernelGGL(comp_k, dim3(nt, (L + kCompLev) / kCompLev), dim3(64 * kCompLev), 0, s, d, T, t0, partdir, co);
      if (bp && bp->levels) hipLaunchKernelGGL(band_k, dim3(nt, 1), dim3(64 * 2), 0, s, d, T, t0, partdir, bo, 1);
      else if (bp) hipLaunchKernelGGL(band_k, dim3(nt, (L + kBandLev) / kBandLev), dim3(64 * kBandLev), 0, s, d, T, t0, partdir, bo, 0);
    });
  ctx->sw_night_reported = night;   // (rrtmg_hip_sw_night_last: this call's counts, once it has completed)
  ctx->sw_pack_reported = false;    // (sw_permuted_call sets it behind the inner call of a packed one)
  // the inner call of a permuted one stops here, enqueued: permuted_tail scatters behind it and runs the epilogue
  if (ctx->inner != kInnerNone) { RRTMG_HIP_CHECK(ctx, hipGetLastError()); return RRTMG_OK; }

  // ---- status + outputs -------------------------------------------------------------------
  return call_finish(c, a->memspace, oc, nout, d.err);
}

// rrtmg_hip_sw_fluxes_f32 (rrtmg_precision.h): every grid array of the structs points to float.  Host pointers: the ordinary
// driver with ctx->f32 set -- HostInputs widens behind the upload, copy_out narrows in front of the download.  Device pointers:
// ONE widen launch for what the driver reads under the call's icld / iaer (kSwIn under sw_call_reads), the ordinary
// device-resident call on the fp64 copies, ONE narrow launch for every requested output.  The checks in front are the driver's
// own, in its order, so that nothing is sized from arguments it would refuse.
int sw_fluxes_f32_impl(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *sp, const rrtmg_sw_components *cp, const rrtmg_sw_band_fluxes *bp) {
  if (a->memspace != 1) {
    ctx->f32 = true;
    const int rc = sw_fluxes_impl(ctx, a, sp, cp, bp);
    ctx->f32 = false;
    return rc;
  }
  const bool clr = ctx->sw_clear_sky;
  if (!clr && (cp || bp)) return sw_fluxes_impl(ctx, a, sp, cp, bp);   // (refused there, before anything is read)
  // (the sorted call has never checked the shard arguments: sw_permuted_call)
  const bool sorted = !sw_call_is_packed(ctx, a) && call_is_sorted(ctx, 0, a, cp || bp || sp || ctx->sw_night_skip || ctx->sw_night_pack || sw_amplitudes_differ_from_one(a));
  if (int rc = sorted ? ctx_prepare_device(ctx) : call_begin(ctx, 0, a)) return rc;
  const CallSite c{ctx, 0, call_stream(ctx, 0, 1)};
  BoundaryF32 bf(ctx, c.s, "sw.f32.");
  SwStructs b(a, sp, cp, bp);
  const unsigned on = sw_call_reads(a, sp, cp, bp, clr);
  const GridShape g = grid_shape(a->ncol, a->nlay, bp ? bp->levels : 0);
  boundary_inputs(bf, kSwIn, on, b, g);
  // (clear-sky outputs off: whatever the three point to is ignored -- absent from the narrow table, and from the inner call)
  boundary_outputs(bf, kSwOut, on, b, g);
  if (!bf.ok) return ctx->status;
  return boundary_f32_tail(c, bf, [&]() { return sw_fluxes_impl(ctx, &b, sp ? &b : nullptr, cp ? &b : nullptr, bp ? &b : nullptr); });
}

}  // namespace rrtmg
