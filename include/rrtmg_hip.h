/*
 * rrtmg_hip.h -- C-ABI of librrtmg_hip.so: MI355X (gfx950) RRTMG longwave + shortwave.
 *
 * Drop-in boundary for CliMT/climt's RRTMG path.  Two layers are exported:
 *
 *  (1) REFERENCE-COMPATIBLE ENTRY POINTS -- same symbol names, argument order, pass-by-pointer
 *      scalars and array layouts as the Fortran bind(c) wrappers that climt's Cython shims bind
 *      (climt/_components/rrtmg/sw/_rrtmg_sw.pyx:22-104, lw/_rrtmg_lw.pyx:19-80):
 *        rrtmg_sw_set_constants      rrtmg_sw_c_binder.f90:19-46
 *        rrtmg_sw_ini_wrapper        rrtmg_sw_c_binder.f90:48-57
 *        mcica_subcol_sw_wrapper     rrtmg_sw_c_binder.f90:59-107
 *        rrtmg_sw_mcica_wrapper      rrtmg_sw_c_binder.f90:109-200
 *        rrtmg_sw_nomcica_wrapper    rrtmg_sw_c_binder.f90:202-294
 *        rrtmg_set_constants         rrlw_con.f90:46-71   (the symbol _rrtmg_lw.pyx:20 binds)
 *        rrtmg_lw_set_constants      rrtmg_lw_c_binder.f90:10-37
 *        rrtmg_lw_ini_wrapper        rrtmg_lw_c_binder.f90:39-48
 *        mcica_subcol_lw_wrapper     rrtmg_lw_c_binder.f90:50-92
 *        rrtmg_lw_mcica_wrapper      rrtmg_lw_c_binder.f90:94-174
 *        rrtmg_lw_nomcica_wrapper    rrtmg_lw_c_binder.f90:176-256
 *      They operate on a process-global default context (the reference keeps the same state in
 *      Fortran module variables) and take HOST pointers.  The reference aborts the process
 *      (Fortran `stop`) on invalid input; these record an error instead, retrievable with
 *      rrtmg_hip_default_status() / rrtmg_hip_default_error().
 *
 *  (2) CONTEXT API -- explicit context (one per GPU / per component instance), host or device
 *      pointers, int status returns.  This is what climt_amd's Python host uses via ctypes.
 *
 * Array layout (both layers), identical to the reference boundary:
 *   layer arrays      double[nlay][ncol]      (Fortran (ncol,nlay)); layer 0 = surface
 *   interface arrays  double[nlay+1][ncol]
 *   per-column        double[ncol]
 *   cloud optics      double[nlay][ncol][nbnd]  (Fortran (nbnd,ncol,nlay))
 *   aerosol           double[nbnd][nlay][ncol]  (Fortran (ncol,nlay,nbnd)); ecaer [6][nlay][ncol]
 *   LW emissivity     double[16][ncol]
 *   McICA sub-columns double[nlay][ncol][ngpt]  (Fortran (ngpt,ncol,nlay))
 * No torch types, no ownership transfer: the caller owns every buffer.
 */
#ifndef RRTMG_HIP_H
#define RRTMG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RRTMG_NBNDSW 14
#define RRTMG_NGPTSW 112
#define RRTMG_NBNDLW 16
#define RRTMG_NGPTLW 140

/* Status codes: 0 ok.  Every distinct `stop` MESSAGE of the reference (the 61 sites of rrtmg_{sw,lw}_cldprop.f90,
 * rrtmg_{sw,lw}_cldprmc.f90, mcica_subcol_gen_{sw,lw}.f90, rrtmg_sw_rad.nomcica.f90 carry 20 different texts) has its own
 * code, and rrtmg_hip_last_error() ends with the reference's text.  Where the reference stops at the first failed check, a
 * call here returns the first failed check of a (column, layer) in the reference's program order, and the largest such code
 * over the grid (the checks run in parallel); the context stays usable.  Code 13 (rounds 1-4: "any cloud optical property
 * out of range") is no longer returned: 30-41 say which. */
enum {
  RRTMG_OK = 0,
  RRTMG_ERR_HIP = 1,               /* HIP runtime failure (message has the hipError string) */
  RRTMG_ERR_NOT_INITIALISED = 2,   /* *_init not called / tables missing */
  RRTMG_ERR_TABLES = 3,            /* data blob unreadable or malformed */
  RRTMG_ERR_ARG = 4,               /* bad argument (null pointer, nlay<=0, struct_size, ...) */
  RRTMG_ERR_PARTIAL_CLOUD = 10,    /* rrtmg_sw_rad.nomcica.f90:618 'PARTIAL CLOUD NOT ALLOWED' */
  RRTMG_ERR_ICE_RADIUS = 11,       /* 'ICE RADIUS OUT OF BOUNDS' (sw_cldprop:194,226 sw_cldprmc:183,213 lw_cldprop:198,209 lw_cldprmc:189,198) */
  RRTMG_ERR_LIQ_RADIUS = 12,       /* 'LIQUID EFFECTIVE RADIUS OUT OF BOUNDS' (sw_cldprop:290 sw_cldprmc:273 lw_cldprop:253 lw_cldprmc:234) */
  RRTMG_ERR_KISS_PRESSURE = 14,    /* 'MCICA_SUBCOL: KISSVEC SEED GENERATOR REQUIRES PMID FROM BOTTOM FOUR LAYERS.' (mcica_subcol_gen_sw:355, _lw:328) */
  RRTMG_ERR_ICLD = 15,             /* 'MCICA_SUBCOL: INVALID ICLD' (mcica_subcol_gen_sw:145, _lw:122) */
  RRTMG_ERR_INFLAG1_MCICA = 16,    /* 'INFLAG = 1 OPTION NOT AVAILABLE WITH MCICA' (sw_cldprmc:166, lw_cldprmc:172) */
  RRTMG_ERR_ICE_GEN_SIZE = 17,     /* 'ICE GENERALIZED EFFECTIVE SIZE OUT OF BOUNDS' (sw_cldprop:250 sw_cldprmc:236 lw_cldprop:225 lw_cldprmc:212) */
  RRTMG_ERR_ICE_RADIUS_SMALL = 18, /* 'ICE RADIUS TOO SMALL' (lw_cldprop:193, lw_cldprmc:185) */
  RRTMG_ERR_UNSUPPORTED = 20,      /* option without an implementation in RRTMG itself (e.g. shortwave inflag = 1, iceflag = 0) */
  /* shortwave cloud-optics checks behind each parameterisation (sw_cldprop:216-220,240-244,264-265,270-274,307-311;
   * sw_cldprmc:204-208,227-231,250-251,256-260,290-294) */
  RRTMG_ERR_ICE_EXT_NEG = 30,      /* 'ICE EXTINCTION LESS THAN 0.0' */
  RRTMG_ERR_ICE_SSA_GT1 = 31,      /* 'ICE SSA GRTR THAN 1.0' */
  RRTMG_ERR_ICE_SSA_NEG = 32,      /* 'ICE SSA LESS THAN 0.0' */
  RRTMG_ERR_ICE_ASYM_GT1 = 33,     /* 'ICE ASYM GRTR THAN 1.0' */
  RRTMG_ERR_ICE_ASYM_NEG = 34,     /* 'ICE ASYM LESS THAN 0.0' */
  RRTMG_ERR_FDELTA_NEG = 35,       /* 'FDELTA LESS THAN 0.0' */
  RRTMG_ERR_FDELTA_GT1 = 36,       /* 'FDELTA GT THAN 1.0' */
  RRTMG_ERR_LIQ_EXT_NEG = 37,      /* 'LIQUID EXTINCTION LESS THAN 0.0' */
  RRTMG_ERR_LIQ_SSA_GT1 = 38,      /* 'LIQUID SSA GRTR THAN 1.0' */
  RRTMG_ERR_LIQ_SSA_NEG = 39,      /* 'LIQUID SSA LESS THAN 0.0' */
  RRTMG_ERR_LIQ_ASYM_GT1 = 40,     /* 'LIQUID ASYM GRTR THAN 1.0' */
  RRTMG_ERR_LIQ_ASYM_NEG = 41      /* 'LIQUID ASYM LESS THAN 0.0' */
};

typedef struct rrtmg_ctx rrtmg_ctx;

/* ---- context lifecycle -------------------------------------------------------------- */
int rrtmg_hip_create(rrtmg_ctx **out, int device_ordinal);
void rrtmg_hip_destroy(rrtmg_ctx *ctx);
const char *rrtmg_hip_last_error(const rrtmg_ctx *ctx);
const char *rrtmg_hip_version(void);
/* Version of the argument structs below (rrtmg_sw_args, rrtmg_lw_args, rrtmg_slab_args): bumped whenever a field is added.
 * 5 = this header.  A caller can compare it with RRTMG_HIP_ABI_VERSION of the header it was built with; the flux calls
 * check `struct_size` themselves. */
#define RRTMG_HIP_ABI_VERSION 5
int rrtmg_hip_abi_version(void);
/* HIP stream (hipStream_t) the work of this context is enqueued on (longwave uses a second one in deferred mode). */
void *rrtmg_hip_stream(rrtmg_ctx *ctx);
int rrtmg_hip_synchronize(rrtmg_ctx *ctx);
/* Device-side ordering: `other_stream` (a hipStream_t of the caller, e.g. the one an RCCL gather of the outputs is issued on)
 * waits for everything enqueued so far on this context's streams; the host does not block. */
int rrtmg_hip_stream_wait(rrtmg_ctx *ctx, void *other_stream);
/* Deferred mode (off by default).  When on, rrtmg_hip_{sw,lw}_fluxes calls with memspace == 1 (device-resident
 * arrays) return as soon as their kernels are enqueued -- shortwave and longwave on separate streams, so the two
 * overlap on the GPU -- and the device-side error flags (the reference's `stop` conditions) are reported by the
 * next rrtmg_hip_synchronize / rrtmg_hip_set_deferred call instead.  Host-memory calls stay synchronous. */
int rrtmg_hip_set_deferred(rrtmg_ctx *ctx, int on);
/* OPT-IN internal column order for device-resident calls (memspace 1) with clouds (env RRTMG_HIP_SORT_COLUMNS=1 sets it at
 * create): the call runs on an internal copy of its inputs in which the cloud-free columns come first and the cloudy ones behind,
 * each block padded to a 64-column tile, and scatters its outputs back -- so that a cloud-free column never shares a tile
 * (= a solve-kernel variant that computes both sky streams) with a cloudy one.  It pays where cloud-free columns are interleaved
 * with cloudy ones more finely than 64 columns AND the grid is large (>= 32 768 columns); it costs a copy of the inputs (as much
 * device memory again) and, on small grids, a clear-sky launch of its own.  Columns are independent, the kissvec masks are seeded
 * per column: a cloudy column's results are the same bits as without the sort; a cloud-free column that used to sit in a cloudy
 * tile now runs in the clear-sky variant, whose shortwave differs from the cloudy variant's clear-sky stream by ~1e-12 W m^-2 --
 * which is why this is not the default (tile-aligned shards == the whole grid bit for bit only when a column's variant is a
 * function of its tile).  Calls with the Mersenne twister (one positional stream) and host-pointer calls are not sorted,
 * nor are shortwave calls whose facular / sunspot amplitudes indsolvar differ from 1 (rescaled once per column in the caller's
 * order: positional too; the caller's array comes back as without the sort), nor are calls that request flux components or band fluxes (rrtmg_hip_sw_fluxes_components, rrtmg_hip_*_fluxes_bands). */
int rrtmg_hip_set_column_sort(rrtmg_ctx *ctx, int on);
/* OPT-IN night-column skip of the shortwave (off by default; with it off nothing changes, and the reference-compatible symbols
 * on the default context never have it).  The reference's driver does not skip night columns: it clamps coszen to 1e-10
 * (rrtmg_sw_rad.nomcica.f90:641-642) and runs the whole solver for fluxes of at most 1e-10 * scon * adjes W m^-2.  With the skip on:
 *  - a NIGHT COLUMN is one with coszen <= 0 as the caller passes it, before the clamp (0.0 and -0.0 are night, NaN is not);
 *    every output of a night column -- the six arrays of rrtmg_sw_args, every requested member of rrtmg_sw_components and
 *    every requested row of rrtmg_sw_band_fluxes -- is +0.0 at every level, layer and band;
 *  - every output of a day column keeps the bits of the same call with the skip off (any mcica / irng / icld / iaer, per-band
 *    albedo, host or device arrays, deferred mode, column chunks, shard_col0 / shard_ncol blocks);
 *  - work is saved per TILE, the 64 consecutive columns 64 t .. 64 t + 63 of the call that the solve kernels work on (the last
 *    tile may be shorter): a tile whose columns are all night is not prepared, its cloud optics and kissvec mask are not formed
 *    and no solve workgroup runs for it.  A mixed tile -- night and day columns -- is solved whole, in the same kernel variant
 *    and at the same place of the Mersenne twister's stream as without the skip, and its night columns are zeroed afterwards:
 *    nothing is saved inside a mixed tile.  With longitude fastest a tile is 64 consecutive longitudes of one latitude row: a
 *    grid with 128 longitudes has two tiles per row and few night tiles, one with 512 or more has close to half of them night.
 *  - status codes: the inputs of a night tile other than coszen are not checked, so no status code can come from them (they
 *    are not read either, but for two passes over the whole grid that raise no code and whose work is not saved: the ECMWF
 *    aerosol mixing of iaer = 6 reads ecaer, the Mersenne twister's mask reads cldfr of every column); the night
 *    columns of a mixed tile run in lockstep with their day neighbours and are checked as without the skip; a day column's bad
 *    input raises the same code as without the skip, and the context stays usable.
 * The host-side scalar set-up (the in-place rescale of indsolvar included) is unchanged.  A call with the skip on is never
 * column-sorted (rrtmg_hip_set_column_sort).  The longwave is not touched.  The switch belongs to the context: a binder that
 * shares one context between callers sets it before each shortwave call.  Probe for it by symbol; the argument structs and
 * RRTMG_HIP_ABI_VERSION are unchanged. */
int rrtmg_hip_set_sw_night_skip(rrtmg_ctx *ctx, int on);
/* OPT-IN day-column pack of the shortwave (off by default; with it off nothing changes, and the reference-compatible symbols
 * on the default context never have it): the night-column skip for grids whose tiles are all mixed.  An ELIGIBLE call runs on
 * an internal copy of its inputs in which the day columns come first, in the caller's order, padded to a 64-column tile
 * boundary with replicas of the last of them, and the night columns follow: no tile holds both kinds, and every tile behind
 * the day block costs no preparation and no solve time, on any grid and in any column order.  The outputs are scattered back
 * to the caller's columns on the device.  The output contract is the skip's: a night column (coszen <= 0 as passed; NaN is
 * day) gets +0.0 in every output -- the six arrays, every requested component, every requested band row -- whether or not
 * rrtmg_hip_set_sw_night_skip is also on.
 *  - Eligible: device pointers (memspace 1), more than 64 columns (at least two tiles), kissvec or no McICA, amplitudes
 *    indsolvar equal to 1 (or NULL).  The Mersenne twister's one stream and rescaled amplitudes are positional, so such calls
 *    are not packed.  HOST-POINTER CALLS (memspace 0, rrtmg_hip_radiation_fluxes included) ARE NOT PACKED in this version.  A
 *    call that is not eligible runs exactly as with rrtmg_hip_set_sw_night_skip(ctx, 1): the tile skip's bits, its counts in
 *    rrtmg_hip_sw_night_last, indsolvar rescaled as always.  Components, band fluxes and the surface struct all run packed.
 *    With the option on no call is column-sorted (rrtmg_hip_set_column_sort).
 *  - Bits: a day column's outputs are, bit for bit, those of a call with the skip off on the day columns alone, in the same
 *    order (ncol = number of day columns).  Against the call with the skip off on the WHOLE grid this means: where every tile
 *    runs one solve variant (icld = 0, or a cloud in every column) day columns keep their bits; in a grid with cloudy and
 *    cloud-free columns a cloudy day column keeps its bits, and a cloud-free day column may change solve variant, because its
 *    tile has other members: it stays within 1e-10 W m^-2 (K d^-1) of the unpacked result (the variants differ by ~1e-12, the
 *    column sort's caveat).  The same caveat applies to shard == whole grid: a shard packs its own day columns.
 *  - Status codes: a night column's inputs other than coszen are never read or checked (but ecaer under iaer = 6, whose
 *    whole-grid pass raises no code); a day column's bad input raises the code it raises with the skip off, and the context
 *    stays usable.
 *  - rrtmg_hip_sw_night_last after a packed call: night_columns = ncol - day columns; night_tiles = ceil(ncol / 64) -
 *    ceil(day columns / 64), the tiles' worth of solve work not done.
 *  - Cost: three small launches for the column map, one gather launch for all inputs (one more for band-fastest cloud arrays),
 *    one scatter launch for all outputs, and an internal copy of inputs and outputs of 64 x (ceil(ncol / 64) + 1) columns.
 * Probe for it by symbol; the argument structs and RRTMG_HIP_ABI_VERSION are unchanged. */
int rrtmg_hip_set_sw_night_pack(rrtmg_ctx *ctx, int on);
/* OPT-IN shortwave call without the clear-sky outputs (on = 1 by default: nothing changes; the reference-compatible symbols on
 * the default context always have 1).  With on = 0 a shortwave call forms no clear-sky stream: tiles with cloud run a one-stream
 * solve (under McICA one layer operator and one adding recurrence per g-point and layer instead of two), and swuflxc, swdflxc
 * and swhrc are neither computed nor copied.
 *  - The three members may be NULL.  Whatever they point to is ignored: on a device-pointer call (memspace 1) not one element
 *    is written; on a host-pointer call the arrays are neither downloaded nor touched.
 *  - swuflx, swdflx and swhr: a column of a cloud-free tile (64 columns) keeps its bits; a column of a tile with cloud agrees with
 *    the default call to rounding (the same operations on the total-sky stream, compiled in another kernel: <= 5e-8 W m-2).
 *  - Covers rrtmg_hip_sw_fluxes, rrtmg_hip_sw_fluxes_surface with the albedo by band, and the shortwave half of
 *    rrtmg_hip_radiation_fluxes; chunks, shards, deferred mode, rrtmg_hip_set_column_sort, rrtmg_hip_set_sw_night_skip and
 *    rrtmg_hip_set_sw_night_pack work as with on = 1 (a night column gets +0.0 in the three outputs).
 *  - rrtmg_hip_sw_fluxes_components, rrtmg_hip_sw_fluxes_bands and a call of rrtmg_hip_sw_fluxes_surface or
 *    rrtmg_hip_radiation_fluxes that requests a component or a band member return RRTMG_ERR_ARG while on = 0 (their clear-sky and
 *    direct-beam members read the stream that is not formed); the context stays usable.
 * The longwave is not touched.  The switch belongs to the context: a binder that shares one context between callers sets it
 * before each shortwave call.  Probe for it by symbol; the argument structs and RRTMG_HIP_ABI_VERSION are unchanged. */
int rrtmg_hip_set_sw_clear_sky(rrtmg_ctx *ctx, int on);
/* OPT-IN longwave call without the clear-sky outputs (on = 1 by default: nothing changes; the reference-compatible symbols on
 * the default context always run with 1).  With on = 0 a longwave call forms no clear-sky stream: tiles with cloud run a one-stream
 * solve (no clear-sky recurrence in either sweep, half the partial flux planes), and uflxc, dflxc, hrc and duflxc_dt are neither
 * computed nor copied.  A NULL context returns RRTMG_ERR_ARG.
 *  - Clear-sky outputs: uflxc, dflxc and hrc may be NULL; with idrv = 1 so may duflxc_dt (duflx_dt is still required).  Whatever
 *    these pointers hold is ignored: on a device-pointer call (memspace 1) not one element is written; on a host-pointer call
 *    the arrays are neither downloaded nor touched.
 *  - All-sky outputs (uflx, dflx, hr, duflx_dt): a column of a cloud-free tile (64 columns) keeps its bits -- it runs the device
 *    functions it always ran, which write the total planes only.  A column of a tile with cloud runs the same operations on the
 *    total-sky stream in another instantiation: same bits as the default call (measured: the largest difference over the GPU
 *    tests of tests/test_lw_allsky_only_gpu.py is 0, and they assert equality).
 *  - Covers rrtmg_hip_lw_fluxes and the longwave half of rrtmg_hip_radiation_fluxes; mcica 0 and 1, icld 0 to 3, both random
 *    number generators, an external cldfmcl, idrv 0 and 1; rtrn, rtrnmc and rtrnmr; column chunks, shard_col0 / shard_ncol and
 *    deferred mode work as with on = 1.  Under rrtmg_hip_set_column_sort the permuted call's output table carries no entry for the
 *    absent arrays.
 *  - Band fluxes: rrtmg_hip_lw_fluxes_bands with upc or dnc requested returns RRTMG_ERR_ARG before anything is enqueued, and the
 *    context stays usable; a band call that requests only up and / or dn is served (those members read the total planes only).
 *    The same rule applies to lw_bands inside rrtmg_hip_radiation_fluxes.
 * The shortwave is not touched: rrtmg_hip_set_sw_clear_sky and this switch are independent of each other.  The switch belongs
 * to the context: a binder that shares one context between callers sets it before each longwave call.  Probe for it by symbol;
 * the argument structs and RRTMG_HIP_ABI_VERSION are unchanged. */
int rrtmg_hip_set_lw_clear_sky(rrtmg_ctx *ctx, int on);
/* Night tiles and night columns (all of them: those of mixed tiles too) of the last completed shortwave call on this context:
 * valid after the call has returned, in deferred mode after rrtmg_hip_synchronize.  0 / 0 if that call ran with the skip off
 * (and the pack off); after a packed call (rrtmg_hip_set_sw_night_pack) the counts stated there.
 * night_tiles * 64 columns of the call's (ncol + 63) / 64 * 64 cost no solve time. */
int rrtmg_hip_sw_night_last(rrtmg_ctx *ctx, int *night_tiles, int *night_columns);
/* Duration (ms, HIP events recorded on the stream the kernel is launched on) of a solve kernel in the last completed call:
 * which = 0 -> sw_solve_all_kernel<false> (clear-sky tiles), 1 -> lw_solve_all_kernel<false,..>, 2 -> sw_solve_cloudy_kernel,
 * 3 -> lw_solve_all_kernel<true,..>.  A call launches that kernel once per column chunk (RRTMG_HIP_CHUNK_TILES tiles of 64
 * columns; one chunk up to 8192 columns by default); every launch has its own event bracket and the value is their SUM -- the time the
 * kernel took for ALL the call's columns.  rrtmg_hip_kernel_launches returns the number of launches (chunks), so that
 * sum / launches is the average launch duration rocprofv3 reports for that kernel (when the GPU is not shared with another
 * stream: a bracket also contains the time its workgroups waited for compute units another stream's kernel held).
 * RRTMG_ERR_ARG / 0 launches if that kernel was not launched by the last call. */
int rrtmg_hip_kernel_ms(rrtmg_ctx *ctx, int which, double *ms);
int rrtmg_hip_kernel_launches(rrtmg_ctx *ctx, int which);

/* physical constants (cgs, as climt passes them): replaces rrtmg[_sw]_set_constants */
int rrtmg_hip_set_constants(rrtmg_ctx *ctx, double pi, double grav, double planck, double boltz,
                            double clight, double avogad, double alosmt, double gascon,
                            double sbcnst, double secdy);

/* table construction + g-point reduction + upload; blob_path NULL -> "<dir of .so>/../data/rrtmg_{sw,lw}_data.bin"
 * replaces rrtmg_sw_ini (rrtmg_sw_init.f90:47-173) / rrtmg_lw_ini (rrtmg_lw_init.f90:28-175) */
int rrtmg_hip_sw_init(rrtmg_ctx *ctx, double cpdair, const char *blob_path);
int rrtmg_hip_lw_init(rrtmg_ctx *ctx, double cpdair, const char *blob_path);
/* 1 if the loaded LW k-distribution tables are synthetic (reference data file missing) */
int rrtmg_hip_lw_tables_synthetic(const rrtmg_ctx *ctx);

/* read back a reduced table built at init (for tests): name e.g. "sw/kg16/absa"; returns element count, or <0 */
long rrtmg_hip_get_table(rrtmg_ctx *ctx, const char *name, double *out, long capacity);

/* ---- upstream of the shortwave: zenith angle (climt Instellation) ----------------------------- */
/* zenith[i] (radians, clamped to pi/2 on the night side) of column i at `julian_centuries` (days since
 * 2000-01-01 12:00 / 36525): replaces climt/_components/instellation/component.py:85-135 (_instellation_kernel_np; sun
 * position helpers :138-191 are evaluated on the host).  lat/lon in degrees; memspace as in the flux calls. */
int rrtmg_hip_zenith_angle(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg,
                           double julian_centuries, double *zenith);

/* Per-column part of climt's BergerSolarInsolation (climt/_components/berger_solar_insolation.py:671-676):
 * zenith[i] = arccos(cos_mu), insolation[i] = irradiance * cos_mu with cos_mu = sin(lat) sin_delta - cos(lat) cos_delta
 * cos(2 pi (fractional_day + lon / 360)).  lat is used as given (the reference passes degrees into sin/cos, :673);
 * sin_delta / cos_delta of the solar declination and irradiance = S0 / rho^2 come from the host-side orbital series
 * (:579-668, climt_amd/berger.py). */
int rrtmg_hip_solar_insolation(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat, const double *lon, double sin_delta,
                               double cos_delta, double fractional_day, double irradiance, double *zenith, double *insolation);

/* ---- downstream of the radiation path: slab surface energy balance (climt SlabSurface) ---------- */
/* Kernel of climt/_components/slab_surface.py:440-517 (default configuration, include_ekman=False): surface
 * temperature tendency (K s^-1) and slab depth (m) per column.  The four flux pointers are the SURFACE rows (row 0 of
 * the [level][column] radiation outputs); area_type codes: land 0, land_ice 1, sea 2, sea_ice 3 (slab_surface.py:9). */
typedef struct rrtmg_slab_args {
  const double *sw_down, *lw_down, *sw_up, *lw_up;      /* surface fluxes W m^-2 */
  const double *lh, *sh;                                /* surface upward latent / sensible heat flux */
  const int32_t *area_type;
  const double *up_heat_soil, *heat_flux_sea_ice, *sea_water_dens, *surf_dens, *heat_cap_soil, *surf_therm_cap;
  const double *ocean_mix_thick, *soil_layer_thick, *ocean_heat_transport;
  double *tend_ts, *depth;                              /* outputs */
} rrtmg_slab_args;
int rrtmg_hip_slab_surface(rrtmg_ctx *ctx, int ncol, int memspace, const rrtmg_slab_args *args);

/* ---- glue of a device-resident radiation step (device pointers only; enqueued on the context's main stream) ----------
 * The numpy that climt's component classes run on the host between the kernels, so that a model loop can stay in HBM. */
/* interface values of a mid-level quantity by log-pressure interpolation, [nlay+1][ncol]: climt/_core/util.py:89-142 */
int rrtmg_hip_interface_values(rrtmg_ctx *ctx, int ncol, int nlay, const double *mid, const double *surf, const double *pmid,
                               const double *pint, double *out);
/* op 0: out = alpha*a (+ beta*b if b != NULL); op 1: out = cos(a) (sw/component.py:567); op 2: out = a*alpha/beta
 * (mass_to_volume_mixing_ratio, util.py:86, with its two roundings); op 3: out = a >= pi/2 ? 0.0 : cos(a) -- cos(zenith) for a
 * shortwave call with rrtmg_hip_set_sw_night_skip on: a zenith angle clamped to pi/2 (Instellation) has a cosine of +6e-17 */
int rrtmg_hip_elementwise(rrtmg_ctx *ctx, int op, long n, const double *a, const double *b, double alpha, double beta, double *out);
/* Adams-Bashforth update out = x + dt * sum_k w[k] f[k], k < order <= 4 (f, w: host arrays of device pointers / weights) */
int rrtmg_hip_ab_step(rrtmg_ctx *ctx, long n, int order, const double *x, const double *const *f, const double *w, double dt, double *out);
/* deferred mode: 0 = the longwave stream waits for the main stream's work so far, 1 = the main stream waits for the longwave's */
int rrtmg_hip_order_streams(rrtmg_ctx *ctx, int direction);
/* Strided copies of nblk two-dimensional blocks of doubles on the device, enqueued on `stream` (a hipStream_t of the caller;
 * NULL = the context's main stream): block b copies rows x cols elements, dst[dst_off + r*dst_stride + c] = src[src_off +
 * r*src_stride + c].  desc: DEVICE array of 6 int64 per block {src_off, dst_off, rows, cols, src_stride, dst_stride};
 * max_rows / max_cols bound the launch.  Used to put an all-gathered output buffer -- [rank][array][level][local column] --
 * into the boundary layout [array][level][column] (column fastest, rrtmg_lw_c_binder.f90:198-202) without leaving the GPU:
 * climt_amd/distributed.py. */
int rrtmg_hip_copy_blocks(rrtmg_ctx *ctx, int nblk, const int64_t *desc, long max_rows, long max_cols, const double *src, double *dst,
                          void *stream);

/* ---- shortwave ------------------------------------------------------------------------ */
typedef struct rrtmg_sw_args {
  int32_t ncol, nlay;
  int32_t memspace;     /* 0: all pointers are host memory; 1: all pointers are device memory */
  int32_t mcica;        /* 0: rrtmg_sw_rad.nomcica.f90 path; 1: McICA path (rrtmg_sw_rad.f90) */
  int32_t icld, iaer;   /* as the reference (icld 0..3; iaer 0/6/10) */
  int32_t inflgsw, iceflgsw, liqflgsw;
  int32_t dyofyr, isolvar;
  int32_t irng;         /* McICA RNG: 0 kissvec, 1 Mersenne twister */
  int32_t permuteseed;  /* McICA changeSeed */
  /* Column shard of a larger grid (multi-GPU): this call's columns are columns shard_col0 .. shard_col0+ncol-1 of a grid of
   * shard_ncol columns; 0, 0 = not sharded.  Two inputs are positional and need it: the Mersenne twister -- the reference
   * draws ONE stream in (sub-column, column, layer) order (mcica_subcol_gen_sw.f90:360-367), so a shard skips the other shards'
   * draws and reproduces the unsharded masks bit for bit (kissvec seeds are per column and ignore it) -- and, in the shortwave,
   * facular / sunspot amplitudes that differ from 1 (see indsolvar). */
  int32_t shard_col0, shard_ncol;
  /* sizeof(rrtmg_sw_args) of the header the CALLER was compiled against: REQUIRED.  Any value that is not the library's own
   * sizeof -- 0 included -- is refused with RRTMG_ERR_ARG: a caller built against another header never has fields dropped
   * or read past its struct.  (This slot was `reserved0` = 0 in two earlier layouts, with and without the unit factors at
   * the end; a zero cannot tell them apart, so it is not guessed.) */
  int32_t struct_size;
  double adjes, scon, solcycfrac;
  const double *bndsolvar;   /* [14] (host) or NULL -> ones */
  double *indsolvar;         /* [2]  (host, under either memspace) or NULL -> ones; IN/OUT: amplitudes != 1 are rescaled in
                              * place once per column, as the reference does (rrtmg_sw_rad.nomcica.f90:1199-1215: inatm_sw sits
                              * inside its column loop).  Column k of the call sees amplitudes rescaled k + 1 times -- night
                              * columns count, whether or not the night-column skip is on -- so with isolvar 1, or isolvar 2 and
                              * scon 0, the solar-variability multipliers of a column depend on its POSITION in the call.  On return:
                              *  - whole grid (shard_ncol 0): rescaled ncol times;
                              *  - shard (shard_col0, shard_ncol): the call performs the shard_col0 steps of the columns in front
                              *    of it first, so its columns get the multipliers they have in the whole grid, and the steps of
                              *    the columns behind it afterwards: rescaled shard_ncol times, what the call on the whole grid
                              *    leaves, on every shard (each shard starts from the amplitudes the whole grid would start from);
                              *  - column sort enabled: as without it -- a call whose amplitudes differ from 1 is not sorted. */
  /* state */
  const double *play, *plev, *tlay, *tlev, *tsfc;
  const double *h2ovmr, *o3vmr, *co2vmr, *ch4vmr, *n2ovmr, *o2vmr;
  const double *asdir, *asdif, *aldir, *aldif, *coszen;
  /* clouds (NULL allowed when icld == 0; optics arrays NULL allowed when inflgsw != 0) */
  const double *cldfr;
  const double *taucld, *ssacld, *asmcld, *fsfcld;   /* [nlay][ncol][14] */
  const double *cicewp, *cliqwp, *reice, *reliq;
  /* aerosol (NULL allowed when iaer == 0) */
  const double *tauaer, *ssaaer, *asmaer;            /* [14][nlay][ncol] */
  const double *ecaer;                               /* [6][nlay][ncol]  */
  /* McICA: optional externally generated sub-column cloud mask, [nlay][ncol][112] of 0.0/1.0
   * (e.g. cldfmcl from mcica_subcol_sw_wrapper). NULL -> generated on the device by either
   * generator (irng 0 kissvec, 1 Mersenne twister: its one stream by jump-ahead). */
  const double *cldfmcl;
  /* outputs */
  double *swuflx, *swdflx, *swhr, *swuflxc, *swdflxc, *swhrc;
  /* Unit factors for HOST arrays (memspace 0), applied by the library on the device after the upload instead of by the
   * caller on the host; 0 = the array is in the unit of the reference already.  play, plev *= pressure_scale (Pa -> mbar:
   * 0.01); cicewp, cliqwp *= water_path_scale (kg m^-2 -> g m^-2: 1000); h2ovmr = h2ovmr * h2o_mul / h2o_div (specific
   * humidity -> volume mixing ratio: 28.964 / 18.02, climt/_core/util.py:86).  One rounding per operation, as numpy.
   * A struct that was zero-initialised gets none of it.  With device
   * pointers (memspace 1) a non-zero factor is an error (RRTMG_ERR_ARG): the caller's device arrays are never modified. */
  double pressure_scale, water_path_scale, h2o_mul, h2o_div;
} rrtmg_sw_args;

int rrtmg_hip_sw_fluxes(rrtmg_ctx *ctx, const rrtmg_sw_args *a);

/* Shortwave flux COMPONENTS: the downward flux split into direct and diffuse parts, and into UV/visible (bands 10-13, the
 * bands that take asdir / asdif) and near-IR (bands 1-9 and 14: aldir / aldif) parts -- the dirdflux, difdflux, dirdnuv,
 * difdnuv, dirdnir, difdnir of rrtmg_sw_rad.nomcica.f90:773-794 / rrtmg_sw_rad.f90:798-819, which the reference computes and
 * does not return.  Every member is [nlay+1][ncol], W m^-2, level 0 = surface like swdflx, in the memspace of the
 * rrtmg_sw_args; NULL = not wanted.  Direct = the delta-scaled direct beam (idelm = 1); diffuse = total - direct:
 *   dirdflx, difdflx    all sky, all bands (difdflx == swdflx - dirdflx, bit for bit)
 *   dirdnuv, difdnuv    all sky, UV/visible bands;   dirdnir, difdnir   all sky, near-IR bands
 *   dirdflxc, difdflxc  clear sky, all bands (difdflxc == swdflxc - dirdflxc)
 * The versioned structs and RRTMG_HIP_ABI_VERSION are unchanged by this struct: it checks its own struct_size, and a caller
 * probes for the feature by the presence of the symbol rrtmg_hip_sw_fluxes_components (dlsym). */
typedef struct rrtmg_sw_components {
  int32_t struct_size;                 /* sizeof(rrtmg_sw_components) of the caller's header: required */
  int32_t reserved;                    /* 0 */
  double *dirdflx, *difdflx;           /* [nlay+1][ncol], same memspace as the rrtmg_sw_args; NULL = not wanted */
  double *dirdnuv, *difdnuv, *dirdnir, *difdnir;
  double *dirdflxc, *difdflxc;
} rrtmg_sw_components;
/* rrtmg_hip_sw_fluxes plus the requested components.  c == NULL, or every member NULL, is exactly rrtmg_hip_sw_fluxes(ctx, a);
 * a struct_size that is not sizeof(rrtmg_sw_components) is refused (RRTMG_ERR_ARG) before anything is enqueued.  The six
 * outputs of the plain call are the same bits with or without components.  Host pointers: the components are downloaded
 * behind the same synchronise as the six outputs; device pointers in deferred mode: the call returns once enqueued.  A call
 * with components is never column-sorted (rrtmg_hip_set_column_sort). */
int rrtmg_hip_sw_fluxes_components(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_components *c);

/* Shortwave fluxes BY BAND: the sums that rrtmg_hip_sw_fluxes forms over all 112 g-points, closed per band instead (what the
 * reference's spcvrt_sw / spcvmc_sw return for istart = iend = band, iout = band).  Band index 0..13 is the reference's
 * band order, RRTMG bands 16..29: band 29 (820-2600 cm^-1) is LAST, out of wavenumber order; rrtmg_hip_band_limits gives
 * the limits.  Every member is [14][nrow][ncol], W m^-2, in the memspace of the rrtmg_sw_args; NULL = not wanted (not
 * computed, its partial sums not read):
 *   levels == 0: nrow = nlay+1, row = interface level (0 = surface, like swdflx)
 *   levels == 1: nrow = 2, row 0 = surface, row 1 = top of the atmosphere (the same bits as rows 0 and nlay of levels == 0)
 *   up, dn, upc, dnc   all-sky / clear-sky upward / downward flux;  dndir, dndirc   delta-scaled direct beam, all / clear sky
 * The sum over the bands equals the broadband output within 256 * 2^-53 * F (another association of the same terms).
 * The versioned structs and RRTMG_HIP_ABI_VERSION are unchanged: the struct checks its own struct_size, and a caller probes
 * for the feature by the presence of the symbol rrtmg_hip_sw_fluxes_bands (dlsym). */
typedef struct rrtmg_sw_band_fluxes {
  int32_t struct_size;                 /* sizeof(rrtmg_sw_band_fluxes) of the caller's header: required */
  int32_t levels;                      /* 0: [14][nlay+1][ncol]   1: [14][2][ncol] (surface, top) */
  double *up, *dn, *upc, *dnc;
  double *dndir, *dndirc;
} rrtmg_sw_band_fluxes;
/* rrtmg_hip_sw_fluxes_components plus the requested band fluxes (c may be NULL).  b == NULL, or every member NULL, is exactly
 * rrtmg_hip_sw_fluxes_components(ctx, a, c); a struct_size that is not sizeof(rrtmg_sw_band_fluxes), or levels not 0 or 1, is
 * refused (RRTMG_ERR_ARG) before anything is enqueued.  The six outputs of the plain call (and the components) are the same
 * bits with or without bands.  Host pointers: downloaded behind the same synchronise as the six outputs; device pointers
 * in deferred mode: the call returns once enqueued.  A call with bands is never column-sorted. */
int rrtmg_hip_sw_fluxes_bands(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_components *c, const rrtmg_sw_band_fluxes *b);
/* Shortwave SURFACE ALBEDO BY BAND: what the reference's solver takes (spcvrt_sw / spcvmc_sw: albdir(nbndsw), albdif(nbndsw)),
 * where rrtmg_sw_args carries the four broadband numbers of the reference's driver, which spreads them over the bands by a
 * fixed rule (rrtmg_sw_rad.nomcica.f90:648-659: bands 10-13 asdir / asdif, bands 1-9 and 14 aldir / aldif).  Both members are
 * [14][ncol], dimensionless, band index 0..13 = the reference's band order (RRTMG bands 16..29: band 29, 820-2600 cm^-1, is
 * LAST; rrtmg_hip_band_limits), in the memspace of the rrtmg_sw_args; NULL = not given.  Each member stands alone: without
 * albdir the direct albedo is asdir / aldir by the band rule, without albdif the diffuse albedo is asdif / aldif.  With both
 * given the four broadband pointers of the rrtmg_sw_args are not read and may be NULL.  The values are not range-checked (the
 * reference has no check).  Per-band arrays filled by the band rule give the bits of the call without them.
 * The versioned structs and RRTMG_HIP_ABI_VERSION are unchanged: the struct checks its own struct_size, and a caller probes
 * for the feature by the presence of the symbol rrtmg_hip_sw_fluxes_surface (dlsym). */
typedef struct rrtmg_sw_surface {
  int32_t struct_size;                 /* sizeof(rrtmg_sw_surface) of the caller's header: required */
  int32_t reserved;                    /* 0 */
  const double *albdir, *albdif;       /* [14][ncol]; NULL = not given */
} rrtmg_sw_surface;
/* rrtmg_hip_sw_fluxes_bands with the surface albedo by band (c and b may be NULL).  surface == NULL, or both members NULL, is
 * exactly rrtmg_hip_sw_fluxes_bands(ctx, a, c, b); a struct_size that is not sizeof(rrtmg_sw_surface) is refused
 * (RRTMG_ERR_ARG) before anything is enqueued.  Host pointers are uploaded like every other input; device pointers are read
 * in place, and in deferred mode the call returns once enqueued.  A call with a surface struct is never column-sorted. */
int rrtmg_hip_sw_fluxes_surface(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *surface, const rrtmg_sw_components *c,
                                const rrtmg_sw_band_fluxes *b);
/* Band limits in cm^-1: spectrum 0 = shortwave (14 values each, bands 16..29 in that order), 1 = longwave (16 values, bands
 * 1..16; hi - lo is the longwave's delwave).  Host arrays; either may be NULL.  Returns the number of bands, or -1 for another spectrum. */
int rrtmg_hip_band_limits(int spectrum, double *wavenumber_lo, double *wavenumber_hi);

/* ---- longwave ------------------------------------------------------------------------- */
typedef struct rrtmg_lw_args {
  int32_t ncol, nlay;
  int32_t memspace;
  int32_t mcica;
  int32_t icld, idrv;
  int32_t inflglw, iceflglw, liqflglw;
  int32_t irng, permuteseed;
  int32_t shard_col0, shard_ncol;                    /* see rrtmg_sw_args */
  int32_t struct_size;                               /* sizeof(rrtmg_lw_args) of the caller's header: required (see rrtmg_sw_args) */
  const double *play, *plev, *tlay, *tlev, *tsfc;      /* tlev NULL: interpolated on the device from tlay, tsfc, play, plev as
                                                         * climt's get_interface_values does (util.py:89-142) */
  const double *h2ovmr, *o3vmr, *co2vmr, *ch4vmr, *n2ovmr, *o2vmr;
  const double *cfc11vmr, *cfc12vmr, *cfc22vmr, *ccl4vmr;
  const double *emis;                                /* [16][ncol] */
  const double *cldfr;
  const double *taucld;                              /* [nlay][ncol][16] */
  const double *cicewp, *cliqwp, *reice, *reliq;
  const double *tauaer;                              /* [16][nlay][ncol]; NULL -> 0 */
  const double *cldfmcl;                             /* optional [nlay][ncol][140] mask */
  double *uflx, *dflx, *hr, *uflxc, *dflxc, *hrc;
  double *duflx_dt, *duflxc_dt;                      /* idrv==1 only, [nlay+1][ncol] */
  double pressure_scale, water_path_scale, h2o_mul, h2o_div;   /* see rrtmg_sw_args */
} rrtmg_lw_args;

int rrtmg_hip_lw_fluxes(rrtmg_ctx *ctx, const rrtmg_lw_args *a);

/* Longwave fluxes BY BAND (see rrtmg_sw_band_fluxes): [16][nrow][ncol], band index 0..15 = bands 1..16, what the reference's
 * rtrn / rtrnmc / rtrnmr return for istart = iend = band, iout = band.  The surface-temperature derivatives (idrv) have no
 * per-band output. */
typedef struct rrtmg_lw_band_fluxes {
  int32_t struct_size;                 /* sizeof(rrtmg_lw_band_fluxes) of the caller's header: required */
  int32_t levels;                      /* 0: [16][nlay+1][ncol]   1: [16][2][ncol] (surface, top) */
  double *up, *dn, *upc, *dnc;         /* all-sky / clear-sky upward / downward flux, W m^-2; NULL = not wanted */
} rrtmg_lw_band_fluxes;
/* rrtmg_hip_lw_fluxes plus the requested band fluxes: the rules of rrtmg_hip_sw_fluxes_bands. */
int rrtmg_hip_lw_fluxes_bands(rrtmg_ctx *ctx, const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *b);

/* ---- shortwave and longwave of one host state in one call ------------------------------- */
/* A host caller (memspace 0) that computes both spectra of the same state says so with this call instead of two separate
 * ones.  The outputs are bit for bit those of rrtmg_hip_sw_fluxes*(sw ...) followed by rrtmg_hip_lw_fluxes*(lw ...) on the
 * same arguments, every optional output included; what differs is the schedule:
 *  - an input that both structs give as the SAME host pointer, with the same element count and the same unit factors (play,
 *    plev, tlay, the gases, the cloud arrays of a model state), crosses to the device once.  Inside one call the caller's
 *    arrays cannot change, so an identical pointer is identical content; nothing is shared across calls, and anything that
 *    differs in pointer, count or factor is uploaded on its own, as by the separate calls;
 *  - the shortwave runs on the context's stream, the longwave on its second stream: the two solves overlap on the GPU, and
 *    each spectrum's outputs come down while the other still computes.  The call returns when both are complete.
 * Every check of the separate entry points is made, for both spectra, before anything is enqueued; on top, with
 * RRTMG_ERR_ARG: both memspace must be 0 (device-resident callers have deferred mode, rrtmg_hip_set_deferred), ncol and nlay
 * must agree, and so must shard_col0 / shard_ncol.  The column sort never applies (it is for device pointers).  Work pending
 * from deferred mode is collected first: its error, if any, is what the call returns, and nothing of the call has run then.
 * Status: the shortwave's if the shortwave fails, else the longwave's; when one spectrum fails the other's outputs are still
 * complete and correct, the context stays usable, and rrtmg_hip_last_error names the spectrum.
 * sw and lw are required; the optional members are those of rrtmg_hip_sw_fluxes_surface and rrtmg_hip_lw_fluxes_bands (NULL, or
 * a struct without a member set: not requested).  RRTMG_HIP_ABI_VERSION is unchanged: probe for the symbol. */
typedef struct rrtmg_radiation_call {
  int struct_size;                       /* sizeof(rrtmg_radiation_call) */
  const rrtmg_sw_args *sw;               /* required */
  const rrtmg_sw_surface *sw_surface;    /* optional, as in rrtmg_hip_sw_fluxes_surface */
  const rrtmg_sw_components *sw_components;
  const rrtmg_sw_band_fluxes *sw_bands;
  const rrtmg_lw_args *lw;               /* required */
  const rrtmg_lw_band_fluxes *lw_bands;
} rrtmg_radiation_call;
int rrtmg_hip_radiation_fluxes(rrtmg_ctx *ctx, const rrtmg_radiation_call *call);
/* The last rrtmg_hip_radiation_fluxes call of the context: arrays_shared = inputs taken from what the call had already
 * brought to the device; bytes_uploaded = host-to-device bytes the call copied; bytes_shared = bytes it did not copy because
 * of that (an array that was filled on the device, or absent, counts 0 in both).  RRTMG_ERR_ARG before any such call. */
int rrtmg_hip_radiation_last(rrtmg_ctx *ctx, int *arrays_shared, long long *bytes_uploaded, long long *bytes_shared);

/* ---- float32 boundary: the flux calls on single-precision arrays ------------------------------- */
/* The three calls above for a caller that keeps its state in 4-byte reals.  They take the SAME structs; what changes is what the
 * pointers point to.  RRTMG_HIP_ABI_VERSION is unchanged: probe for the symbols (dlsym), as for rrtmg_hip_sw_fluxes_components.
 *  - In an _f32 call every pointer member that holds a grid array points to float: all state, cloud, aerosol, albedo, coszen, emis,
 *    tsfc and cldfmcl inputs, albdir / albdif of rrtmg_sw_surface, and every output of the argument, components and band structs.
 *    Element counts and layouts are unchanged; the arrays need only 4-byte alignment, under either memspace.
 *  - bndsolvar, indsolvar and the by-value doubles (adjes, scon, solcycfrac, the unit factors) stay double.
 *  - Precision is chosen per call, by the entry point; there is no switch on the context that a later call could forget (an fp64
 *    kernel would read twice past a float buffer).  fp64 and _f32 calls may alternate freely on one context.
 *  - Result: the same bits as the fp64 entry point called on the inputs converted float -> double (exact), with each output
 *    rounded once to float, to nearest-even (what numpy.astype(float32) does), results in the subnormal range included.  The
 *    arithmetic is fp64: no kernel that does physics is another one.
 *  - Unit factors (host arrays only, as in the fp64 calls) are applied in fp64 after the widening: double(x) * mul, then / div,
 *    one rounding per operation.
 *  - The caller's input arrays are never modified, and nothing is written outside the n * 4 bytes of an output.
 *  - Everything that modifies a call composes with unchanged meaning: deferred mode, rrtmg_hip_set_sw_night_skip / _night_pack,
 *    rrtmg_hip_set_column_sort, rrtmg_hip_set_sw_clear_sky / _lw_clear_sky (NULL clear-sky outputs included), shard_col0 /
 *    shard_ncol, both McICA generators and an external cldfmcl, idrv, levels 0 / 1.
 *  - The argument checks, their order and their status codes are those of the fp64 entry points (rrtmg_hip_sw_fluxes_surface,
 *    rrtmg_hip_lw_fluxes_bands, rrtmg_hip_radiation_fluxes); surface, c and b may be NULL.
 *  - Cost.  Device pointers (memspace 1): one widen launch for all inputs in front of the call and one narrow launch for all
 *    requested outputs behind it, on the call's stream, and an internal fp64 copy of inputs and outputs (grow-only work buffers of
 *    the context).  Host pointers: an input crosses as 4 n bytes and is widened on the device, an output is narrowed on the device
 *    and comes down as 4 n bytes -- half the PCIe traffic of the fp64 call.  A uniform array is detected by its 4-byte pattern and
 *    filled on the device; "all zero" means every element is +0.0f (a -0.0f makes the array present, as -0.0 does).
 *  - The joint call shares an input under the same key as rrtmg_hip_radiation_fluxes plus the element type, and
 *    rrtmg_hip_radiation_last reports the bytes actually copied (4 per element).
 * Not covered (fp64 only): the reference-compatible symbols, rrtmg_hip_mcica_mask, the zenith-angle, slab-surface and glue calls. */
int rrtmg_hip_sw_fluxes_f32(rrtmg_ctx *ctx, const rrtmg_sw_args *a, const rrtmg_sw_surface *surface, const rrtmg_sw_components *c,
                            const rrtmg_sw_band_fluxes *b);
int rrtmg_hip_lw_fluxes_f32(rrtmg_ctx *ctx, const rrtmg_lw_args *a, const rrtmg_lw_band_fluxes *b);
int rrtmg_hip_radiation_fluxes_f32(rrtmg_ctx *ctx, const rrtmg_radiation_call *call);

/* sub-column generators on their own (mcica_subcol_gen_{sw,lw}.f90); host pointers.
 * which: 0 = SW (112 sub-columns), 1 = LW (140).  cldfmcl out: [nlay][ncol][ngpt] of 0/1. */
int rrtmg_hip_mcica_mask(rrtmg_ctx *ctx, int which, int ncol, int nlay, int icld, int permuteseed,
                         int irng, const double *play, const double *cldfrac, double *cldfmcl);

/* ---- McICA: exponential and exponential-random cloud overlap (opt-in; not in the reference) ------------------------------
 * icld 1, 2, 3 are the reference's random, maximum-random and maximum overlap.  Maximum-random overlap treats a contiguous cloud
 * deck as perfectly correlated however deep it is and so underestimates total cloud cover.  Exponential overlap lets the rank
 * correlation of adjacent layers decay, alpha = exp(-dz / L) for a decorrelation length L; its exponential-random variant makes
 * cloud blocks separated by clear air independent.  While rank correlations are set for a spectrum, a McICA call of that
 * spectrum with icld = 4 (exponential) or 5 (exponential-random) and cldfmcl == NULL generates its sub-column mask on the
 * device as follows, with either irng.  Only the mask changes: the solves consume mask bits as ever.
 *
 * Definition, for one column and one sub-column g, layers l = 0 .. L-1 from the surface up:
 *  - cf_l = cldfr[l], set to 0 where < 1e-20 (the generators' cldmin rule).
 *  - The sub-column consumes 2 L draws, in the order x_0, y_0, x_1, y_1, ..., x_{L-1}, y_{L-1}; y_0 is drawn and unused.  A draw
 *    becomes a real number as in the generator's other modes (kissvec: kiss * 2.328306e-10 + 0.5; Mersenne twister: getRandomReal).
 *  - alpha_l = alpha[l][col] of the array set below; row 0 is ignored; values are used as given, with no clamp.
 *      icld = 4: a_l = alpha_l;      icld = 5: a_l = 0 if cf_{l-1} == 0, else alpha_l.
 *  - Ranks: c_0 = x_0; for l >= 1, c_l = c_{l-1} if y_l < a_l (strictly), otherwise c_l = x_l.
 *  - Bit l of the mask is set iff c_l >= 1 - cf_l (the comparison of the other modes).
 * Stream positions: kissvec -- sub-column g of a column starts changeSeed + g * 2 L draws into that column's stream; Mersenne
 * twister -- the one stream is ordered (sub-column, column, layer, {x, y}), and a shard (shard_col0 / shard_ncol) skips
 * shard_col0 * 2 L draws per sub-column, so that shards reproduce the whole grid bit for bit.
 *
 * rrtmg_hip_set_mcica_overlap_alpha: which = 0 shortwave, 1 longwave, 2 both; alpha [nlay][ncol] under memspace 0 (host) or 1
 * (device); alpha = NULL clears the setting (ncol, nlay, memspace are then ignored).  The array is COPIED into a buffer of the
 * context: host memory before the call returns, device memory in order on the stream the spectrum's calls run on -- the caller
 * may reuse its array at once, and sets it again when the state changes.  A sharded caller sets its block's columns: the shape
 * is that of the flux call.
 *  - While set: a flux call of that spectrum with icld 4 or 5 and mcica = 0 returns RRTMG_ERR_ARG (there is no non-McICA
 *    exponential overlap), and so does one whose ncol, nlay differ from the stored shape; nothing is enqueued and the context
 *    stays usable.  icld 0..3 behaves as without the setting.  rrtmg_hip_mcica_mask with icld 4 or 5 returns the exponential
 *    mask (shape mismatch: RRTMG_ERR_ARG).  With an external cldfmcl the rank correlations are not read.
 *  - While not set (the default): nothing changes -- a flux call resets icld > 3 to 2 as the reference does, and
 *    rrtmg_hip_mcica_mask answers RRTMG_ERR_ICLD.  The reference-compatible symbols below never see the setting: it belongs to
 *    a context, and they reset icld > 3 before the call.
 *  - The column sort and the day-column pack gather the rank correlations with the call's other inputs; deferred mode, the
 *    night-column skip, the joint call and the float32 boundary (alpha itself stays double) compose unchanged.
 * rrtmg_hip_overlap_alpha: alpha [nlay][ncol] from mid-layer pressure and temperature, one streaming kernel: row 0 is 1; for
 * l >= 1, alpha_l = exp(-dz_l / decorrelation_m) with dz_l = rd_over_g * 0.5 * (T_l + T_{l-1}) * ln(p_{l-1} / p_l) -- the
 * hypsometric distance of the two mid-layer pressures, rd_over_g = gas constant of dry air / gravity (m K^-1).  memspace as in
 * the flux calls; with device pointers the kernel is enqueued on the main stream (deferred mode: the call returns at once).
 * Probe for both by symbol; the argument structs and RRTMG_HIP_ABI_VERSION are unchanged. */
int rrtmg_hip_set_mcica_overlap_alpha(rrtmg_ctx *ctx, int which, int ncol, int nlay, int memspace, const double *alpha);
int rrtmg_hip_overlap_alpha(rrtmg_ctx *ctx, int ncol, int nlay, int memspace, const double *play, const double *tlay,
                            double rd_over_g, double decorrelation_m, double *alpha);

/* ---- shortwave between radiation calls: interval-mean zenith, flux rescale (OPT-IN) ------------- */
/* A model that calls the radiation every few steps (Hogan & Hirahara 2016; Manners et al. 2009) hands the call the cosine of
 * the zenith angle averaged over the SUNLIT part of the interval the call stands for, and rescales the call's fluxes and heating
 * rates at every step by that step's own insolation: dst = src * (mean * fraction of the step) / (mean of the call).
 *
 * rrtmg_hip_mean_coszen: sibling of rrtmg_hip_zenith_angle (memspace, deferred mode and status codes as there) for the interval
 * t0 < t1 in Julian centuries, 12 hours at the most -- anything else, t1 <= t0 included, returns RRTMG_ERR_ARG.  The sun's
 * position (as rrtmg_hip_zenith_angle forms it) is evaluated on the host at t0, t1 and the midpoint: sin_dec, cos_dec of the
 * midpoint; g0 = gmst(t0) - ra(t0), the hour angle of Greenwich at t0; D = ((gmst(t1) - ra(t1)) - g0) mod 2 pi in (0, 2 pi), its
 * advance.  One thread per column: A = sin(lat) sin_dec, B = cos(lat) cos_dec (cos(lat) = 0 at latitude +-90 degrees exactly);
 * h0 = g0 + lon reduced to [-pi, pi), h1 = h0 + D; H = acos(clamp(-A / B, -1, 1)), the sunset hour angle (pi or 0 by the sign
 * of A where B = 0).  The sunlit set is [h0, h1] n U_k [-H + 2 pi k, H + 2 pi k], k = -1, 0, 1: up to TWO pieces (an interval
 * that spans a short polar-summer night).  S = the pieces' total length, I = sum over the pieces [a, b] of
 * A (b - a) + B (sin b - sin a), every operation rounded on its own.
 *   sunlit_fraction[i] = S / D
 *   coszen_mean[i]     = S > 0 ? I / S : 0, clamped to [0, 1]
 *   zenith_mean[i]     = acos(coszen_mean[i]), and pi/2 (1.5707963267948966, what the night-column skip tests against) where
 *                        coszen_mean is 0: the zenith angle to hand the shortwave call of the interval       (may be NULL)
 *   insolation[i]      = coszen_mean[i] * sunlit_fraction[i], the interval-mean insolation factor I / D      (may be NULL)
 * rrtmg_hip_mean_coszen_sun is the same kernel for a caller with a sun of its own (another orbit, a fixed declination): the four
 * host-side numbers are arguments; hour_angle_advance outside (0, 2 pi) returns RRTMG_ERR_ARG.
 *
 * rrtmg_hip_scale_columns: dst[r][c] = src[r][c] * s[c], s[c] = den[c] > 0 ? num[c] / den[c] : +0.0, for up to 16 arrays
 * [rows][ncol] in ONE launch -- everything a shortwave call returned.  A column with s = 0 is written as +0.0 whatever src
 * holds (never -0.0, never NaN * 0).  dst == src scales in place; else the two must not overlap.  DEVICE pointers only (num,
 * den and every src / dst; `entries` itself is a host array, copied before the call returns), on the context's main stream; in
 * deferred mode the call returns once enqueued.  nentries outside 1..16, a NULL array or rows <= 0 return RRTMG_ERR_ARG.
 * Probe for the three by symbol; the argument structs and RRTMG_HIP_ABI_VERSION are unchanged. */
int rrtmg_hip_mean_coszen(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, double t0_centuries,
                          double t1_centuries, double *coszen_mean, double *sunlit_fraction, double *zenith_mean, double *insolation);
int rrtmg_hip_mean_coszen_sun(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, double sin_dec,
                              double cos_dec, double hour_angle0, double hour_angle_advance, double *coszen_mean, double *sunlit_fraction,
                              double *zenith_mean, double *insolation);
typedef struct rrtmg_scale_entry {
  const double *src;   /* [rows][ncol] */
  double *dst;         /* [rows][ncol]; == src: in place */
  int32_t rows;
  int32_t reserved;    /* 0 */
} rrtmg_scale_entry;
#define RRTMG_SCALE_MAX_ENTRIES 16
int rrtmg_hip_scale_columns(rrtmg_ctx *ctx, int ncol, const double *num, const double *den, int nentries, const rrtmg_scale_entry *entries);

/* ---- longwave between radiation calls: surface-temperature flux adjustment (OPT-IN) ------------- */
/* The consumer of idrv = 1: a model that calls the longwave every few steps corrects the kept upward fluxes at every step for
 * the surface temperature of that step (the comment on idrv in rrtmg_lw_rad; Hogan & Bozzo 2015), and forms the heating rates
 * again.  By column, dT = tsfc_now - tsfc_call:
 *   uflx_out[l] = uflx[l] + duflx_dt[l] * dT                          l = 0..nlay; the product rounded, then the sum
 *   hr_out[k]   = heatfac * ((uflx_out[k] - dflx[k]) - (uflx_out[k+1] - dflx[k+1])) / (plev[k] - plev[k+1])      k = 0..nlay-1
 * -- the expression and the order of the flux call's own heating rate, heatfac that of rrtmg_hip_lw_init (before it:
 * RRTMG_ERR_NOT_INITIALISED); pressure_scale as in rrtmg_lw_args (0: plev is in mbar; else every plev is multiplied by it first,
 * then the difference taken, as the flux call does) -- here with device pointers too.  dT = 0 returns the bits of uflx and of the
 * hr the flux call wrote.  The same for the clear-sky stream where uflxc, dflxc, duflxc_dt, uflxc_out and hrc_out are given (all
 * five, or none: the call of rrtmg_hip_set_lw_clear_sky(ctx, 0) has none).  dflx and dflxc are only read.  FIRST ORDER in dT, and
 * not clamped: the neglected term is about 0.5 % of the correction per kelvin in the window bands.
 * DEVICE pointers only.  uflx_out may be uflx, uflxc_out may be uflxc (in place: the launch then gives each column to one
 * thread); any other overlap of an output with an input or another output returns RRTMG_ERR_ARG, as do a struct_size other than
 * sizeof(rrtmg_lw_adjust), ncol or nlay <= 0, a NULL array of the all-sky stream and a clear-sky stream given in part.  One
 * launch on the stream of the longwave flux call (deferred mode: the longwave's own stream, and the call returns once enqueued;
 * consumers on the main stream order themselves behind it with rrtmg_hip_order_streams(ctx, 1)); otherwise the call waits.
 * Probe for it by symbol; the argument structs of the flux calls and RRTMG_HIP_ABI_VERSION are unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay;
  const double *tsfc_call, *tsfc_now;                 /* [ncol] */
  const double *plev; double pressure_scale;          /* [nlay+1][ncol] */
  const double *uflx, *dflx, *duflx_dt;               /* [nlay+1][ncol] */
  const double *uflxc, *dflxc, *duflxc_dt;            /* all three NULL: no clear-sky stream */
  double *uflx_out, *hr_out, *uflxc_out, *hrc_out;    /* uflx_out may be uflx (in place); hr [nlay][ncol] */
} rrtmg_lw_adjust;
int rrtmg_hip_lw_adjust_surface(rrtmg_ctx *ctx, const rrtmg_lw_adjust *a);

/* ---- dry convective adjustment: the step behind the radiation in a radiative-convective column ------------- */
/* climt's DryConvectiveAdjustment (dry_convection/component.py), by column; level 0 is the surface.  ONE sweep k = nlay-1 .. 0:
 *   theta_q[m] = t[m] * pow(pref / pmid[m], rd_cp[m]) * (1 + q[m] * (rv / rd) - q[m]),  rd_cp = (rd (1-q) + rv q) / (cpd (1-q) + cvap q)
 *   scan m = k .. nlay-1 with the running sum of theta_q in that order: theta_avg = sum / (m - k + 1); the highest m > k with
 *   theta_avg > theta_q[m] (strictly) is the top of the unstable run; where there is one, the layers k .. top are mixed:
 *     mean_q     = sum(q dp) / (pint[k] - pint[top+1]),   dp[m] = pint[m] - pint[m+1]
 *     cp_mixed   = cpd (1 - mean_q) + cvap mean_q,        rdcp_mixed = (rd (1 - mean_q) + rv mean_q) / cp_mixed
 *     mean_theta = sum((cpd (1-q) + cvap q) t dp) / sum(cp_mixed pow(pmid / pref, rdcp_mixed) dp)
 *     q[m] = mean_q,  t[m] = mean_theta * pow(pmid[m] / pref, rdcp_mixed)
 * -- the reference's order of operations, every one rounded on its own; what one sweep leaves unadjusted stays so.  A column
 * is one thread's: about 2 nlay pow and nlay^2 / 2 additions, whatever the profile.
 * t, q, pmid [nlay][ncol] and pint [nlay+1][ncol] under memspace 0 (host) or 1 (device); pref in the units of pmid and pint
 * (only ratios and differences of pressures enter).  t_out may be t and q_out may be q (in place); any other overlap of an
 * output with an input or another output returns RRTMG_ERR_ARG, as do a struct_size other than sizeof(rrtmg_dry_adjust),
 * ncol or nlay <= 0, a memspace other than 0 and 1, a NULL t, q, pmid, pint, t_out or q_out, and cpd, rd or pref <= 0 -- before
 * anything is read or enqueued.  mixed_top (may be NULL): [ncol], the highest layer a mixing wrote, -1 where the column was
 * left alone (its t_out, q_out then have the bits of t, q).  Needs neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Work space:
 * two [nlay][ncol] arrays of the context.  Host pointers: four arrays go up, two (and mixed_top) come back.  Device pointers:
 * one launch on the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  const double *t, *q, *pmid;                         /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  double cpd, cvap, rd, rv, pref;
  double *t_out, *q_out;                              /* [nlay][ncol]; t_out may be t, q_out may be q (in place) */
  int32_t *mixed_top;                                 /* [ncol], or NULL */
} rrtmg_dry_adjust;
int rrtmg_hip_dry_adjustment(rrtmg_ctx *ctx, const rrtmg_dry_adjust *a);

/* ---- simple boundary layer: bulk surface fluxes and implicit diffusion, the atmosphere's side of the slab ---- */
/* climt's SimpleBoundaryLayer (simple_boundary_layer/component.py with _core/tridiagonal.py), by column; level 0 is the surface,
 * interface i (0 .. nlay-2) lies between the layers i and i+1 at pint[i+1].  In the reference's order of operations:
 *   x_int = 0.5 (x[i+1] + x[i]);  rho[i] = pint[i+1] / (rd (1 + 0.608 q_int) t_int);
 *   theta_v[i] = t_int pow(p0 / pint[i+1], rd / cp) (1 + 0.608 q_int), the surface's from ts, ps, qs;
 *   z[i] = z[i-1] + (rd (1 + 0.608 q[i]) t[i] / g) log(pint[i] / pint[i+1]), the first term with ps;  wind[i] = max(|(u, v)_int|, 1)
 *   Ri_a = g z[0] (theta_v[0] - theta_v_s) / (theta_v_s wind[0]^2);  C = karman^2 / log(z[0] / z0)^2 where Ri_a < 0, that times
 *   (1 - Ri_a / ric)^2 where Ri_a < ric, else 0;  the top: the first i with g z[i] (theta_v[i] - theta_v[0]) / (theta_v[0] wind[i]^2) > ric,
 *   count = i + 1 and h = z[i]; where there is none, count = 0 and h = z[nlay-2] (the reference's z[-1]): no layer diffuses, the
 *   surface exchange still acts.  diff[i < count] by the K-profile: K_b(z) = karman wind[0] sqrt(C) z, damped by
 *   1 + (Ri_a / ric) log(z / z0) / (1 - Ri_a / ric) where Ri_a > 0, below fb h; K_b(fb h) z / (fb h) (1 - (z - fb h) / ((1 - fb) h))^2 above.
 *   Backward-Euler diffusion of t, q, u, v: off-diagonals g^2 rho^2 diff dt / dp_mid / dp_int, Thomas sweeps with divisions.
 *   bulk = rho[0] C wind[0], beta = g bulk dt / (pint[0] - pint[1]).  flux_mode 0 (none): no surface term.  1 (bulk): beta on
 *   diag[0] and beta ts, beta qs, 0, 0 on rhs[0].  2 (external): g dt sh_in / (cp dp0) and g dt lh_in / (lv dp0) on rhs[0] of t and
 *   q; the winds keep beta on diag[0].  Diagnostics (each may be NULL): height = h, stress_north = bulk v_out[0], stress_east =
 *   bulk u_out[0] (in every mode; advisory in mode 0), sh_out = cp bulk (ts - t_out[0]), lh_out = lv bulk (qs - q_out[0]).
 * t and q share one matrix, u and v one; the elimination runs once per distinct matrix with all right-hand sides -- the same
 * operands in the same order as four separate solves.  A column is one thread's: about nlay log and pow and 5 nlay divisions.
 * Pressures: pmid and pint are read as p * pressure_scale, ps as ps * ps_scale -- Pa per unit of the arrays, 1.0 where they hold
 * Pa (rho and the off-diagonals need Pa: the rule is not unit-free).  Arrays under memspace 0 (host) or 1 (device).  Each of
 * t_out, q_out, u_out, v_out may be exactly its own input (in place); any other overlap of an output with an input or another
 * output returns RRTMG_ERR_ARG, as do a NULL struct, a struct_size other than sizeof(rrtmg_boundary_layer), ncol <= 0, nlay < 2
 * (the reference indexes an empty array with one layer), a memspace other than 0 and 1, a flux_mode outside 0 .. 2, a NULL input
 * or profile output, a NULL sh_in or lh_in in mode 2 (they are ignored otherwise), a dt, constant or scale that is not positive,
 * and fb outside (0, 1) -- before anything is read or enqueued.  Needs neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Work
 * space: two [nlay-1][ncol] arrays of the context.  Host pointers: the inputs go up, the four profiles and the diagnostics asked
 * for come back.  Device pointers: one launch on the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace, flux_mode;
  const double *t, *q, *u, *v, *pmid;                 /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  const double *ps, *ts, *qs;                         /* [ncol] */
  const double *sh_in, *lh_in;                        /* [ncol]; required in mode 2, ignored otherwise */
  double dt;
  double rd, cp, g, lv, karman, z0, fb, p0, ric;
  double pressure_scale, ps_scale;
  double *t_out, *q_out, *u_out, *v_out;              /* [nlay][ncol]; each may be its own input (in place) */
  double *stress_north, *stress_east, *height, *sh_out, *lh_out;   /* [ncol]; each may be NULL */
} rrtmg_boundary_layer;
int rrtmg_hip_boundary_layer(rrtmg_ctx *ctx, const rrtmg_boundary_layer *a);

/* ---- Emanuel moist convection: what condenses and rains out the water the boundary layer brings up ---- */
/* climt's EmanuelConvection (emanuel/component.py around convect43c.f90), by column, in the order of operations of the reference's
 * numpy statement emanuel/pure_python.py (_convect, _tlift); level 0 is the surface.  The component's configuration: IPBL = 0 (no
 * dry-adjustment block), no tracers, NL = nlay - 3, MINORIG = minorig.  With P = pmid * pressure_scale and PH = pint * pressure_scale
 * in hPa:
 *   GZ, CPN, H, LV, HM, TV of the levels 0 .. NL; IHMIN = the level >= minorig - 1 of minimum HM below its lower neighbour's, capped
 *   at NL - 1; NK = the level of maximum HM in minorig - 1 .. IHMIN.  iflag 0, cbmf_out = 0: t[NK] < 250, q[NK] <= 0 or IHMIN == NL - 1.
 *   RH = q[NK] / qs[NK], CHI = t[NK] / (1669 - 122 RH - t[NK]), PLCL = P[NK] pow(RH, CHI).  iflag 2, cbmf_out = 0: PLCL < 200 or
 *   PLCL >= 2000.  ICB = the first level above NK with P < PLCL, at most NL - 1.  iflag 3, cbmf_out = 0: ICB >= NL - 1.
 *   The parcel of NK lifted to ICB: a dry adiabat below, at ICB two Newton steps on saturation with es = 6.112 exp(17.67 tc /
 *   (243.5 + tc)) where tc >= 0 and exp(23.33086 - 6111.72784 / T + 0.15215 log T) below.  iflag 0, cbmf_out = cbmf UNTOUCHED:
 *   cbmf == 0 and TVP[ICB] <= TV[ICB] - dtmax.  Otherwise iflag 1: the parcel lifted to NL; the precipitation efficiency from elcrit and
 *   tlcrit; the level of neutral buoyancy INB, cape, FRAC; cbmf_out = max((1 - damp dt / delt0) cbmf + 0.1 alpha DTMA, 0), DTMA the
 *   sub-cloud buoyancy excess.  cbmf_out == 0 and cbmf == 0: iflag 1 with zero tendencies.  Otherwise the mass fluxes M[ICB+1 .. INB], the
 *   mixing fractions SIJ of every origin i and destination j in ICB .. INB (a denominator of magnitude below 0.01 is set to 0.01) and,
 *   where 0 < SIJ < 0.9, the entrained q, u, v, condensate and mass (QENT, UENT, VENT, ELIJ, MENT), normalised over the spectrum of
 *   every origin; where EP[INB] >= 1e-4 the unsaturated downdraft (rain above 273 K with omtrain, coeffr; snow with omtsnow, coeffs;
 *   area sigd, fraction outside the cloud sigs) and precip; wd, tprime, qprime; the tendencies of the levels 0 .. INB, iflag 4 where a
 *   mass flux violates 2 g (0.01 / dPH) AMP1 < 1 / dt; the dp-weighted means of cpn ft + lv fq, fu and fv subtracted; fu, fv times
 *   1 - cu.  Every operation is rounded on its own; the rule is reproduced with its quirks, not improved.
 * A column is one thread's: O((INB - ICB)^2) work where it convects, one pass over the levels where it leaves early.
 * t, q, u, v, pmid [nlay][ncol], pint [nlay+1][ncol] and cbmf [ncol] under memspace 0 (host) or 1 (device).  pressure_scale: hPa per
 * unit of pmid and pint -- 1.0 for mbar, 0.01 for Pa (the 1000 hPa of the LCL, the PLCL limits and the downdraft constants make the
 * rule not unit-free).  qs [nlay][ncol] may be NULL: the kernel then forms the reference's bolton_q_sat(t, 100 P, rd, rv) =
 * (rd / rv) es / (100 P - (1 - rd / rv) es), es = 611.2 exp(17.67 (t - 273.15) / (t - 29.65)).
 * Outputs: ft [K/s], fq [1/s], fu, fv [m/s^2] [nlay][ncol], zero above INB and where nothing convects; cbmf_out [ncol], which may be
 * exactly cbmf (in place).  Each of precip [mm/day], wd [m/s], tprime [K], qprime, cape [J/kg] [ncol], iflag (int32) [ncol] and
 * ft_per_day [nlay][ncol] (= 86400 ft) may be NULL.  Any overlap of an output with an input or another output other than cbmf_out ==
 * cbmf returns RRTMG_ERR_ARG, as do a NULL struct, a struct_size other than sizeof(rrtmg_emanuel), ncol <= 0, nlay < 4 (NL >= 1: the
 * cap NL - 1 of IHMIN must be a level; with fewer than 6 layers every column leaves by one of the first exits), a memspace other than
 * 0 and 1, a NULL t, q, u, v, pmid, pint, cbmf, ft, fq, fu, fv or cbmf_out, a dt, pressure_scale, cpd, rd, rv or g that is not positive,
 * minorig < 1 and cu, sigd or sigs outside [0, 1] (the reference's ValueError) -- before anything is read or enqueued.  Needs neither
 * rrtmg_hip_sw_init nor rrtmg_hip_lw_init.
 * Work space, of the context: 8 (22 (nlay + 1) + 6 (nlay - 4) (nlay - 3)) bytes per column -- 22 one-dimensional slabs and the six
 * two-dimensional ones cut to the origins 2 .. NL and destinations 1 .. NL that can ever be written; 169 600 bytes per column at 61
 * layers.  It is sized per chunk of whole 64-column tiles against the context's scratch budget (RRTMG_HIP_MAX_SCRATCH_BYTES, default an
 * eighth of the device's memory; RRTMG_HIP_CHUNK_TILES, where given, caps the chunk too) and re-used by the chunks, one launch each;
 * results do not depend on the chunking.  Host pointers: the inputs go up, the tendencies, cbmf_out and the diagnostics asked for
 * come back.  Device pointers: the launches go to the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  const double *t, *q, *u, *v, *pmid;                 /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  const double *cbmf;                                 /* [ncol] */
  const double *qs;                                   /* [nlay][ncol], or NULL: formed by the kernel */
  double dt, pressure_scale;
  int32_t minorig, reserved;                          /* reserved: 0 */
  double elcrit, tlcrit, entp, sigd, sigs, omtrain, omtsnow, coeffr, coeffs, cu, beta, dtmax, alpha, damp, delt0;
  double cpd, cpv, cl, rv, rd, lv0, g, rowl;
  double *ft, *fq, *fu, *fv;                          /* [nlay][ncol] */
  double *precip, *wd, *tprime, *qprime, *cape;       /* [ncol]; each may be NULL */
  int32_t *iflag;                                     /* [ncol], or NULL */
  double *ft_per_day;                                 /* [nlay][ncol], or NULL */
  double *cbmf_out;                                   /* [ncol]; may be cbmf (in place) */
} rrtmg_emanuel;
int rrtmg_hip_emanuel_convection(rrtmg_ctx *ctx, const rrtmg_emanuel *a);

/* ---- simple physics: large-scale condensation, surface fluxes and boundary-layer mixing (Reed and Jablonowski 2012) ---- */
/* climt's SimplePhysics (simple_physics/component.py around simple_physics_custom.f90), by column; level 0 is the surface (the
 * reference runs top-down and its binder flips the levels), interface i lies below layer i at pint[i].  The three processes are
 * time-split in this order, each behind its switch (a switch is on where it is 1), in the reference's order of operations:
 *   epsilo = rair / rh2o, zvir = rh2o / rair - 1;  za = rair / g t[0] (1 + zvir q[0]) 0.5 (log(ps) - log(pint[1])) of the state as given.
 *   do_lsc: by layer qsat = epsilo 610.78 / pmid exp(-latvap / rh2o (1 / t - 1 / 273.16)); where q > qsat,
 *   tmp = 1 / dt (q - qsat) / (1 + (latvap / cpair) (epsilo latvap qsat / (rair t t))), t += latvap / cpair tmp dt, q -= tmp dt and
 *   precl += tmp (pint[i] - pint[i+1]) / (g rhow), summed from the model top downwards.
 *   do_surf_flux, on layer 0: wind = |(u, v)|, Cd = cd0 + cd1 wind below 20 m/s and cm from there; u, v /= 1 + Cd wind dt / za;
 *   rho = pmid / (rair t), F = c_heat wind (Tsurf - t), sh_out = rho cpair F, t += F rho g / (pint[0] - pint[1]) dt; then with rho of
 *   the new t: F = c_heat wind (qsats - q), lh_out = latvap rho F, q += F rho g / (pint[0] - pint[1]) dt.  Tsurf is ts where
 *   use_ts_ext is 1; else the moist baroclinic wave's latitude-dependent surface temperature where test is 1 (lat is taken as
 *   radians) and 302.15 K otherwise.  qsats is qsurf where use_qsurf_ext is 1, else epsilo es / (ps - 0.378 es) with the
 *   reference's two fits of es (over water where Tsurf > 271, over ice otherwise), whose constants are the doubles of
 *   single-precision literals.  lh_out is written as it comes out, negative over dew, unless clamp_latent_heat_flux is set: then
 *   lh < 0 ? 0 : lh (a NaN stays one); q has taken the negative flux either way.  Without do_surf_flux sh_out and lh_out are +0.0.
 *   do_pbl: Km = Cd wind za and Ke = c_heat wind za at every interface with pint >= pbltop, times
 *   exp(-(pbltop - pint)^2 / pblconst^2) above; rho = pint / (rair (t[i-1] + t[i]) / 2); backward-Euler diffusion of u, v (Km)
 *   and q, theta = t pow(1e5 / pmid, rair / cpair) (Ke): off-diagonals (1 / dp_int) dt g g K rho rho / dp_mid, the elimination from
 *   the surface upwards and the back-substitution downwards, t recovered layer by layer with the reference's own pow calls.
 *   do_pbl without do_surf_flux reads diffusivities the reference never set: RRTMG_ERR_ARG.
 * A column is one thread's: about nlay exp and divisions for the condensation, 3 nlay pow, nlay exp and 10 nlay divisions for the
 * mixing.  Pressures: pmid and pint are read as p * pressure_scale, ps as ps * ps_scale -- Pa per unit of the arrays, 1.0 where
 * they hold Pa (the saturation formulas, the densities and pbltop need Pa: the rule is not unit-free).  Arrays under memspace 0
 * (host) or 1 (device).  Each of t_out, q_out, u_out, v_out may be exactly its own input (in place); any other overlap of an
 * output with an input or another output returns RRTMG_ERR_ARG, as do a NULL struct, a struct_size other than
 * sizeof(rrtmg_simple_physics), ncol <= 0, nlay < 1, a memspace other than 0 and 1, a NULL t, q, u, v, pmid, pint, ps or profile
 * output, and a NULL ts, qsurf or lat where the switches have it read (ts: do_surf_flux and use_ts_ext; qsurf: do_surf_flux and
 * use_qsurf_ext; lat: do_surf_flux, no use_ts_ext and test 1; each is ignored and may be NULL otherwise) -- before anything is read
 * or enqueued.  precl, sh_out and lh_out may each be NULL.  Needs neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Work space:
 * two [nlay][ncol] arrays of the context.  Host pointers: the inputs go up, the four profiles and the diagnostics asked for come
 * back.  Device pointers: one launch on the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  int32_t do_lsc, do_pbl, do_surf_flux, use_ts_ext, use_qsurf_ext, test, clamp_latent_heat_flux, reserved;   /* reserved: 0 */
  const double *t, *q, *u, *v, *pmid;                 /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  const double *ps, *ts, *qsurf, *lat;                /* [ncol]; ts, qsurf, lat may be NULL where unread */
  double dt;
  double g, cpair, rair, latvap, rh2o, radius, omega, rhow, pbltop, pblconst, c_heat, cd0, cd1, cm;
  double pressure_scale, ps_scale;
  double *t_out, *q_out, *u_out, *v_out;              /* [nlay][ncol]; each may be its own input (in place) */
  double *precl, *sh_out, *lh_out;                    /* [ncol]; each may be NULL */
} rrtmg_simple_physics;
int rrtmg_hip_simple_physics(rrtmg_ctx *ctx, const rrtmg_simple_physics *a);

/* ---- gray radiation: the Frierson optical depth, the gray longwave sweep, grid-scale condensation ---- */
/* climt's Frierson06LongwaveOpticalDepth (_components/radiation.py), by column; level 0 is the surface:
 *   tau_0 = tau0e + (tau0p - tau0e) sin(lat pi / 180)^2;  sigma = pint / ps;  tau = tau_0 (1 - (fl sigma + (1 - fl) sigma^4)),
 * 0 at the surface and tau_0 at the top, as the reference has it.  pint is read as pint * pressure_scale, ps as ps * ps_scale (only
 * their ratio enters).  lat in degrees north.  Arrays under memspace 0 (host) or 1 (device).  tau may overlap no input.
 * RRTMG_ERR_ARG: a NULL struct, a struct_size other than sizeof(rrtmg_frierson_optical_depth), ncol <= 0, nlay < 1, a memspace
 * other than 0 and 1, a NULL pint, ps, lat or tau, tau over an input -- before anything is read or enqueued.  Needs neither
 * rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Host pointers: the inputs go up, tau comes back.  Device pointers: one launch on the
 * context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  const double *pint;                                 /* [nlay+1][ncol] */
  const double *ps, *lat;                             /* [ncol] */
  double tau0e, tau0p, fl;
  double pressure_scale, ps_scale;
  double *tau;                                        /* [nlay+1][ncol] */
} rrtmg_frierson_optical_depth;
int rrtmg_hip_frierson_optical_depth(rrtmg_ctx *ctx, const rrtmg_frierson_optical_depth *a);

/* climt's GrayLongwaveRadiation (_components/radiation.py), by column, in the reference's order of operations:
 *   up[0] = sigma_sb tsfc^4;  upwards dtau = tau[k] - tau[k-1], trans = exp(-dtau), up[k] = up[k-1] trans + (sigma_sb t[k-1]^4) (1 - trans);
 *   dn[nlay] = +0.0;  downwards dn[k] = dn[k+1] trans + (sigma_sb t[k]^4) (1 - trans) with the trans of layer k.  dtau is not clamped:
 *   a depth that decreases upwards gives trans > 1, as in the reference.  net = up - dn;
 *   tend[k] = ((g / cpd) (net[k+1] - net[k])) / (pint[k+1] - pint[k]) in K/s, pint read as pint * pressure_scale (Pa per unit);
 *   hr = tend * 86400.0 in K/day.
 * frierson 0: tau [nlay+1][ncol] is read; ps and lat are ignored and may be NULL.  frierson 1 (the fused call): tau is ignored and
 * may be NULL; the optical depth of every interface is formed inside the sweep from pint, ps and lat by the rule of
 * rrtmg_hip_frierson_optical_depth (tau0e, tau0p, fl, ps_scale as there) and is written only where tau_out is given -- every output
 * has the bits of rrtmg_hip_frierson_optical_depth followed by a frierson 0 call on its tau.  One launch, two passes over the column;
 * the transmittance is not stored in an array of its own: the upward pass carries it in dn and the emission in tend, which the
 * downward pass overwrites.  hr and tau_out may each be NULL.  No output may overlap an input or another output.
 * RRTMG_ERR_ARG: a NULL struct, a struct_size other than sizeof(rrtmg_gray_longwave), ncol <= 0, nlay < 1, a memspace other than 0
 * and 1, a frierson other than 0 and 1, a NULL t, tsfc, pint, up, dn or tend, a NULL ps or lat with frierson 1, a NULL tau with
 * frierson 0, any overlap of an output -- before anything is read or enqueued.  Needs neither rrtmg_hip_sw_init nor
 * rrtmg_hip_lw_init.  Host pointers: the inputs that are read go up, the outputs asked for come back.  Device pointers: one launch
 * on the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  int32_t frierson, reserved;                         /* reserved: 0 */
  const double *t;                                    /* [nlay][ncol] */
  const double *tsfc;                                 /* [ncol] */
  const double *pint, *tau;                           /* [nlay+1][ncol]; tau may be NULL with frierson 1 */
  const double *ps, *lat;                             /* [ncol]; each may be NULL with frierson 0 */
  double tau0e, tau0p, fl, sigma_sb, g, cpd;
  double pressure_scale, ps_scale;
  double *up, *dn;                                    /* [nlay+1][ncol] */
  double *tend;                                       /* [nlay][ncol] */
  double *hr;                                         /* [nlay][ncol], or NULL */
  double *tau_out;                                    /* [nlay+1][ncol], or NULL */
} rrtmg_gray_longwave;
int rrtmg_hip_gray_longwave(rrtmg_ctx *ctx, const rrtmg_gray_longwave *a);

/* climt's GridScaleCondensation (_components/grid_scale_condensation.py), by column and layer from the surface up:
 *   es = 611.2 exp(17.67 (t - 273.15) / (t - 29.65)), eps = rd / rh2o, q_sat = eps es / (pmid - (1 - eps) es);  where q > q_sat:
 *   dqsat_dT = lv q_sat / (rh2o t t), condensed = (q - q_sat) / (1 + lv / cpd dqsat_dT), q_out = q - condensed, t_out = t + lv / cpd
 *   condensed and precip += condensed ((pint[k+1] - pint[k]) / (g rhow)); a layer that is not supersaturated keeps its input bits.
 * With level 0 at the surface pint[k+1] - pint[k] is negative, and so is precip (kg m^-2 in the reference's units): the
 * reference's own sign, reproduced.  No time step enters.  pmid and pint are read as p * pressure_scale, Pa per unit of the arrays.
 * Each of t_out and q_out may be exactly its own input (in place); any other overlap of an output with an input or another output
 * returns RRTMG_ERR_ARG, as do a NULL struct, a struct_size other than sizeof(rrtmg_grid_scale_condensation), ncol <= 0, nlay < 1,
 * a memspace other than 0 and 1 and a NULL t, q, pmid, pint, t_out or q_out -- before anything is read or enqueued.  precip may be
 * NULL.  Needs neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Host pointers: the inputs go up, the two profiles and precip
 * come back.  Device pointers: one launch on the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  const double *t, *q, *pmid;                         /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  double cpd, lv, rd, rh2o, g, rhow;
  double pressure_scale;
  double *t_out, *q_out;                              /* [nlay][ncol]; each may be its own input (in place) */
  double *precip;                                     /* [ncol], or NULL */
} rrtmg_grid_scale_condensation;
int rrtmg_hip_grid_scale_condensation(rrtmg_ctx *ctx, const rrtmg_grid_scale_condensation *a);

/* ---- cork: the table-driven correlated-k longwave ---- */
/* A correlated-k table of climt's cork scheme (climt/_components/cork/optics/correlated_k.py) resident on the device.  The arrays
 * of the description are host arrays in the reference's own layout; they are read during the call only.
 *   k            [ngas][nband][ngpt][nT][nP] and, where nX > 0, [nX] (the H2O axis) and, where nC > 0, [nC] (the CO2 axis);
 *                float where k_is_f32 is 1, else double.  An element counts as its value promoted to double.
 *   weights      [nband][ngpt];  planck [nband][ngpt][nT]: the Planck fraction;  t_grid [nT];  p_grid_log [nP]
 *   x_grid_log   [nX]: log(max(h2o_vmr_grid, 1e-30)), x_clip the first and the last node of h2o_vmr_grid itself; c_grid_log [nC]
 *                and c_clip likewise for the CO2 axis
 *   log_cont     [nband][nT][nP][nX]: log(max(continuum_kappa, 1e-40)), or NULL (no band-grey continuum); needs nX > 0
 * RRTMG_ERR_ARG -- before anything is uploaded -- for a NULL struct or `out`, a struct_size other than sizeof
 * (rrtmg_cork_table_desc), ngas outside 1..8, nband outside 1..32, ngpt outside 1..16, nT or nP below 2, nX or nC that is neither
 * 0 nor at least 2, nC > 0 without nX > 0, log_cont without nX > 0, a NULL array that the sizes ask for, a grid that does not
 * strictly increase or a clip interval that does not.  The handle belongs to the context: rrtmg_hip_cork_table_destroy frees it,
 * and rrtmg_hip_destroy frees what is left.  Any number of tables may be resident at once.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct rrtmg_cork_table rrtmg_cork_table;
typedef struct {
  uint32_t struct_size; int32_t ngas, nband, ngpt, nT, nP, nX, nC;
  int32_t k_is_f32, reserved;                         /* reserved: 0 */
  const void *k;
  const double *weights, *planck, *t_grid, *p_grid_log;
  const double *x_grid_log, *c_grid_log;              /* NULL where nX / nC is 0 */
  double x_clip[2], c_clip[2];
  const double *log_cont;                             /* or NULL */
} rrtmg_cork_table_desc;
int rrtmg_hip_cork_table_create(rrtmg_ctx *ctx, const rrtmg_cork_table_desc *d, rrtmg_cork_table **out);
int rrtmg_hip_cork_table_destroy(rrtmg_ctx *ctx, rrtmg_cork_table *table);

/* climt's CorkLongwaveRadiation with optics "correlated_k" and additive overlap (_components/cork/lw/component.py), by column, in
 * the reference's order of operations (rrtmg_cork.h states every rule).  Level 0 is the surface.  By layer: the brackets of t,
 * log(max(pmid, 1)) and -- where the table has the axes -- of the clipped H2O and CO2 mole fractions; the layer's gas amounts by
 * gas_rule; by band and g-point the interpolated k summed over the gases from 0.0, the continuum times the amount of gas 0, the
 * cloud depth; the Planck fraction interpolated in t times sigma_sb t^4; the upward sweep from emis times the surface source and
 * the downward one from +0.0 with trans = exp(-diffusivity tau); the g-points summed by weight from 0.0 into the per-band fluxes
 * and the bands summed from 0.0 in ascending order into up and dn;  tend = ((g / cpd) (net[k+1] - net[k])) / (pint[k+1] - pint[k])
 * in K/s, hr = tend 86400.0;  tau_band the weighted sum of the optical depths of a band, trans_band = exp(-diffusivity tau_band),
 * hr_band the heating of the band's own net flux in K/day.  One thread per column and band forms all of this in registers: no
 * array with a g-point axis exists.  pmid and pint are read as p * pressure_scale (Pa per unit).
 * gas_rule 0 (fully premixed): the amount of gas 0 is the layer's air mass |dp| / g, no gas array is read.
 * gas_rule 1 (premixed background): the same amount; gas0 is the specific humidity, which gives the H2O mole fraction
 *   q / max(q + (1 - q) m_h2o, 1e-30) of the H2O axis; gas1 is the CO2 mole fraction of the CO2 axis (read where nC > 0).
 * gas_rule 2 (per gas): gas<i> is read for every gas of the table, amount = ((gas<i> gas_scale[i]) |dp|) / g (gas_scale 1.0 is exact:
 *   water vapour).  A table with an H2O axis is refused under rules 0 and 2, one without under rule 1 where gas0 is NULL.
 * taucld [nlay][ncol][nband] may be NULL (no cloud).  hr, up_band, dn_band, tau_band, trans_band and hr_band may each be NULL.
 * No output may overlap an input or another output.
 * RRTMG_ERR_ARG: a NULL struct, a struct_size other than sizeof(rrtmg_cork_longwave), ncol <= 0, nlay < 1, a memspace other than
 * 0 and 1, reserved != 0, a gas_rule outside 0..2, a NULL table or one of another context, a NULL t, pmid, pint, tsfc, emis, up, dn or
 * tend, a NULL gas array that the table and the rule need, any overlap of an output -- before anything is read or enqueued.
 * Needs neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Host pointers: the inputs that are read go up, the outputs asked for
 * come back.  Device pointers: two launches on the context's main stream; in deferred mode the call returns once enqueued.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  int32_t gas_rule, reserved;                         /* reserved: 0 */
  const rrtmg_cork_table *table;
  const double *t, *pmid;                             /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  const double *tsfc;                                 /* [ncol] */
  const double *emis;                                 /* [nband][ncol] */
  const double *taucld;                               /* [nlay][ncol][nband], or NULL */
  const double *gas0, *gas1, *gas2, *gas3, *gas4, *gas5, *gas6, *gas7;   /* [nlay][ncol]; NULL where unread */
  double gas_scale[8];
  double m_h2o, sigma_sb, g, cpd, diffusivity, pressure_scale;
  double *up, *dn;                                    /* [nlay+1][ncol] */
  double *tend;                                       /* [nlay][ncol] */
  double *hr;                                         /* [nlay][ncol], or NULL */
  double *up_band, *dn_band;                          /* [nband][nlay+1][ncol], or NULL */
  double *tau_band, *trans_band, *hr_band;            /* [nband][nlay][ncol], or NULL */
} rrtmg_cork_longwave;
int rrtmg_hip_cork_longwave(rrtmg_ctx *ctx, const rrtmg_cork_longwave *a);

/* ---- cork: the table-driven correlated-k two-stream shortwave ---- */
/* A shortwave table of the cork scheme: k, weights, the grids and log_cont as in rrtmg_cork_table_desc, and in place of the Planck
 * fraction
 *   solar_source [nband][ngpt]: solar_source_per_gpoint, float where solar_is_f32 is 1, else double (the reference multiplies it by
 *                the earth-sun factor in the table's own element type: the call does the same)
 *   rayleigh     [nband]: rayleigh_coefficient, or NULL (no Rayleigh scattering)
 * The reference's shortwave passes no CO2 mole fraction: tables of rank 5 and 6 only, nC must be 0.  Everything else that
 * rrtmg_hip_cork_table_create refuses is refused here, and a NULL solar_source and a solar_is_f32 other than 0 and 1.  The handle
 * is of the same type, tagged by kind: rrtmg_hip_cork_table_destroy frees it; the longwave call refuses a shortwave table and the
 * shortwave call a longwave one.  Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ngas, nband, ngpt, nT, nP, nX, nC;   /* nC: 0 */
  int32_t k_is_f32, solar_is_f32;
  const void *k;
  const double *weights, *t_grid, *p_grid_log;
  const double *x_grid_log;                           /* NULL where nX is 0 */
  double x_clip[2];
  const double *log_cont;                             /* or NULL */
  const void *solar_source;
  const double *rayleigh;                             /* or NULL */
} rrtmg_cork_sw_table_desc;
int rrtmg_hip_cork_sw_table_create(rrtmg_ctx *ctx, const rrtmg_cork_sw_table_desc *d, rrtmg_cork_table **out);

/* climt's CorkShortwaveRadiation with optics "correlated_k" and additive overlap (_components/cork/sw/component.py), by column, in
 * the reference's order of operations (rrtmg_cork_sw.h states every rule).  Level 0 is the surface.  By layer, band and g-point: the
 * gas optical depth exactly as the longwave call forms it (brackets, gas_rule, continuum); with a Rayleigh coefficient tau_ray =
 * (rayleigh |dp|) / g added and ssa = tau_ray / tau; the cloud (taucld, ssacld, asycld [nlay][ncol][nband], all three or none: then
 * zeros are mixed in) mixed in by optical depth and scattering; delta-Eddington scaling; the Meador-Weaver / PIFM layer operator
 * with its floors and its two energy clamps; the direct beam from 1.0 at the top; the Shonk-Hogan adding recursion upward from
 * the surface (albedo, and the beam it reflects) and the flux recursion downward; up_band and dn_band (direct + diffuse) the sums
 * over the g-points, in ascending order from 0.0, of the flux times (solar_flux cos(zenith)) weight; up and dn the ascending band
 * sums;  tend, hr and hr_band as in the longwave call; tau_band the weighted sum of the unscaled total depths.
 * A column with cos(zenith) <= 1e-4 contributes nothing: +0.0 in every flux, the heating the formula makes of zeros; its tau_band is
 * formed all the same.  solar_flux = solar_source earth_sun[0]: the factor of the FIRST column for every column, and in a table with
 * solar_is_f32 the factor rounded to float and the product a float product; both are formed on the device from earth_sun.
 * One thread per column and band; the beam, the combined albedo and the combined source of every (g-point, level) go through a
 * work space of the context of at most 512 MiB: the columns are run in chunks that fit (max_chunk_cols > 0: in chunks of at most
 * that many columns; 0: the library's choice).  Chunking changes no bit.
 * RRTMG_ERR_ARG: what rrtmg_hip_cork_longwave refuses (of its own arrays: a NULL t, pmid, pint, zenith, albedo, earth_sun, up, dn or
 * tend); a longwave table; a table with a CO2 axis; one or two of the three cloud arrays; max_chunk_cols < 0 -- before anything is
 * read or enqueued.  Host and device pointers as in the longwave call; per chunk one launch, then the band reduction.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  int32_t gas_rule, max_chunk_cols;                   /* max_chunk_cols: 0, or the most columns of a chunk */
  const rrtmg_cork_table *table;
  const double *t, *pmid;                             /* [nlay][ncol] */
  const double *pint;                                 /* [nlay+1][ncol] */
  const double *zenith, *albedo, *earth_sun;          /* [ncol]; zenith in radians */
  const double *taucld, *ssacld, *asycld;             /* [nlay][ncol][nband], all three or all NULL */
  const double *gas0, *gas1, *gas2, *gas3, *gas4, *gas5, *gas6, *gas7;   /* [nlay][ncol]; NULL where unread */
  double gas_scale[8];
  double m_h2o, g, cpd, pressure_scale;
  double *up, *dn;                                    /* [nlay+1][ncol] */
  double *tend;                                       /* [nlay][ncol] */
  double *hr;                                         /* [nlay][ncol], or NULL */
  double *up_band, *dn_band;                          /* [nband][nlay+1][ncol], or NULL */
  double *tau_band, *hr_band;                         /* [nband][nlay][ncol], or NULL */
} rrtmg_cork_shortwave;
int rrtmg_hip_cork_shortwave(rrtmg_ctx *ctx, const rrtmg_cork_shortwave *a);

/* ---- sea ice and land ice: one implicit snow/ice column ---- */
/* climt's SeaIce (kind 0, _components/sea_ice/component.py) and LandIce (kind 1, _components/land_ice/component.py), by column,
 * with their shared Crank-Nicolson solver and Thomas sweep, in the reference's order of operations.  nlay counts the ice
 * interface levels (nodes): node 0 is the base and node nlay-1 the surface; at least 3.
 *   active: kind 0 area_type == 3 (sea_ice) && thick > 0 && thick + snow >= eps;  kind 1 area_type 0 (land) or 1 (land_ice) and
 *   thick + snow >= eps.  net = sw_down + lw_down - sw_up - lw_up - sh - lh.  base: kind 0 the ocean heat flux (the base is a flux
 *   boundary at -base), kind 1 the soil surface temperature (a Dirichlet base).  The top is held at t_melt where t[nlay-1] >=
 *   t_melt - eps; where the flux conducted to the surface then exceeds net, the column is solved again with a flux top.  Melt
 *   energy is rounded to 1e-6 (half-even) and clamped at 0; melt eats the snow first, then the ice.
 *   base_flux_out: kind 0 the heat flux to the sea water, rounded to 1e-6, plus what a negative thickness leaves over (the
 *   thickness is then an exact 0.0); kind 1 the upward ground flux (t_out[0] - t_out[1]) kappa[0] / dz, thickness and snow clamped at
 *   0.0.  height_out[j] = (thick_out + snow_out) j / (nlay - 1).  tsfc_out = t_out[nlay-1].  cond_flux: kind 0 the flux conducted
 *   to the surface, kind 1 +0.0.  albedo: albedo_snow where snow is left, else albedo_ice; albedo_melt where anything melted.
 * A column that is not active keeps the bits of t, height, thick and snow, gets tsfc_out = t[nlay-1], base_flux_out = base (kind 0)
 * and +0.0 for every other diagnostic.  A column that would be active and is taller than max_height is left as inactive and
 * flagged (the reference raises).  flags: bit 0 active, bit 1 negative melt energy was clamped, bit 2 taller than max_height.
 * cond_flux, albedo and flags may each be NULL.  In place: t_out == t, height_out == height, thick_out == thick, snow_out ==
 * snow and, for kind 0 only, base_flux_out == base -- exactly; any other overlap of an output with an input or another output
 * returns RRTMG_ERR_ARG, as do a NULL struct, a struct_size other than sizeof(rrtmg_surface_ice), ncol <= 0, nlay < 3, a memspace
 * other than 0 and 1, a kind other than 0 and 1, reserved != 0, dt <= 0, a NULL required array and base_flux_out == base with kind 1
 * -- before anything is read or enqueued.  Needs neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init.  Host pointers: the inputs go up,
 * the outputs asked for come back.  Device pointers: one launch on the context's main stream; in deferred mode the call returns
 * once enqueued.  The four radiative fluxes are [ncol] rows: the surface row of a resident [level][ncol] array is such a pointer.
 * Probe for it by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  int32_t kind, reserved;                             /* kind: 0 sea ice, 1 land ice; reserved: 0 */
  const double *t, *height;                           /* [nlay][ncol]; height is read for the columns that are not active only */
  const double *thick, *snow, *base;                  /* [ncol]; base: kind 0 the ocean heat flux, kind 1 the soil temperature */
  const double *sw_down, *lw_down, *sw_up, *lw_up, *lh, *sh;   /* [ncol] */
  const int32_t *area_type;                           /* [ncol]: 0 land, 1 land_ice, 2 sea, 3 sea_ice */
  double dt;
  double rho_ice, rho_snow, c_ice, c_snow, k_ice, k_snow, lf, t_melt, eps, max_height, albedo_snow, albedo_ice, albedo_melt;
  double *t_out, *height_out;                         /* [nlay][ncol]; each may be its own input (in place) */
  double *thick_out, *snow_out, *tsfc_out;            /* [ncol]; thick_out and snow_out may be their own inputs */
  double *base_flux_out;                              /* [ncol]; kind 0: may be base */
  double *cond_flux, *albedo;                         /* [ncol], or NULL */
  int32_t *flags;                                     /* [ncol], or NULL */
} rrtmg_surface_ice;
int rrtmg_hip_surface_ice(rrtmg_ctx *ctx, const rrtmg_surface_ice *a);

/* ---- the land surface: BucketHydrology and SecondBEST ---- */
/* Both components read only the lowest model level of the atmosphere and the surface level of the four radiative fluxes, so
 * every atmospheric and flux array is [ncol]: a caller with resident [level][ncol] arrays passes the address of row 0.
 * pressure_scale (and ps_scale): Pa per unit of p_air (of ps).  Physical constants and component parameters are scalars of the
 * structs.  Both entries need neither rrtmg_hip_sw_init nor rrtmg_hip_lw_init; host pointers: the inputs go up, the outputs asked
 * for come back; device pointers: one launch on the context's main stream, in deferred mode the call returns once enqueued.  An
 * output may be exactly its own input (in place); any other overlap of an output with an input or another output is refused.
 * Probe for them by symbol; RRTMG_HIP_ABI_VERSION is unchanged. */

/* climt's BucketHydrology (_components/bucket_hydrology/component.py), by column, in the reference's order of operations.  Every
 * array is [ncol] and nlay must be 1 (the struct has no profile; anything else is refused).  layers: 1 or 2.
 *   wind = sqrt(v v + u u);  rho = p_air / (rd t_air);  potential = rho bulk_coefficient wind (q_sfc - q_air);  precip = precip_conv +
 *   precip_strat;  beta = soil_moisture / (beta_parameter soil_moisture_max) where soil_moisture <= beta_parameter soil_moisture_max,
 *   else 1;  mass flux = beta potential;  evaporation = mass flux / rho_water;  lh = lv mass flux;  sh = rho cp bulk_coefficient wind
 *   (ts - t_air);  net = sw_down + lw_down - sw_up - lw_up - sh - lh.
 *   layers 1: the moisture tendency is precip - evaporation where soil_moisture < soil_moisture_max or precip <= evaporation, else 0;
 *   ts_out = ts + net / (density thickness heat_capacity) dt;  soil_moisture_out = min(soil_moisture + tendency dt, soil_moisture_max).
 *   layers 2: exchange F = (w_s / S_s - w_d / S_d) (0.5 (S_s + S_d)) / tau_m, drainage D = w_d / tau_drain where has_drain (else 0),
 *   overflow of either layer is runoff, both layers are clipped to [0, S]; the skin and the deep store (deep_ratio times as thick)
 *   exchange heat by conduction with k_soil = 2.0.  deep_moisture and deep_temperature and their outputs are required then, and
 *   not read or written with layers 1 (they may be anything); runoff and deep_fraction likewise.
 * precip, lh, sh, evaporation, runoff and deep_fraction may each be NULL.  Every column is stepped: the reference does not look
 * at the area type here.  RRTMG_ERR_ARG: a NULL struct, a struct_size other than sizeof(rrtmg_bucket_hydrology), ncol <= 0, nlay != 1,
 * a memspace other than 0 and 1, a NULL required array, dt <= 0, layers other than 1 and 2, reserved != 0 and, with layers 2,
 * tau_m <= 0 or a NULL two-layer array -- before anything is read or enqueued. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  int32_t layers, has_drain, reserved, reserved2;     /* layers: 1 or 2; has_drain: whether tau_drain is read; reserved: 0 */
  const double *t_air, *q_air, *u, *v, *p_air;        /* [ncol]: the lowest model level */
  const double *ts, *q_sfc;                           /* [ncol] */
  const double *sw_down, *lw_down, *sw_up, *lw_up;    /* [ncol]: the surface level */
  const double *soil_moisture, *precip_conv, *precip_strat, *density, *thickness, *heat_capacity;   /* [ncol] */
  const double *deep_moisture, *deep_temperature;     /* [ncol]; layers 2 only */
  double dt, rd, cp, rho_water, lv, bulk_coefficient, beta_parameter, soil_moisture_max, deep_soil_moisture_max, tau_m, deep_ratio, tau_drain;
  double pressure_scale;
  double *ts_out, *soil_moisture_out;                 /* [ncol]; each may be its own input */
  double *deep_moisture_out, *deep_temperature_out;   /* [ncol]; layers 2 only; each may be its own input */
  double *precip, *lh, *sh, *evaporation;             /* [ncol], or NULL */
  double *runoff, *deep_fraction;                     /* [ncol], or NULL; layers 2 only */
} rrtmg_bucket_hydrology;
int rrtmg_hip_bucket_hydrology(rrtmg_ctx *ctx, const rrtmg_bucket_hydrology *a);

/* climt's SecondBEST (_components/second_best/) with its five default processes, by column, in the reference's order of
 * operations.  nlay counts the soil interface levels (nodes): node 0 is the bottom and node nlay-1 the surface; at least 2.
 *   active: area_type 0 (land) or 1 (land_ice).  wind = max(sqrt(u u + v v), min_wind);  rho = p_air / (rd t_air);  z_mid =
 *   max(((rd t_air) / g) log(ps / p_air), 2.0);  z0 = 0.01 (land) or 0.001 (land_ice).  Drag: C_DN = (karman / (log z_mid - log z0))^2,
 *   zeta = exp(-karman / sqrt(C_DN)), Ri = -((g z_mid) / (ts U U)) (ts - t_air) with U = max(wind, 1e-3); Ri < 0 is the unstable
 *   branch (56.768 for momentum, 41.801 for heat), otherwise the stable one with eps = 0.01.  Soil: texture 0.07 and wilting point
 *   0.01 over land_ice; porosity = 0.6 - 0.03 texture; W_Lu = x_w[nlay-1] / porosity, W_Fu = x_i[nlay-1] / porosity.  Albedo: 0.60 + 0.06
 *   (1 - W_Lu) over land_ice, else (0.10 + 0.1 colour) + 0.06 (1 - W_Lu).  q_sat: Bolton, at ts and p_air.  Fluxes: sh = rho cp wind
 *   C_Dh (ts - t_air); E_P = rho (C_Dh wind) (q_sat - q_air); Theta = clip((W_Lu - 0.01) / max(1 - W_Fu, 1e-6), 1e-3, 1); K_HD =
 *   (-4 K_H0 B psi_0 rho_water porosity (1 - W_Fu)) / (pi dt); E_max = K_HD Theta^(0.5 B + 2) - K_H0 Theta^(2 B + 3); beta =
 *   clip(W_Fu lv / (lv + lf) + (|E_P| > 1e-12 ? clip(E_max / E_P, 0, 1) : 0), 0, 1); evaporation = beta E_P / rho; lh = lv rho
 *   evaporation.  net = sw_down + lw_down - sw_up - lw_up - sh - lh.  Soil column: dz = |height[1] - height[0]|, r = kappa_soil dt /
 *   (cv_soil dz dz); the tridiagonal system has -r on both off-diagonals, 1 + 2 r on the diagonal and 1 + r in its first and last
 *   row; the right-hand side is t_soil with net dt / (cv_soil dz) added at the surface; Thomas sweep; freeze/melt Gamma = (cv_soil /
 *   lf) (t_freeze - T) / dt limited to [-rho_water x_i / dt, rho_water x_w / dt]; x_i += Gamma dt / rho_water, x_w -= the same, both
 *   clamped at 0; T += lf Gamma dt / cv_soil; where net <= 0, T = min(T, t_freeze).  ts_out = t_soil_out[nlay-1]; snow_out = snow.
 *   t2m, q2m (from the effective surface humidity beta q_sat + (1 - beta) q_air) and the 10 m wind follow the reference's
 *   interpolate_to_height; u10 = v10 = +0.0 where sqrt(u u + v v) is exactly 0.
 * A column that is not active keeps the bits of every output's input (untouched when in place) and gets +0.0 in every diagnostic
 * and 0 in flags.  flags: bit 0 active, bit 1 the unstable branch, bit 2 net <= 0 (the cap at t_freeze applies).  Every
 * diagnostic may be NULL.  RRTMG_ERR_ARG: a NULL struct, a struct_size other than sizeof(rrtmg_second_best), ncol <= 0, nlay < 2, a
 * memspace other than 0 and 1, a NULL required array, dt <= 0 and reserved != 0 -- before anything is read or enqueued. */
typedef struct {
  uint32_t struct_size; int32_t ncol, nlay, memspace;
  const double *t_soil, *x_w, *x_i, *height;          /* [nlay][ncol] */
  const double *t_air, *q_air, *u, *v, *p_air;        /* [ncol]: the lowest model level */
  const double *ps, *ts, *snow;                       /* [ncol] */
  const double *sw_down, *lw_down, *sw_up, *lw_up;    /* [ncol]: the surface level */
  const int32_t *area_type;                           /* [ncol]: 0 land, 1 land_ice, 2 sea, 3 sea_ice */
  double dt, rd, g, cp, lv, lf, rho_water, karman, t_freeze, min_wind, kappa_soil, cv_soil;
  double colour, texture, B, K_H0, psi_0;             /* the soil type, resolved by the caller */
  double pressure_scale, ps_scale;
  int32_t reserved, reserved2;                        /* 0 */
  double *t_soil_out, *x_w_out, *x_i_out;             /* [nlay][ncol]; each may be its own input */
  double *ts_out, *snow_out;                          /* [ncol]; each may be its own input */
  double *sh, *lh, *evaporation, *albedo_direct, *albedo_diffuse, *cd_heat, *cd_momentum, *t2m, *q2m, *u10, *v10;   /* [ncol], or NULL */
  int32_t *flags;                                     /* [ncol], or NULL */
} rrtmg_second_best;
int rrtmg_hip_second_best(rrtmg_ctx *ctx, const rrtmg_second_best *a);

/* ---- reference-compatible entry points (host pointers, default context) ---------------- */
int rrtmg_hip_default_status(void);
const char *rrtmg_hip_default_error(void);

void rrtmg_sw_set_constants(double *pi, double *grav, double *planck, double *boltz, double *clight,
                            double *avogad, double *alosmt, double *gascon, double *sbcnst, double *secdy);
void rrtmg_sw_ini_wrapper(double *cpdair);
void mcica_subcol_sw_wrapper(int32_t *iplon, int32_t *ncol, int32_t *nlay, int32_t *icld,
                             int32_t *permuteseed, int32_t *irng, double *play, double *cldfrac,
                             double *ciwp, double *clwp, double *rei, double *rel, double *tauc,
                             double *ssac, double *asmc, double *fsfc, double *cldfmcl,
                             double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl,
                             double *taucmcl, double *ssacmcl, double *asmcmcl, double *fsfcmcl);
void rrtmg_sw_mcica_wrapper(int32_t *ncol, int32_t *nlay, int32_t *icld, int32_t *iaer, double *play,
                            double *plev, double *tlay, double *tlev, double *tsfc, double *h2ovmr,
                            double *o3vmr, double *co2vmr, double *ch4vmr, double *n2ovmr, double *o2vmr,
                            double *asdir, double *asdif, double *aldir, double *aldif, double *coszen,
                            double *adjes, int32_t *dyofyr, double *scon, int32_t *isolvar,
                            int32_t *inflgsw, int32_t *iceflgsw, int32_t *liqflgsw, double *cldfmcl,
                            double *taucmcl, double *ssacmcl, double *asmcmcl, double *fsfcmcl,
                            double *ciwpmcl, double *clwpmcl, double *reicmcl, double *relqmcl,
                            double *tauaer, double *ssaaer, double *asmaer, double *ecaer,
                            double *swuflx, double *swdflx, double *swhr, double *swuflxc,
                            double *swdflxc, double *swhrc, double *bndsolvar, double *indsolvar,
                            double *solcycfrac);
void rrtmg_sw_nomcica_wrapper(int32_t *ncol, int32_t *nlay, int32_t *icld, int32_t *iaer, double *play,
                              double *plev, double *tlay, double *tlev, double *tsfc, double *h2ovmr,
                              double *o3vmr, double *co2vmr, double *ch4vmr, double *n2ovmr, double *o2vmr,
                              double *asdir, double *asdif, double *aldir, double *aldif, double *coszen,
                              double *adjes, int32_t *dyofyr, double *scon, int32_t *isolvar,
                              int32_t *inflgsw, int32_t *iceflgsw, int32_t *liqflgsw, double *cldfr,
                              double *taucld, double *ssacld, double *asmcld, double *fsfcld,
                              double *cicewp, double *cliqwp, double *reice, double *reliq,
                              double *tauaer, double *ssaaer, double *asmaer, double *ecaer,
                              double *swuflx, double *swdflx, double *swhr, double *swuflxc,
                              double *swdflxc, double *swhrc, double *bndsolvar, double *indsolvar,
                              double *solcycfrac);

void rrtmg_set_constants(double *pi, double *grav, double *planck, double *boltz, double *clight,
                         double *avogad, double *alosmt, double *gascon, double *sbcnst, double *secdy);
void rrtmg_lw_set_constants(double *pi, double *grav, double *planck, double *boltz, double *clight,
                            double *avogad, double *alosmt, double *gascon, double *sbcnst, double *secdy);
void rrtmg_lw_ini_wrapper(double *cpdair);
void mcica_subcol_lw_wrapper(int32_t *iplon, int32_t *ncol, int32_t *nlay, int32_t *icld,
                             int32_t *permuteseed, int32_t *irng, double *play, double *cldfrac,
                             double *ciwp, double *clwp, double *rei, double *rel, double *tauc,
                             double *cldfmcl, double *ciwpmcl, double *clwpmcl, double *reicmcl,
                             double *relqmcl, double *taucmcl);
void rrtmg_lw_mcica_wrapper(int32_t *ncol, int32_t *nlay, int32_t *icld, int32_t *idrv, double *play,
                            double *plev, double *tlay, double *tlev, double *tsfc, double *h2ovmr,
                            double *o3vmr, double *co2vmr, double *ch4vmr, double *n2ovmr, double *o2vmr,
                            double *cfc11vmr, double *cfc12vmr, double *cfc22vmr, double *ccl4vmr,
                            double *emis, int32_t *inflglw, int32_t *iceflglw, int32_t *liqflglw,
                            double *cldfmcl, double *taucmcl, double *ciwpmcl, double *clwpmcl,
                            double *reicmcl, double *relqmcl, double *tauaer, double *uflx, double *dflx,
                            double *hr, double *uflxc, double *dflxc, double *hrc, double *duflx_dt,
                            double *duflxc_dt);
void rrtmg_lw_nomcica_wrapper(int32_t *ncol, int32_t *nlay, int32_t *icld, int32_t *idrv, double *play,
                              double *plev, double *tlay, double *tlev, double *tsfc, double *h2ovmr,
                              double *o3vmr, double *co2vmr, double *ch4vmr, double *n2ovmr, double *o2vmr,
                              double *cfc11vmr, double *cfc12vmr, double *cfc22vmr, double *ccl4vmr,
                              double *emis, int32_t *inflglw, int32_t *iceflglw, int32_t *liqflglw,
                              double *cldfr, double *taucld, double *cicewp, double *cliqwp,
                              double *reice, double *reliq, double *tauaer, double *uflx, double *dflx,
                              double *hr, double *uflxc, double *dflxc, double *hrc, double *duflx_dt,
                              double *duflxc_dt);

#ifdef __cplusplus
}
#endif
#endif /* RRTMG_HIP_H */
