// rrtmg_call.h -- the host steps that a shortwave and a longwave flux call have in common (private to rrtmg_sw.hip and
// rrtmg_lw.hip; host code only: no kernel lives here, and the kernels launched here are those of rrtmg_mcica_kernels.h).
// In the order of a call: the gate to the sorted call, the argument checks, the call's stream, the walks of the array tables, the
// chunk plan, the error flag, the McICA mask, the chunk loop, the epilogue, the tail of a permuted call -- and every walk of the
// call's array tables (rrtmg_call_arrays.h): input registration, output binding, gathers and scatter, widen and narrow.  The
// drivers keep what differs: the rules of their inputs, work buffers and the kernels of every launch stage with their geometry.
// which: 0 shortwave, 1 longwave -- the index of rrtmg_ctx::hint, plans, pending, kiss_* and of the err_dev slot.
#pragma once
#include "rrtmg_call_arrays.h"
#include "rrtmg_ctx.h"
#include "rrtmg_mcica_kernels.h"
#include "rrtmg_permute.h"

namespace rrtmg {

struct CallSite { rrtmg_ctx *ctx; int which; hipStream_t s; };
// ---- entry gate ---------------------------------------------------------------------------------------------------------------
inline bool spectrum_ready(const rrtmg_ctx *ctx, int which) { return which == 0 ? ctx->sw_ready : ctx->lw_ready; }
// The call runs sorted (rrtmg_permute.h): opt-in, device pointers, clouds, at least two tiles, kissvec or no McICA, and not
// the inner call itself.  excluded: what the spectrum never sorts (outputs that would need a scatter, inputs a gather, of their own;
// in the shortwave a second positional input besides the twister's stream: amplitudes indsolvar != 1, rescaled once per column)
template <class Args>
inline bool call_is_sorted(const rrtmg_ctx *ctx, int which, const Args *a, bool excluded) {
  return !excluded && spectrum_ready(ctx, which) && a && ctx->sort_columns && ctx->inner == kInnerNone && a->memspace == 1 && a->icld != 0 && a->cldfr && a->ncol >= 128 && a->nlay > 0 && a->nlay <= 256 && !(a->mcica && a->irng != 0);
}
// the four argument checks every call makes, then the device (hipSetDevice, and the streams and flags where they do not exist yet)
template <class Args>
inline int call_begin(rrtmg_ctx *ctx, int which, const Args *a) {
  if (!spectrum_ready(ctx, which)) return ctx->fail(RRTMG_ERR_NOT_INITIALISED, "%s", which == 0 ? "rrtmg_hip_sw_init has not been called" : "rrtmg_hip_lw_init has not been called");
  if (!a || a->ncol <= 0 || a->nlay <= 0) return ctx->fail(RRTMG_ERR_ARG, "ncol/nlay must be positive");
  if (a->nlay > 256) return ctx->fail(RRTMG_ERR_ARG, "nlay > 256 not supported (cloud-mask words)");
  if (a->shard_ncol != 0 && (a->shard_col0 < 0 || a->shard_col0 + a->ncol > a->shard_ncol)) return ctx->fail(RRTMG_ERR_ARG, "shard_col0/shard_ncol do not contain ncol columns");
  return ctx_prepare_device(ctx);
}
// the outputs the call must be given (rrtmg_call_arrays.h: `required`, group on) are there
template <class Out, size_t n, class All>
inline int check_outputs(rrtmg_ctx *ctx, const Out (&t)[n], unsigned on, const All &x) {
  for (const Out &e : t)
    if (e.required && array_is_read(e.need, on) && !(x.*(e.m))) return ctx->fail(RRTMG_ERR_ARG, "output array is NULL");
  return RRTMG_OK;
}
// The stream rule: the shortwave is always on ctx->stream; the longwave moves to stream_lw when the call is deferred and
// device-resident, or half of a joint call (rrtmg_hip_radiation_fluxes: host pointers), so that the two spectra overlap on the
// GPU.  (After ctx_prepare_device: the streams are created there.)
inline hipStream_t call_stream(const rrtmg_ctx *ctx, int which, int memspace) { return (which == 1 && (ctx->joint || (ctx->deferred && memspace == 1))) ? ctx->stream_lw : ctx->stream; }
// the table of a joint call's inputs for HostInputs, or nullptr
inline ShareTable *call_share(const rrtmg_ctx *ctx) { return ctx->joint ? &ctx->joint->table : nullptr; }
// ---- the driver's walks of the array tables (rrtmg_call_arrays.h) ----------------------------------------------------------------
// Inputs -> HostInputs, in table order.  What is the driver's own comes as `rules`, keyed by the bound member, for the inputs
// that differ from the default: required, InPolicy::Plain, no unit factor, registered wherever the group is on.
struct InRule { bool required = true; InPolicy policy = InPolicy::Plain; double mul = 0.0, div = 0.0; bool skip = false; };
template <class Bound> struct InRuleFor { const double *Bound::*dev; InRule rule; };
template <class In, size_t n, class All, class Bound, size_t nr>
inline void register_inputs(HostInputs &hi, const In (&t)[n], unsigned on, const All &x, Bound &d, const GridShape &g, const InRuleFor<Bound> (&rules)[nr]) {
  for (const In &e : t) {
    if (!array_is_read(e.need, on)) continue;
    InRule r;
    for (const InRuleFor<Bound> &o : rules)
      if (o.dev == e.dev) r = o.rule;
    if (!r.skip) hi.add(&(d.*(e.dev)), x.*(e.m), ext_count(e.ext, e.k, g), e.name, r.required, r.policy, r.mul, r.div);
  }
}
// Outputs.  The device array of one that is read (its group on, the caller's pointer set; nullptr: the kernel skips it) is the
// caller's pointer under memspace 1, else the named work buffer (wd: the driver's allocator of doubles), which the epilogue
// downloads behind one synchronise: oc[] in table order -> the number of copies.
template <class Out, size_t n, class All, class Bound, class Wd>
inline int bind_outputs(const Out (&t)[n], unsigned on, const All &x, Bound &d, const GridShape &g, int memspace, Wd wd, OutCopy *oc) {
  int nout = 0;
  for (const Out &e : t) {
    double *const user = x.*(e.m);
    if (!user || !array_is_read(e.need, on)) continue;
    const size_t count = ext_count(e.ext, e.k, g);
    d.*(e.dev) = memspace == 1 ? user : wd(e.wname, count);
    oc[nout++] = {user, d.*(e.dev), count};
  }
  return nout;
}
// ---- chunk plan -----------------------------------------------------------------------------------------------------------------
// what the previous call found (rrtmg_ctx::CallHint): read without waiting, used for speed only; -1: another grid, or nothing yet
inline int call_hint_cloudy(const rrtmg_ctx *ctx, int which, int ntile, int nlay) {
  return (ctx->hint[which].ntile == ntile && ctx->hint[which].nlay == nlay) ? ctx->hint[which].ncloudy : -1;
}
// -> tiles per solve chunk; the chunk's tile lists in d.tcap, d.tlist, d.tcnt (d.tlist == nullptr: allocation failed).  plan_cloudy:
// the cloudy tiles to plan for (the hint, or the shortwave's night-scaled share); tile_bytes: work space per tile of a mixed grid's chunk
template <class Dev>
inline int plan_call_chunks(rrtmg_ctx *ctx, int which, Dev &d, bool clouds, int plan_cloudy, size_t tile_bytes) {
  const int ntile = (d.ncol + 63) / 64, L = d.nlay;
  int chunk_tiles = ctx->chunk_tiles;
  if (ctx->chunk_auto && L > 80 && plan_cloudy >= 0 && 10 * plan_cloudy >= 9 * ntile) chunk_tiles = 64;   // deep cloudy grid: DESIGN.md 5
  // (a sorted grid keeps the small chunks: its tiles are segregated by kind, every chunk but one is of one kind)
  chunk_tiles = ctx->plan_chunks(which, chunk_tiles, ntile, L, (clouds && ctx->inner != kInnerSorted) ? plan_cloudy : -1, tile_bytes, which == 0 ? "sw.w.scratch" : "lw.w.scratch");
  const int ctile = ntile < chunk_tiles ? ntile : chunk_tiles;
  int32_t *tlist = (int32_t *)ctx->buf(which == 0 ? "sw.w.tilelist" : "lw.w.tilelist", (size_t)(2 * ctile + 2) * 4);
  d.tcap = ctile; d.tlist = tlist; d.tcnt = tlist ? tlist + 2 * d.tcap : nullptr;
  return ctile;
}
// ---- error flag and deferred prologue ---------------------------------------------------------------------------------------------
// d.err = the spectrum's slot of err_dev.  A synchronous call owns its flag: flags of calls still pending from deferred mode are
// collected first, then the slot is cleared on the call's stream.  A deferred call (device-resident, in deferred mode) leaves
// it: the flag accumulates (atomicMax) until rrtmg_hip_synchronize collects and clears it.
template <class Dev>
inline int call_own_flag(const CallSite &c, int memspace, Dev &d) {
  rrtmg_ctx *ctx = c.ctx;
  d.err = ctx->err_dev + c.which;
  if (ctx->deferred && memspace == 1) return RRTMG_OK;
  if (ctx->pending[0] || ctx->pending[1]) { const int prc = rrtmg_hip_synchronize(ctx); if (prc) return prc; }
  RRTMG_HIP_CHECK(ctx, hipMemsetAsync(d.err, 0, sizeof(int), c.s));
  return RRTMG_OK;
}
// ---- McICA sub-column mask (d.mask) -------------------------------------------------------------------------------------------
// cldfmcl given: from the caller's sub-columns (cldfmcl_dev: their device copy); irng 0: kissvec, every thread jumping to its
// sub-column's first draw; else the Mersenne twister.  ngpt: the spectrum's g-points = sub-columns.  night_kernel, coszen: the
// shortwave's kissvec kernel that draws nothing for a night tile, with the night-column skip on.
using KissNightKernel = void (*)(int, int, int, const double *, const double *, uint64_t *, int, int *, const uint32_t *, const double *);
// Exponential and exponential-random overlap (icld 4, 5; rrtmg_hip_set_mcica_overlap_alpha): the siblings kiss_mask_exp_kernel,
// the shortwave's exp_night_kernel and mt_mask_exp_kernel, with alpha -- call_overlap's answer -- as one more input.
using KissExpNightKernel = void (*)(int, int, int, const double *, const double *, const double *, uint64_t *, int, int *, const uint32_t *, const double *);
template <class Dev, class Args>
inline int mcica_mask_launch(const CallSite &c, int ngpt, const Dev &d, const Args *a, const double *cldfmcl_dev, KissNightKernel night_kernel = nullptr, const double *coszen = nullptr,
                             const double *alpha = nullptr, KissExpNightKernel exp_night_kernel = nullptr) {
  rrtmg_ctx *ctx = c.ctx;
  const int N = d.ncol, L = d.nlay, ntile = (N + 63) / 64;
  const dim3 blk(64);
  const bool expo = d.icld >= 4;
  if (a->cldfmcl) {
    hipLaunchKernelGGL(mask_from_cldfmcl_kernel, dim3(ntile, ngpt), blk, 0, c.s, N, L, ngpt, cldfmcl_dev, d.mask, d.nw);
  } else if (expo && !alpha) {
    return ctx->fail(RRTMG_ERR_ARG, "icld %d: no rank correlations for this call", d.icld);
  } else if (expo && hipStreamWaitEvent(c.s, ctx->alpha_ev[c.which], 0) != hipSuccess) {
    // (a copy from device memory may have gone on the spectrum's other stream -- the longwave's own in deferred mode, while a
    //  host-pointer call runs on the main one: the mask step waits for it on the device, the host does not block)
    return ctx->fail(RRTMG_ERR_HIP, "hipStreamWaitEvent on the rank correlations' copy failed");
  } else if (a->irng == 0) {
    const uint32_t *jumps = kiss_jumps_device(ctx, c.which, ngpt, L, d.icld, a->permuteseed, c.s);
    if (!jumps) return ctx->status;
    if (expo && night_kernel) hipLaunchKernelGGL(exp_night_kernel, dim3(ngpt, ntile), blk, 0, c.s, N, L, d.icld, d.play, d.cldfr, alpha, d.mask, d.nw, d.err, jumps, coszen);
    else if (expo) hipLaunchKernelGGL(kiss_mask_exp_kernel, dim3(ngpt, ntile), blk, 0, c.s, N, L, d.icld, d.play, d.cldfr, alpha, d.mask, d.nw, d.err, jumps);
    else if (night_kernel) hipLaunchKernelGGL(night_kernel, dim3(ngpt, ntile), blk, 0, c.s, N, L, d.icld, d.play, d.cldfr, d.mask, d.nw, d.err, jumps, coszen);
    else hipLaunchKernelGGL(kiss_mask_kernel, dim3(ngpt, ntile), blk, 0, c.s, N, L, d.icld, d.play, d.cldfr, d.mask, d.nw, d.err, jumps);
  } else {
    return mt_mask_device(ctx, c.which, N, L, ngpt, d.icld, a->permuteseed, d.cldfr, d.mask, d.nw, a->shard_col0, a->shard_ncol, c.s, alpha);
  }
  return RRTMG_OK;
}
// The overlap rule a call runs under.  icld 4 and 5 exist only while the spectrum has rank correlations set
// (rrtmg_hip_set_mcica_overlap_alpha), and only for McICA; otherwise any icld outside 0..3 is 2, as in the reference.
template <class Args>
inline bool call_overlap_exp(const rrtmg_ctx *ctx, int which, const Args *a) { return a && (a->icld == 4 || a->icld == 5) && ctx->alpha[which].dev != nullptr; }
// the checks of such a call, in front of the gates to the permuted calls: nothing is enqueued for a call that is refused
template <class Args>
inline int call_overlap_check(rrtmg_ctx *ctx, int which, const Args *a) {
  if (ctx->inner != kInnerNone || !call_overlap_exp(ctx, which, a)) return RRTMG_OK;
  if (!a->mcica) return ctx->fail(RRTMG_ERR_ARG, "icld %d (exponential overlap) needs mcica = 1: there is no non-McICA exponential overlap", (int)a->icld);
  const rrtmg_ctx::OverlapAlpha &o = ctx->alpha[which];
  if (o.ncol != a->ncol || o.nlay != a->nlay) return ctx->fail(RRTMG_ERR_ARG, "icld %d: the rank correlations were set for %d x %d columns x layers, the call has %d x %d", (int)a->icld, o.ncol, o.nlay, (int)a->ncol, (int)a->nlay);
  return RRTMG_OK;
}
// -> the driver's icld; alpha: what the mask step reads under icld 4 and 5 (the inner call of a permuted one: the gathered copy)
template <class Args>
inline int call_overlap(const rrtmg_ctx *ctx, int which, const Args *a, const double *&alpha) {
  alpha = nullptr;
  if (call_overlap_exp(ctx, which, a)) { alpha = ctx->inner != kInnerNone ? ctx->alpha_inner[which] : ctx->alpha[which].dev; return a->icld; }
  return (a->icld < 0 || a->icld > 3) ? 2 : a->icld;
}
// ---- chunk loop -----------------------------------------------------------------------------------------------------------------
// Preparation, solve and integration, one column chunk of d.tcap tiles at a time.  Per chunk (first tile t0, nt tiles) the driver
// supplies its launches: before(t0, nt) -- preparation, McICA cloud optics, tile lists; clear(t0, nt) and cloudy(t0, nt) -- the two
// solve variants, each bracketed here by the event pair chunk_event(which | which + 2, chunk, side) of rrtmg_hip_kernel_ms;
// after(t0, nt) -- the integration launches, which find d.hint_out set in the call's last chunk.
// The variant expected to find nothing goes first, and the cloudy one is launched only with clouds (order is speed only: each tile
// belongs to exactly one of them).  A sorted grid -- rrtmg_permute.h -- has its cloud-free tiles first: the chunks in front of the
// previous call's cloudy-tile count (hint_cloudy) are expected to hold no cloudy tile.
template <class Dev, class Before, class Clear, class Cloudy, class After>
inline void run_chunks(const CallSite &c, Dev &d, bool clouds, int hint_cloudy, Before before, Clear clear, Cloudy cloudy, After after) {
  rrtmg_ctx *ctx = c.ctx;
  const int w = c.which, ntile = (d.ncol + 63) / 64, ctile = d.tcap;
  for (int t0 = 0; t0 < ntile; t0 += ctile) {
    const int nt = ntile - t0 < ctile ? ntile - t0 : ctile, ci = t0 / ctile;
    d.col0 = t0 * 64; d.pcols = ctile * 64;
    before(t0, nt);
    auto variant = [&](int k, auto &launch) { (void)hipEventRecord(ctx->chunk_event(k, ci, 0), c.s); launch(t0, nt); (void)hipEventRecord(ctx->chunk_event(k, ci, 1), c.s); };
    const bool expect_clear = clouds && hint_cloudy >= 0 && (hint_cloudy == 0 || (ctx->inner == kInnerSorted && t0 + nt <= ntile - hint_cloudy));
    if (expect_clear) { variant(w + 2, cloudy); variant(w, clear); }
    else { variant(w, clear); if (clouds) variant(w + 2, cloudy); }
    d.hint_out = t0 + ctile >= ntile ? (int32_t *)&ctx->hint[w].ncloudy : nullptr;
    after(t0, nt);
  }
  ctx->hint[w].ntile = ntile; ctx->hint[w].nlay = d.nlay;
  ctx->ev_chunks[w] = (ntile + ctile - 1) / ctile; ctx->ev_chunks[w + 2] = clouds ? ctx->ev_chunks[w] : 0;
}
// ---- epilogue: status + outputs ---------------------------------------------------------------------------------------------------
// oc[nout]: the standard outputs plus what opt_out_append added (read for a host-pointer call only).  A deferred call returns
// once enqueued, its flag pending; a host-pointer call downloads outputs and flag behind one synchronise; a synchronous
// device-resident call reads the flag.  Half of a joint call: the copies of outputs and flag are enqueued behind the
// spectrum's integration kernels and the call returns; joint_collect waits for both spectra and reads the flags.
inline int spectrum_fail(rrtmg_ctx *ctx, int which, int herr) {
  return which == 0 ? ctx->fail(herr, "shortwave: %s", status_message(herr)) : ctx->fail(herr, "longwave: %s", status_message(herr));
}
inline int call_finish(const CallSite &c, int memspace, const OutCopy *oc, int nout, int *err_dev) {
  rrtmg_ctx *ctx = c.ctx;
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (ctx->joint) return copy_out_enqueue(ctx, c.s, oc, nout, err_dev, ctx->joint->out[c.which], c.which);
  if (ctx->deferred && memspace == 1) { ctx->pending[c.which] = true; ctx->status = 0; return RRTMG_OK; }
  int herr = 0;
  if (memspace == 0) {
    if (const int rc = copy_out(ctx, c.s, oc, nout, err_dev, &herr)) return rc;
  } else {
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(&herr, err_dev, sizeof(int), hipMemcpyDeviceToHost, c.s));
    RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(c.s));
  }
  if (herr) return spectrum_fail(ctx, c.which, herr);
  ctx->status = 0;
  return RRTMG_OK;
}
// ---- the permuted call (rrtmg_permute.h: sorted or packed; what is gathered and scattered: rrtmg_call_arrays.h) -----------------
// x: the copy of the caller's structs.  Every input the call reads becomes its gathered copy (nullptr stays nullptr: an absent
// optional array), every other one nullptr; likewise the outputs, registered for the scatter.
template <class In, size_t n, class All>
inline void permute_inputs(ColumnPermute &pm, const In (&t)[n], unsigned on, All &x, const GridShape &g) {
  for (const In &e : t)
    x.*(e.m) = !array_is_read(e.need, on) ? nullptr : e.ext == Ext::LayColK ? pm.gather_elem(e.name, x.*(e.m), e.k) : pm.gather(e.name, x.*(e.m), ext_rows(e.ext, e.k, g), e.whole);
}
template <class Out, size_t n, class All>
inline void permute_outputs(ColumnPermute &pm, const Out (&t)[n], unsigned on, All &x, const GridShape &g) {
  for (const Out &e : t) x.*(e.m) = array_is_read(e.need, on) ? pm.out(e.name, x.*(e.m), ext_rows(e.ext, e.k, g)) : nullptr;
}
// The scatter cannot run before the inner call: its table must hold a call's whole output list (a band member: k entries)
template <class Out, size_t n> constexpr int scatter_entries(const Out (&t)[n]) {
  int s = 0;
  for (const Out &e : t) s += e.ext == Ext::KBandLev ? e.k : 1;
  return s;
}
static_assert(scatter_entries(kSwOut) <= kPermuteMaxEntries && scatter_entries(kLwOut) <= kPermuteMaxEntries, "kPermuteMaxEntries: one scatter table for every output");
// inner(): the spectrum's driver on the copy, which returns once it is enqueued (it finds ctx->inner set).  Behind it ONE
// scatter launch for every output registered with pm -- which also leaves the counts of rrtmg_hip_sw_night_last where
// night_out is given -- and the one epilogue: a permuted call is device-resident, so only the flag is read.
template <class Inner>
inline int permuted_tail(const CallSite &c, ColumnPermute &pm, Inner inner, int32_t *night_out = nullptr) {
  rrtmg_ctx *ctx = c.ctx;
  ctx->inner = pm.kind;
  const int rc = inner();
  ctx->inner = kInnerNone;
  ctx->alpha_inner[c.which] = nullptr;
  if (rc) return rc;
  pm.flush_scatter(night_out);
  return call_finish(c, 1, nullptr, 0, ctx->err_dev + c.which);
}
// ---- the float32 boundary of a device-resident call (rrtmg_precision.h; what is widened and narrowed: rrtmg_call_arrays.h) -------
// The caller's device arrays hold float.  in(): the internal fp64 copy of an input (nullptr stays nullptr), registered for the
// ONE widen launch; out(): the inner call's fp64 array for the caller's `user`, registered for the ONE narrow launch.  The
// copies live in named grow-only work buffers ("sw.f32.", "lw.f32.").  The inner call is the ordinary device-resident driver:
// the sort, the pack, deferred mode and every other option run inside it unchanged.
struct BoundaryF32 {
  rrtmg_ctx *ctx;
  std::string prefix;
  PrecisionBatch widen, narrow;
  bool ok = true;
  BoundaryF32(rrtmg_ctx *c, hipStream_t s, const char *pre) : ctx(c), prefix(pre), widen(s, true), narrow(s, false) {}
  double *buf(const char *name, size_t n) {
    double *p = (double *)ctx->buf(prefix + name, n * sizeof(double));
    if (!p) ok = false;
    return p;
  }
  const double *in(const char *name, const double *user, size_t n) {
    if (!user) return nullptr;
    double *p = buf(name, n);
    if (p) widen.add(user, p, n);
    return p;
  }
  double *out(const char *name, double *user, size_t n) {
    if (!user) return nullptr;
    double *p = buf(name, n);
    if (p) narrow.add(p, user, n);
    return p;
  }
};
// x: the copy of the caller's structs -- what the call reads becomes its fp64 copy, the rest nullptr (see permute_inputs)
template <class In, size_t n, class All>
inline void boundary_inputs(BoundaryF32 &bf, const In (&t)[n], unsigned on, All &x, const GridShape &g) {
  for (const In &e : t) x.*(e.m) = array_is_read(e.need, on) ? bf.in(e.name, x.*(e.m), ext_count(e.ext, e.k, g)) : nullptr;
}
template <class Out, size_t n, class All>
inline void boundary_outputs(BoundaryF32 &bf, const Out (&t)[n], unsigned on, All &x, const GridShape &g) {
  for (const Out &e : t) x.*(e.m) = array_is_read(e.need, on) ? bf.out(e.name, x.*(e.m), ext_count(e.ext, e.k, g)) : nullptr;
}
// ONE widen and ONE narrow launch: each table holds a whole list
static_assert(table_size(kSwIn) <= kPrecisionMaxEntries && table_size(kSwOut) <= kPrecisionMaxEntries && table_size(kLwIn) <= kPrecisionMaxEntries && table_size(kLwOut) <= kPrecisionMaxEntries, "kPrecisionMaxEntries");
// inner(): the fp64 driver on the copies.  It returns with its own epilogue done -- enqueued in deferred mode, else complete
// and its flag read -- and the narrow launch goes behind its last kernel (or its scatter) on the same stream; a synchronous
// call then waits for it.  A call that fails returns the inner call's status, and the caller's outputs are not written.
template <class Inner>
inline int boundary_f32_tail(const CallSite &c, BoundaryF32 &bf, Inner inner) {
  rrtmg_ctx *ctx = c.ctx;
  bf.widen.flush();
  if (const int rc = inner()) return rc;
  bf.narrow.flush();
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (!ctx->deferred) RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(c.s));
  return RRTMG_OK;
}
// ---- the joint call: both spectra of one host state in one call -----------------------------------------------------------------
// sw(), lw(): the two drivers on their checked arguments.  While ctx->joint is set they differ from separate calls in three
// places, all above: call_stream (the longwave on stream_lw), call_share (inputs the shortwave has brought to the device are
// taken, not uploaded again) and call_finish (output copies enqueued, not waited for).  So the shortwave's inputs, launches
// and copies are enqueued first, then the longwave's; each spectrum's copies run under the other's solve.  Then one wait per
// stream, the shortwave's first: its staged outputs reach the caller's arrays while the longwave still runs.  The flags are
// read behind both.  Status: the shortwave's if it failed -- at a check or on the device -- else the longwave's; the spectrum
// that did not fail has its outputs complete either way.  Work pending from deferred mode is collected first, as
// call_own_flag does for a separate call.
template <class Sw, class Lw>
inline int joint_run(rrtmg_ctx *ctx, Sw sw, Lw lw) {
  if (int rc = ctx_prepare_device(ctx)) return rc;
  if (ctx->pending[0] || ctx->pending[1]) { if (const int prc = rrtmg_hip_synchronize(ctx)) return prc; }
  JointCall j;
  ctx->joint = &j;
  int rc[2];
  std::string msg[2];
  rc[0] = sw(); msg[0] = ctx->err;
  rc[1] = lw(); msg[1] = ctx->err;
  ctx->joint = nullptr;
  hipStream_t st[2] = {ctx->stream, ctx->stream_lw};
  int hip_rc = RRTMG_OK;
  for (int w = 0; w < 2; ++w) {
    const hipError_t e = hipStreamSynchronize(st[w]);   // (also where a spectrum failed half-way: nothing of it stays in flight)
    if (e != hipSuccess && !hip_rc) hip_rc = ctx->fail(RRTMG_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    if (e == hipSuccess && !rc[w] && j.out[w].enqueued) copy_out_complete(ctx, j.out[w]);
  }
  ctx->joint_seen = true;
  ctx->joint_arrays_shared = j.table.arrays_shared(); ctx->joint_bytes_uploaded = j.table.bytes_uploaded(); ctx->joint_bytes_shared = j.table.bytes_shared();
  if (hip_rc) return hip_rc;
  for (int w = 0; w < 2; ++w) {
    if (rc[w]) { ctx->err = msg[w]; ctx->status = rc[w]; return rc[w]; }
    if (j.out[w].herr) return spectrum_fail(ctx, w, j.out[w].herr);
  }
  ctx->status = 0;
  return RRTMG_OK;
}

}  // namespace rrtmg
