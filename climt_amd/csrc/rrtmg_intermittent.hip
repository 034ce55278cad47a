// rrtmg_intermittent.hip -- the two kernels of the shortwave between radiation calls (rrtmg_intermittent.h) and their C entries:
//   rrtmg_hip_mean_coszen[_sun]   sibling of rrtmg_hip_zenith_angle (rrtmg_neighbours.hip): one thread per column, streaming,
//                                 compute-light (a handful of sin / cos / acos) and latency-hidden by occupancy
//   rrtmg_hip_scale_columns       every [rows][ncol] array a shortwave call returned times a per-column factor, ONE launch
#include "rrtmg_ctx.h"
#include "rrtmg_intermittent.h"

namespace rrtmg {

// zenith, insolation: nullptr = not requested
__global__ void __launch_bounds__(256) mean_coszen_kernel(int n, const double *lat_deg, const double *lon_deg, IntervalSun s, double *mean,
                                                          double *fraction, double *zenith, double *insolation) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const MeanCoszen r = mean_coszen_column(lat_deg[i], lon_deg[i], s);
  mean[i] = r.mean;
  fraction[i] = r.fraction;
  if (zenith) zenith[i] = mean_zenith(r.mean);
  if (insolation) insolation[i] = mean_insolation(r);
}

// grid (column tiles of 256, row groups, entries): a thread owns one column of one entry's row groups y, y + gridDim.y, ...;
// s[col] is formed once and stays in a register across them.  Columns fastest: each row is a coalesced run of 8-byte accesses
// on both sides; non-temporal (every element is read once and written once, and the next reader is another kernel).
__global__ void __launch_bounds__(256) scale_columns_kernel(ScaleTable t, const double *num, const double *den, int ncol) {
  const int col = blockIdx.x * 256 + threadIdx.x;
  const ScaleEntry e = t.e[blockIdx.z];
  if (col >= ncol || (int)blockIdx.y * kScaleRows >= e.rows) return;
  scale_thread(e, ncol, col, blockIdx.y, gridDim.y, scale_factor(num[col], den[col]));
}

static int mean_coszen_call(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, const IntervalSun &sun,
                            double *coszen_mean, double *sunlit_fraction, double *zenith_mean, double *insolation) {
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const size_t bytes = (size_t)ncol * sizeof(double);
  const double *dlat = lat_deg, *dlon = lon_deg;
  double *out[4] = {coszen_mean, sunlit_fraction, zenith_mean, insolation}, *dev[4] = {coszen_mean, sunlit_fraction, zenith_mean, insolation};
  if (memspace == 0) {
    double *a = (double *)ctx->buf("mcz.lat", bytes), *b = (double *)ctx->buf("mcz.lon", bytes), *o = (double *)ctx->buf("mcz.out", 4 * bytes);
    if (!a || !b || !o) return ctx->status;
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(a, lat_deg, bytes, hipMemcpyHostToDevice, s));
    RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(b, lon_deg, bytes, hipMemcpyHostToDevice, s));
    dlat = a; dlon = b;
    for (int k = 0; k < 4; ++k) dev[k] = out[k] ? o + (size_t)k * ncol : nullptr;
  }
  hipLaunchKernelGGL(mean_coszen_kernel, dim3((ncol + 255) / 256), dim3(256), 0, s, ncol, dlat, dlon, sun, dev[0], dev[1], dev[2], dev[3]);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (memspace == 0)
    for (int k = 0; k < 4; ++k)
      if (out[k]) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(out[k], dev[k], bytes, hipMemcpyDeviceToHost, s));
  if (ctx->deferred && memspace == 1) return RRTMG_OK;   // ordered before later shortwave work on the same stream
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}

}  // namespace rrtmg

using namespace rrtmg;

static bool mean_coszen_args_ok(int ncol, int memspace, const double *lat_deg, const double *lon_deg, const double *coszen_mean, const double *sunlit_fraction) {
  return ncol > 0 && (memspace == 0 || memspace == 1) && lat_deg && lon_deg && coszen_mean && sunlit_fraction;
}

extern "C" int rrtmg_hip_mean_coszen(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, double t0_centuries,
                                     double t1_centuries, double *coszen_mean, double *sunlit_fraction, double *zenith_mean, double *insolation) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!mean_coszen_args_ok(ncol, memspace, lat_deg, lon_deg, coszen_mean, sunlit_fraction)) return ctx->fail(RRTMG_ERR_ARG, "mean_coszen: bad argument");
  if (!interval_ok(t0_centuries, t1_centuries))
    return ctx->fail(RRTMG_ERR_ARG, "mean_coszen: an interval t0 < t1 of 12 hours at the most is served (t1 - t0 = %g days)", (t1_centuries - t0_centuries) * 36525.0);
  return mean_coszen_call(ctx, ncol, memspace, lat_deg, lon_deg, interval_sun(t0_centuries, t1_centuries), coszen_mean, sunlit_fraction, zenith_mean, insolation);
}

extern "C" int rrtmg_hip_mean_coszen_sun(rrtmg_ctx *ctx, int ncol, int memspace, const double *lat_deg, const double *lon_deg, double sin_dec,
                                         double cos_dec, double hour_angle0, double hour_angle_advance, double *coszen_mean, double *sunlit_fraction,
                                         double *zenith_mean, double *insolation) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!mean_coszen_args_ok(ncol, memspace, lat_deg, lon_deg, coszen_mean, sunlit_fraction)) return ctx->fail(RRTMG_ERR_ARG, "mean_coszen_sun: bad argument");
  const IntervalSun sun{sin_dec, cos_dec, hour_angle0, hour_angle_advance};
  if (!interval_sun_ok(sun) || !(fabs(hour_angle0) <= 1.0e6))
    return ctx->fail(RRTMG_ERR_ARG, "mean_coszen_sun: the advance of the hour angle must lie in (0, 2 pi), the hour angle be finite");
  return mean_coszen_call(ctx, ncol, memspace, lat_deg, lon_deg, sun, coszen_mean, sunlit_fraction, zenith_mean, insolation);
}

extern "C" int rrtmg_hip_scale_columns(rrtmg_ctx *ctx, int ncol, const double *num, const double *den, int nentries, const rrtmg_scale_entry *entries) {
  static_assert(sizeof(rrtmg_scale_entry) == sizeof(ScaleEntry), "rrtmg_scale_entry is the kernel's table entry");
  if (!ctx) return RRTMG_ERR_ARG;
  if (ncol <= 0 || !num || !den || !entries || nentries <= 0) return ctx->fail(RRTMG_ERR_ARG, "scale_columns: bad argument");
  if (nentries > kScaleMaxEntries) return ctx->fail(RRTMG_ERR_ARG, "scale_columns: %d entries, %d at the most in one call", nentries, kScaleMaxEntries);
  ScaleTable t{};
  int most = 0;
  for (int k = 0; k < nentries; ++k) {
    if (!entries[k].src || !entries[k].dst || entries[k].rows <= 0) return ctx->fail(RRTMG_ERR_ARG, "scale_columns: entry %d: NULL array or no rows", k);
    t.e[k] = {entries[k].src, entries[k].dst, entries[k].rows, 0};
    if (entries[k].rows > most) most = entries[k].rows;
  }
  int rc = ctx_prepare_device(ctx);
  if (rc) return rc;
  hipLaunchKernelGGL(scale_columns_kernel, dim3((ncol + 255) / 256, scale_grid_y(most), nentries), dim3(256), 0, ctx->stream, t, num, den, ncol);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  if (!ctx->deferred) RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
  return RRTMG_OK;
}
