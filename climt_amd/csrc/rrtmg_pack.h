// rrtmg_pack.h -- OPT-IN day-column packing of the shortwave (rrtmg_hip_set_sw_night_pack): day columns first, night behind.
//
// The night-column skip (rrtmg_sw.hip) saves work per 64-column TILE: a tile with one day column is solved whole.  On a grid
// with 128 longitudes every tile of every latitude row is mixed and the skip saves nothing, though half the planet is dark.
// With the pack a device-resident call (memspace 1) runs on an internal copy of its inputs of Np = 64 x (tiles + 1) slots --
// what the host can size without knowing the counts:
//   [0, nday)        the day columns, stable in the caller's order
//   [nday, ndpad)    replicas of the last day column up to the tile boundary ndpad = 64 x ceil(nday / 64): dropped at the scatter
//   [ndpad, Np)      night slots: the caller's night columns in stable order, then filler; coszen is the caller's value for a
//                    night column and 0.0 for a filler slot
// so that no tile holds both kinds and every tile behind the day block is a night tile of the existing night path, which gives
// it no work at all: the inner call is the ordinary driver with the night kernels on ncol = Np.  Night tiles read nothing but
// coszen, so the gathers leave every other array of the slots from ndpad on untouched -- but ecaer (iaer = 6), whose mixing
// pass runs over the whole grid and raises no code: it is gathered whole, zeros in the filler slots.
// Columns are independent in every routine and kissvec seeds per column (rrtmg_sort.h); the Mersenne twister's stream and
// amplitudes indsolvar != 1 are positional: such calls are not packed.
//
// Everything is on the device and on the call's stream.  The column sort pays a launch per array (up to 30 gathers and 6
// scatters: +22 % at 8192 columns); here ONE launch gathers every [rows][N] input and ONE scatters every requested output, each
// through a by-value table with one entry per blockIdx.z (an array of more than nlay + 1 rows is several entries, so that the
// entries are about equally deep and blockIdx.y has no idle tail), and one more gathers the band-fastest cloud arrays where
// they are present: 3 map launches + 1 or 2 gathers + 1 scatter around the inner call, whatever the call requests.
#pragma once
#include <string>

#include "rrtmg_ctx.h"

namespace rrtmg {

struct PackHead { int32_t nday, ndpad, last_day, pad; };   // last_day: the last day column (-1: none)

__device__ __forceinline__ bool pack_is_day(const double *coszen, int col) { return !(coszen[col] <= 0.0); }   // (NaN is day)

// one wavefront per tile: cnt[tile] = how many of the tile's columns are day
static __global__ void __launch_bounds__(64) pack_count_kernel(const double *coszen, int ncol, int32_t *cnt) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  const unsigned long long m = __ballot(col < ncol && pack_is_day(coszen, col));
  if (threadIdx.x == 0) cnt[blockIdx.x] = __popcll(m);
}

// one workgroup: exclusive prefix of the tiles' day counts (base[tile]), the totals and the last day column
static __global__ void __launch_bounds__(1024) pack_scan_kernel(const double *coszen, const int32_t *cnt, int ntile, int ncol, int32_t *base, PackHead *head) {
  __shared__ int part[1024];
  __shared__ int sh_last;
  const int t = threadIdx.x, per = (ntile + 1023) / 1024;
  if (t == 0) sh_last = -1;
  int s = 0, last = -1;
  for (int i = t * per; i < ntile && i < (t + 1) * per; ++i) { s += cnt[i]; if (cnt[i] > 0) last = i; }
  part[t] = s;
  __syncthreads();
  if (last >= 0) atomicMax(&sh_last, last);
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = t == 0 ? 0 : part[t - 1];
  for (int i = t * per; i < ntile && i < (t + 1) * per; ++i) { base[i] = run; run += cnt[i]; }
  if (t < 64) {   // the first wavefront: the highest day column of the last tile that has one
    const int tile = sh_last, col = tile * 64 + t;
    const unsigned long long m = __ballot(tile >= 0 && col < ncol && pack_is_day(coszen, col));
    if (t == 0) {
      const int nday = part[1023];
      head->nday = nday; head->ndpad = (nday + 63) / 64 * 64; head->last_day = m ? tile * 64 + 63 - __clzll((long long)m) : -1; head->pad = 0;
    }
  }
}

// one wavefront per tile of SLOTS (npad / 64 of them).  As the tile of source columns blockIdx.x: src[slot] = dst[slot] =
// column, stable within each kind; as 64 slots: the replicas behind the day block and the filler behind the night columns
// (slots no source column maps to: no two threads write one element).  src -1: a filler slot; dst -1: nothing to scatter.
static __global__ void __launch_bounds__(64) pack_map_kernel(const double *coszen, const int32_t *base, const PackHead *head, int ncol, int32_t *src, int32_t *dst) {
  const int lane = threadIdx.x, col = blockIdx.x * 64 + lane;
  const int nday = head->nday, ndpad = head->ndpad, nnight = ncol - nday;
  const bool in = col < ncol, day = in && pack_is_day(coszen, col);
  const unsigned long long md = __ballot(day), mn = __ballot(in && !day), lower = (1ull << lane) - 1ull;
  if (in) {
    const int day_before = base[blockIdx.x], night_before = blockIdx.x * 64 - day_before;
    const int slot = day ? day_before + __popcll(md & lower) : ndpad + night_before + __popcll(mn & lower);
    src[slot] = col; dst[slot] = col;
  }
  const int slot = col;
  if (slot >= nday && slot < ndpad) { src[slot] = head->last_day; dst[slot] = -1; }   // (nday > 0 here: ndpad > nday)
  else if (slot >= ndpad + nnight) { src[slot] = -1; dst[slot] = -1; }
}

// The tables of the gather and scatter launches, passed by value: one entry per blockIdx.z.
// aux: gather of [rows][N] arrays -- 1 = every slot is filled (coszen, ecaer), 0 = the slots in front of ndpad only;
//      gather of band-fastest arrays -- the elements per (row, column); scatter: unused
struct PackEntry { const double *in; double *out; int32_t rows, aux; };
constexpr int kPackMaxEntries = 104;   // 6 outputs + 8 components + 6 band members of 14 entries each (2.5 KB of kernel arguments)
struct PackTable { PackEntry e[kPackMaxEntries]; };
constexpr int kPackMaxElemEntries = 5;   // taucld, ssacld, asmcld, fsfcld, cldfmcl
struct PackElemTable { PackEntry e[kPackMaxElemEntries]; };

// in [rows][ncol] -> out [rows][npad]: a thread owns one slot, reads its source column once and keeps kPackRows rows of it in
// flight (sort_gather1_kernel's scheme).  A filler slot of an array that is filled whole gets 0.0.
constexpr int kPackRows = 8;
static __global__ void __launch_bounds__(256) pack_gather_kernel(PackTable t, const int32_t *src, const PackHead *head, int ncol, int npad) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  const PackEntry e = t.e[blockIdx.z];
  const int r0 = blockIdx.y * kPackRows;
  if (slot >= npad || r0 >= e.rows) return;
  if (!e.aux && slot >= head->ndpad) return;
  const int c = src[slot];
  double v[kPackRows];
#pragma unroll
  for (int k = 0; k < kPackRows; ++k) if (r0 + k < e.rows) v[k] = c >= 0 ? __builtin_nontemporal_load(e.in + (long)(r0 + k) * ncol + c) : 0.0;
#pragma unroll
  for (int k = 0; k < kPackRows; ++k) if (r0 + k < e.rows) __builtin_nontemporal_store(v[k], e.out + (long)(r0 + k) * npad + slot);
}
// in [rows][ncol][elem] -> out [rows][npad][elem], row = blockIdx.y, the slots in front of ndpad only
static __global__ void __launch_bounds__(256) pack_gather_elem_kernel(PackElemTable t, const int32_t *src, const PackHead *head, int ncol, int npad) {
  const PackEntry e = t.e[blockIdx.z];
  const int elem = e.aux;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if ((int)blockIdx.y >= e.rows || i >= (long)head->ndpad * elem) return;
  const int slot = (int)(i / elem), k = (int)(i - (long)slot * elem);
  const long r = blockIdx.y;
  e.out[(r * npad + slot) * elem + k] = e.in[(r * ncol + src[slot]) * elem + k];
}
// internal [rows][npad] -> caller's [rows][ncol]: a day slot's rows as the inner call left them, +0.0 for a night column (what
// the inner call's night kernels wrote there: not read back); replica and filler slots are dropped.  Every caller's column is
// the target of exactly one slot.  night_out: where rrtmg_hip_sw_night_last looks (page-locked; the inner call's last launch
// has left ITS counts there, this launch runs behind it): the tiles' worth of solve work not done, and the night columns.
static __global__ void __launch_bounds__(256) pack_scatter_kernel(PackTable t, const int32_t *dst, const PackHead *head, int ncol, int npad, int32_t *night_out) {
  if (night_out && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
    night_out[0] = (ncol + 63) / 64 - head->ndpad / 64; night_out[1] = ncol - head->nday;
  }
  const int slot = blockIdx.x * 256 + threadIdx.x;
  const PackEntry e = t.e[blockIdx.z];
  const int r0 = blockIdx.y * kPackRows;
  if (slot >= npad || r0 >= e.rows) return;
  const int col = dst[slot];
  if (col < 0) return;
  const bool dark = slot >= head->ndpad;
  double v[kPackRows];
#pragma unroll
  for (int k = 0; k < kPackRows; ++k) if (r0 + k < e.rows) v[k] = dark ? 0.0 : __builtin_nontemporal_load(e.in + (long)(r0 + k) * npad + slot);
#pragma unroll
  for (int k = 0; k < kPackRows; ++k) if (r0 + k < e.rows) e.out[(long)(r0 + k) * ncol + col] = v[k];
}

struct DayPack {
  rrtmg_ctx *ctx;
  hipStream_t s;
  int N, L, Np, depth;   // depth: rows per table entry at the most
  int32_t *src = nullptr, *dst = nullptr;
  PackHead *head = nullptr;
  bool ok = true;
  PackTable tab{};
  PackElemTable etab{};
  int ntab = 0, netab = 0, emax = 0;
  DayPack(rrtmg_ctx *c, hipStream_t st, int ncol, int nlay) : ctx(c), s(st), N(ncol), L(nlay), Np(((ncol + 63) / 64 + 1) * 64), depth(nlay + 1) {}
  template <class T> T *buf(const char *name, size_t n) {
    T *p = (T *)ctx->buf(std::string("sw.pack.") + name, n * sizeof(T));
    if (!p) ok = false;
    return p;
  }
  bool prepare(const double *coszen) {
    const int ntile = (N + 63) / 64;
    int32_t *cnt = buf<int32_t>("cnt", ntile), *base = buf<int32_t>("base", ntile);
    head = buf<PackHead>("head", 1);
    src = buf<int32_t>("src", Np); dst = buf<int32_t>("dst", Np);
    if (!ok) return false;
    hipLaunchKernelGGL(pack_count_kernel, dim3(ntile), dim3(64), 0, s, coszen, N, cnt);
    hipLaunchKernelGGL(pack_scan_kernel, dim3(1), dim3(1024), 0, s, coszen, cnt, ntile, N, base, head);
    hipLaunchKernelGGL(pack_map_kernel, dim3(Np / 64), dim3(64), 0, s, coszen, base, head, N, src, dst);
    return true;
  }
  dim3 grid() const { return dim3((Np + 255) / 256, (depth + kPackRows - 1) / kPackRows, ntab); }
  // entries of at most `depth` rows: in advances by in_cols per row, out by out_cols
  template <class Flush> void add(const double *in, double *out, size_t rows, int aux, size_t in_cols, size_t out_cols, Flush flush) {
    for (size_t r = 0; r < rows; r += depth) {
      if (ntab == kPackMaxEntries) flush();
      const size_t n = rows - r < (size_t)depth ? rows - r : (size_t)depth;
      tab.e[ntab++] = {in + r * in_cols, out + r * out_cols, (int32_t)n, aux};
    }
  }
  // ---- inputs: nullptr stays nullptr (an absent optional array) ----
  const double *gather(const char *name, const double *in, size_t rows, bool whole = false) {
    if (!in) return nullptr;
    double *out = buf<double>(name, rows * (size_t)Np);
    if (!out) return nullptr;
    add(in, out, rows, whole ? 1 : 0, N, Np, [&]() { flush_gather(); });
    return out;
  }
  const double *gather_elem(const char *name, const double *in, int elem) {
    if (!in) return nullptr;
    double *out = buf<double>(name, (size_t)L * Np * elem);
    if (!out) return nullptr;
    if (netab == kPackMaxElemEntries) flush_gather();
    etab.e[netab++] = {in, out, L, elem};
    if (elem > emax) emax = elem;
    return out;
  }
  void flush_gather() {
    if (ntab) hipLaunchKernelGGL(pack_gather_kernel, grid(), dim3(256), 0, s, tab, src, head, N, Np);
    if (netab) hipLaunchKernelGGL(pack_gather_elem_kernel, dim3((unsigned)(((long)Np * emax + 255) / 256), L, netab), dim3(256), 0, s, etab, src, head, N, Np);
    ntab = 0; netab = 0; emax = 0;
  }
  // ---- outputs: the inner call's array for the caller's `user` (nullptr: not requested), registered for the scatter ----
  double *out(const char *name, double *user, size_t rows) {
    if (!user) return nullptr;
    double *o = buf<double>(name, rows * (size_t)Np);
    if (!o) return nullptr;
    // (98 entries at the most -- 6 + 8 + 6 x 14 -- so the table never overflows: the scatter must not run before the inner call)
    add(o, user, rows, 0, Np, N, [&]() { ctx->fail(RRTMG_ERR_ARG, "day-column pack: too many output rows for one scatter table"); ok = false; ntab = 0; });
    return o;
  }
  void flush_scatter(int32_t *night_out) {
    if (ntab) hipLaunchKernelGGL(pack_scatter_kernel, grid(), dim3(256), 0, s, tab, dst, head, N, Np, night_out);
    ntab = 0;
  }
};

}  // namespace rrtmg
