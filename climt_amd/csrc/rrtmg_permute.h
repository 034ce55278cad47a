// rrtmg_permute.h -- the two OPT-IN modes that run a device-resident call (memspace 1) on an internal, re-ordered copy of its
// columns, on one engine:
//   column sort      (rrtmg_hip_set_column_sort; shortwave and longwave)   kind A = cloud-free columns, kind B = cloudy ones
//   day-column pack  (rrtmg_hip_set_sw_night_pack; shortwave)              kind A = day columns,        kind B = night ones
//
// A solve kernel variant is chosen, and the night-column skip (rrtmg_sw.hip) saves work, per 64-column TILE.  Where the two
// kinds are interleaved more finely than a tile, every tile is mixed: cloud-free columns pay for both sky streams, a tile with
// one day column is solved whole.  The copy has Np = 64 x (tiles + 1) slots -- what the host can size without knowing the
// counts -- and no tile of it holds both kinds:
//   [0, nA)              kind A, stable in the caller's order
//   [nA, nApad)          replicas of the last A column up to the tile boundary nApad = 64 x ceil(nA / 64): dropped at the scatter
//   [nApad, nApad + nB)  kind B, stable in the caller's order
//   [nApad + nB, Np)     tail: dropped at the scatter
// One policy bit separates the two users:
//   sort (both blocks live)    tail = replicas of the last B column (of the last A column when nB = 0); the gathers fill every
//                              slot; the scatter copies every slot that has a column
//   pack (second block dead)   every tile from nApad on is a night tile of the existing night path, which gives it no work at
//                              all and reads nothing of it but coszen.  Tail src = -1; the gathers fill the slots from nApad on
//                              only for the arrays marked `whole`, 0.0 in tail slots -- coszen, and ecaer (iaer = 6), whose
//                              mixing pass runs over the whole grid and raises no code; the scatter writes +0.0 for a B slot
//                              (what the night kernels wrote there: not read back) and publishes the night counts
// Columns are independent in every routine (rrtmg_sw_rad.f90:616, rrtmg_lw_rad.nomcica.f90:453); the kissvec sub-column
// generator seeds per column from the column's own pressures, so the masks are the same wherever a column sits.  The Mersenne
// twister's ONE stream is positional, and so are shortwave amplitudes indsolvar != 1 (the host rescales them once per column in
// the caller's order -- sw_scalar_setup -- and the inner call on the copy must never rescale the caller's IN/OUT array): such
// calls are not permuted.  Why the sort is not the default: a cloud-free column then runs in the clear-sky variant, whose
// shortwave differs from the cloudy variant's clear-sky stream by ~1e-12 W m^-2 (docs/EXPERIMENTS.md C) -- the default keeps a
// column's variant a function of its tile, so that tile-aligned shards reproduce the whole grid bit for bit.
//
// Everything is on the device and on the call's stream: 3 map launches (classification, scan, map), ONE gather launch for every
// [rows][N] input and one more for the band-fastest arrays where they are present, the inner call, ONE scatter launch for every
// requested output.  The gather and the scatter take a by-value table with one entry per blockIdx.z; an array of more than
// nlay + 1 rows is several entries, so that the entries are about equally deep and blockIdx.y has no idle tail.
//
// The first part is plain C++ -- the slot rule, the head and the table builder: tools/permute_check.cpp runs it on the CPU --
// the kernels and the host struct follow under __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>

#ifdef __HIPCC__
#define RRTMG_PERMUTE_HD __host__ __device__ inline
#else
#define RRTMG_PERMUTE_HD inline
#endif

namespace rrtmg {

// What the scan leaves for every later step.  lastA, lastB: the last column of each kind (-1: none); live: the slots in front
// of which the inner call works -- Np when both blocks are live, nApad when the second one is dead
struct PermuteHead { int32_t nA, nApad, lastA, lastB, live, pad; };
RRTMG_PERMUTE_HD PermuteHead permute_head(int nA, int lastA, int lastB, int npad, bool both_live) {
  const int nApad = (nA + 63) / 64 * 64;
  return {nA, nApad, lastA, lastB, both_live ? npad : nApad, 0};
}
// THE SLOT RULE.  A caller's column of tile `tile`: kindB, `before` = the columns of its kind in front of it within the tile,
// baseB = the B columns in front of the tile -> its slot
RRTMG_PERMUTE_HD int permute_slot(bool kindB, int before, int tile, int baseB, const PermuteHead &h) {
  return kindB ? h.nApad + baseB + before : tile * 64 - baseB + before;
}
// ... and a slot no column maps to -> the column it replicates, -1 for a dead tail slot; kPermuteMapped for any other slot
constexpr int kPermuteMapped = -2;
RRTMG_PERMUTE_HD int permute_replica(int slot, const PermuteHead &h, int ncol, bool both_live) {
  if (slot >= h.nA && slot < h.nApad) return h.lastA;   // (nA > 0 here: nApad > nA)
  if (slot >= h.nApad + (ncol - h.nA)) return !both_live ? -1 : h.lastB >= 0 ? h.lastB : h.lastA;
  return kPermuteMapped;
}

// The tables of the gather and scatter launches, passed by value: one entry per blockIdx.z.
// aux: gather of [rows][N] arrays -- 1 = `whole`: every slot is filled, 0 = the live slots only;
//      gather of band-fastest arrays -- the elements per (row, column); scatter: unused
struct PermuteEntry { const double *in; double *out; int32_t rows, aux; };
// The scatter's table must hold a call's whole output list (it cannot run before the inner call): rrtmg_call.h asserts that
// the lists of rrtmg_call_arrays.h fit, a band member counting as one entry per band.  The gathers may flush a full table and
// go on (an input list never fills one at nlay + 1 >= 14).  104 entries are 2496 bytes; with the launch's other arguments 2536
// bytes of kernel arguments, of 4096 at the most.
constexpr int kPermuteMaxEntries = 104;
struct PermuteTable { PermuteEntry e[kPermuteMaxEntries]; };
constexpr int kPermuteMaxElemEntries = 5;   // the band-fastest inputs of a spectrum (a full table is flushed: gather_elem)
struct PermuteElemTable { PermuteEntry e[kPermuteMaxElemEntries]; };
static_assert(sizeof(PermuteTable) + 40 <= 4096 && sizeof(PermuteElemTable) + 40 <= 4096, "kernel arguments: 4 KB at the most");
constexpr int permute_entries(size_t rows, int depth) { return (int)((rows + depth - 1) / depth); }
// rows of `in` -> entries of at most `depth` rows behind the n the table holds: in advances by in_cols per row, out by out_cols.
// A full table is flushed first: flush() launches, or gives up, and sets n = 0
template <class Flush>
inline void permute_table_add(PermuteTable &t, int &n, int depth, const double *in, double *out, size_t rows, int aux, size_t in_cols, size_t out_cols, Flush flush) {
  for (size_t r = 0; r < rows; r += depth) {
    if (n == kPermuteMaxEntries) flush();
    const size_t m = rows - r < (size_t)depth ? rows - r : (size_t)depth;
    t.e[n++] = {in + r * in_cols, out + r * out_cols, (int32_t)m, aux};
  }
}

}  // namespace rrtmg

#ifdef __HIPCC__
#include <string>

#include "rrtmg_ctx.h"

namespace rrtmg {

// one wavefront per tile: flag[col] = the column is of kind B; cnt[tile] = how many of the tile's columns are.
// CLOUD: B = cldfr > 0 in any layer (what the preparation kernels use); else B = coszen <= 0 (NaN compares false: day)
template <bool CLOUD>
static __global__ void __launch_bounds__(64) permute_class_kernel(const double *x, int ncol, int nlay, int32_t *flag, int32_t *cnt) {
  const int col = blockIdx.x * 64 + threadIdx.x;
  bool b = false;
  if (col < ncol) {
    if (CLOUD) for (int l = 0; l < nlay; ++l) b = b || x[(long)l * ncol + col] > 0.0;
    else b = x[col] <= 0.0;
    flag[col] = b ? 1 : 0;
  }
  const unsigned long long m = __ballot(b);
  if (threadIdx.x == 0) cnt[blockIdx.x] = __popcll(m);
}

// one workgroup: exclusive prefix of the tiles' B counts (base[tile]) and the head
static __global__ void __launch_bounds__(1024) permute_scan_kernel(const int32_t *flag, const int32_t *cnt, int ntile, int ncol, int npad, int both_live, int32_t *base, PermuteHead *head) {
  __shared__ int part[1024];
  __shared__ int sh_last[2];   // the last tile that has a column of kind A, of kind B
  const int t = threadIdx.x, per = (ntile + 1023) / 1024;
  if (t < 2) sh_last[t] = -1;
  int s = 0, lastA = -1, lastB = -1;
  for (int i = t * per; i < ntile && i < (t + 1) * per; ++i) {
    const int n = cnt[i], cols = ncol - i * 64 < 64 ? ncol - i * 64 : 64;
    s += n;
    if (n < cols) lastA = i;
    if (n > 0) lastB = i;
  }
  part[t] = s;
  __syncthreads();
  if (lastA >= 0) atomicMax(&sh_last[0], lastA);
  if (lastB >= 0) atomicMax(&sh_last[1], lastB);
  for (int d = 1; d < 1024; d <<= 1) {
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = t == 0 ? 0 : part[t - 1];
  for (int i = t * per; i < ntile && i < (t + 1) * per; ++i) { base[i] = run; run += cnt[i]; }
  if (t < 64) {   // the first wavefront: the highest column of each kind in the last tile that has one
    const int tA = sh_last[0], tB = sh_last[1], cA = tA * 64 + t, cB = tB * 64 + t;
    const unsigned long long mA = __ballot(tA >= 0 && cA < ncol && flag[cA] == 0), mB = __ballot(tB >= 0 && cB < ncol && flag[cB] != 0);
    if (t == 0)
      *head = permute_head(ncol - part[1023], mA ? tA * 64 + 63 - __clzll((long long)mA) : -1, mB ? tB * 64 + 63 - __clzll((long long)mB) : -1, npad, both_live != 0);
  }
}

// one wavefront per tile of SLOTS (npad / 64 of them).  As the tile of source columns blockIdx.x: src[slot] = dst[slot] =
// column (permute_slot); as 64 slots: the replicas and the tail (permute_replica: slots no source column maps to, so no two
// threads write one element).  src -1: a dead tail slot; dst -1: nothing to scatter.
static __global__ void __launch_bounds__(64) permute_map_kernel(const int32_t *flag, const int32_t *base, const PermuteHead *head, int ncol, int both_live, int32_t *src, int32_t *dst) {
  const int lane = threadIdx.x, col = blockIdx.x * 64 + lane;
  const PermuteHead h = *head;
  const bool in = col < ncol, b = in && flag[col] != 0;
  const unsigned long long mb = __ballot(b), ma = __ballot(in && !b), lower = (1ull << lane) - 1ull;
  if (in) {
    const int slot = permute_slot(b, __popcll((b ? mb : ma) & lower), blockIdx.x, base[blockIdx.x], h);
    src[slot] = col; dst[slot] = col;
  }
  const int slot = col, r = permute_replica(slot, h, ncol, both_live != 0);
  if (r != kPermuteMapped) { src[slot] = r; dst[slot] = -1; }
}

// in [rows][ncol] -> out [rows][npad]: a thread owns one slot, reads its source column once and keeps kPermuteRows rows of it
// in flight (8 loads, no index traffic per row).  A dead tail slot of an array that is filled whole gets 0.0.
constexpr int kPermuteRows = 8;
static __global__ void __launch_bounds__(256) permute_gather_kernel(PermuteTable t, const int32_t *src, const PermuteHead *head, int ncol, int npad) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  const PermuteEntry e = t.e[blockIdx.z];
  const int r0 = blockIdx.y * kPermuteRows;
  if (slot >= npad || r0 >= e.rows) return;
  if (!e.aux && slot >= head->live) return;
  const int c = src[slot];
  double v[kPermuteRows];
#pragma unroll
  for (int k = 0; k < kPermuteRows; ++k) if (r0 + k < e.rows) v[k] = c >= 0 ? __builtin_nontemporal_load(e.in + (long)(r0 + k) * ncol + c) : 0.0;
#pragma unroll
  for (int k = 0; k < kPermuteRows; ++k) if (r0 + k < e.rows) __builtin_nontemporal_store(v[k], e.out + (long)(r0 + k) * npad + slot);
}
// in [rows][ncol][elem] -> out [rows][npad][elem], row = blockIdx.y, the live slots only
static __global__ void __launch_bounds__(256) permute_gather_elem_kernel(PermuteElemTable t, const int32_t *src, const PermuteHead *head, int ncol, int npad) {
  const PermuteEntry e = t.e[blockIdx.z];
  const int elem = e.aux;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if ((int)blockIdx.y >= e.rows || i >= (long)head->live * elem) return;
  const int slot = (int)(i / elem), k = (int)(i - (long)slot * elem);
  const long r = blockIdx.y;
  e.out[(r * npad + slot) * elem + k] = e.in[(r * ncol + src[slot]) * elem + k];
}
// internal [rows][npad] -> caller's [rows][ncol]: a live slot's rows as the inner call left them, +0.0 for a column in the dead
// block; replica and tail slots are dropped.  Every caller's column is the target of exactly one slot.  night_out (the pack;
// else nullptr): where rrtmg_hip_sw_night_last looks (page-locked; the inner call's last launch has left ITS counts there, this
// launch runs behind it): the tiles' worth of solve work not done, and the night columns.
static __global__ void __launch_bounds__(256) permute_scatter_kernel(PermuteTable t, const int32_t *dst, const PermuteHead *head, int ncol, int npad, int32_t *night_out) {
  if (night_out && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && threadIdx.x == 0) {
    night_out[0] = (ncol + 63) / 64 - head->nApad / 64; night_out[1] = ncol - head->nA;
  }
  const int slot = blockIdx.x * 256 + threadIdx.x;
  const PermuteEntry e = t.e[blockIdx.z];
  const int r0 = blockIdx.y * kPermuteRows;
  if (slot >= npad || r0 >= e.rows) return;
  const int col = dst[slot];
  if (col < 0) return;
  const bool dead = slot >= head->live;
  double v[kPermuteRows];
#pragma unroll
  for (int k = 0; k < kPermuteRows; ++k) if (r0 + k < e.rows) v[k] = dead ? 0.0 : __builtin_nontemporal_load(e.in + (long)(r0 + k) * npad + slot);
#pragma unroll
  for (int k = 0; k < kPermuteRows; ++k) if (r0 + k < e.rows) e.out[(long)(r0 + k) * ncol + col] = v[k];
}

// The host side of one permuted call: kind = kInnerSorted | kInnerPacked; prefix names the work buffers ("sw.sort.", "lw.sort.",
// "sw.pack.").  prepare, the gathers, flush_gather, the outputs, the inner call, flush_scatter.
struct ColumnPermute {
  rrtmg_ctx *ctx;
  hipStream_t s;
  InnerCall kind;
  int N, L, Np, depth;   // depth: rows per table entry at the most
  std::string prefix;
  int32_t *src = nullptr, *dst = nullptr;
  PermuteHead *head = nullptr;
  bool ok = true;
  PermuteTable tab{};
  PermuteElemTable etab{};
  int ntab = 0, netab = 0, emax = 0;
  ColumnPermute(rrtmg_ctx *c, hipStream_t st, InnerCall k, int ncol, int nlay, const char *pre)
      : ctx(c), s(st), kind(k), N(ncol), L(nlay), Np(((ncol + 63) / 64 + 1) * 64), depth(nlay + 1), prefix(pre) {}
  template <class T> T *buf(const char *name, size_t n) {
    T *p = (T *)ctx->buf(prefix + name, n * sizeof(T));
    if (!p) ok = false;
    return p;
  }
  // key: cldfr [nlay][N] for the sort, coszen [N] for the pack
  bool prepare(const double *key) {
    const int ntile = (N + 63) / 64, both = kind == kInnerSorted ? 1 : 0;
    int32_t *flag = buf<int32_t>("flag", N), *cnt = buf<int32_t>("cnt", ntile), *base = buf<int32_t>("base", ntile);
    head = buf<PermuteHead>("head", 1);
    src = buf<int32_t>("src", Np); dst = buf<int32_t>("dst", Np);
    if (!ok) return false;
    if (both) hipLaunchKernelGGL(permute_class_kernel<true>, dim3(ntile), dim3(64), 0, s, key, N, L, flag, cnt);
    else hipLaunchKernelGGL(permute_class_kernel<false>, dim3(ntile), dim3(64), 0, s, key, N, L, flag, cnt);
    hipLaunchKernelGGL(permute_scan_kernel, dim3(1), dim3(1024), 0, s, flag, cnt, ntile, N, Np, both, base, head);
    hipLaunchKernelGGL(permute_map_kernel, dim3(Np / 64), dim3(64), 0, s, flag, base, head, N, both, src, dst);
    return true;
  }
  dim3 grid() const { return dim3((Np + 255) / 256, (depth + kPermuteRows - 1) / kPermuteRows, ntab); }
  // ---- inputs: nullptr stays nullptr (an absent optional array) ----
  const double *gather(const char *name, const double *in, size_t rows, bool whole = false) {
    if (!in) return nullptr;
    double *out = buf<double>(name, rows * (size_t)Np);
    if (!out) return nullptr;
    permute_table_add(tab, ntab, depth, in, out, rows, whole ? 1 : 0, N, Np, [&]() { flush_gather(); });
    return out;
  }
  const double *gather_elem(const char *name, const double *in, int elem) {
    if (!in) return nullptr;
    double *out = buf<double>(name, (size_t)L * Np * elem);
    if (!out) return nullptr;
    if (netab == kPermuteMaxElemEntries) flush_gather();
    etab.e[netab++] = {in, out, L, elem};
    if (elem > emax) emax = elem;
    return out;
  }
  void flush_gather() {
    if (ntab) hipLaunchKernelGGL(permute_gather_kernel, grid(), dim3(256), 0, s, tab, src, head, N, Np);
    if (netab) hipLaunchKernelGGL(permute_gather_elem_kernel, dim3((unsigned)(((long)Np * emax + 255) / 256), L, netab), dim3(256), 0, s, etab, src, head, N, Np);
    ntab = 0; netab = 0; emax = 0;
  }
  // ---- outputs: the inner call's array for the caller's `user` (nullptr: not requested), registered for the scatter ----
  double *out(const char *name, double *user, size_t rows) {
    if (!user) return nullptr;
    double *o = buf<double>(name, rows * (size_t)Np);
    if (!o) return nullptr;
    permute_table_add(tab, ntab, depth, o, user, rows, 0, Np, N, [&]() { ctx->fail(RRTMG_ERR_ARG, "permuted call: too many output rows for one scatter table"); ok = false; ntab = 0; });
    return o;
  }
  void flush_scatter(int32_t *night_out) {
    if (ntab) hipLaunchKernelGGL(permute_scatter_kernel, grid(), dim3(256), 0, s, tab, dst, head, N, Np, night_out);
    ntab = 0;
  }
};

}  // namespace rrtmg
#endif  // __HIPCC__
