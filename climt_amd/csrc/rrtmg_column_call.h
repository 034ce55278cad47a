// rrtmg_column_call.h -- ONE staging and launch path for the column components (host code only), twelve entries: dry adjustment,
// boundary layer, Emanuel convection, simple physics; Frierson optical depth, gray longwave, grid-scale condensation; the snow/ice
// column; BucketHydrology and SecondBEST; the correlated-k longwave and shortwave.  Each .hip file holds a table per entry, a row per array of its
// public struct (include/rrtmg_hip.h).
// A row states once: the member of the public struct and its name in messages, the member of the kernel's call struct, the
// extent, and -- read off the member's own type -- the element type (double or int32) and the direction (const: an input);
// for an output, the one input it may be exactly (in place); whether NULL is refused.  Every path that enumerates the arrays
// walks the table: the "must be given" refusal, the aliasing check, the staging plan of a host-pointer call, the uploads, the
// binding of the call struct under either memspace and the downloads.  Whether an optional input is read at all stays the
// entry's decision: it hands the walkers the rows it does NOT read (`unread`, column_bits).
// The plan and the aliasing check are plain C++ (tools/column_table_check.h holds their checks once; the five check programs that
// include it run them under the host sanitizers); what calls HIP is behind __HIPCC__.  A new column component is one table, its
// checks, its kernel.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <type_traits>

#include "../../include/rrtmg_hip.h"

namespace rrtmg {

enum class ColumnExt { Lay, Lev, Col,         // [nlay][ncol], [nlay+1][ncol], [ncol]
                       BandLay, BandLev, BandCol };   // the same times the call's nband (rrtmg_cork.hip), in the order the entry documents
struct ColumnRow {
  const char *name;
  size_t pub, dev;           // offsetof the pointer in the public struct and in the kernel's call struct
  bool i32, out;             // int32 elements (else double); written (else only read)
  ColumnExt ext;
  bool required;
  const char *in_place_of = nullptr;   // an output: the input it may be exactly
};
struct ColumnTable {
  const char *entry, *strct;                 // the prefix of every message; the public struct's name
  int nlay_min;
  const char *ncol_msg, *nlay_msg, *note;    // the two refusals of the sizes; what follows "aliases an input" for an in-place row
  const ColumnRow *rows;
  int n;
};
constexpr int kColumnMaxRows = 64;           // the rows of a table are the bits of a ColumnMask
using ColumnMask = uint64_t;
template <int N>
constexpr ColumnTable column_table(const char *entry, const char *strct, int nlay_min, const char *ncol_msg, const char *nlay_msg, const char *note, const ColumnRow (&rows)[N]) {
  static_assert(N <= kColumnMaxRows, "a table has at most 64 rows");
  return {entry, strct, nlay_min, ncol_msg, nlay_msg, note, rows, N};
}

template <class P> struct ColumnMember;      // element type and direction of a pointer member
template <> struct ColumnMember<const double *> { static constexpr bool i32 = false, out = false; };
template <> struct ColumnMember<double *> { static constexpr bool i32 = false, out = true; };
template <> struct ColumnMember<int32_t *> { static constexpr bool i32 = true, out = true; };
template <> struct ColumnMember<const int32_t *> { static constexpr bool i32 = true, out = false; };
template <class P, class D> constexpr size_t column_same_type(size_t offset) {
  static_assert(std::is_same<P, D>::value, "the public struct and the call struct disagree about a member's type");
  return offset;
}
// RRTMG_COLUMN_ROW(public struct, call struct, member): the first five fields of a row (the member has one name in both)
#define RRTMG_COLUMN_ROW(P, C, m) #m, offsetof(P, m), rrtmg::column_same_type<decltype(P::m), decltype(C::m)>(offsetof(C, m)), \
                                  rrtmg::ColumnMember<decltype(P::m)>::i32, rrtmg::ColumnMember<decltype(P::m)>::out

inline const void *column_ptr(const void *strct, size_t offset) {
  const void *p;
  memcpy(&p, (const char *)strct + offset, sizeof p);
  return p;
}
// (nband: what a band-multiplied extent is multiplied by; the entries without such rows leave it at 1)
inline size_t column_bytes(const ColumnRow &r, size_t ncol, size_t nlay, size_t nband = 1) {
  const bool banded = r.ext == ColumnExt::BandLay || r.ext == ColumnExt::BandLev || r.ext == ColumnExt::BandCol;
  const size_t rows = r.ext == ColumnExt::Lay || r.ext == ColumnExt::BandLay ? nlay : r.ext == ColumnExt::Lev || r.ext == ColumnExt::BandLev ? nlay + 1 : 1;
  return (banded ? nband : 1) * rows * ncol * (r.i32 ? sizeof(int32_t) : sizeof(double));
}
constexpr bool column_same_name(const char *a, const char *b) {
  for (; *a && *a == *b; ++a, ++b) {}
  return *a == *b;
}
constexpr int column_index(const ColumnTable &t, const char *name) {
  for (int i = 0; i < t.n; ++i)
    if (column_same_name(t.rows[i].name, name)) return i;
  return -1;
}
// the bits of the named rows.  An entry keeps the result in a constexpr variable: a name no row has is then a shift by -1 in a
// constant expression, which does not compile
constexpr ColumnMask column_bits(const ColumnTable &t, std::initializer_list<const char *> names) {
  ColumnMask bits = 0;
  for (const char *name : names) bits |= ColumnMask(1) << column_index(t, name);
  return bits;
}
// the rows of a call: given (not NULL) and not among those the entry does not read
inline ColumnMask column_present(const ColumnTable &t, const void *a, ColumnMask unread) {
  ColumnMask bits = 0;
  for (int i = 0; i < t.n; ++i)
    if (column_ptr(a, t.rows[i].pub)) bits |= ColumnMask(1) << i;
  return bits & ~unread;
}

// ---- overlap and aliasing (sizes in bytes) -------------------------------------------------------------------------------------------
inline bool ranges_overlap(const void *p, size_t n, const void *q, size_t m) {
  return p && q && (uintptr_t)p < (uintptr_t)q + m && (uintptr_t)q < (uintptr_t)p + n;
}
struct ColumnSpan { const char *name; const void *p; size_t bytes; bool out; const void *may_be; };
// An output may overlap no input and no earlier output; in place means exactly its own input (may_be).  -> whether the call
// is refused, and with what (the text behind the entry's prefix).  Outputs in the order of `s`, each against the inputs first.
inline bool aliasing_refusal(const ColumnSpan *s, int n, const char *note, char *msg, size_t cap) {
  for (int i = 0; i < n; ++i) {
    if (!s[i].out) continue;
    for (int e = 0; e < n; ++e)
      if (!s[e].out && ranges_overlap(s[i].p, s[i].bytes, s[e].p, s[e].bytes) && !(s[i].may_be && s[i].p == s[i].may_be && s[e].p == s[i].may_be))
        return snprintf(msg, cap, "%s aliases an input%s", s[i].name, s[i].may_be ? note : ""), true;
    for (int j = 0; j < i; ++j)
      if (s[j].out && ranges_overlap(s[i].p, s[i].bytes, s[j].p, s[j].bytes)) return snprintf(msg, cap, "%s overlaps %s", s[i].name, s[j].name), true;
  }
  return false;
}
inline int column_spans(const ColumnTable &t, const void *a, size_t ncol, size_t nlay, ColumnMask present, ColumnSpan *s, size_t nband = 1) {
  int n = 0;
  for (int i = 0; i < t.n; ++i) {
    const ColumnRow &r = t.rows[i];
    if (present >> i & 1) s[n++] = {r.name, column_ptr(a, r.pub), column_bytes(r, ncol, nlay, nband), r.out, r.in_place_of ? column_ptr(a, t.rows[column_index(t, r.in_place_of)].pub) : nullptr};
  }
  return n;
}
// the names of the required rows that are NULL make the call refused: -> whether, and the entry's "a, b and c must be given"
inline bool column_required_refusal(const ColumnTable &t, const void *a, char *msg, size_t cap) {
  bool missing = false;
  int left = 0, at = 0;
  for (int i = 0; i < t.n; ++i) left += t.rows[i].required;
  for (int i = 0; i < t.n; ++i) {
    if (!t.rows[i].required) continue;
    missing |= !column_ptr(a, t.rows[i].pub);
    --left;
    at += snprintf(msg + at, at < (int)cap ? cap - at : 0, "%s%s", t.rows[i].name, left > 1 ? ", " : left == 1 ? " and " : " must be given");
  }
  return missing;
}

// ---- the staging buffer of a host-pointer call ----------------------------------------------------------------------------------------
// One buffer: the rows that are present in the table's order, the doubles first and the int32 rows behind them (so every slot
// is aligned for its type); an in-place output has the slot of its input (the kernel runs in place in the device copy); an
// absent row has no slot.
struct ColumnPlan { size_t at[kColumnMaxRows], total; };
constexpr size_t kColumnNoSlot = ~(size_t)0;
inline ColumnPlan column_plan(const ColumnTable &t, size_t ncol, size_t nlay, ColumnMask present, size_t nband = 1) {
  ColumnPlan p;
  p.total = 0;
  for (int i = 0; i < kColumnMaxRows; ++i) p.at[i] = kColumnNoSlot;
  for (int pass = 0; pass < 2; ++pass)
    for (int i = 0; i < t.n; ++i) {
      const ColumnRow &r = t.rows[i];
      if (!(present >> i & 1) || r.i32 != (pass == 1)) continue;
      const int partner = r.in_place_of ? column_index(t, r.in_place_of) : -1;
      if (partner >= 0 && p.at[partner] != kColumnNoSlot) { p.at[i] = p.at[partner]; continue; }
      p.at[i] = p.total;
      p.total += column_bytes(r, ncol, nlay, nband);
    }
  return p;
}

}  // namespace rrtmg

#ifdef __HIPCC__
#include "rrtmg_ctx.h"

namespace rrtmg {

// ---- the head of refusals every entry shares, in this order (A: a public struct that begins struct_size, ncol, nlay, memspace) ----
template <class A>
int column_head(rrtmg_ctx *ctx, const ColumnTable &t, const A *a) {
  if (!ctx) return RRTMG_ERR_ARG;
  if (!a) return ctx->fail(RRTMG_ERR_ARG, "%s: NULL argument struct", t.entry);
  if (a->struct_size != sizeof(A)) return ctx->fail(RRTMG_ERR_ARG, "%s: struct_size %u, this library's %s has %zu bytes", t.entry, a->struct_size, t.strct, sizeof(A));
  if (a->ncol <= 0) return ctx->fail(RRTMG_ERR_ARG, "%s: %s", t.entry, t.ncol_msg);
  if (a->nlay < t.nlay_min) return ctx->fail(RRTMG_ERR_ARG, "%s: %s", t.entry, t.nlay_msg);
  if (a->memspace != 0 && a->memspace != 1) return ctx->fail(RRTMG_ERR_ARG, "%s: memspace must be 0 (host) or 1 (device)", t.entry);
  return RRTMG_OK;
}
inline int column_required(rrtmg_ctx *ctx, const ColumnTable &t, const void *a) {
  char msg[256];
  return column_required_refusal(t, a, msg, sizeof msg) ? ctx->fail(RRTMG_ERR_ARG, "%s: %s", t.entry, msg) : RRTMG_OK;
}

// the aliasing refusal of a call (column_call makes it; an entry whose own checks come behind it makes it first itself)
template <class A>
int column_aliasing(rrtmg_ctx *ctx, const ColumnTable &t, const A *a, ColumnMask unread, size_t nband = 1) {
  ColumnSpan spans[kColumnMaxRows];
  char msg[160];
  const int n = column_spans(t, a, (size_t)a->ncol, (size_t)a->nlay, column_present(t, a, unread), spans, nband);
  return aliasing_refusal(spans, n, t.note, msg, sizeof msg) ? ctx->fail(RRTMG_ERR_ARG, "%s: %s", t.entry, msg) : RRTMG_OK;
}

// one thread per column, tiles of 64 columns, on the context's main stream
template <class Kernel, class C>
int column_launch(rrtmg_ctx *ctx, Kernel kernel, size_t ncol, const C &c) {
  hipLaunchKernelGGL(kernel, dim3((unsigned)((ncol + 63) / 64)), dim3(64), 0, ctx->stream, c);
  RRTMG_HIP_CHECK(ctx, hipGetLastError());
  return RRTMG_OK;
}

// The call behind an entry's own checks: the aliasing refusal (not made again where the entry has made it: `aliasing_checked`); the device; `work` -- the entry's work slabs, allocated before
// anything is queued, so a failed allocation leaves the stream as it was; under memspace 0 the staging buffer `io` and the inputs
// that are present going up; the pointers of the call struct `c` bound (memspace 0: the plan's slots, 1: the caller's own; an
// absent row: nullptr); `launch` -- the entry's launch(es); under memspace 0 the outputs that are present coming back.
// Device pointers in deferred mode: the call returns once enqueued; otherwise it waits.  `nband`: the factor of the band-multiplied
// extents, for the entry that has such rows.
template <class A, class C, class Work, class Launch>
int column_call(rrtmg_ctx *ctx, const ColumnTable &t, const A *a, C &c, ColumnMask unread, const char *io, Work work, Launch launch, bool aliasing_checked = false, size_t nband = 1) {
  const size_t ncol = (size_t)a->ncol, nlay = (size_t)a->nlay;
  const ColumnMask present = column_present(t, a, unread);
  int rc = aliasing_checked ? RRTMG_OK : column_aliasing(ctx, t, a, unread, nband);
  if (rc) return rc;
  rc = ctx_prepare_device(ctx);
  if (!rc) rc = work();
  if (rc) return rc;
  hipStream_t s = ctx->stream;
  const bool host = a->memspace == 0;
  const ColumnPlan plan = column_plan(t, ncol, nlay, host ? present : ColumnMask(0), nband);
  char *const staged = host ? (char *)ctx->buf(io, plan.total) : nullptr;
  if (host && !staged) return ctx->status;
  void *bound[kColumnMaxRows];
  for (int i = 0; i < t.n; ++i) {
    const ColumnRow &r = t.rows[i];
    void *const mine = present >> i & 1 ? const_cast<void *>(column_ptr(a, r.pub)) : nullptr;
    bound[i] = mine && host ? staged + plan.at[i] : mine;
    memcpy((char *)&c + r.dev, &bound[i], sizeof(void *));
    if (host && mine && !r.out) RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(bound[i], mine, column_bytes(r, ncol, nlay, nband), hipMemcpyHostToDevice, s));
  }
  rc = launch();
  if (rc) return rc;
  for (int i = 0; host && i < t.n; ++i)
    if (t.rows[i].out && bound[i])
      RRTMG_HIP_CHECK(ctx, hipMemcpyAsync(const_cast<void *>(column_ptr(a, t.rows[i].pub)), bound[i], column_bytes(t.rows[i], ncol, nlay, nband), hipMemcpyDeviceToHost, s));
  if (ctx->deferred && !host) return RRTMG_OK;
  RRTMG_HIP_CHECK(ctx, hipStreamSynchronize(s));
  return RRTMG_OK;
}

}  // namespace rrtmg
#endif
