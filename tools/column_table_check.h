// column_table_check.h -- the checks every table of a column component gets (climt_amd/csrc/rrtmg_column_call.h), once, for the
// `tables` mode of the stand-alone host check programs: column_call_check.cpp, gray_check.cpp, surface_ice_check.cpp,
// land_surface_check.cpp and cork_check.cpp.  Plain C++: the tables and the pure walkers only, no HIP.  Included with a quoted
// include behind the .hip file(s) whose tables the program checks; a program keeps its own list of tables and their "must be
// given" texts.
//
//   print_table(t)      Line: <entry> <in|out> <struct> <member> <extent> <f64|i32> <required or -> <the input it may be, or ->
//                       and the rules of a row: one name one row; an in-place output has an earlier input of its own extent and type.
//   check_plan(t, ...)  the staging plan at ncol 1, 63, 64, 65 x nlay minimum, minimum + 1, 61 x every nband of the list x every
//                       subset of the optional rows (or of `vary`, where the full set is too large): a slot per present row and
//                       none for an absent one, inside the total, aligned for its type, pairwise disjoint but for an in-place
//                       output and its input, which share one; the sizes of all six extents; the total nothing but the rows;
//                       with `before`, every row present takes at most that many bytes.
//   check_aliasing<A>(t, note, must_be_given)
//                       with made-up addresses: an output over each input is refused, x_out == x accepted and x + 8 refused, an
//                       input the entry does not read takes no part, an output over an earlier output is refused, a NULL required
//                       output is refused and a NULL optional one is not -- and the "must be given" text.
#pragma once
#include <initializer_list>
#include <string>

#include "../climt_amd/csrc/rrtmg_column_call.h"
#include "check_common.h"

namespace rrtmg {

inline const char *column_ext_name(ColumnExt e) {
  static const char *const ext[] = {"[nlay][ncol]", "[nlay+1][ncol]", "[ncol]", "[nband][nlay][ncol]", "[nband][nlay+1][ncol]", "[nband][ncol]"};
  return ext[(int)e];
}

inline void print_table(const ColumnTable &t) {
  for (int i = 0; i < t.n; ++i) {
    const ColumnRow &r = t.rows[i];
    CHECK(r.name && r.name[0] && column_index(t, r.name) == i);      // a name is one row
    if (r.in_place_of) {      // an earlier input of the same shape and type, required exactly when the output is.  (Every in-place
      // output but BucketHydrology's two deep ones is in its table's "must be given" text, which check_aliasing holds to
      // column_required_refusal: for those tables this is the older wording, "the input is required".)
      const int p = column_index(t, r.in_place_of);
      CHECK(r.out && p >= 0 && p < i && !t.rows[p].out && t.rows[p].ext == r.ext && t.rows[p].i32 == r.i32 && t.rows[p].required == r.required);
    }
    printf("%s %s %s %s %s %s %s %s\n", t.entry, r.out ? "out" : "in", t.strct, r.name, column_ext_name(r.ext), r.i32 ? "i32" : "f64", r.required ? "required" : "-",
           r.in_place_of ? r.in_place_of : "-");
  }
}

// bytes of the staging of a host-pointer call before the tables, every optional array given
typedef size_t (*ColumnBytesBefore)(size_t ncol, size_t nlay);

// `vary`: the optional rows whose every subset is walked, the other optional rows being absent (0: all of them)
inline void check_plan(const ColumnTable &t, std::initializer_list<size_t> nbands = {1}, ColumnMask vary = 0, ColumnBytesBefore before = nullptr) {
  ColumnMask required = 0, optional = 0;
  for (int i = 0; i < t.n; ++i) (t.rows[i].required ? required : optional) |= ColumnMask(1) << i;
  CHECK((vary & ~optional) == 0);
  if (!vary) vary = optional;
  for (size_t ncol : {(size_t)1, (size_t)63, (size_t)64, (size_t)65})
    for (size_t nlay : {(size_t)t.nlay_min, (size_t)t.nlay_min + 1, (size_t)61})
      for (size_t nband : nbands) {
        if (before) CHECK(column_plan(t, ncol, nlay, required | optional, nband).total <= before(ncol, nlay));
        for (ColumnMask sub = vary;; sub = (sub - 1) & vary) {      // every subset
          const ColumnMask present = required | sub;
          const ColumnPlan p = column_plan(t, ncol, nlay, present, nband);
          size_t sum = 0;
          for (int i = 0; i < t.n; ++i) {
            const ColumnRow &r = t.rows[i];
            if (!(present >> i & 1)) { CHECK(p.at[i] == kColumnNoSlot); continue; }
            const size_t n = column_bytes(r, ncol, nlay, nband);
            const size_t rows = r.ext == ColumnExt::Col || r.ext == ColumnExt::BandCol ? 1 : r.ext == ColumnExt::Lay || r.ext == ColumnExt::BandLay ? nlay : nlay + 1;
            const bool banded = r.ext == ColumnExt::BandLay || r.ext == ColumnExt::BandLev || r.ext == ColumnExt::BandCol;
            CHECK(n == (banded ? nband : 1) * rows * ncol * (r.i32 ? 4 : 8));
            if (!banded) CHECK(column_bytes(r, ncol, nlay) == n);      // (the default nband is 1)
            CHECK(p.at[i] != kColumnNoSlot && p.at[i] + n <= p.total && p.at[i] % (r.i32 ? 4 : 8) == 0);
            const bool shares = r.in_place_of && (present >> column_index(t, r.in_place_of) & 1);
            if (!shares) sum += n;
            for (int j = 0; j < i; ++j) {
              if (!(present >> j & 1)) continue;
              if (r.in_place_of && column_index(t, r.in_place_of) == j) CHECK(p.at[i] == p.at[j]);
              else CHECK(!ranges_overlap((const void *)(p.at[i] + 8), n, (const void *)(p.at[j] + 8), column_bytes(t.rows[j], ncol, nlay, nband)));
            }
          }
          CHECK(p.total == sum);      // nothing but the rows that are present
          if (sub == 0) break;
        }
      }
}

// a public struct whose every array sits at a made-up address, 16 MiB apart (never dereferenced)
template <class A>
A made_up(const ColumnTable &t) {
  A a{};
  for (int i = 0; i < t.n; ++i) {
    const void *p = (const void *)((uintptr_t)(i + 1) << 24);
    memcpy((char *)&a + t.rows[i].pub, &p, sizeof p);
  }
  return a;
}
template <class A>
std::string refusal(const ColumnTable &t, const A &a, size_t ncol, size_t nlay, size_t nband, ColumnMask unread = 0) {
  ColumnSpan s[kColumnMaxRows];
  char msg[160] = "";
  const bool refused = aliasing_refusal(s, column_spans(t, &a, ncol, nlay, column_present(t, &a, unread), s, nband), t.note, msg, sizeof msg);
  CHECK(refused == (msg[0] != 0));
  return msg;
}
template <class A>
void set(const ColumnTable &t, A &a, int row, const void *p) { memcpy((char *)&a + t.rows[row].pub, &p, sizeof p); }

template <class A>
void check_aliasing(const ColumnTable &t, const char *note, const char *must_be_given, size_t nband = 1) {
  const size_t ncol = 65, nlay = (size_t)t.nlay_min;
  A a = made_up<A>(t);
  CHECK(refusal(t, a, ncol, nlay, nband).empty());
  char msg[512];
  CHECK(!column_required_refusal(t, &a, msg, sizeof msg) && std::string(msg) == must_be_given);
  const A none{};      // nothing given: refused, with the same text
  CHECK(column_required_refusal(t, &none, msg, sizeof msg) && std::string(msg) == must_be_given);
  for (int o = 0; o < t.n; ++o) {
    const ColumnRow &out = t.rows[o];
    if (!out.out) continue;
    const int partner = out.in_place_of ? column_index(t, out.in_place_of) : -1;
    const std::string aliases = std::string(out.name) + " aliases an input" + (partner >= 0 ? note : "");
    for (int i = 0; i < t.n; ++i) {
      if (t.rows[i].out) continue;
      a = made_up<A>(t);
      set(t, a, o, column_ptr(&a, t.rows[i].pub));
      CHECK(refusal(t, a, ncol, nlay, nband) == (i == partner ? "" : aliases));      // x_out == x: in place
      if (!t.rows[i].required) CHECK(refusal(t, a, ncol, nlay, nband, ColumnMask(1) << i).empty());      // an input the entry does not read takes no part
      if (i != partner) continue;
      set(t, a, o, (const char *)column_ptr(&a, t.rows[i].pub) + 8);          // in place means exactly in place
      CHECK(refusal(t, a, ncol, nlay, nband) == aliases);
    }
    for (int e = 0; e < o; ++e) {
      if (!t.rows[e].out) continue;
      for (size_t shift : {(size_t)0, (size_t)4}) {
        a = made_up<A>(t);
        set(t, a, o, (const char *)column_ptr(&a, t.rows[e].pub) + shift);
        CHECK(refusal(t, a, ncol, nlay, nband) == std::string(out.name) + " overlaps " + t.rows[e].name);
      }
    }
    a = made_up<A>(t);      // a required row that is NULL is refused, an optional one is not
    set(t, a, o, nullptr);
    CHECK(column_required_refusal(t, &a, msg, sizeof msg) == out.required && refusal(t, a, ncol, nlay, nband).empty());
  }
}

}  // namespace rrtmg
