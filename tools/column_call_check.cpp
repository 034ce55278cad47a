// column_call_check.cpp -- the tables of the four column components (climt_amd/csrc/rrtmg_column_call.h and the table at the head of
// rrtmg_{dry_adjust,boundary_layer,emanuel,simple_physics}.hip) on the CPU: no device, no GPU call, no HIP.  A stand-alone program
// for tests/test_call_arrays.py and the host sanitizers; a plain C++ compiler sees the tables and the pure walkers only:
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -x c++ tools/column_call_check.cpp -o column_call_check && ./column_call_check
//
// Line: <entry> <in|out> <struct> <member> <extent> <f64|i32> <required or -> <the input it may be, or ->
// It also checks, for every table:
//   the staging plan at ncol 1, 63, 64, 65 x nlay minimum, minimum + 1, 61 x every combination of optional rows: slots pairwise
//     disjoint but for an in-place output and its input, inside the total, aligned for their type, none for an absent row; with every
//     row present the total is at most what the hand-written layout before the tables took (the formulae below);
//   the aliasing refusals with made-up addresses: an output over each input, x_out == x accepted, x + 8 refused, an output over
//     an earlier output -- with the texts the entries had before the tables;
//   the "must be given" text.
// Exit status 0 and a last line "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "../climt_amd/csrc/rrtmg_boundary_layer.hip"
#include "../climt_amd/csrc/rrtmg_dry_adjust.hip"
#include "../climt_amd/csrc/rrtmg_emanuel.hip"
#include "../climt_amd/csrc/rrtmg_simple_physics.hip"

using namespace rrtmg;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

// bytes of the staging of a host-pointer call before the tables, every optional array given
typedef size_t (*Before)(size_t ncol, size_t nlay);
static size_t dry_before(size_t ncol, size_t nlay) { const size_t bl = nlay * ncol * 8, bl1 = bl + ncol * 8; return 3 * bl + bl1 + 4 * ncol; }
static size_t bl_before(size_t ncol, size_t nlay) { const size_t b1 = ncol * 8, bl = nlay * b1, bl1 = bl + b1; return 5 * bl + bl1 + 10 * b1; }
static size_t emanuel_before(size_t ncol, size_t nlay) { const size_t nl = nlay * ncol; return 8 * (12 * nl + 8 * ncol + (ncol + 1) / 2); }
static size_t sp_before(size_t ncol, size_t nlay) { const size_t b1 = ncol * 8, bl = nlay * b1, bl1 = bl + b1; return 5 * bl + bl1 + 7 * b1; }

static void print_table(const ColumnTable &t) {
  static const char *const ext[] = {"[nlay][ncol]", "[nlay+1][ncol]", "[ncol]"};
  for (int i = 0; i < t.n; ++i) {
    const ColumnRow &r = t.rows[i];
    CHECK(r.name && r.name[0] && column_index(t, r.name) == i);      // a name is one row
    if (r.in_place_of) {      // an earlier input of the same shape and type
      const int p = column_index(t, r.in_place_of);
      CHECK(r.out && p >= 0 && p < i && !t.rows[p].out && t.rows[p].ext == r.ext && t.rows[p].i32 == r.i32 && t.rows[p].required);
    }
    printf("%s %s %s %s %s %s %s %s\n", t.entry, r.out ? "out" : "in", t.strct, r.name, ext[(int)r.ext], r.i32 ? "i32" : "f64", r.required ? "required" : "-", r.in_place_of ? r.in_place_of : "-");
  }
}

static void check_plan(const ColumnTable &t, Before before) {
  unsigned required = 0, all = (t.n == 32 ? 0u : 1u << t.n) - 1u;
  for (int i = 0; i < t.n; ++i) required |= t.rows[i].required ? 1u << i : 0;
  for (size_t ncol : {(size_t)1, (size_t)63, (size_t)64, (size_t)65})
    for (size_t nlay : {(size_t)t.nlay_min, (size_t)t.nlay_min + 1, (size_t)61}) {
      CHECK(column_plan(t, ncol, nlay, all).total <= before(ncol, nlay));
      for (unsigned present = 0; present <= all; ++present) {
        if ((present & required) != required) continue;
        const ColumnPlan p = column_plan(t, ncol, nlay, present);
        for (int i = 0; i < t.n; ++i) {
          const ColumnRow &r = t.rows[i];
          if (!(present >> i & 1)) { CHECK(p.at[i] == kColumnNoSlot); continue; }
          const size_t n = column_bytes(r, ncol, nlay);
          CHECK(n == (r.ext == ColumnExt::Col ? 1 : r.ext == ColumnExt::Lay ? nlay : nlay + 1) * ncol * (r.i32 ? 4 : 8));
          CHECK(p.at[i] != kColumnNoSlot && p.at[i] + n <= p.total && p.at[i] % (r.i32 ? 4 : 8) == 0);
          for (int j = 0; j < i; ++j) {
            if (!(present >> j & 1)) continue;
            const bool pair = r.in_place_of && column_index(t, r.in_place_of) == j;
            if (pair) CHECK(p.at[i] == p.at[j]);
            else CHECK(!ranges_overlap((const void *)(p.at[i] + 8), n, (const void *)(p.at[j] + 8), column_bytes(t.rows[j], ncol, nlay)));
          }
        }
      }
    }
}

// a public struct whose every array sits at a made-up address, 16 MiB apart (never dereferenced)
template <class A>
static A made_up(const ColumnTable &t) {
  A a{};
  for (int i = 0; i < t.n; ++i) {
    const void *p = (const void *)((uintptr_t)(i + 1) << 24);
    memcpy((char *)&a + t.rows[i].pub, &p, sizeof p);
  }
  return a;
}
template <class A>
static std::string refusal(const ColumnTable &t, const A &a, size_t ncol, size_t nlay) {
  ColumnSpan s[kColumnMaxRows];
  char msg[160] = "";
  const bool refused = aliasing_refusal(s, column_spans(t, &a, ncol, nlay, column_present(t, &a, 0), s), t.note, msg, sizeof msg);
  CHECK(refused == (msg[0] != 0));
  return msg;
}
template <class A>
static void set(const ColumnTable &t, A &a, int row, const void *p) { memcpy((char *)&a + t.rows[row].pub, &p, sizeof p); }

template <class A>
static void check_aliasing(const ColumnTable &t, const char *note, const char *must_be_given) {
  const size_t ncol = 65, nlay = (size_t)t.nlay_min + 1;
  A a = made_up<A>(t);
  CHECK(refusal(t, a, ncol, nlay).empty());
  char msg[256];
  CHECK(!column_required_refusal(t, &a, msg, sizeof msg) && std::string(msg) == must_be_given);
  for (int o = 0; o < t.n; ++o) {
    const ColumnRow &out = t.rows[o];
    if (!out.out) continue;
    const int partner = out.in_place_of ? column_index(t, out.in_place_of) : -1;
    const std::string aliases = std::string(out.name) + " aliases an input" + (partner >= 0 ? note : "");
    for (int i = 0; i < t.n; ++i) {
      if (t.rows[i].out) continue;
      a = made_up<A>(t);
      set(t, a, o, column_ptr(&a, t.rows[i].pub));
      CHECK(refusal(t, a, ncol, nlay) == (i == partner ? "" : aliases));      // x_out == x: in place
      if (i != partner) continue;
      set(t, a, o, (const char *)column_ptr(&a, t.rows[i].pub) + 8);          // in place means exactly in place
      CHECK(refusal(t, a, ncol, nlay) == aliases);
    }
    for (int e = 0; e < o; ++e) {
      if (!t.rows[e].out) continue;
      for (size_t shift : {(size_t)0, (size_t)4}) {
        a = made_up<A>(t);
        set(t, a, o, (const char *)column_ptr(&a, t.rows[e].pub) + shift);
        CHECK(refusal(t, a, ncol, nlay) == std::string(out.name) + " overlaps " + t.rows[e].name);
      }
    }
    // a required row that is NULL is refused, an optional one is not
    a = made_up<A>(t);
    set(t, a, o, nullptr);
    CHECK(column_required_refusal(t, &a, msg, sizeof msg) == out.required && refusal(t, a, ncol, nlay).empty());
  }
  // an input the entry does not read takes no part
  for (int i = 0; i < t.n; ++i) {
    if (t.rows[i].out || t.rows[i].required) continue;
    a = made_up<A>(t);
    int first_out = 0;
    while (!t.rows[first_out].out) ++first_out;
    set(t, a, first_out, column_ptr(&a, t.rows[i].pub));
    ColumnSpan s[kColumnMaxRows];
    CHECK(!aliasing_refusal(s, column_spans(t, &a, ncol, nlay, column_present(t, &a, 1u << i), s), t.note, msg, sizeof msg));
  }
}

int main() {
  print_table(kDryAdjust); print_table(kBoundaryLayer); print_table(kEmanuel); print_table(kSimplePhysics);
  check_plan(kDryAdjust, dry_before); check_plan(kBoundaryLayer, bl_before); check_plan(kEmanuel, emanuel_before); check_plan(kSimplePhysics, sp_before);
  check_aliasing<rrtmg_dry_adjust>(kDryAdjust, " (in place: exactly its own input)", "t, q, pmid, pint, t_out and q_out must be given");
  check_aliasing<rrtmg_boundary_layer>(kBoundaryLayer, " (in place: exactly its own input)", "t, q, u, v, pmid, pint, ps, ts, qs, t_out, q_out, u_out and v_out must be given");
  check_aliasing<rrtmg_emanuel>(kEmanuel, " (in place: exactly cbmf)", "t, q, u, v, pmid, pint, cbmf, ft, fq, fu, fv and cbmf_out must be given");
  check_aliasing<rrtmg_simple_physics>(kSimplePhysics, " (in place: exactly its own input)", "t, q, u, v, pmid, pint, ps, t_out, q_out, u_out and v_out must be given");
  static_assert(column_bits(kBoundaryLayer, {"sh_in", "lh_in"}) == (1u << 9 | 1u << 10), "the bits of the named rows");
  printf("ok\n");
  return 0;
}
