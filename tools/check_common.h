// check_common.h -- what the stand-alone host check programs (tools/*_check.cpp) share: the CHECK that ends a run, the binary files
// of doubles they read and write, the guarded array, and the two bitwise comparisons.  Plain C++, included with a quoted include
// next to the sources; everything is inline, so a program uses what it needs.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

inline bool same_bits(float a, float b) { return memcmp(&a, &b, sizeof a) == 0; }
inline bool same_bits(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
inline bool equal(const std::vector<double> &a, const std::vector<double> &b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), a.size() * sizeof(double)) == 0); }

inline std::vector<double> read_all(const char *path) {
  FILE *f = fopen(path, "rb");
  CHECK(f != nullptr);
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<double> v((size_t)bytes / sizeof(double));
  CHECK(fread(v.data(), sizeof(double), v.size(), f) == v.size());
  fclose(f);
  return v;
}
inline void write_all(const char *path, const std::vector<double> &v) {
  FILE *f = fopen(path, "wb");
  CHECK(f != nullptr);
  CHECK(fwrite(v.data(), sizeof(double), v.size(), f) == v.size());
  fclose(f);
}

// An array of doubles between two runs of guard elements; what is not copied in is poison (or `fill`: a program whose rule may
// legitimately write the poison's value, or that wants to see untouched elements as something else).
constexpr size_t kGuard = 8;
constexpr double kPoison = -777.25;
struct Guarded {
  std::vector<double> v;
  size_t n = 0;
  void set(const double *src, size_t len, double fill = kPoison) {
    n = len; v.assign(len + 2 * kGuard, fill);
    for (size_t g = 0; g < kGuard; ++g) v[g] = v[kGuard + len + g] = kPoison;
    if (src) memcpy(v.data() + kGuard, src, len * sizeof(double));
  }
  double *p() { return v.data() + kGuard; }
  void check_guards() const { for (size_t g = 0; g < kGuard; ++g) CHECK(v[g] == kPoison && v[kGuard + n + g] == kPoison); }
  bool holds(const double *src) { return memcmp(p(), src, n * sizeof(double)) == 0; }
  bool untouched() { for (size_t i = 0; i < n; ++i) if (p()[i] != kPoison) return false; return true; }
  bool written() { for (size_t i = 0; i < n; ++i) if (p()[i] == kPoison) return false; return true; }
  std::vector<double> get() { return std::vector<double>(p(), p() + n); }
};
