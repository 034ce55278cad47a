// rrtmg_share.h -- the table of host inputs that one joint shortwave + longwave call (rrtmg_hip_radiation_fluxes) has already
// brought to the device, and the call's byte accounting.  Plain C++, no HIP: tools/joint_share_check.cpp runs it on the CPU
// under the sanitizers.
//
// Inside ONE call the caller's arrays cannot change, so an identical host pointer means identical content; what the device
// holds for it depends, besides, on how many elements were taken, on the unit factors applied after the upload and on the
// policy that may replace an all-zero array by "absent", and on the element type on the host (8-byte reals, or 4-byte ones in a
// float32-boundary call).  The key is those six; anything that differs in one of them is uploaded on its own.  The table lives for one call: nothing is shared across calls.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace rrtmg {

struct ShareKey {
  const void *host; size_t n; uint64_t mul, div; int policy;   // (mul, div: the factors' bit patterns -- 0.0 and -0.0 differ, a NaN equals itself)
  int elem;                                                    // bytes per element on the host: 8, or 4
  bool operator==(const ShareKey &o) const { return host == o.host && n == o.n && mul == o.mul && div == o.div && policy == o.policy && elem == o.elem; }
};
inline ShareKey share_key(const void *host, size_t n, double mul, double div, int policy, int elem = 8) {
  ShareKey k{host, n, 0, 0, policy, elem};
  memcpy(&k.mul, &mul, sizeof mul); memcpy(&k.div, &div, sizeof div);
  return k;
}

class ShareTable {
 public:
  enum class Found { New, Pending, Hit };
  // New: the key was not there; it is now, unresolved, and the caller (`owner`: 0 shortwave, 1 longwave) brings the array to
  // the device and calls resolve().  Pending: an input registered earlier in the caller's own batch has the key and is not
  // resolved yet: take() once the batch is.  Hit: resolved.  *index: the entry, for resolve / take / owner_of.
  Found acquire(const ShareKey &k, int owner, int *index) {
    for (size_t i = 0; i < e_.size(); ++i)
      if (e_[i].key == k) { *index = (int)i; return e_[i].resolved ? Found::Hit : Found::Pending; }
    e_.push_back(Entry{k, nullptr, 0, owner, false});
    *index = (int)e_.size() - 1;
    return Found::New;
  }
  // what the device holds for the entry: dev (nullptr: all zero, absent) and the H2D bytes it took (0: filled, or absent)
  void resolve(int index, const double *dev, size_t copied_bytes) {
    Entry &e = e_[(size_t)index];
    e.dev = dev; e.bytes = copied_bytes; e.resolved = true;
    bytes_uploaded_ += (long long)copied_bytes;
  }
  bool resolved(int index) const { return e_[(size_t)index].resolved; }
  int owner_of(int index) const { return e_[(size_t)index].owner; }
  // a second taker of a resolved entry: counted, nothing scanned, copied or scaled
  const double *take(int index) {
    const Entry &e = e_[(size_t)index];
    ++arrays_shared_; bytes_shared_ += (long long)e.bytes;
    return e.dev;
  }
  // a batch that failed leaves no key behind that nobody will resolve: the next batch uploads such an array itself
  void drop_unresolved() {
    size_t w = 0;
    for (size_t i = 0; i < e_.size(); ++i)
      if (e_[i].resolved) { if (w != i) e_[w] = e_[i]; ++w; }
    e_.resize(w);
  }
  size_t size() const { return e_.size(); }
  int arrays_shared() const { return arrays_shared_; }
  long long bytes_uploaded() const { return bytes_uploaded_; }
  long long bytes_shared() const { return bytes_shared_; }

 private:
  struct Entry { ShareKey key; const double *dev; size_t bytes; int owner; bool resolved; };
  std::vector<Entry> e_;
  int arrays_shared_ = 0;
  long long bytes_uploaded_ = 0, bytes_shared_ = 0;
};

}  // namespace rrtmg
