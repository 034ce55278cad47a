// joint_share_check.cpp -- the joint call's sharing table and byte accounting (climt_amd/csrc/rrtmg_share.h) on the CPU, no
// device: a stand-alone program for the host sanitizers.
//
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/joint_share_check.cpp -o joint_share_check && ./joint_share_check
//
// It plays the two batches of a joint call the way HostInputs::finish does -- acquire every input, bring the new ones "to the
// device" (resolve: uploaded, filled, or absent), take the rest -- and checks keys, lookups, counters and the clean-up after a
// batch that failed.  Exit status 0 and "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../climt_amd/csrc/rrtmg_share.h"
#include "check_common.h"

using namespace rrtmg;

struct Input { const double *host; size_t n; double mul, div; int policy; int how; };   // how: 0 upload, 1 fill, 2 absent

// one HostInputs::finish: -> the device pointers the inputs got
static std::vector<const double *> batch(ShareTable &t, int owner, const std::vector<Input> &in, std::vector<double> &device, bool fail_first_upload = false) {
  std::vector<int> idx(in.size());
  std::vector<bool> taken(in.size());
  std::vector<const double *> slot(in.size(), nullptr);
  for (size_t i = 0; i < in.size(); ++i)
    taken[i] = t.acquire(share_key(in[i].host, in[i].n, in[i].mul, in[i].div, in[i].policy), owner, &idx[i]) != ShareTable::Found::New;
  bool failed = false;
  for (size_t i = 0; i < in.size(); ++i) {
    if (taken[i]) continue;
    if (in[i].how == 0 && fail_first_upload && !failed) { failed = true; continue; }
    if (in[i].how == 2) { t.resolve(idx[i], nullptr, 0); continue; }
    device.push_back(0.0);
    slot[i] = &device.back();
    t.resolve(idx[i], slot[i], in[i].how == 0 ? in[i].n * sizeof(double) : 0);
  }
  for (size_t i = 0; i < in.size(); ++i)
    if (taken[i] && t.resolved(idx[i])) slot[i] = t.take(idx[i]);
  t.drop_unresolved();
  return slot;
}

int main() {
  std::vector<double> device;
  device.reserve(256);   // (addresses stay valid: they stand for device pointers)
  std::vector<double> play(100), plev(101), co2(100), taucld(1400), q(100);
  const size_t B = sizeof(double);

  // keys: every one of the five parts separates
  {
    const ShareKey k = share_key(play.data(), 100, 0.01, 0.0, 0);
    CHECK(k == share_key(play.data(), 100, 0.01, 0.0, 0));
    CHECK(!(k == share_key(plev.data(), 100, 0.01, 0.0, 0)));
    CHECK(!(k == share_key(play.data(), 99, 0.01, 0.0, 0)));
    CHECK(!(k == share_key(play.data(), 100, 0.0, 0.0, 0)));
    CHECK(!(k == share_key(play.data(), 100, 0.01, 2.0, 0)));
    CHECK(!(k == share_key(play.data(), 100, 0.01, 0.0, 1)));
    CHECK(!(share_key(play.data(), 100, 0.0, 0.0, 0) == share_key(play.data(), 100, -0.0, 0.0, 0)));
  }
  // a joint call: the shortwave's batch, then the longwave's
  {
    ShareTable t;
    const std::vector<Input> sw = {{play.data(), 100, 0.01, 0, 0, 0}, {plev.data(), 101, 0.01, 0, 0, 0}, {co2.data(), 100, 0, 0, 0, 1},
                                   {taucld.data(), 1400, 0, 0, 1, 2}, {q.data(), 100, 28.964, 18.02, 0, 0}};
    const std::vector<const double *> s = batch(t, 0, sw, device);
    CHECK(t.size() == 5 && t.arrays_shared() == 0 && t.bytes_shared() == 0);
    CHECK(t.bytes_uploaded() == (long long)((100 + 101 + 100) * B));
    CHECK(s[0] && s[1] && s[2] && !s[3] && s[4]);
    // same pointers and factors: taken; another count (1600 against 1400 elements), another factor, another pointer: its own
    const std::vector<Input> lw = {{play.data(), 100, 0.01, 0, 0, 0}, {plev.data(), 101, 0.01, 0, 0, 0}, {co2.data(), 100, 0, 0, 0, 1},
                                   {taucld.data(), 1600, 0, 0, 1, 0}, {q.data(), 100, 1.6, 0, 0, 0}, {plev.data() + 1, 100, 0.01, 0, 0, 0},
                                   {taucld.data(), 1400, 0, 0, 1, 2}};
    const std::vector<const double *> l = batch(t, 1, lw, device);
    CHECK(l[0] == s[0] && l[1] == s[1] && l[2] == s[2] && l[6] == nullptr);
    CHECK(l[3] && l[3] != s[3] && l[4] && l[4] != s[4] && l[5] && l[5] != s[1]);
    CHECK(t.arrays_shared() == 4);                                        // play, plev, co2 (filled) and taucld (absent)
    CHECK(t.bytes_shared() == (long long)((100 + 101) * B));              // the filled and the absent one count 0
    CHECK(t.bytes_uploaded() == (long long)((100 + 101 + 100 + 1600 + 100 + 100) * B));
    CHECK(t.owner_of(0) == 0 && t.owner_of(5) == 1 && t.size() == 8);
  }
  // one array twice in ONE batch (cicewp and cliqwp as the same pointer): the second waits for the first, then takes it
  {
    ShareTable t;
    const std::vector<const double *> s = batch(t, 0, {{q.data(), 100, 0, 0, 0, 0}, {q.data(), 100, 0, 0, 0, 0}}, device);
    CHECK(s[0] && s[0] == s[1] && t.size() == 1 && t.arrays_shared() == 1);
    CHECK(t.bytes_uploaded() == (long long)(100 * B) && t.bytes_shared() == (long long)(100 * B));
  }
  // a batch whose upload failed leaves no key behind: the next batch brings the array itself
  {
    ShareTable t;
    const std::vector<const double *> s = batch(t, 0, {{play.data(), 100, 0, 0, 0, 0}, {play.data(), 100, 0, 0, 0, 0}, {co2.data(), 100, 0, 0, 0, 1}}, device, true);
    CHECK(!s[0] && !s[1] && s[2] && t.size() == 1 && t.arrays_shared() == 0 && t.bytes_uploaded() == 0);
    const std::vector<const double *> l = batch(t, 1, {{play.data(), 100, 0, 0, 0, 0}, {co2.data(), 100, 0, 0, 0, 1}}, device);
    CHECK(l[0] && l[1] == s[2] && t.size() == 2 && t.arrays_shared() == 1 && t.owner_of(1) == 1);
    CHECK(t.bytes_uploaded() == (long long)(100 * B) && t.bytes_shared() == 0);
  }
  // many entries: the table grows, lookups stay exact
  {
    ShareTable t;
    std::vector<double> big(4096);
    int idx = -1;
    for (size_t i = 0; i < big.size(); ++i) { CHECK(t.acquire(share_key(&big[i], 1, 0, 0, 0), 0, &idx) == ShareTable::Found::New); t.resolve(idx, &big[i], B); }
    for (size_t i = 0; i < big.size(); ++i) { CHECK(t.acquire(share_key(&big[i], 1, 0, 0, 0), 1, &idx) == ShareTable::Found::Hit); CHECK(t.take(idx) == &big[i]); }
    CHECK(t.size() == big.size() && t.arrays_shared() == (int)big.size() && t.bytes_shared() == t.bytes_uploaded());
  }
  puts("ok");
  return 0;
}
