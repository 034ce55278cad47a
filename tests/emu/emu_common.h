// TEST INFRASTRUCTURE ONLY -- what the emulation drivers of emu_sw.hip and emu_lw.hip do alike: the error return, the table
// set-up and the McICA mask.  Header only; never seen by the product.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "../../climt_amd/csrc/rrtmg_kiss_host.h"
#include "../../climt_amd/csrc/rrtmg_tables.h"

namespace rrtmg {
void mt_mask_host(int ncol, int nlay, int nsub, int icld, int seed, const double *cldfr, std::vector<uint64_t> &mask, int nw, int col0 = 0, int ncol_total = 0);

// `return fail(code, message)`: the message into the caller's buffer (which may be NULL), the code back
struct EmuFail {
  char *errbuf;
  int errlen;
  int operator()(int code, const std::string &m) const {
    if (errbuf) { strncpy(errbuf, m.c_str(), errlen - 1); errbuf[errlen - 1] = 0; }
    return code;
  }
};

// blob file -> tables of one spectrum ("sw" | "lw") and the ten physical constants in the order of tests/helpers.py
inline bool emu_tables(const char *blob_path, const char *which, double cpdair, const double *consts, TableSet &ts, Constants &k, std::string &err) {
  Blob blob;
  if (!blob.load(blob_path, err)) return false;
  k = Constants{};
  k.pi = consts[0]; k.grav = consts[1]; k.planck = consts[2]; k.boltz = consts[3]; k.clight = consts[4];
  k.avogad = consts[5]; k.alosmt = consts[6]; k.gascon = consts[7]; k.sbcnst = consts[8]; k.secdy = consts[9];
  return build_tables(blob, which, cpdair, k.grav, k.secdy, ts, err);
}

// The McICA mask [nsub][nw][ncol] of a call (a: rrtmg_sw_args | rrtmg_lw_args): from the sub-columns given (cldfmcl), from
// kissvec (irng = 0) or from the Mersenne twister's host stream
template <class Args>
uint64_t *emu_mcica_mask(const Args *a, int nsub, int icld, int nw, int *err, std::vector<uint64_t> &mask) {
  const int N = a->ncol, L = a->nlay;
  mask.assign((size_t)nsub * nw * N, 0);
  if (a->cldfmcl) {
    for (int g = 0; g < nsub; ++g) for (int l = 0; l < L; ++l) for (int c = 0; c < N; ++c)
      if (a->cldfmcl[((size_t)l * N + c) * nsub + g] > 1.e-12) mask[((size_t)g * nw + (l >> 6)) * N + c] |= 1ull << (l & 63);
  } else if (a->irng == 0) {
    for (int c = 0; c < N; ++c) kiss_mask_column(N, L, nsub, icld, a->permuteseed, a->play, a->cldfr, mask.data(), nw, err, c);
  } else {
    mt_mask_host(N, L, nsub, icld, a->permuteseed, a->cldfr, mask, nw, a->shard_col0, a->shard_ncol);
  }
  return mask.data();
}
}  // namespace rrtmg
