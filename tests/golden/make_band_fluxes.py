"""Writes tests/golden/ref_bands_<case>.npz, the reference values of the fluxes by band (tests/band_cases.py), from the
reference Fortran in oracle/_ref and our drivers of its procedures (tests/refshim/build.sh).  Needs both built
(build()).  Before a fixture is written the shims check themselves: over the full band range they reproduce the binder's
broadband outputs bit for bit, and the per-band rows sum to that broadband within the rounding bound.

    python tests/golden/make_band_fluxes.py [case ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import band_cases as B  # noqa: E402


def self_check(name):
    which = name[:2]
    _, binder, out = B.reference(name)
    for i, m in enumerate(B.MEMBERS[which]):
        bb = B.BROADBAND[which].get(m)
        if bb is not None:
            assert np.array_equal(out[0, i], binder[bb]), (name, m, "full-range call != binder")
        full = out[0, i]
        assert np.all(out[1:, i] >= 0.0), (name, m)
        assert np.all(np.abs(out[1:, i].sum(axis=0) - full) <= B.SUM_BOUND * np.abs(full)), (name, m, "bands do not sum to the broadband")


def main(names):
    if not B.shims_available():
        sys.exit("oracle/_ref or tests/_refshim (tests/refshim/build.sh) is not built")
    for name in names or list(B.CASES):
        self_check(name)
        path = os.path.join(HERE, "ref_bands_%s.npz" % name)
        np.savez_compressed(path, **B.fixture_arrays(name))
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1:])
