"""Writes tests/golden/ref_albedo_<case>.npz, the reference values of the shortwave with the surface albedo by band
(tests/albedo_cases.py), from the reference Fortran in oracle/_ref and our driver of its procedures
(tests/refshim/build.sh).  Needs both built (build()).  Before a fixture is written the driver checks itself: with
the per-band albedos filled by the reference driver's band rule it reproduces the binder's six outputs bit for bit.

    python tests/golden/make_spectral_albedo.py [case ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import albedo_cases as A  # noqa: E402


def main(names):
    if not A.shim_available():
        sys.exit("oracle/_ref or tests/_refshim/libsw_shim.so (tests/refshim/build.sh) is not built")
    for name in names or list(A.CASES):
        arr = A.fixture_arrays(name)      # (asserts shim == binder under the band rule)
        albdir, albdif = arr["in/albdir"], arr["in/albdif"]
        assert albdir.min() >= 0.02 and albdir.max() <= 0.95 and albdif.min() >= 0.02 and albdif.max() <= 0.95
        assert np.all(albdir != albdif) and all(len(set(col)) == A.NBAND for a in (albdir, albdif) for col in a.T)
        path = os.path.join(HERE, "ref_albedo_%s.npz" % name)
        np.savez_compressed(path, **arr)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1:])
