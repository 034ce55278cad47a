"""Writes tests/golden/ref_swcomp_<case>.npz, the reference values of the shortwave flux components (tests/swcomp_cases.py),
from the reference Fortran in oracle/_ref and our driver of its procedures (tests/refshim).  Needs both built (build()).

    python tests/golden/make_sw_components.py [case ...]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import swcomp_cases as S  # noqa: E402


def main(names):
    if not S.shim_available():
        sys.exit("oracle/_ref or tests/_refshim is not built")
    for name in names or list(S.CASES):
        path = os.path.join(HERE, "ref_swcomp_%s.npz" % name)
        np.savez_compressed(path, **S.fixture_arrays(name))
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1:])
