"""Writes tests/golden/ref_solvar_<case>.npz, the reference values of the shortwave's solar variability at a shape where a
column's position matters (tests/solvar_cases.py), from the reference Fortran in oracle/_ref -- ONE call over the case's 136
columns -- and, for the band rows, our driver of its procedures (tests/refshim/build.sh).  Needs both built (build()).  The
input hashes go into tests/golden/input_hashes.json.  Before a fixture is written it has to discriminate
(solvar_cases.discriminates): the last two sunlit columns still get different multipliers and the returned amplitudes are not
1 -- a fixture whose amplitudes have decayed could be met by a library that ignores a column's position.

    python tests/golden/make_solar_variability.py [case ...]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import numpy as np  # noqa: E402

import solvar_cases as S  # noqa: E402


def main(names):
    if not S.shims_available():
        sys.exit("oracle/_ref or tests/_refshim (tests/refshim/build.sh) is not built")
    pins_path = os.path.join(HERE, "input_hashes.json")
    pins = json.load(open(pins_path))
    for name in names or list(S.CASES):
        arr = S.fixture_arrays(name)
        c, _ = S.case_inputs(name)
        diff, away = S.discriminates(c, arr["sw/swdflx"], arr["indsolvar"])
        if "call2/swdflx" in arr:
            S.discriminates(c, arr["call2/swdflx"], arr["indsolvar2"])
        path = os.path.join(HERE, "ref_solvar_%s.npz" % name)
        np.savez_compressed(path, **arr)
        assert os.path.getsize(path) <= 200 * 1024, (path, os.path.getsize(path))
        pins["ref_solvar_" + name] = str(arr["pin"])
        print("wrote %s (%d bytes): last two sunlit columns differ by %.3e W m-2, max |indsolvar - 1| = %.3e" % (path, os.path.getsize(path), diff, away))
    json.dump(pins, open(pins_path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main(sys.argv[1:])
