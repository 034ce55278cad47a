"""Writes tests/golden/column_call_python.json: what the eleven column-component methods of climt_amd._lib.Context put into
their structs, return and refuse (tests/column_call_python_cases.py), recorded against a stand-in library -- no .so, no device.
The committed file was made at commit 49b6b10, before COLUMN_ARRAYS became the single description of an entry's arrays and
cork_longwave went through Context._column_call; tests/test_column_call_python.py holds every later _lib.py to it.

    python tests/golden/make_column_call_python_golden.py [out.json]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import column_call_python_cases as X  # noqa: E402

if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "column_call_python.json")
    with open(out, "w") as f:
        f.write(X.dumps(X.record()) + "\n")
    print("wrote", out)
