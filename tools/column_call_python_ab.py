"""Python time per call of the column components' array path (Context._column_call), on the CPU with no library: the
methods are driven with device pointers (memspace=1) against a stand-in whose entries return 0, so what is timed is the
struct's scalar setup, the extent lookup and the pointer binding -- everything the Python layer adds to a device call.

    python tools/column_call_python_ab.py [calls]      (default 20000; run it in three processes and take the median)

Prints one line per method: microseconds per call (the best of five batches, which is what the interpreter can do).
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import column_call_python_cases as X  # noqa: E402


class SilentLibrary:
    def __getattr__(self, name):
        if not name.startswith("rrtmg_hip_"):
            raise AttributeError(name)
        return lambda handle, ref: 0


def main(calls):
    for name in ("cork_longwave", "boundary_layer", "second_best"):
        v, ctx = X.Variant(name), X.make_context(SilentLibrary())
        A, O, D = v.pointers(v.IN, 0x10000000), v.pointers(v.OUT, 0x20000000), v.pointers(v.DIAG, 0x30000000)
        best = float("inf")
        for batch in range(5):
            t0 = time.perf_counter()
            for i in range(calls // 5):
                v.call(ctx, A, O, D, memspace=1, **v.sizes())
            best = min(best, (time.perf_counter() - t0) / (calls // 5))
        print("%-16s %7.2f us per call (%d calls)" % (v.method, best * 1e6, calls))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20000)
