"""Host cost of one call through the ctypes binding, no GPU: avt_clip_sample_table (host-only, returns a status) into preallocated
buffers, as `_lib.check(_lib.lib().avt_X(...), "avt_X")` (the call sites' form before the checked namespace) and as
`_lib.checked.avt_X(...)`, in alternating repeats.  Prints ns per call for every repeat, then mean and standard deviation per form.

    python tools/bench_binding_call.py [CALLS_PER_REPEAT=300000] [REPEATS=7]
"""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avtex import _lib  # noqa: E402

K = _lib.checked


def via_check(n, f, s):
    for _ in range(n):
        _lib.check(_lib.lib().avt_clip_sample_table(20, f, s), "avt_clip_sample_table")


def via_checked(n, f, s):
    for _ in range(n):
        K.avt_clip_sample_table(20, f, s)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 300000
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    fast, slow = np.empty(32, np.int32), np.empty(8, np.int32)
    f, s = fast.ctypes.data, slow.ctypes.data
    forms = (("check(lib().avt_X())", via_check), ("checked.avt_X()", via_checked))
    for _, fn in forms:
        fn(n // 10, f, s)
    ns = {name: [] for name, _ in forms}
    for r in range(reps):
        for name, fn in forms:
            t0 = time.perf_counter()
            fn(n, f, s)
            ns[name].append((time.perf_counter() - t0) / n * 1e9)
        print("repeat %d: " % r + ", ".join("%s %.1f ns" % (name, ns[name][-1]) for name, _ in forms))
    for name, _ in forms:
        print("%-22s mean %.1f ns, stdev %.1f ns, fastest %.1f ns over %d repeats of %d calls"
              % (name, statistics.mean(ns[name]), statistics.stdev(ns[name]), min(ns[name]), reps, n))


if __name__ == "__main__":
    main()
