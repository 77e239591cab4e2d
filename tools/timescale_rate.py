#!/usr/bin/env python3
"""What the pair time-scale pass costs, beside the neighbour pass as the yardstick: in ONE process on one device, at every N asked for,
NBody.neighbors() over all rows in both loop forms (NBODY_NEIGHBORS_LOOP = 1 the scan — the time-scale pass's loop shape less one
source stream and one division — and 2 the window form, the default), then NBody.timescales() over all rows with the source split
automatic and forced to 1, 4 and 16 chunks, and NBody.min_timescale().  One warm-up call and --reps timed calls per configuration,
alternating the configurations, timed on the host around the synchronous entry point (launch, stream sync, copy back).  One line per
configuration: rows x sources per second; then the ratio to the neighbour pass's scan form.  The table of profiles/r09_timescale.txt.
usage (GPU box): python tools/timescale_rate.py [--n N [N ...]] [--reps R] [--fp64]
For the kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/timescale_rate.py`."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def equal(a, b):
    """the same values: floats, or tuples of arrays, scalars and None"""
    if isinstance(a, tuple):
        return all(equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a is b or a == b


def with_env(name, value, fn):
    def run():
        if value is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = value
        out = fn()
        os.environ.pop(name, None)
        return out
    return run


def measure(n, reps, fp64):
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        rows = [("neighbors() scan", with_env("NBODY_NEIGHBORS_LOOP", "1", lambda: eng.neighbors())),
                ("neighbors() window", with_env("NBODY_NEIGHBORS_LOOP", "2", lambda: eng.neighbors())),
                ("timescales() split auto", with_env("NBODY_TIMESCALE_SPLIT", None, lambda: eng.timescales())),
                ("timescales() split 1", with_env("NBODY_TIMESCALE_SPLIT", "1", lambda: eng.timescales())),
                ("timescales() split 4", with_env("NBODY_TIMESCALE_SPLIT", "4", lambda: eng.timescales())),
                ("timescales() split 16", with_env("NBODY_TIMESCALE_SPLIT", "16", lambda: eng.timescales())),
                ("min_timescale()", lambda: eng.min_timescale())]
        first = {name: fn() for name, fn in rows}   # warm-up: every shape the timed calls use
        ms = {name: [] for name, fn in rows}
        same = dict.fromkeys(ms, True)
        for _ in range(reps):   # alternating
            for name, fn in rows:
                t, out = timed(fn)
                ms[name].append(t)
                same[name] &= equal(out, first[name])
        print("N %d %s, %d CUs, clock %d kHz" % (n, "fp64" if fp64 else "fp32", eng.info(nb._lib.INFO_CU_COUNT), eng.info(nb._lib.INFO_CLOCK_KHZ)))
        for name, fn in rows:
            best = min(ms[name])
            print("%-24s rows %8d: %s ms (spread %.3f), %.1f G pairs/s at the fastest, identical results %s"
                  % (name, n, " / ".join("%.3f" % v for v in ms[name]), max(ms[name]) - best, 1e-6 * n * n / best, same[name]), flush=True)
        ok = all(equal(first["timescales() split auto"], first["timescales() split %s" % k]) for k in ("1", "4", "16"))
        ok = ok and equal(first["timescales() split auto"][2], first["neighbors() scan"][1])
        print("every split agrees and d2min is the neighbour pass's d2: %s" % ok)
        base = min(ms["neighbors() scan"])
        for name in ("neighbors() window", "timescales() split auto", "timescales() split 1"):
            print("%s / neighbors() scan: %.2f x the time" % (name, min(ms[name]) / base), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16, 1 << 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fp64", action="store_true")
    a = ap.parse_args()
    for n in a.n:
        measure(n, a.reps, a.fp64)


if __name__ == "__main__":
    main()
