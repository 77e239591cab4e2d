#!/usr/bin/env python3
"""What the neighbour pass costs, beside the energy pass as the yardstick: in ONE process on one device, NBody.neighbors() over all
rows at N bodies with the count off and on, in both loop forms (NBODY_NEIGHBORS_LOOP = 1 the scan, 2 the window form), NBody.energy()
between them, then NBody.nearest() for M points with the split automatic and forced to 1.  One warm-up call and --reps timed calls per
configuration, alternating the configurations, timed on the host around the synchronous entry point (launch, stream sync, copy back).
One line per configuration; the table of profiles/r08_neighbors.txt.
usage (GPU box): python tools/neighbors_rate.py [--n N] [--m M] [--reps R] [--fp64]
For the kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/neighbors_rate.py`."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fp64", action="store_true")
    a = ap.parse_args()
    dtype = np.float64 if a.fp64 else np.float32
    n, m = a.n, a.m
    pos, vel = nb.make_bodies(n, dtype=dtype)
    pts = (1.5 * nb.make_bodies(m, seed=7, dtype=dtype)[0]).astype(dtype)
    r2 = dtype(1e-4)

    def loop(form, fn):
        def run():
            os.environ["NBODY_NEIGHBORS_LOOP"] = form
            out = fn()
            os.environ.pop("NBODY_NEIGHBORS_LOOP", None)
            return out
        return run

    def split(value, fn):
        def run():
            if value == "auto":
                os.environ.pop("NBODY_NEIGHBORS_SPLIT", None)
            else:
                os.environ["NBODY_NEIGHBORS_SPLIT"] = value
            out = fn()
            os.environ.pop("NBODY_NEIGHBORS_SPLIT", None)
            return out
        return run

    with nb.NBody(n, fp64=a.fp64) as eng:
        eng.upload(pos, vel)
        rows = [("energy()", n, lambda: eng.energy()["potential"]),
                ("neighbors() scan", n, loop("1", lambda: eng.neighbors())),
                ("neighbors() window", n, loop("2", lambda: eng.neighbors())),
                ("neighbors(r2) scan", n, loop("1", lambda: eng.neighbors(r2=r2))),
                ("neighbors(r2) window", n, loop("2", lambda: eng.neighbors(r2=r2))),
                ("closest_pair() default", n, lambda: eng.closest_pair()),
                ("nearest(m) split auto", m, split("auto", lambda: eng.nearest(pts))),
                ("nearest(m) split 1", m, split("1", lambda: eng.nearest(pts)))]
        os.environ.pop("NBODY_NEIGHBORS_LOOP", None)
        first = {name: fn() for name, q, fn in rows}   # warm-up: every shape the timed calls use
        ms = {name: [] for name, q, fn in rows}
        same = dict.fromkeys(ms, True)
        for _ in range(a.reps):   # alternating
            for name, q, fn in rows:
                t, out = timed(fn)
                ms[name].append(t)
                same[name] &= equal(out, first[name])
        clock = eng.info(nb._lib.INFO_CLOCK_KHZ)
        print("N %d %s, m %d, %d CUs, clock %d kHz" % (n, "fp64" if a.fp64 else "fp32", m, eng.info(nb._lib.INFO_CU_COUNT), clock))
        for name, q, fn in rows:
            best = min(ms[name])
            print("%-24s queries %8d: %s ms (spread %.3f), %.1f G pairs/s at the fastest, identical results %s"
                  % (name, q, " / ".join("%.3f" % v for v in ms[name]), max(ms[name]) - best, 1e-6 * q * n / best, same[name]), flush=True)
        ok = equal(first["neighbors() scan"], first["neighbors() window"]) and equal(first["neighbors(r2) scan"], first["neighbors(r2) window"])
        print("scan and window forms agree: %s" % ok)


if __name__ == "__main__":
    main()
