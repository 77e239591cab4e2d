#!/usr/bin/env python3
"""What the k-nearest-neighbour pass costs, beside the neighbour pass as the yardstick: in ONE process on one device,
NBody.knn(k) over all rows at N bodies for k = 1, 8 and 32 with NBody.neighbors() (its window form, the default) beside them, in fp32
at --n and in fp64 at --n64, then NBody.knn_at() for M points at --n with the split automatic and forced to 1.  One warm-up call and
--reps timed calls per configuration in interleaved rounds, timed on the host around the synchronous entry point (launch, stream sync,
copy back); median and min per configuration.  Both passes do the same first walk over the sources, so the expectation to confirm or
refute is that knn(1) costs about what neighbors() costs: "about" is twice the spread between the repeated neighbors() rounds of this
run, and the last line of each block says on which side knn(1) fell.  The table of profiles/r08_knn_rate.txt.
usage (GPU box): python tools/knn_rate.py [--n N] [--n64 N] [--m M] [--reps R] [--timeout SECONDS]
The measurement runs in a child process under a time limit (--timeout, default 600 s): this process never opens the device, and a
child that hangs is killed, not waited for.  For the kernels' own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/knn_rate.py --worker`."""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (1, 8, 32)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def equal(a, b):
    """the same values: tuples of arrays and None"""
    if isinstance(a, tuple):
        return all(equal(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    return a is b or a == b


def split(value, fn):
    def run():
        if value == "auto":
            os.environ.pop("NBODY_KNN_SPLIT", None)
        else:
            os.environ["NBODY_KNN_SPLIT"] = value
        out = fn()
        os.environ.pop("NBODY_KNN_SPLIT", None)
        return out
    return run


def measure(nb, eng, rows, reps, n):
    first = {name: fn() for name, q, fn in rows}   # warm-up: every shape the timed calls use
    ms = {name: [] for name, q, fn in rows}
    same = dict.fromkeys(ms, True)
    for _ in range(reps):   # interleaved rounds
        for name, q, fn in rows:
            t, out = timed(fn)
            ms[name].append(t)
            same[name] &= equal(out, first[name])
    for name, q, fn in rows:
        v = ms[name]
        print("%-26s queries %8d: median %9.3f ms, min %9.3f (spread %.3f; %s), %.1f G pairs/s at the fastest, identical results %s"
              % (name, q, statistics.median(v), min(v), max(v) - min(v), " / ".join("%.3f" % x for x in v), 1e-6 * q * n / min(v), same[name]),
              flush=True)
    return first, ms


def rows_block(nb, n, fp64, reps):
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        print("N %d %s, %d CUs, clock %d kHz" % (n, "fp64" if fp64 else "fp32", eng.info(nb._lib.INFO_CU_COUNT), eng.info(nb._lib.INFO_CLOCK_KHZ)))
        rows = [("neighbors()", n, lambda: eng.neighbors())] + [("knn(%d)" % k, n, (lambda k: lambda: eng.knn(k))(k)) for k in KS]
        first, ms = measure(nb, eng, rows, reps, n)
        ok = equal((first["knn(1)"][0][:, 0], first["knn(1)"][1][:, 0]), first["neighbors()"][:2])
        near, one = ms["neighbors()"], ms["knn(1)"]
        margin = 2 * (max(near) - min(near))
        diff = statistics.median(one) - statistics.median(near)
        print("knn(1) column 0 equals neighbors(): %s" % ok)
        print("knn(1) - neighbors() = %+.3f ms at the medians (%+.1f %%); margin 2 x the neighbors() spread = %.3f ms: %s"
              % (diff, 100 * diff / statistics.median(near), margin, "within" if abs(diff) <= margin else "OUTSIDE"), flush=True)


def points_block(nb, n, m, reps):
    pos, vel = nb.make_bodies(n)
    pts = (1.5 * nb.make_bodies(m, seed=7)[0]).astype(np.float32)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        print("N %d fp32, m %d" % (n, m))
        rows = []
        for k in KS:
            rows.append(("knn_at(m, %d) split auto" % k, m, split("auto", (lambda k: lambda: eng.knn_at(pts, k))(k))))
            rows.append(("knn_at(m, %d) split 1" % k, m, split("1", (lambda k: lambda: eng.knn_at(pts, k))(k))))
        first, ms = measure(nb, eng, rows, reps, n)
        print("split auto and split 1 agree: %s" % all(equal(first["knn_at(m, %d) split auto" % k], first["knn_at(m, %d) split 1" % k]) for k in KS))


def worker(a):
    sys.path.insert(0, ROOT)
    import mini_nbody_amd as nb
    rows_block(nb, a.n, False, a.reps)
    rows_block(nb, a.n64, True, a.reps)
    points_block(nb, a.n, a.m, a.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--n64", type=int, default=1 << 18)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=600.0)
    ap.add_argument("--worker", action="store_true", help="measure in this process (what the supervising process starts)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(a.n), "--n64", str(a.n64), "--m", str(a.m), "--reps", str(a.reps)]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print("knn_rate: the measurement did not finish within %.0f s and was killed" % a.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
