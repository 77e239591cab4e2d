#!/usr/bin/env python3
"""What the radial-count pass costs, beside the neighbour pass's count-only call as the yardstick: in ONE process on one device,
NBody.radial_counts() for n_bins = 4, 8, 16 and 32 in both loop forms (NBODY_HIST_LOOP = 1: the scan, 2: the gated form) with edges
that reach few sources (the last edge 1e-3: a 64-source window rarely holds a body that close to any of a wave's 64 queries) and
edges that reach all of them (the last edge +inf), at --n bodies over all rows and at --big bodies over a window of --rows rows, in
fp32 and fp64, with nbody_neighbors_rows(count only) over the same rows beside them (both through the C entry points into buffers
allocated once); NBody.pair_histogram() at --n and at --big in the same configurations; then NBody.radial_counts_at() for --m points at --big with the split automatic and forced to 1,
and NBody.radial_counts() over all rows at --n with the split automatic and forced to 1 .. 32 (is kQueryFill enough for this pass?).
One warm-up call and --reps timed calls per configuration in interleaved rounds, timed on the host around the synchronous entry point
(launch, stream sync, copy back); median and min per configuration, pairs/s at the fastest.  The table of profiles/r10_hist_rate.txt.
usage (GPU box): python tools/hist_rate.py [--n N] [--big N] [--rows R] [--m M] [--reps R] [--timeout SECONDS]
The measurement runs in a child process under a time limit (--timeout, default 900 s): this process never opens the device, and a
child that hangs is killed, not waited for.  For the kernels' own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/hist_rate.py --worker`."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINS = (4, 8, 16, 32)
FEW = 1e-3   # the last edge of the edges that reach few sources


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def with_env(env, fn):
    def run():
        os.environ.update(env)
        try:
            return fn()
        finally:
            for k in env:
                os.environ.pop(k, None)
    return run


def edges_of(n_bins, reach, dtype):
    if reach == "few":
        e = np.geomspace(1e-6, FEW, n_bins + 1).astype(dtype)
    else:
        e = np.geomspace(1e-3, 16, n_bins + 1).astype(dtype)
        e[-1] = np.inf
    e[0] = 0
    return e


def measure(rows, reps):
    """rows: (name, pairs of a call, fn) -> {name: first result}"""
    first = {name: np.array(fn(), copy=True) for name, pairs, fn in rows}   # warm-up: every shape the timed calls use (a copy: calls may share a buffer)
    ms = {name: [] for name, pairs, fn in rows}
    same = dict.fromkeys(ms, True)
    for _ in range(reps):   # interleaved rounds
        for name, pairs, fn in rows:
            t, out = timed(fn)
            ms[name].append(t)
            same[name] &= np.array_equal(out, first[name])
    for name, pairs, fn in rows:
        v = ms[name]
        print("%-44s median %10.3f ms, min %10.3f (%s), %8.1f G pairs/s at the fastest, identical results %s"
              % (name, statistics.median(v), min(v), " / ".join("%.3f" % x for x in v), 1e-6 * pairs / min(v), same[name]), flush=True)
    return first


def hist_rows(call, pairs, dtype, label, bins=BINS):
    rows = []
    for nb in bins:
        for reach in ("few", "all"):
            for loop in ("1", "2"):
                e = edges_of(nb, reach, dtype)
                rows.append(("%s %2d bins %s loop %s" % (label, nb, reach, loop), pairs, with_env({"NBODY_HIST_LOOP": loop}, (lambda e: lambda: call(e))(e))))
    return rows


def check_forms_agree(first, label, bins=BINS):
    ok = all(np.array_equal(first["%s %2d bins %s loop 1" % (label, nb, reach)], first["%s %2d bins %s loop 2" % (label, nb, reach)])
             for nb in bins for reach in ("few", "all"))
    print("%s: loop 1 and loop 2 agree: %s" % (label, ok), flush=True)


def into_buffers(nb, eng, cnt):
    """(radial_counts, neighbors count) over rows [first, first + cnt) through the C entry points into ONE pair of buffers allocated
    here: NBody.radial_counts() returns a fresh numpy array per call, and the first touch of its pages (up to 8 MB at 32 bins) by the
    blocking copy back showed up as rounds several times slower than their neighbours, for the same kernel, in an earlier table"""
    lib, fp = eng.lib, C.POINTER(C.c_double if eng.fp64 else C.c_float)
    counts = np.zeros(cnt * nb._lib.HIST_MAX_BINS, np.int32)
    near = np.zeros(cnt, np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))

    def radial(e, first):
        fn = lib.nbody_radial_counts_rows_d if eng.fp64 else lib.nbody_radial_counts_rows
        nb._lib.check(fn(first, cnt, e.ctypes.data_as(fp), len(e) - 1, ip(counts)))
        return counts[:cnt * (len(e) - 1)].reshape(cnt, len(e) - 1)

    def neighbors(r2, first):
        fn = lib.nbody_neighbors_rows_d if eng.fp64 else lib.nbody_neighbors_rows
        nb._lib.check(fn(first, cnt, None, None, float(eng.dtype(r2)), ip(near)))
        return near
    return radial, neighbors


def block(nb, n, first, cnt, fp64, reps, pair_bins):
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        radial, neighbors = into_buffers(nb, eng, cnt)
        print("N %d %s, rows [%d, %d), %d CUs, clock %d kHz" % (n, "fp64" if fp64 else "fp32", first, first + cnt, eng.info(nb._lib.INFO_CU_COUNT),
                                                               eng.info(nb._lib.INFO_CLOCK_KHZ)))
        pairs = cnt * n
        rows = [("neighbors(r2=%g) count only" % r2, pairs, (lambda r2: lambda: neighbors(r2, first))(r2)) for r2 in (FEW, 16.0)]
        rows += hist_rows(lambda e: radial(e, first), pairs, dtype, "radial_counts")
        got = measure(rows, reps)
        check_forms_agree(got, "radial_counts")
        one = eng.radial_counts(np.array([0, np.nextafter(dtype(FEW), dtype(np.inf))], dtype), first, cnt)[:, 0]
        print("one bin {0, nextafter(r2)} equals the neighbour pass's count: %s" % np.array_equal(one, got["neighbors(r2=%g) count only" % FEW]))
        if pair_bins:
            got = measure(hist_rows(eng.pair_histogram, n * n, dtype, "pair_histogram", pair_bins), reps)
            check_forms_agree(got, "pair_histogram", pair_bins)


def points_block(nb, n, m, reps):
    pos, vel = nb.make_bodies(n)
    pts = (1.5 * nb.make_bodies(m, seed=7)[0]).astype(np.float32)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        print("N %d fp32, m %d points" % (n, m))
        rows = []
        for nbins in (4, 32):
            for loop in ("1", "2"):
                for split in ("auto", "1"):
                    env = {"NBODY_HIST_LOOP": loop}
                    if split != "auto":
                        env["NBODY_HIST_SPLIT"] = split
                    e = edges_of(nbins, "all", np.float32)
                    rows.append(("radial_counts_at %2d bins all loop %s split %s" % (nbins, loop, split), m * n,
                                 with_env(env, (lambda e: lambda: eng.radial_counts_at(pts, e))(e))))
        got = measure(rows, reps)
        names = list(got)
        print("split auto and split 1 agree: %s" % all(np.array_equal(got[a], got[b]) for a, b in zip(names[0::2], names[1::2])))


def fill_block(nb, n, reps):
    """how many workgroups a launch wants: all rows of n bodies with the source split automatic (kQueryFill workgroups per CU) and forced"""
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        print("N %d fp32, all rows (%d workgroups of 256 queries), the source split automatic and forced" % (n, (n + 255) // 256))
        rows = []
        for nbins in (4, 32):
            e = edges_of(nbins, "all", np.float32)
            for split in ("auto", "1", "4", "8", "16", "32"):
                env = {"NBODY_HIST_LOOP": "1"}
                if split != "auto":
                    env["NBODY_HIST_SPLIT"] = split
                rows.append(("radial_counts %2d bins all loop 1 split %s" % (nbins, split), n * n, with_env(env, (lambda e: lambda: eng.radial_counts(e))(e))))
        got = measure(rows, reps)
        names = list(got)
        for k, nbins in enumerate((4, 32)):   # six splits per n_bins
            group = names[6 * k:6 * k + 6]
            print("%2d bins: every split agrees: %s" % (nbins, all(np.array_equal(got[group[0]], got[x]) for x in group[1:])))


def worker(a):
    sys.path.insert(0, ROOT)
    import mini_nbody_amd as nb
    for k in ("NBODY_HIST_LOOP", "NBODY_HIST_SPLIT", "NBODY_HIST_SCRATCH_MB"):
        os.environ.pop(k, None)
    for fp64 in (False, True):
        block(nb, a.n, 0, a.n, fp64, a.reps, BINS)
        block(nb, a.big, (a.big - a.rows) // 2, a.rows, fp64, a.reps, BINS)
    points_block(nb, a.big, a.m, a.reps)
    fill_block(nb, a.n, a.reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--big", type=int, default=1 << 20)
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=900.0)
    ap.add_argument("--worker", action="store_true", help="measure in this process (what the supervising process starts)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + [x for k in ("n", "big", "rows", "m", "reps") for x in ("--" + k, str(getattr(a, k)))]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print("hist_rate: the measurement did not finish within %.0f s and was killed" % a.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
