#!/usr/bin/env python3
"""What the friends-of-friends pass costs, beside the neighbour pass as the yardstick: in ONE process on one device, at N bodies fp32,
NBody.neighbors(r2=b2) over all rows (its window form, the default, with the count on) and NBody.fof(b2) at linking lengths of 0.2,
0.7 and 1.5 mean spacings, each once more with NBODY_FOF_ALL_ROWS=1.  One warm-up call and --reps timed calls per configuration in
interleaved rounds, timed on the host around the synchronous entry point (uploads, launches, stream syncs, copies back and the host's
union-find); median and min per configuration, with the rounds of the call and the rows it walked in total (NBODY_FOF_TRACE=1 makes
the library print them per round).  One round over all rows does the neighbour pass's first walk with one compare in place of the
count, so the expectation to confirm or refute is that one round over all rows costs about what neighbors() costs: a call's median over
its `rows walked / N` passes' worth of rows against the neighbors() median, "about" being twice the spread between the repeated
neighbors() rounds of this run; the last lines say on which side each linking length fell.  The table of profiles/r09_fof_rate.txt.
usage (GPU box): python tools/fof_rate.py [--n N] [--reps R] [--timeout SECONDS]
The measurement runs in a child process under a time limit (--timeout, default 600 s): this process never opens the device, and a
child that hangs is killed, not waited for.  For the kernels' own time run it under
`rocprofv3 --kernel-trace --stats -- python tools/fof_rate.py --worker`."""
import argparse
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = (0.2, 0.7, 1.5)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def with_env(name, value, fn):
    def run():
        os.environ[name] = value
        try:
            return fn()
        finally:
            os.environ.pop(name, None)
    return run


def parse_trace(text):
    """[(round, rows walked, rows that reported)] from the library's NBODY_FOF_TRACE lines"""
    return [tuple(int(v) for v in m) for m in re.findall(r"nbody_fof: round (\d+): (\d+) rows, (\d+) reported", text)]


def traced(fn):
    """fn() with NBODY_FOF_TRACE=1 and the process's stderr in a file: (the trace's rounds, fn's result)"""
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+") as f:
        keep = os.dup(2)
        os.dup2(f.fileno(), 2)
        try:
            out = with_env("NBODY_FOF_TRACE", "1", fn)()
        finally:
            os.dup2(keep, 2)
            os.close(keep)
        f.seek(0)
        return parse_trace(f.read()), out


def worker(a):
    sys.path.insert(0, ROOT)
    import mini_nbody_amd as nb
    n = a.n
    pos, vel = nb.make_bodies(n)
    b2 = {r: np.float32((r * 2.0 / n ** (1.0 / 3.0)) ** 2) for r in RATIOS}
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        print("N %d fp32, %d CUs, clock %d kHz" % (n, eng.info(nb._lib.INFO_CU_COUNT), eng.info(nb._lib.INFO_CLOCK_KHZ)))
        rows = [("neighbors(r2=b2(0.7))", lambda: eng.neighbors(r2=b2[0.7]))]
        for r in RATIOS:
            call = (lambda r: lambda: eng.fof(b2[r]) + (eng.fof_rounds,))(r)
            rows.append(("fof(%.1f)" % r, call))
            rows.append(("fof(%.1f) all rows" % r, with_env("NBODY_FOF_ALL_ROWS", "1", call)))
        first, walked = {}, {}
        for name, fn in rows:   # warm-up: every shape the timed calls use; the fof calls traced
            if name.startswith("fof"):
                trace, first[name] = traced(fn)
                walked[name] = sum(t[1] for t in trace)
                print("%-22s %d groups, %d rounds, rows per round %s = %d = %.2f N" % (name, first[name][1], first[name][2], " + ".join(str(t[1]) for t in trace),
                                                                                 walked[name], walked[name] / n), flush=True)
            else:
                first[name] = fn()
        ms = {name: [] for name, fn in rows}
        same = dict.fromkeys(ms, True)
        for _ in range(a.reps):   # interleaved rounds
            for name, fn in rows:
                t, out = timed(fn)
                ms[name].append(t)
                same[name] &= all(np.array_equal(x, y) for x, y in zip(out, first[name]) if x is not None)
        for name, fn in rows:
            v = ms[name]
            print("%-22s median %9.3f ms, min %9.3f (spread %.3f; %s), identical results %s"
                  % (name, statistics.median(v), min(v), max(v) - min(v), " / ".join("%.3f" % x for x in v), same[name]), flush=True)
        near = ms["neighbors(r2=b2(0.7))"]
        unit, spread = statistics.median(near), max(near) - min(near)
        for r in RATIOS:
            for name in ("fof(%.1f)" % r, "fof(%.1f) all rows" % r):
                passes = walked[name] / n
                per_pass = statistics.median(ms[name]) / passes
                diff = per_pass - unit
                print("%-22s %.2f passes' worth of rows: %.3f ms per pass - neighbors() %.3f = %+.3f ms (%+.1f %%); margin 2 x the neighbors() spread = %.3f ms: %s"
                      % (name, passes, per_pass, unit, diff, 100 * diff / unit, 2 * spread, "within" if abs(diff) <= 2 * spread else "OUTSIDE"), flush=True)
            print("fof(%.1f): the same groups and rounds with and without the active-row list: %s"
                  % (r, all(np.array_equal(x, y) for x, y in zip(first["fof(%.1f)" % r], first["fof(%.1f) all rows" % r]))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=float, default=600.0)
    ap.add_argument("--worker", action="store_true", help="measure in this process (what the supervising process starts)")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--n", str(a.n), "--reps", str(a.reps)]
    try:
        return subprocess.run(cmd, timeout=a.timeout).returncode
    except subprocess.TimeoutExpired:
        print("fof_rate: the measurement did not finish within %.0f s and was killed" % a.timeout, file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
