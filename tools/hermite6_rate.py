#!/usr/bin/env python3
"""What the snap pass and a sixth-order Hermite step cost beside the jerk pass and a fourth-order step: N bodies in one process, one
warm-up call of each operation and then the median of `reps` synchronous calls by the host clock (every call ends in a copy back or a
drain): NBody.jerk() (the jerk rows pass), NBody.snap() (the jerk rows pass, then the snap rows pass: the difference of the two calls is
the snap pass with its third output's copy), and NBody.step_hermite / NBody.step_hermite6 as a call of 1 step and a call of 16 — the
marginal step, (16-call - 1-call) / 15, leaves the opening passes and the per-call overhead out and is one jerk (one snap) rows pass with
the elementwise kernels.  A library without the sixth-order scheme (NBODY_LIB pointing at an older build) is timed on what it has.
One JSON line; profiles/r17_hermite6.txt was put together from alternating processes of this.
usage (GPU box): python tools/hermite6_rate.py [--n N] [--fp64] [--reps R] [--tag NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402

STEPS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    n, dt = a.n, 1.0 / 1024
    pos, vel = nb.make_bodies(n, dtype="float64" if a.fp64 else "float32")
    has6 = hasattr(nb._lib.load(), "nbody_step_hermite6")
    out = {"tag": a.tag, "n": n, "fp64": int(a.fp64), "reps": a.reps}
    with nb.NBody(n, fp64=a.fp64) as eng:
        eng.upload(pos, vel)
        calls = {"jerk_rows": eng.jerk, "hermite_1": lambda: eng.step_hermite(dt, 1), "hermite_16": lambda: eng.step_hermite(dt, STEPS)}
        if has6:
            calls.update({"snap_rows": eng.snap, "hermite6_1": lambda: eng.step_hermite6(dt, 1), "hermite6_16": lambda: eng.step_hermite6(dt, STEPS)})
        for f in calls.values():   # the warm-up
            f()
        ms = {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                t0 = time.perf_counter()
                f()
                ms[k].append(1e3 * (time.perf_counter() - t0))
        med = {k: statistics.median(v) for k, v in ms.items()}
        out.update({k: round(v, 4) for k, v in med.items()})
        out["hermite_marginal"] = round((med["hermite_16"] - med["hermite_1"]) / (STEPS - 1), 4)
        if has6:
            out["hermite6_marginal"] = round((med["hermite6_16"] - med["hermite6_1"]) / (STEPS - 1), 4)
            out["snap_minus_jerk"] = round(med["snap_rows"] - med["jerk_rows"], 4)
            out["marginal6_over_marginal4"] = round(out["hermite6_marginal"] / out["hermite_marginal"], 4)
        out["clock_khz"] = eng.info(nb._lib.INFO_CLOCK_KHZ)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
