#!/usr/bin/env python3
"""What the pair binding-energy pass costs, beside the pair time-scale pass as the yardstick: in ONE process on one device, at every N
asked for and in the precisions asked for, NBody.timescales() over all rows with the source split automatic and forced to 1 and 16
chunks, then NBody.pair_energy() over all rows with the split automatic, forced to every value of --splits and automatic again (the
same configuration in two positions of the alternation: what a position costs), and NBody.binaries() end
to end (the all-rows pass, the download, the mutual test, the members' state and the elements) on a state with a few hundred binaries:
a hot cloud — the library's seeded bodies with their velocities times 1000, so that hardly any chance pair is bound — with --planted
pairs of neighbours in the array set 0.001 apart at relative rest.  One warm-up call and --reps timed calls per configuration,
alternating the configurations, timed on the host around the synchronous entry point (launch, stream sync, copy back).  One line per
configuration with every time and the MEDIAN; then the ratios to the time-scale pass and of the automatic split to the best forced one.
The table of profiles/r15_pair_energy.txt.
usage (GPU box): python tools/pair_energy_rate.py [--n N [N ...]] [--reps R] [--splits K [K ...]] [--precisions fp32 fp64] [--planted B]
For the kernels' own time run it under `rocprofv3 --kernel-trace --stats -- python tools/pair_energy_rate.py`."""
import argparse
import os
import statistics
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
    """the same values: tuples of arrays"""
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


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


def hot_cloud(n, planted, dtype):
    pos, vel = nb.make_bodies(n, dtype=dtype)
    vel[:, :3] *= 1000
    for k in range(min(planted, n // 2)):
        pos[2 * k + 1, :3] = pos[2 * k, :3]
        pos[2 * k + 1, 0] += dtype(0.001)
        vel[2 * k + 1, :3] = vel[2 * k, :3]
    return pos, vel


def measure(n, reps, fp64, splits, planted):
    dtype = np.float64 if fp64 else np.float32
    pos, vel = hot_cloud(n, planted, dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        rows = [("timescales() split %s" % (k or "auto"), with_env("NBODY_TIMESCALE_SPLIT", k, lambda: eng.timescales())) for k in (None, "1", "16")]
        rows += [("pair_energy() split %s" % (k or "auto"), with_env("NBODY_PAIR_ENERGY_SPLIT", k, lambda: eng.pair_energy()))
                 for k in [None] + [str(s) for s in splits]]
        # the automatic split once more, in another position of the alternation: two rows of one configuration show what the position costs
        rows += [("pair_energy() split auto, again", with_env("NBODY_PAIR_ENERGY_SPLIT", None, lambda: eng.pair_energy()))]
        rows += [("binaries()", lambda: eng.binaries())]
        first = {name: fn() for name, fn in rows}   # warm-up: every shape the timed calls use
        ms = {name: [] for name, fn in rows}
        same = dict.fromkeys(ms, True)
        for _ in range(reps):   # alternating
            for name, fn in rows:
                t, out = timed(fn)
                ms[name].append(t)
                same[name] &= equal(out, first[name])
        print("N %d %s, %d CUs, clock %d kHz, %d timed calls each (measured)"
              % (n, "fp64" if fp64 else "fp32", eng.info(nb._lib.INFO_CU_COUNT), eng.info(nb._lib.INFO_CLOCK_KHZ), reps))
        med = {name: statistics.median(v) for name, v in ms.items()}
        for name, fn in rows:
            print("%-32s rows %8d: %s ms, median %.3f (spread %.3f), %.1f G pairs/s at the median, identical results %s"
                  % (name, n, " / ".join("%.3f" % v for v in ms[name]), med[name], max(ms[name]) - min(ms[name]), 1e-6 * n * n / med[name],
                     same[name]), flush=True)
        forced = ["pair_energy() split %d" % s for s in splits]
        print("every split agrees: %s" % all(equal(first["pair_energy() split auto"], first[k]) for k in forced))
        print("binaries(): %d found, %d listed with a < 0.001" % (eng.binaries_found, int(np.sum(first["binaries()"][2][:, 1] < 0.001))))
        best = min(forced, key=lambda k: med[k])
        print("pair_energy() split auto / %s (the best forced split): %.3f x the time" % (best, med["pair_energy() split auto"] / med[best]))
        print("pair_energy() split auto, again / %s: %.3f x the time" % (best, med["pair_energy() split auto, again"] / med[best]))
        for k in ("auto", "1", "16"):
            print("pair_energy() split %s / timescales() split %s: %.2f x the time"
                  % (k, k, med["pair_energy() split %s" % k] / med["timescales() split %s" % k]), flush=True)
        print("binaries() / pair_energy() split auto: %.2f x the time" % (med["binaries()"] / med["pair_energy() split auto"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1 << 16])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--splits", type=int, nargs="+", default=[1, 2, 4, 8, 16, 32, 64])
    ap.add_argument("--precisions", nargs="+", default=["fp32", "fp64"], choices=["fp32", "fp64"])
    ap.add_argument("--planted", type=int, default=300)
    a = ap.parse_args()
    if not {1, 16} <= set(a.splits):
        ap.error("--splits must hold 1 and 16 (the ratios to the time-scale pass are taken there)")
    for n in a.n:
        for p in a.precisions:
            measure(n, a.reps, p == "fp64", a.splits, a.planted)


if __name__ == "__main__":
    main()
