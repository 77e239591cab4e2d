#!/usr/bin/env python3
"""What a sub-step of the sixth-order block time steps (NBody.step_hermite6_block) costs — one of a single active row and one of all
rows — beside the marginal step of NBody.step_hermite6 in the same process, and, so that a build can be held against another, what
NBody.step_hermite_block and NBody.step_hermite6 cost themselves: N bodies in one process, one warm-up call of each operation and
then the median of `reps` synchronous calls by the host clock (every call drains its streams before it returns), the calls of a round
in alternation.

The sub-steps are separated as tools/hermite_block_rate.py separates them, on its system of m = 1 mover (N bodies at rest on a lattice,
one row far away and fast: it sits on the finest level, all others on level 0, dt_max = 2^-40 so that nothing moves): a block then has
S = 2^(levels - 1) - 1 sub-steps of one row and one of N, and the call's counters are asserted to say exactly that.  With
    A = call(1 level, 1 block) = opening + t_N        B = call(1 level, 9 blocks) = opening + 9 t_N
    C = call(levels, 4 blocks) = opening + 4 S t_1 + 4 t_N
t_N = (B - A) / 8 and t_1 = (C - A - 3 t_N) / (4 S); the shared step's marginal cost is (step_hermite6(16) - step_hermite6(1)) / 15.
A, B and the shared calls are timed on make_bodies(N).  A library without the sixth-order block scheme (an older checkout) is timed on
what it has.  One JSON line; profiles/r18_hermite6_block.txt was put together from alternating processes of this.
usage (GPU box): python tools/hermite6_block_rate.py [--n N] [--fp64] [--reps R] [--tag NAME]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402
from hermite_block_rate import BLOCKS, DT_MAX, MAX_LEVELS, mover_system, ratio   # noqa: E402

STEPS = 16


def median_ms(calls, reps, before=None):
    """{name: median ms} of `reps` rounds over `calls`, one warm-up round first; before(): what every call starts from"""
    ms = {k: [] for k in calls}
    for r in range(reps + 1):
        for k, f in calls.items():
            if before:
                before()
            t0 = time.perf_counter()
            f()
            if r:
                ms[k].append(1e3 * (time.perf_counter() - t0))
    return {k: statistics.median(v) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    a = ap.parse_args()
    n, dt = a.n, 1.0 / 1024
    dtype = np.float64 if a.fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    has = hasattr(nb.NBody, "step_hermite6_block")
    out = {"tag": a.tag, "n": n, "fp64": int(a.fp64), "reps": a.reps, "has_hermite6_block": int(has)}
    with nb.NBody(n, fp64=a.fp64) as eng:
        eng.upload(pos, vel)
        calls = {"hermite6_1": lambda: eng.step_hermite6(dt, 1), "hermite6_16": lambda: eng.step_hermite6(dt, STEPS),
                 "block4_1level_1": lambda: eng.step_hermite_block(DT_MAX, 1, levels=1), "block4_1level_9": lambda: eng.step_hermite_block(DT_MAX, 9, levels=1)}
        if has:
            calls.update({"block6_1level_1": lambda: eng.step_hermite6_block(DT_MAX, 1, levels=1),
                          "block6_1level_9": lambda: eng.step_hermite6_block(DT_MAX, 9, levels=1)})
        med = median_ms(calls, a.reps)
        out["hermite6_marginal"] = (med["hermite6_16"] - med["hermite6_1"]) / (STEPS - 1)
        out["block4_all_rows"] = (med["block4_1level_9"] - med["block4_1level_1"]) / 8
        if has:
            out["block6_all_rows"] = (med["block6_1level_9"] - med["block6_1level_1"]) / 8
            out["block6_all_rows_over_hermite6_marginal"] = out["block6_all_rows"] / out["hermite6_marginal"]
        # one mover: the level count and eta from the ratios the state gives, as tools/hermite_block_rate.py chooses them
        mp, mv, movers = mover_system(n, 1)
        mp, mv = mp.astype(dtype), mv.astype(dtype)
        eng.upload(mp, mv)
        q = ratio(*eng.jerk())
        others = np.ones(n, bool)
        others[movers] = False
        top, hi = q[movers].max(), q[others].min()
        levels = MAX_LEVELS
        while levels > 1 and not top * 4 ** (levels - 2) * 4 < hi:
            levels -= 1
        out["mover_levels"] = levels
        if levels >= 2:
            sub = 2 ** (levels - 1) - 1
            eta = DT_MAX / np.sqrt(np.sqrt(top * 4 ** (levels - 2) * hi))
            want = (BLOCKS * (sub + 1), BLOCKS * (sub + n))
            one = {"block4_mover": lambda: eng.step_hermite_block(DT_MAX, BLOCKS, eta=eta, levels=levels)}
            if has:
                one["block6_mover"] = lambda: eng.step_hermite6_block(DT_MAX, BLOCKS, eta=eta, levels=levels)
            for k, f in list(one.items()):   # the counters must say S sub-steps of one row and one of N per block: no figure otherwise
                eng.upload(mp, mv)
                got = f()
                out[k + "_counters_ok"] = int(got == want)
                if got != want:
                    del one[k]
            has = has and "block6_mover" in one
            mover = median_ms(one, a.reps, before=lambda: eng.upload(mp, mv))
            med.update(mover)
            if "block4_mover" in mover:
                out["block4_one_row"] = (mover["block4_mover"] - med["block4_1level_1"] - (BLOCKS - 1) * out["block4_all_rows"]) / (BLOCKS * sub)
            if has:
                out["block6_one_row"] = (mover["block6_mover"] - med["block6_1level_1"] - (BLOCKS - 1) * out["block6_all_rows"]) / (BLOCKS * sub)
                out["block6_one_row_over_hermite6_marginal"] = out["block6_one_row"] / out["hermite6_marginal"]
        out.update(med)
        out = {k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}
        out["clock_khz"] = eng.info(nb._lib.INFO_CLOCK_KHZ)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
