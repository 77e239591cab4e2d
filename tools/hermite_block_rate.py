#!/usr/bin/env python3
"""What a sub-step of the block time steps (NBody.step_hermite_block) costs against its active count m, and what the all-active sub-step
costs beside nbody_step_hermite's step: N bodies in one process, fp32 timed arithmetic, HIP events on the null stream around each
synchronous call and the host clock beside them, `reps` rounds that alternate the calls.

The active count cannot be asked for, so the system is built to give it: N bodies at rest on a jittered cubic lattice of spacing 1
(no close pair, no jerk of their own), of which m rows, spread evenly over the rows ("movers"), are taken out to a line 1e4 away, 10
apart, with velocities of 1e7 in random directions.  A mover's jerk comes from its neighbours on the line and from all N sources
coherently, and its |a|^2 / |j|^2 is below 1e-6; everybody else feels the movers' velocities at 1e4 only and keeps a ratio many orders
above that.  dt_max is 2^-40, so nothing moves, and only dt_max / eta matters: it is put at the geometric middle between the movers'
largest ratio (times 4^(levels - 2)) and the others' smallest, read from NBody.jerk(), with as many levels (up to 6) as the gap between
the two allows, so that the movers sit on the finest level and all others on level 0.  A block then has 2^(levels - 1) - 1 sub-steps
of m rows and one of N, and the call's counters are asserted to say exactly that.  With S = 2^(levels - 1) - 1 and
    A = call(1 level, 1 block) = opening + t_N        B = call(1 level, 9 blocks) = opening + 9 t_N
    C = call(levels, 4 blocks) = opening + 4 S t_m + 4 t_N
t_N = (B - A) / 8 and t_m = (C - A - 3 t_N) / (4 S).  The shared step's marginal cost is (step_hermite(9) - step_hermite(1)) / 8; A, B
and the two shared calls are timed on make_bodies(N).
usage (GPU box): python tools/hermite_block_rate.py [--n N] [--reps R] [--out FILE]
Default: N = 65536, m = 1, 64, 256, 4096: the shape of profiles/r14_hermite_block.txt."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402
from tidal_rate import Events   # noqa: E402

DT_MAX = 2.0 ** -40
MAX_LEVELS = 6
BLOCKS = 4


def mover_system(n, m, seed=7):
    """(pos, vel, movers) words: n bodies at rest on a cubic lattice of spacing 1 jittered by up to 0.2, m of them — spread evenly over
    the rows — moved to a line at x = 1e4, 10 apart, with velocities of 1e7 in random directions"""
    side = int(np.ceil(n ** (1.0 / 3.0)))
    rng = np.random.default_rng(seed)
    idx = np.arange(n)
    pos, vel = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32)
    pos[:, 0], pos[:, 1], pos[:, 2] = idx % side, (idx // side) % side, idx // (side * side)
    pos[:, :3] += rng.uniform(-0.2, 0.2, (n, 3)).astype(np.float32)
    movers = np.arange(m) * (n // m) + (n // m) // 2
    pos[movers, :3] = 0.0
    pos[movers, 0] = 1e4 + 10.0 * np.arange(m)
    u = rng.normal(size=(m, 3))
    vel[movers, :3] = (1e7 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
    return pos, vel, movers


def ratio(a, j):
    a, j = a[:, :3].astype(np.float64), j[:, :3].astype(np.float64)
    with np.errstate(all="ignore"):
        return (a * a).sum(1) / (j * j).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--m", type=int, nargs="*", default=[1, 64, 256, 4096])
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    n = a.n
    pos, vel = nb.make_bodies(n)
    lines = []
    with nb.NBody(n) as eng:
        ev = Events()
        eng.upload(pos, vel)
        calls = {"block 1 level 1 block": lambda: eng.step_hermite_block(DT_MAX, 1, levels=1), "block 1 level 9 blocks": lambda: eng.step_hermite_block(DT_MAX, 9, levels=1),
                 "hermite 1 step": lambda: eng.step_hermite(DT_MAX, 1), "hermite 9 steps": lambda: eng.step_hermite(DT_MAX, 9)}
        for f in calls.values():   # the warm-up
            f()
        dev, wall = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                _, d, w = ev.ms(f)
                dev[k].append(d)
                wall[k].append(w)
        for k in calls:
            lines.append("%s N %d fp32 timed: events %s ms, host clock %s ms"
                         % (k, n, " / ".join("%.3f" % v for v in dev[k]), " / ".join("%.3f" % v for v in wall[k])))
        call_a = min(dev["block 1 level 1 block"])
        t_n = (min(dev["block 1 level 9 blocks"]) - call_a) / 8
        t_h = (min(dev["hermite 9 steps"]) - min(dev["hermite 1 step"])) / 8
        lines.append("all-active sub-step %.3f ms, shared Hermite step %.3f ms (both marginal): ratio %.3f; opening %.3f ms" % (t_n, t_h, t_n / t_h, call_a - t_n))
        for m in a.m:
            pos, v, movers = mover_system(n, m)
            eng.upload(pos, v)
            q = ratio(*eng.jerk())
            others = np.ones(n, bool)
            others[movers] = False
            top, hi = q[movers].max(), q[others].min()
            levels = MAX_LEVELS
            while levels > 1 and not top * 4 ** (levels - 2) * 4 < hi:      # a factor 2 of room on either side of dt_max / eta
                levels -= 1
            if levels < 2:
                lines.append("m %d: the movers' q (max %.3e) and the others' (min %.3e) are not a factor 4 apart: not measured" % (m, top, hi))
                continue
            sub = 2 ** (levels - 1) - 1
            eta = DT_MAX / np.sqrt(np.sqrt(top * 4 ** (levels - 2) * hi))
            f = lambda: eng.step_hermite_block(DT_MAX, BLOCKS, eta=eta, levels=levels)
            steps, evals = f()
            assert (steps, evals) == (BLOCKS * (sub + 1), BLOCKS * (sub * m + n)), (m, levels, steps, evals)
            d, w = [], []
            for _ in range(a.reps):
                eng.upload(pos, v)
                _, dd, ww = ev.ms(f)
                d.append(dd)
                w.append(ww)
            t_m = (min(d) - call_a - (BLOCKS - 1) * t_n) / (BLOCKS * sub)
            lines.append("m %d: call of %d blocks on %d levels (%d sub-steps of m, %d of N): events %s ms, host clock %s ms; sub-step of m rows %.3f ms"
                         % (m, BLOCKS, levels, BLOCKS * sub, BLOCKS, " / ".join("%.3f" % x for x in d), " / ".join("%.3f" % x for x in w), t_m))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
