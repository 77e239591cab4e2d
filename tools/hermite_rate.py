#!/usr/bin/env python3
"""What a fourth-order Hermite step (NBody.step_hermite) costs beside one NBody.jerk() call and one nbody_step step: N bodies in one
process, one warm-up call of each and then `reps` rounds that alternate them, HIP events on the null stream around each synchronous call
and the host clock beside them.  A Hermite call of k steps takes k + 1 jerk rows passes (the opening evaluation), so two figures are
printed: the call of 16 steps over 16, and the marginal step (call of 16 - call of 1) / 15, which leaves the opening pass and the
per-call overhead out.  nbody_step is timed as 16 steps and a sync over 16, with the library's defaults.
usage (GPU box): python tools/hermite_rate.py [--n N] [--reps R] [--out FILE]
Default: N = 65536, fp32 timed arithmetic, the automatic source split: the shape of profiles/r13_hermite.txt."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402
from tidal_rate import Events   # noqa: E402

STEPS = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    n, dt = a.n, 1.0 / 1024
    pos, vel = nb.make_bodies(n)
    lines = []
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        ev = Events()

        def steps():
            eng.step(dt, STEPS)
            eng.sync()

        calls = {"hermite %d steps" % STEPS: lambda: eng.step_hermite(dt, STEPS), "hermite 1 step": lambda: eng.step_hermite(dt, 1),
                 "jerk rows": lambda: eng.jerk(), "min_aarseth": lambda: eng.min_aarseth(), "nbody_step %d steps" % STEPS: steps}
        for f in calls.values():   # the warm-up
            f()
        dev, wall = {k: [] for k in calls}, {k: [] for k in calls}
        for _ in range(a.reps):
            for k, f in calls.items():
                _, d, w = ev.ms(f)
                dev[k].append(d)
                wall[k].append(w)
        for k in calls:
            lines.append("%s N %d fp32 timed, split auto: events %s ms, host clock %s ms"
                         % (k, n, " / ".join("%.3f" % v for v in dev[k]), " / ".join("%.3f" % v for v in wall[k])))
        h16, h1 = min(dev["hermite %d steps" % STEPS]), min(dev["hermite 1 step"])
        jerk, step = min(dev["jerk rows"]), min(dev["nbody_step %d steps" % STEPS]) / STEPS
        marginal = (h16 - h1) / (STEPS - 1)
        lines.append("Hermite step: %.3f ms as call / %d, %.3f ms marginal; jerk rows call %.3f ms; nbody_step step %.3f ms" % (h16 / STEPS, STEPS, marginal, jerk, step))
        lines.append("marginal Hermite step / jerk rows call: %.3f; / nbody_step step: %.3f; %.1f G pairs/s of the jerk pass in a step"
                     % (marginal / jerk, marginal / step, 1e-6 * n * n / marginal))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
