#!/usr/bin/env python3
"""What NBody.jerk_at (without and with a skip array) and NBody.jerk cost beside NBody.field and NBody.tidal: m queries against N sources
in one process, one warm-up call of each and then `reps` rounds that alternate the five, HIP events on the null stream around each synchronous entry point (upload
of the queries — the rows form uploads nothing —, launch(es), copy back) and the host clock beside them.  One line per pass; the rate is
m * N pairs over the fastest call, an end-to-end figure of the call and not the kernel's own time.
usage (GPU box): python tools/jerk_rate.py [--shape M,N] [--reps R] [--out FILE]
Default: (65536, 65536), fp32 timed arithmetic, the automatic source split: the shape of profiles/r12_jerk.txt.  The rows form takes
rows 0 .. min(M, N) - 1."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402
from tidal_rate import Events   # noqa: E402

VALU = {"field": 12, "tidal": 20, "jerk": 25}   # per pair in the compiled fp32 timed loops, beside one v_rsq_f32 each


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536,65536", help="M,N (queries, sources)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    m, n = (int(v) for v in a.shape.split(","))
    pos, vel = nb.make_bodies(n)
    pts = (1.5 * nb.make_bodies(m, seed=7)[0].astype(np.float64)).astype(np.float32)
    pvel = nb.make_bodies(m, seed=78)[1]
    rows = min(m, n)
    lines = []
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        ev = Events()
        skip = ((np.arange(m, dtype=np.int64) * 7919) % n).astype(np.int32)   # every query leaves one body out: the kernel's SKIP form
        passes = {"jerk_at": (m, lambda: eng.jerk_at(pts, pvel)[1]), "jerk_at skip": (m, lambda: eng.jerk_at(pts, pvel, skip)[1]),
                  "jerk rows": (rows, lambda: eng.jerk(0, rows)[1]),
                  "tidal": (m, lambda: eng.tidal(pts)), "field": (m, lambda: eng.field(pts)[0])}
        first = {k: f() for k, (_, f) in passes.items()}   # the warm-up
        dev, wall, same = {k: [] for k in passes}, {k: [] for k in passes}, {k: True for k in passes}
        for _ in range(a.reps):
            for k, (_, f) in passes.items():
                got, d, w = ev.ms(f)
                dev[k].append(d)
                wall[k].append(w)
                same[k] = same[k] and np.array_equal(got.view(np.uint8), first[k].view(np.uint8))
        rate = {k: 1e-6 * q * n / min(dev[k]) for k, (q, _) in passes.items()}
        for k, (q, _) in passes.items():
            lines.append("%s m %d N %d fp32 timed, split auto: events %s ms, host clock %s ms, %.1f G pairs/s at the fastest (events), identical bits %s"
                         % (k, q, n, " / ".join("%.3f" % v for v in dev[k]), " / ".join("%.3f" % v for v in wall[k]), rate[k], same[k]))
        for k in ("jerk_at", "jerk_at skip", "jerk rows"):
            for other in ("field", "tidal"):
                lines.append("%s / %s rate: %.3f (by instruction count %d / %d = %.3f)"
                             % (k, other, rate[k] / rate[other], VALU[other] + 1, VALU["jerk"] + 1, (VALU[other] + 1) / (VALU["jerk"] + 1)))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
