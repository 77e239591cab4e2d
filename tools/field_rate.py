#!/usr/bin/env python3
"""What NBody.field costs: m points against N sources, one warm-up call and three timed calls, timed on the host around the synchronous
entry point (upload of the points, launch(es), copy back).  One line per configuration.
usage (GPU box): python tools/field_rate.py [--shape M,N ...] [--split K|auto ...] [--fp64] [--skip]
Defaults: the four shapes of profiles/r08_field.txt, fp32 timed arithmetic, NBODY_FIELD_SPLIT=1 and auto.  For the kernels' own time run
one configuration under `rocprofv3 --kernel-trace --stats -- python tools/field_rate.py --shape M,N --split K`."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402

SHAPES = ["256,1048576", "4096,1048576", "65536,65536", "262144,65536"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", action="append", help="M,N (points, sources)")
    ap.add_argument("--split", action="append", help="NBODY_FIELD_SPLIT value, or auto (unset)")
    ap.add_argument("--fp64", action="store_true")
    ap.add_argument("--skip", action="store_true", help="points = the first M bodies, each with itself left out")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    dtype = np.float64 if a.fp64 else np.float32
    for shape in a.shape or SHAPES:
        m, n = (int(v) for v in shape.split(","))
        pos, vel = nb.make_bodies(n, dtype=dtype)
        pts = pos[:m].copy() if a.skip else (1.5 * nb.make_bodies(m, seed=7, dtype=dtype)[0]).astype(dtype)
        skip = np.arange(m, dtype=np.int32) if a.skip else None
        with nb.NBody(n, fp64=a.fp64) as eng:
            eng.upload(pos, vel)
            for split in a.split or ["1", "auto"]:
                if split == "auto":
                    os.environ.pop("NBODY_FIELD_SPLIT", None)
                else:
                    os.environ["NBODY_FIELD_SPLIT"] = split
                first = eng.field(pts, skip)
                ms = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    got = eng.field(pts, skip)
                    ms.append(1e3 * (time.perf_counter() - t0))
                same = all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(first, got))
                best = min(ms)
                print("m %7d N %8d %s split %-4s skip %d: %s ms (spread %.3f), %.1f G pairs/s at the fastest, identical bits %s"
                      % (m, n, "fp64" if a.fp64 else "fp32", split, int(a.skip), " / ".join("%.3f" % v for v in ms), max(ms) - min(ms),
                         1e-6 * m * n / best, same), flush=True)


if __name__ == "__main__":
    main()
