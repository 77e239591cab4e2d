#!/usr/bin/env python3
"""What NBody.tidal costs beside NBody.field: m points against N sources in one process, one warm-up call of each and then `reps`
rounds that alternate the two, HIP events on the null stream around each synchronous entry point (upload of the points, launch(es),
copy back) and the host clock beside them.  One line per pass; the rate is m * N pairs over the fastest call, an end-to-end figure of
the call and not the kernel's own time.
usage (GPU box): python tools/tidal_rate.py [--shape M,N] [--reps R] [--out FILE]
Default: (65536, 65536), fp32 timed arithmetic, the automatic source split: the shape of profiles/r08_tidal.txt."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mini_nbody_amd as nb   # noqa: E402


class Events:
    """two HIP events on the null stream: the entry points are synchronous, so the pair brackets everything a call does on the device"""

    def __init__(self):
        self.hip = C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        self.e = [C.c_void_p(), C.c_void_p()]
        for e in self.e:
            self.check(self.hip.hipEventCreate(C.byref(e)))

    @staticmethod
    def check(rc):
        if rc:
            raise RuntimeError("HIP error %d" % rc)

    def ms(self, call):
        self.check(self.hip.hipEventRecord(self.e[0], None))
        t0 = time.perf_counter()
        out = call()
        wall = 1e3 * (time.perf_counter() - t0)
        self.check(self.hip.hipEventRecord(self.e[1], None))
        self.check(self.hip.hipEventSynchronize(self.e[1]))
        dev = C.c_float()
        self.check(self.hip.hipEventElapsedTime(C.byref(dev), self.e[0], self.e[1]))
        return out, float(dev.value), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="65536,65536", help="M,N (points, sources)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", help="also write the lines to this file")
    a = ap.parse_args()
    m, n = (int(v) for v in a.shape.split(","))
    pos, vel = nb.make_bodies(n)
    pts = (1.5 * nb.make_bodies(m, seed=7)[0].astype(np.float64)).astype(np.float32)
    lines = []
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        ev = Events()
        passes = {"tidal": lambda: eng.tidal(pts), "field": lambda: eng.field(pts)[0]}
        first = {k: f() for k, f in passes.items()}   # the warm-up
        dev, wall, same = {k: [] for k in passes}, {k: [] for k in passes}, {k: True for k in passes}
        for _ in range(a.reps):
            for k, f in passes.items():
                got, d, w = ev.ms(f)
                dev[k].append(d)
                wall[k].append(w)
                same[k] = same[k] and np.array_equal(got.view(np.uint8), first[k].view(np.uint8))
        for k in passes:
            lines.append("%s m %d N %d fp32 timed, split auto: events %s ms, host clock %s ms, %.1f G pairs/s at the fastest (events), identical bits %s"
                         % (k, m, n, " / ".join("%.3f" % v for v in dev[k]), " / ".join("%.3f" % v for v in wall[k]),
                            1e-6 * m * n / min(dev[k]), same[k]))
        lines.append("tidal / field rate: %.3f (by instruction count 15 / 22 = %.3f)" % (min(dev["field"]) / min(dev["tidal"]), 15 / 22))
    print("\n".join(lines), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
