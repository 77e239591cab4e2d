"""Writes tests/golden/force_dispatch.json from csrc/kernels.hip AS IT STANDS (tests/test_force_dispatch.py explains the file).  Run it
only on a kernels.hip whose selection is known good — the file in the repository was taken from the hand-unrolled switches and ladders
that select_force_kernel replaced — and only when a kernel is added or a launch rule is meant to change:
    python tests/golden/make_force_dispatch.py"""
import json
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import test_force_dispatch as T   # noqa: E402

if __name__ == "__main__":
    out = {}
    for build in sorted(T.BUILDS):
        with tempfile.TemporaryDirectory() as tmp:
            out[build] = T.dispatch_table(build, tmp)
        print(build, out[build]["cases"], "cases,", len(out[build]["kernels"]), "kernels,", sum(1 for c in out[build]["kernels"].values() if c), "reached")
    with open(T.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
