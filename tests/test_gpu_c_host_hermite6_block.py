"""The C host program's --hermite6-block line (mini_nbody_amd/host/nbody.c over nbody_step_hermite6_block) end to end on the GPU, at
the energy system's size: it runs, names its loop, prints the counters of the timed call, the energies before and after — the drift is
what the scheme is for — and leaves the state NBody.step_hermite6_block leaves; --masses is honoured; the options it excludes are
refused."""
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "build", "nbody")


def test_c_host_program_hermite6_block_line(nb):
    if not os.path.exists(EXE):
        pytest.fail("build/nbody is missing: run `make host`")
    n, iters, levels = 8, 2, 8
    r = subprocess.run([EXE, str(n), str(iters), "--hermite6-block", str(levels)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device Hermite-6 block loop" in r.stdout
    m = re.search(r"^hermite6 block: (\d+) levels, (\d+) sub-steps, (\d+) row evaluations \((\S+) of sub-steps x N\)$", r.stdout, flags=re.M)
    lines = re.findall(r"^energy at step (\d+): E (\S+) T (\S+) U (\S+)", r.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [0, iters] and "drift" in r.stdout, r.stdout
    got = [float(v) for v in re.search(r"^checksum \(sum of positions\): (\S+) (\S+) (\S+)$", r.stdout, flags=re.M).groups()]
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        e0 = eng.energy()["total"]
        steps, evals = eng.step_hermite6_block(np.float32(0.01), iters, eta=np.float32(0.02), levels=levels)
        p = eng.download()[0]
        e1 = eng.energy()["total"]
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (levels, steps, evals), r.stdout
    assert float(m.group(4)) == float("%.4f" % (evals / (steps * n)))
    want = [0.0] * 3
    for k in range(n):   # plain ascending fp64 sums, printed with nine digits
        for c in range(3):
            want[c] += float(p[k, c])
    assert [float("%.9g" % w) for w in want] == got, (got, want)
    assert [float(lines[0][1]), float(lines[1][1])] == [e0, e1]
    r = subprocess.run([EXE, str(n), str(iters), "--hermite6-block", str(levels), "--masses"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device Hermite-6 block loop" in r.stdout and len(re.findall(r"^energy at step", r.stdout, flags=re.M)) == 2, r.stdout + r.stderr
    for extra in (["--host-loop"], ["--hermite-block", "4"], ["--hermite6"]):
        r = subprocess.run([EXE, str(n), str(iters), "--hermite6-block", "4"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and r.stderr, extra
    r = subprocess.run([EXE, str(n), str(iters), "--hermite6-block", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--hermite6-block" in r.stderr
