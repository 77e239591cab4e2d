"""The work units of the mutual pairing (csrc/mutual_args.hpp: mutual_units, mutual_unit), checked on the CPU against the library's own
function: a small driver with its own main (tests/host_stub/mutual_units_driver.cpp) prints every unit for nb = 1 .. 40 blocks and several
run lengths.  For every nb: every unordered pair of blocks is taken exactly once, every diagonal exactly once, no unit is longer than the
run, the blocks of a unit are consecutive modulo nb, the row blocks' work differs by at most one block, and the diagonal units come last."""
import collections
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
NB_MAX = 40
RUNS = (1, 3, 8, 16, 64)


@pytest.fixture(scope="module")
def units(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ under /opt/rocm")
    exe = str(tmp_path_factory.mktemp("mutual_units") / "driver")
    src = os.path.join(ROOT, "tests", "host_stub", "mutual_units_driver.cpp")
    r = subprocess.run([CXX, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", src, "-o", exe],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode(errors="replace")[-3000:]
    out = subprocess.run([exe, str(NB_MAX)] + [str(r) for r in RUNS], capture_output=True, timeout=600, check=True).stdout.decode()
    table = collections.defaultdict(list)
    for line in out.splitlines():
        nb, run, u, a, d0, count = map(int, line.split())
        assert u == len(table[nb, run])
        table[nb, run].append((a, d0, count))
    return table


@pytest.mark.parametrize("run", RUNS)
def test_every_block_pair_once(units, run):
    for nb in range(1, NB_MAX + 1):
        us = units[nb, run]
        pairs, diagonal, work = collections.Counter(), collections.Counter(), collections.Counter()
        seen_diagonal = False
        for a, d0, count in us:
            assert 0 <= a < nb and 0 <= count <= run
            if d0 == 0:
                assert count == 1
                diagonal[a] += 1
                seen_diagonal = True
                continue
            assert not seen_diagonal, "the diagonal units come last"
            for k in range(count):
                d = d0 + k
                assert 1 <= d <= nb // 2
                b = (a + d) % nb
                assert b != a
                pairs[frozenset((a, b))] += 1
                work[a] += 1
        assert diagonal == collections.Counter(range(nb)), (nb, run)
        assert len(pairs) == nb * (nb - 1) // 2 and set(pairs.values()) <= {1}, (nb, run)
        loads = [work[a] for a in range(nb)]
        assert max(loads) - min(loads) <= 1, (nb, run, loads)
