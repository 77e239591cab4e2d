"""The pair binding-energy pass's HOST code (nbody_pair_energy_rows(_d), nbody_binaries: pair_energy.cpp on query_pass.hpp's ranges,
split, batches and gathers) under AddressSanitizer + UBSan on the CPU: a stand-alone program with its own main, linked from the host
files of tests/test_host_sanitizers.py (its compiler, flags and HOST list; its CASES table is not touched) and pair_energy.cpp,
hip_stub.cpp, the stub of pair_energy.hip (pair_energy_stub.cpp: predictable values pushed through the real PairEnergyArgs, refused by
the real launch predicates) and the driver pair_energy_sanity.cpp.  Nothing is loaded into Python under a sanitizer.  The driver covers
one and three ragged stub devices, windows of rows across the devices, forced and automatic splits, the batched path, the all-rows
walk and the mutual test of nbody_binaries with e_max and max_pairs, every NBODY_ERR_ARG case and the failure sweep."""
import os
import shutil
import subprocess

import pytest

from test_host_sanitizers import ASAN, FLAGS, HOST, ROOT, clang

HOST_FILES = HOST + ("pair_energy.cpp",)
STUB_FILES = ("hip_stub.cpp", "pair_energy_stub.cpp", "pair_energy_sanity.cpp")
CLEAR = ("NBODY_PAIR_ENERGY_SPLIT", "NBODY_PAIR_ENERGY_SCRATCH_MB")


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_pair_energy_host_code_is_address_and_ub_clean(tmp_path):
    sources = [os.path.join(ROOT, "mini_nbody_amd", "csrc", f) for f in HOST_FILES] + [os.path.join(ROOT, "tests", "host_stub", f) for f in STUB_FILES]
    objs = []
    for k, src in enumerate(sources):
        objs.append(str(tmp_path / ("%d_%s.o" % (k, os.path.basename(src)))))
        clang(FLAGS + ASAN + ["-c", src, "-o", objs[-1]])
    exe = str(tmp_path / "pair_energy_sanity")
    clang(ASAN + objs + ["-o", exe, "-ldl", "-lpthread"])
    env = dict(os.environ, STUB_DEVICES="3", NBODY_OVERSUBSCRIBE="1", ASAN_OPTIONS="detect_leaks=1")
    for k in CLEAR:
        env.pop(k, None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "pair_energy_sanity ok" in out.stdout and "runtime error" not in out.stderr, out.stderr[-4000:]
