"""timescale.cpp — the host side of the pair time-scale pass and of the shared adaptive step — under AddressSanitizer + UBSan on the
CPU, as tests/test_hist_host_sanitizers.py runs its sibling: a stand-alone program with its own main
(tests/host_stub/timescale_sanity.cpp), linked from the host files under test, hip_stub.cpp and timescale_stub.cpp (predictable values
pushed through the real TimescaleArgs: chunk bounds, the chunks' scratch layout of two minima and an index, the combine, both source
streams); nothing is loaded into Python under a sanitizer.  The driver covers one and three stub devices with ragged slices, windows of
rows across the devices, the source split forced and automatic, the batched path under a small scratch bound, the gather of all N
velocities on three devices after steps have changed them, every NBODY_ERR_ARG case, the driver loop against nbody_step and the failure
sweep of sanity_common.hpp.  It uses the helpers of test_host_sanitizers.py and leaves its CASES alone."""
import atexit
import os
import shutil
import subprocess
import tempfile

import pytest

from test_host_sanitizers import ASAN, FLAGS, HOST, ROOT, clang

HOST_FILES = HOST + ("timescale.cpp",)
STUB_FILES = ("hip_stub.cpp", "timescale_stub.cpp", "timescale_sanity.cpp")   # the driver last
CLEAR = ("NBODY_TIMESCALE_SPLIT", "NBODY_TIMESCALE_SCRATCH_MB")


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_timescale_host_code_is_address_and_ub_clean():
    tmp = tempfile.mkdtemp(prefix="nbody_timescale_sanitizers_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    objs = []
    for src in [os.path.join(ROOT, "mini_nbody_amd", "csrc", f) for f in HOST_FILES] + [os.path.join(ROOT, "tests", "host_stub", f) for f in STUB_FILES]:
        objs.append(os.path.join(tmp, os.path.basename(src) + ".o"))
        clang(FLAGS + ASAN + ["-c", src, "-o", objs[-1]])
    exe = os.path.join(tmp, "timescale_sanity")
    clang(ASAN + objs + ["-o", exe, "-ldl", "-lpthread"])
    env = dict(os.environ, STUB_DEVICES="3", NBODY_OVERSUBSCRIBE="1", ASAN_OPTIONS="detect_leaks=1")
    for k in CLEAR:
        env.pop(k, None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "timescale_sanity ok" in out.stdout and "runtime error" not in out.stderr, out.stderr[-4000:]
