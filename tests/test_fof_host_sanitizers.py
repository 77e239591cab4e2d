"""fof.cpp — the host side of nbody_fof — under AddressSanitizer + UBSan on the CPU, beside the library's other host files, as
tests/test_knn_host_sanitizers.py runs knn.cpp: a stand-alone program with its own main.  tests/host_stub/hip_stub.cpp stands in for the
HIP runtime ("device" memory is malloc'd, so ASan sees every offset the host computed), tests/host_stub/fof_stub.cpp for fof.hip (the
real m of the definition computed from the real FofArgs: the active-row list, the labels, chunk bounds, the chunks' [chunk][m] scratch
layout, the combine), the neighbour, field and knn stubs for the passes linked beside it, and tests/host_stub/fof_sanity.cpp drives the
C-ABI on a one-dimensional system whose groups it finds by sorting: N = 1, 255, 256, 257 and 5000 over one and three stub devices with
ragged ranges, the source split forced and automatic, the batched path, the active-row list against NBODY_FOF_ALL_ROWS=1, each output
NULL in turn, every NBODY_ERR_ARG case, and the failure sweep (the k-th allocating call fails: the call says so, nothing is live after
nbody_shutdown, the same call then works).  Nothing is loaded into Python under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
SRC = [os.path.join(ROOT, "mini_nbody_amd", "csrc", f) for f in ("context.cpp", "comm.cpp", "mailbox.cpp", "energy.cpp", "neighbors.cpp", "field.cpp",
                                                                  "knn.cpp", "fof.cpp")] + \
      [os.path.join(ROOT, "tests", "host_stub", f) for f in ("hip_stub.cpp", "neighbors_stub.cpp", "field_stub.cpp", "knn_stub.cpp", "fof_stub.cpp",
                                                             "fof_sanity.cpp")]


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_fof_host_code_is_address_and_ub_clean(tmp_path):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ under /opt/rocm")
    exe = str(tmp_path / "fof_sanity_asan")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wall",
                        "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + SRC +
                       ["-o", exe, "-ldl", "-lpthread"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0 and "sanitize" in r.stderr and "unsupported" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, STUB_DEVICES="3", NBODY_OVERSUBSCRIBE="1", ASAN_OPTIONS="detect_leaks=1")
    for k in ("NBODY_FOF_SPLIT", "NBODY_FOF_SCRATCH_MB", "NBODY_FOF_ALL_ROWS"):
        env.pop(k, None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "fof_sanity ok" in out.stdout and "runtime error" not in out.stderr, out.stderr[-4000:]
