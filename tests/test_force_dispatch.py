"""Which kernel a force launch takes (csrc/kernels.hip: select_force_kernel and the one launch behind it), pinned on the CPU.

Every delivery variant returns the same bits by design, so the parity suite cannot see a launch routed to the wrong kernel.  Here the
HOST half of kernels.hip (hipcc --cuda-host-only, seconds) is linked with a stand-in for the eight runtime entry points it needs
(tests/host_stub/dispatch_stub.cpp) and a driver with its own main (tests/host_stub/dispatch_driver.cpp) that calls
nbl::launch_force_kernel over the product of everything that selects a kernel, out-of-range values included: 768 000 cases per build.
The stand-in prints the device name, the block size, the dynamic LDS and whether the dynamic-LDS attribute was set for that kernel.

tests/golden/force_dispatch.json was written by tests/golden/make_force_dispatch.py from the kernels.hip that still picked its
instantiation with hand-unrolled switches and ladders, before the selection became one function.  Per build (product, and the diagnostic
build -DNBODY_DIAG_LOOPS) it holds the sha256 of the whole table, and for every kernel the object registers the number of cases that
reach it (0: not a force kernel).  The test asserts the hash, the counts, and that the set of registered kernels is the golden's."""
import collections
import hashlib
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mini_nbody_amd", "csrc")
STUB = os.path.join(ROOT, "tests", "host_stub")
GOLDEN = os.path.join(ROOT, "tests", "golden", "force_dispatch.json")
BUILDS = {"product": [], "diag": ["-DNBODY_DIAG_LOOPS"]}
CASES = 2 * 5 * 5 * 5 * 4 * 6 * 2 * 2 * 4 * 2 * 2 * 2
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CXX = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Wno-unused-function"]


def run(cmd, **kw):
    r = subprocess.run(cmd, capture_output=True, timeout=600, **kw)
    assert r.returncode == 0, (cmd, r.stderr.decode(errors="replace")[-3000:])
    return r.stdout


def dispatch_table(build, tmp):
    """{"sha256", "cases", "kernels": {device name: cases that launch it}} of kernels.hip as it stands, built with BUILDS[build]"""
    tmp = str(tmp)
    objs = [os.path.join(tmp, n + ".o") for n in ("kernels", "stub", "driver")]
    run([HIPCC, "--offload-arch=gfx950", "--cuda-host-only"] + FLAGS + BUILDS[build] + ["-c", os.path.join(CSRC, "kernels.hip"), "-o", objs[0]])
    for src, obj in (("dispatch_stub.cpp", objs[1]), ("dispatch_driver.cpp", objs[2])):
        run([CXX, "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"] + FLAGS + ["-c", os.path.join(STUB, src), "-o", obj])
    exe = os.path.join(tmp, "dispatch_" + build)
    # the fat-binary data symbol of a host-only object stays unresolved: the stand-in never reads it
    run([CXX] + objs + ["-o", exe, "-Wl,--unresolved-symbols=ignore-all"])
    table = run([exe])
    names = run([exe, "names"]).decode().split()
    lines = table.decode().splitlines()
    counts = collections.Counter(ln.split(" -> ", 1)[1].split(" ", 1)[0] for ln in lines)
    assert set(counts) <= set(names), sorted(set(counts) - set(names))
    return {"sha256": hashlib.sha256(table).hexdigest(), "cases": len(lines), "kernels": {k: counts.get(k, 0) for k in sorted(names)}}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_every_launch_takes_the_kernel_it_took(build, golden, tmp_path):
    got, want = dispatch_table(build, tmp_path), golden[build]
    assert got["cases"] == want["cases"] == CASES
    assert sorted(got["kernels"]) == sorted(want["kernels"])          # the same instantiations exist
    moved = {k: (want["kernels"][k], got["kernels"][k]) for k in want["kernels"] if want["kernels"][k] != got["kernels"][k]}
    assert not moved, moved                                           # (kernel: cases then, cases now)
    assert got["sha256"] == want["sha256"]


def test_golden_shape(golden):
    """the product library has 124 kernels, 116 of them force kernels that some case reaches; the diagnostic build only adds to them"""
    p, d = golden["product"]["kernels"], golden["diag"]["kernels"]
    assert len(p) == 124 and sum(1 for c in p.values() if c) == 116
    assert set(p) < set(d) and all(d[k] <= p[k] for k in p)
    assert sum(p.values()) == sum(d.values()) == CASES
