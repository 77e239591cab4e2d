"""The snap pass's and the sixth-order Hermite integrator's HOST code (nbody_snap(_d), nbody_snap_rows(_d), nbody_step_hermite6(_d),
nbody_step_hermite6_adaptive(_d): point_sums.cpp's third output, third source stream and opening jerk pass, query_pass.hpp's gather of a
per-row array, hermite6.cpp on hermite.cpp's buffers, minimum and loop) under AddressSanitizer + UBSan on the CPU, as
tests/test_host_sanitizers.py runs its cases and with its build() and run(): a stand-alone program with its own main, linked from the
host files, hip_stub.cpp, the stub of point_sums.hip that knows all four passes and sizes its sums for nine (snap_stub.cpp), the stubs
of hermite.hip and hermite6.hip (hermite_stub.cpp, hermite6_stub.cpp: the step's arithmetic pushed through the real argument blocks)
and the driver snap_sanity.cpp.  Nothing is loaded into Python under a sanitizer.  The driver covers rows and points, each output NULL
in turn, one and three stub devices with ragged slices, the forced and the automatic split, the batched path, every NBODY_ERR_ARG
case, three Hermite-6 steps as one call and as three — the same state on one device and on three — and the failure sweep."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "snap"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("point_sums.cpp", "hermite.cpp", "hermite6.cpp"),
                        ("hip_stub.cpp", "snap_stub.cpp", "hermite_stub.cpp", "hermite6_stub.cpp", "snap_sanity.cpp"), [],
                        ("NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB", "NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"), "snap_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_snap_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
