"""The sixth-order block time steps' HOST code (nbody_step_hermite6_block(_d): hermite6_block.cpp on hermite6.cpp's opening,
hermite_block.cpp's next-time read, hermite.cpp's gathers, point_sums.cpp's snap points pass over queries left on the device and
query_pass.hpp's gather of the predicted accelerations) under AddressSanitizer + UBSan on the CPU, as tests/test_host_sanitizers.py runs
its cases and with its build() and run(): a stand-alone program with its own main, linked from the host files, hip_stub.cpp, the stubs of
point_sums.hip (snap_stub.cpp), hermite.hip (hermite_stub.cpp), hermite_block.hip (hermite_block_stub.cpp: the next-time reduction),
hermite6.hip (hermite6_stub.cpp) and hermite6_block.hip (hermite6_block_stub.cpp: the scheme's arithmetic and level rules pushed through
the real Block6Args) and the driver hermite6_block_sanity.cpp.  Nothing is loaded into Python under a sanitizer.  The driver covers three
ragged stub devices, a device with no active row in a sub-step, one level against nbody_step_hermite6 itself, the forced split and the
batches, block calls interleaved with the other integrators and nbody_snap_rows on one context, every NBODY_ERR_ARG case and the failure
sweep."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "hermite6_block"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("point_sums.cpp", "hermite.cpp", "hermite_block.cpp", "hermite6.cpp", "hermite6_block.cpp"),
                        ("hip_stub.cpp", "snap_stub.cpp", "hermite_stub.cpp", "hermite_block_stub.cpp", "hermite6_stub.cpp", "hermite6_block_stub.cpp",
                         "hermite6_block_sanity.cpp"), [],
                        ("NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB", "NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"), "hermite6_block_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_hermite6_block_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
