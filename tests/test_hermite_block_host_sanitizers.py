"""The block time steps' HOST code (nbody_step_hermite_block(_d): hermite_block.cpp on hermite.cpp's opening and gathers, point_sums.cpp's
jerk points pass over queries left on the device and query_pass.hpp's exchange of the ranks' words) under AddressSanitizer + UBSan on the
CPU, as tests/test_host_sanitizers.py runs its cases and with its build() and run(): a stand-alone program with its own main, linked
from the host files, hip_stub.cpp, the stubs of point_sums.hip (jerk_stub.cpp), hermite.hip (hermite_stub.cpp) and hermite_block.hip
(hermite_block_stub.cpp: the scheme's arithmetic and level rules pushed through the real BlockArgs) and the driver
hermite_block_sanity.cpp.  Nothing is loaded into Python under a sanitizer.  The driver covers three ragged stub devices, a device with
no active row in a sub-step, one level against nbody_step_hermite itself, the forced split and the batches, block calls interleaved with
nbody_step_hermite and nbody_jerk_rows on one context, every NBODY_ERR_ARG case and the failure sweep."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "hermite_block"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("point_sums.cpp", "hermite.cpp", "hermite_block.cpp"),
                        ("hip_stub.cpp", "jerk_stub.cpp", "hermite_stub.cpp", "hermite_block_stub.cpp", "hermite_block_sanity.cpp"), [],
                        ("NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"), "hermite_block_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_hermite_block_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
