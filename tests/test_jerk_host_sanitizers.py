"""The jerk pass's HOST code (nbody_jerk(_d), nbody_jerk_rows(_d): point_sums.cpp and query_pass.hpp's velocity gather) under
AddressSanitizer + UBSan on the CPU, as tests/test_host_sanitizers.py runs its cases and with its build() and run(): a stand-alone
program with its own main, linked from the host files, hip_stub.cpp, the stub of point_sums.hip that knows all three passes
(jerk_stub.cpp: values pushed through both velocity pointers and the rows form's offset) and the driver jerk_sanity.cpp.  Nothing is
loaded into Python under a sanitizer.  The driver covers m = 1, 255, 256, 257 and 5000, skip present and absent, either output NULL, row
windows that straddle three ragged stub devices after steps have changed the velocities, nbody_field calls between jerk calls on one
context, the source split forced and automatic, the batched path, every NBODY_ERR_ARG case and the failure sweep."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "jerk"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("point_sums.cpp",), ("hip_stub.cpp", "jerk_stub.cpp", "jerk_sanity.cpp"), [],
                        ("NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB", "NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"), "jerk_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_jerk_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
