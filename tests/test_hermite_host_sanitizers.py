"""The Hermite integrator's HOST code (nbody_step_hermite(_d), nbody_min_aarseth, nbody_step_hermite_adaptive(_d): hermite.cpp on
point_sums.cpp's jerk rows pass and query_pass.hpp's gathers) under AddressSanitizer + UBSan on the CPU, as tests/test_host_sanitizers.py
runs its cases and with its build() and run(): a stand-alone program with its own main, linked from the host files, hip_stub.cpp, the
stub of point_sums.hip that knows the jerk (jerk_stub.cpp), the stub of hermite.hip (hermite_stub.cpp: the step's arithmetic pushed
through the real HermiteArgs) and the driver hermite_sanity.cpp.  Nothing is loaded into Python under a sanitizer.  The driver covers
three ragged stub devices, calls of 1 and 3 steps, the adaptive loop hitting max_steps and hitting t_end, nbody_min_aarseth with either
pointer NULL, Hermite calls interleaved with nbody_step and nbody_jerk_rows on one context, the forced split and the batches, every
NBODY_ERR_ARG case and the failure sweep."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "hermite"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("point_sums.cpp", "hermite.cpp"), ("hip_stub.cpp", "jerk_stub.cpp", "hermite_stub.cpp", "hermite_sanity.cpp"), [],
                        ("NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"), "hermite_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_hermite_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
