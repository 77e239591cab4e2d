"""NBODY_OPT_MASSES in the library's HOST code (the option and its info key in context.cpp, the flag in energy.cpp's EnergyArgs and
point_sums.cpp's PointSumsArgs, the refusals of the unit-mass entry points in context.cpp, timescale.cpp, pair_energy.cpp and
mailbox.cpp) under AddressSanitizer + UBSan on the CPU, as tests/test_host_sanitizers.py runs its cases and with its build() and run():
a stand-alone program with its own main, linked from the host files, masses_stub.cpp (hip_stub.cpp itself plus stand-ins that echo the
`masses` member of both argument blocks), the stubs of timescale.hip and pair_energy.hip and the driver masses_sanity.cpp.  Nothing is
loaded into Python under a sanitizer.  The driver covers the option's values and read-back, a fresh context's 0, the flag in every
weighted pass unsplit and split on one and three stub devices in both precisions, a switch of the option between calls, every refusal
(nothing created, outputs and state untouched) and the same calls once the option is off, the mailbox's refusals and the failure sweep."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "masses"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("point_sums.cpp", "timescale.cpp", "pair_energy.cpp"),
                        ("masses_stub.cpp", "timescale_stub.cpp", "pair_energy_stub.cpp", "masses_sanity.cpp"), [],
                        ("NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB", "NBODY_TIDAL_SPLIT", "NBODY_TIDAL_SCRATCH_MB", "NBODY_JERK_SPLIT",
                         "NBODY_JERK_SCRATCH_MB", "NBODY_TIMESCALE_SPLIT", "NBODY_TIMESCALE_SCRATCH_MB", "NBODY_PAIR_ENERGY_SPLIT",
                         "NBODY_PAIR_ENERGY_SCRATCH_MB"), "masses_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_masses_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
