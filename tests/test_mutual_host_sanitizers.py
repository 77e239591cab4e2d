"""NBODY_OPT_PAIRING in the library's HOST code (mutual.cpp: which passes take the mutual pairing, its table and counters; the option, its
info key and the step loop in context.cpp) under AddressSanitizer + UBSan on the CPU, as tests/test_host_sanitizers.py runs its cases and
with its build() and run(): a stand-alone program with its own main, linked from the host files and mutual.cpp, mutual_stub.cpp
(hip_stub.cpp itself plus a stand-in for the launch of mutual.hip that walks the library's own unit enumeration through the real argument
block and aborts unless every word of the table is written exactly once) and the driver mutual_sanity.cpp.  Nothing is loaded into Python
under a sanitizer."""
import shutil

import pytest

from test_host_sanitizers import ASAN, CASES, HOST, build, run

NAME = "mutual"
# one more row of the harness's case table, in its form (host files, stubs and driver, arguments, variables to clear, the line of success)
CASES.setdefault(NAME, (HOST + ("mutual.cpp",), ("mutual_stub.cpp", "mutual_sanity.cpp"), [], (), "mutual_sanity ok"))


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
def test_mutual_host_code_is_address_and_ub_clean():
    run(NAME, build(NAME, ASAN), CASES[NAME][2], {"ASAN_OPTIONS": "detect_leaks=1"})
