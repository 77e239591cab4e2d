"""The block time step entry points (nbody_step_hermite_block(_d); include/nbody.h "individual block time steps") as far as no GPU is
needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement tests/hermite_block_ref.c itself —
levels = 1 against tests/hermite_ref.c bit for bit, binary64 against a plain numpy block scheme on the system of the energy test, the
invariant on every trace, the counters the GPU tests rely on, and the energy figures their bound is taken from."""
import ctypes as C
import re

import numpy as np
import pytest

from field_common import ROOT
from hermite_block_common import ENERGY_RATIO_BOUND, ENERGY_RUN, BlockRef, compile_ref, energy_system, equal_slices, numpy_block, shared_steps_for
from hermite_common import HermiteRef, energy, kepler, worst
from hermite_common import compile_ref as compile_hermite_ref
from pass_common import same

NAMES = (("nbody_step_hermite_block", 6), ("nbody_step_hermite_block_d", 6))
CASE = dict(eta=0.04, dt_max=1.0 / 64, levels=8, nblocks=1)   # the run of the GPU tests' bit-for-bit cases


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return BlockRef(compile_ref(tmp_path_factory.mktemp("hermite_block_ref")))


@pytest.fixture(scope="module")
def shared_ref(tmp_path_factory):
    return HermiteRef(compile_hermite_ref(tmp_path_factory.mktemp("hermite_ref")))


def test_symbols_are_declared_exported_and_bound(nb):
    header = open(ROOT + "/include/nbody.h").read()
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs
    assert callable(nb.NBody.step_hermite_block)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    s, e = C.c_longlong(7), C.c_longlong(7)
    assert lib.nbody_step_hermite_block(0.02, 0.0625, 8, 1, C.byref(s), C.byref(e)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite_block_d(0.02, 0.0625, 8, 1, C.byref(s), C.byref(e)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite_block(0.02, 0.0625, 8, 1, None, None) == nb._lib.ERR_NOT_INIT
    assert (s.value, e.value) == (7, 7)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_level_is_the_shared_step_bit_for_bit(nb, ref, shared_ref, dtype):
    """levels = 1: every row is active in every sub-step with h = dt_max, the points form with skip = self is the rows form"""
    for n in (1, 2, 63, 257, 1025):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        pos[:, 3], vel[:, 3] = np.arange(n) % 977, np.arange(n) % 31 + 0.25
        for is_ref in ((False, True) if dtype == np.float32 else (False,)):
            for dt in (1.0 / 256, 0.01):
                p, v, steps, evals, trace = ref.run(pos, vel, dtype, 0.02, dt, 1, 3, ref=is_ref)
                assert same((p, v), shared_ref.step(pos, vel, dtype, dtype(dt), 3, ref=is_ref)), (n, dt, is_ref)
                assert (steps, evals) == (3, 3 * n) and all(len(r) == n for r in trace.rows)


def test_binary64_is_the_numpy_block_scheme_on_the_energy_system(ref):
    """the same counters, the state to 1e-12 (measured 1.4e-13), and the energy figures the GPU test's bound is taken from: the block
    call loses 1.58e-6, the shared step with as many row evaluations rounded up to 16 steps (496) 2.90e-3, ratio 5.45e-4 — a factor 18
    inside ENERGY_RATIO_BOUND = 1e-2 (at least the factor 10 the bound needs to stay).  (480 shared steps lose 3.42e-3: ratio 4.6e-4.)"""
    pos, vel = energy_system()
    p, v, steps, evals, trace = ref.run(pos, vel, np.float64, **ENERGY_RUN)
    wp, wv, wsteps, wevals = numpy_block(pos, vel, **ENERGY_RUN)
    assert (steps, evals) == (wsteps, wevals) == (1839, 3876)
    err = worst(p, v, wp, wv)
    print("hermite_block_f64 against numpy: %.3e" % err)
    assert err <= 1e-12
    trace.check_invariant(8, ENERGY_RUN["levels"], ENERGY_RUN["nblocks"])
    assert evals < steps * 8 / 2
    e0 = energy(pos, vel)
    de_block = abs(energy(p, v) - e0) / abs(e0)
    de_numpy = abs(energy(wp, wv) - e0) / abs(e0)
    k = shared_steps_for(evals, 8)
    assert k == 496
    shared = HermiteRefOf(ref).step(pos, vel, k)
    de_shared = abs(energy(*shared) - e0) / abs(e0)
    print("|dE/E|: block %.3e (numpy %.3e), shared dt with %d steps %.3e, ratio %.3e" % (de_block, de_numpy, k, de_shared, de_block / de_shared))
    assert de_block <= 2e-6 and de_numpy <= 2e-6
    assert de_block <= ENERGY_RATIO_BOUND / 10 * de_shared


class HermiteRefOf:
    """the shared step through hermite_block_ref.c itself: levels = 1 (asserted above to be hermite_ref.c's step)"""

    def __init__(self, ref):
        self.ref = ref

    def step(self, pos, vel, nsteps):
        return self.ref.run(pos, vel, np.float64, 0.02, 1.0 / nsteps, 1, nsteps, trace=False)[:2]


def case_bodies(nb, n, dtype):
    return kepler(0.9, dtype) if n == 2 else nb.make_bodies(n, dtype=dtype)


def test_the_invariant_and_the_counters_of_the_gpu_cases(nb, ref):
    """every size of the GPU tests' bit-for-bit cases in strict binary32: the invariant on the trace, and the counters and level
    occupancy the tests' inputs are chosen for"""
    seen = {}
    for n in (1, 2, 63, 257, 1025, 2100):
        pos, vel = case_bodies(nb, n, np.float32)
        p, v, steps, evals, trace = ref.run(pos, vel, np.float32, **CASE)
        trace.check_invariant(n, CASE["levels"], CASE["nblocks"])
        seen[n] = (len(set(trace.level0.tolist())), steps, evals)
        assert any(len(r) == n for r in trace.rows)
        if n >= 63:
            assert trace.occupied_levels() >= 3
        if n >= 1025:
            assert trace.crosses_tile_edge()
    print(seen)
    assert seen[1] == (1, 1, 1) and seen[2][0] == 1
    assert seen[63][:2] == (5, 104) and seen[1025][:2] == (8, 128) and seen[2100][:2] == (8, 128)
    assert seen[2100][2] < 268800 * 0.3      # (70641 in strict binary32; 70639 in plain numpy binary64)


def test_idle_slices_of_the_layout_cases(nb, ref):
    """contiguous equal slices: make_bodies(257) on three has a slice without an active row in 14 of its 107 sub-steps (14 on two as well),
    N = 63 in 84 of 104"""
    for n, parts, want in ((257, 3, (107, 14)), (257, 2, (107, 14)), (63, 3, (104, 84))):
        pos, vel = nb.make_bodies(n)
        steps, trace = ref.run(pos, vel, np.float32, **CASE)[2::2]
        assert (steps, len(trace.idle_substeps(equal_slices(n, parts)))) == want, (n, parts)
