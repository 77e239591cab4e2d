"""The sixth-order block time step entry points (nbody_step_hermite6_block(_d); include/nbody.h "sixth-order individual block time
steps") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement
tests/hermite6_block_ref.c itself — levels = 1 against tests/hermite6_ref.c bit for bit, binary64 against a plain numpy scheme on the
system of the energy test, the invariant on every trace, the energy figures the bounds are taken from (against the fourth-order block
statement and against the shared sixth-order step with as many row evaluations), what the GPU tests' inputs exercise, and the
zero-mass tracers."""
import ctypes as C
import re

import numpy as np
import pytest

from field_common import ROOT
from hermite_block_common import BlockRef
from hermite_block_common import compile_ref as compile_block4
from hermite_common import energy, worst
from hermite6_common import Hermite6Ref
from hermite6_common import compile_ref as compile_hermite6
from hermite6_block_common import (ENERGY_RATIO_BOUND_BLOCK4, ENERGY_RATIO_BOUND_SHARED6, ENERGY_RUN, ENERGY_STRICT_F32, GPU_CASE, GPU_LEVELS,
                                   GPU_SIZES, Block6Ref, case_bodies, compile_ref, energy_system, equal_slices, numpy_ajs, numpy_block6,
                                   row_traces, shared_steps_for)
from pass_common import same

NAMES = (("nbody_step_hermite6_block", 6), ("nbody_step_hermite6_block_d", 6))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Block6Ref(compile_ref(tmp_path_factory.mktemp("hermite6_block_ref")))


@pytest.fixture(scope="module")
def shared_ref(tmp_path_factory):
    return Hermite6Ref(compile_hermite6(tmp_path_factory.mktemp("hermite6_ref")))


@pytest.fixture(scope="module")
def block4_ref(tmp_path_factory):
    return BlockRef(compile_block4(tmp_path_factory.mktemp("hermite_block_ref")))


def test_symbols_are_declared_exported_and_bound(nb):
    header = open(ROOT + "/include/nbody.h").read()
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs
    assert callable(nb.NBody.step_hermite6_block)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    s, e = C.c_longlong(7), C.c_longlong(7)
    assert lib.nbody_step_hermite6_block(0.02, 0.0625, 8, 1, C.byref(s), C.byref(e)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite6_block_d(0.02, 0.0625, 8, 1, C.byref(s), C.byref(e)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite6_block(0.02, 0.0625, 8, 1, None, None) == nb._lib.ERR_NOT_INIT
    assert (s.value, e.value) == (7, 7)


def test_numpy_ajs_is_the_snap_statement(nb, shared_ref):
    """the plain numpy (a, j, s) the numpy scheme is built on, against tests/snap_ref.c's rows form in binary64: 300 bodies, relative to
    the largest component of each output (sums of 299 terms in another order: a few 1e-16 per term)"""
    pos, vel = nb.make_bodies(300, dtype=np.float64)
    fn = shared_ref.lib.snap_rows_f64
    fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3, None
    want = [np.zeros((300, 4)) for _ in range(3)]
    fn(pos.ctypes.data, vel.ctypes.data, 300, 0, 0, *(w.ctypes.data for w in want))
    for got, w in zip(numpy_ajs(pos[:, :3].copy(), vel[:, :3].copy()), want):
        assert np.abs(got - w[:, :3]).max() <= 1e-12 * np.abs(w).max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_one_level_is_the_shared_step_bit_for_bit(nb, ref, shared_ref, dtype):
    """levels = 1: every row is active in every sub-step with h = dt_max, the points form with skip = self is the rows form, and the
    per-row coefficients are the shared step's; both d2 forms, with and without masses"""
    for n in (1, 2, 63, 257, 1025):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        pos[:, 3], vel[:, 3] = np.arange(n) % 7 * 0.25, np.arange(n) % 31 + 0.25
        for is_ref in ((False, True) if dtype == np.float32 else (False,)):
            for mass in (False, True):
                for dt in (1.0 / 256, 0.01):
                    p, v, steps, evals, trace = ref.run(pos, vel, dtype, 0.02, dt, 1, 3, ref=is_ref, mass=mass)
                    assert same((p, v), shared_ref.step(pos, vel, dtype, dtype(dt), 3, flags=int(is_ref) | 2 * int(mass))), (n, dt, is_ref, mass)
                    assert (steps, evals) == (3, 3 * n) and all(len(r) == n for r in trace.rows)
                    assert same(p[:, 3], pos[:, 3]) and same(v[:, 3], vel[:, 3])


def test_binary64_is_the_numpy_scheme_and_the_energy_figures(ref, shared_ref, block4_ref):
    """energy_system() under ENERGY_RUN in binary64: the statement gives the plain numpy scheme's counters, its state to 1e-12 (measured
    3.4e-13) and its |dE/E| (5.926e-07 both); the invariant holds on the trace.  The figures the bounds are taken from
    (hermite6_block_common says what they mean): the fourth-order block statement on the same run loses 1.583e-06, ratio 0.374 — the
    condition that the sixth-order block run loses less; the shared sixth-order step with as many row evaluations (496 steps) loses
    1.093e-04, ratio 5.42e-3 against a bound of 5e-2."""
    pos, vel = energy_system()
    p, v, steps, evals, trace = ref.run(pos, vel, np.float64, **ENERGY_RUN)
    wp, wv, wsteps, wevals = numpy_block6(pos, vel, **ENERGY_RUN)
    assert (steps, evals) == (wsteps, wevals) == (1839, 3876)
    err = worst(p, v, wp, wv)
    print("hermite6_block_f64 against numpy: %.3e" % err)
    assert err <= 1e-12
    trace.check_invariant(8, ENERGY_RUN["levels"], ENERGY_RUN["nblocks"])
    assert evals < steps * 8 / 2
    e0 = energy(pos, vel)
    de = lambda state: abs(energy(*state) - e0) / abs(e0)
    de_block, de_numpy = de((p, v)), de((wp, wv))
    b4 = block4_ref.run(pos, vel, np.float64, **ENERGY_RUN)
    de_block4 = de(b4[:2])
    k = shared_steps_for(evals, 8)
    assert k == 496
    de_shared = de(shared_ref.step(pos, vel, np.float64, 1.0 / k, k))
    print("|dE/E|: sixth-order block %.3e (numpy %.3e); fourth-order block %.3e (%d sub-steps, %d row evaluations), ratio %.3e; "
          "sixth-order shared dt with %d steps %.3e, ratio %.3e" % (de_block, de_numpy, de_block4, b4[2], b4[3], de_block / de_block4, k, de_shared,
                                                                 de_block / de_shared))
    assert de_block <= 7e-7 and de_numpy <= 7e-7
    assert abs(de_block - de_numpy) <= 1e-3 * de_block                # the same figure to three digits, as the fourth-order pair's 1.58e-6
    assert de_block < ENERGY_RATIO_BOUND_BLOCK4 * de_block4
    assert de_block <= ENERGY_RATIO_BOUND_SHARED6 * de_shared


def test_strict_binary32_energy_figure(ref):
    """the figure the timed binary32 GPU test's bound is 4 x of: the statement in binary32 on the same run, both d2 forms"""
    pos, vel = energy_system()
    e0 = energy(pos, vel)
    seen = {}
    for is_ref in (False, True):
        p, v, steps, evals, trace = ref.run(pos, vel, np.float32, ref=is_ref, **ENERGY_RUN)
        trace.check_invariant(8, ENERGY_RUN["levels"], ENERGY_RUN["nblocks"])
        seen[is_ref] = (steps, evals, abs(energy(p, v) - e0) / abs(e0))
    print(seen)
    assert seen[False][:2] == (1840, 3877)
    assert abs(seen[False][2] - ENERGY_STRICT_F32) <= 1e-3 * ENERGY_STRICT_F32


def test_what_the_gpu_cases_exercise(nb, ref):
    """every size and level count of the GPU tests' bit-for-bit cases in strict binary32: the invariant on the trace, a sub-step of all
    rows in every case, and on 8 levels the occupancy, the one-row sub-step, the tile edge and the idle slices they are chosen for"""
    seen = {}
    for n in GPU_SIZES:
        pos, vel = case_bodies(nb, n, np.float32)
        for levels in GPU_LEVELS:
            p, v, steps, evals, trace = ref.run(pos, vel, np.float32, levels=levels, **GPU_CASE)
            trace.check_invariant(n, levels, GPU_CASE["nblocks"])
            assert any(len(r) == n for r in trace.rows)
            assert levels > 1 or (steps, evals) == (2, 2 * n)
            if levels == 8:
                seen[n] = dict(occupied=trace.occupied_levels(), one_row=sum(len(r) == 1 for r in trace.rows), edge=trace.crosses_tile_edge(),
                               idle3=len(trace.idle_substeps(equal_slices(n, 3))), idle2=len(trace.idle_substeps(equal_slices(n, 2))),
                               steps=steps, evals=evals)
    print(seen)
    assert seen[1]["steps"] == 2 and seen[8]["occupied"] >= 3
    for n in (257, 611):
        s = seen[n]
        assert s["occupied"] >= 3 and s["one_row"] >= 1 and s["edge"] and s["idle3"] >= 1 and s["idle2"] >= 1, (n, s)
        assert s["evals"] < s["steps"] * n / 2
    assert (seen[611]["occupied"], seen[611]["steps"]) == (8, 255) and (seen[257]["steps"], seen[257]["idle3"]) == (235, 14)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_zero_mass_tracers_change_nothing_of_the_massive_rows(nb, ref, dtype):
    """with masses, 40 tracers (w = +0) behind 257 massive bodies, some of them close to a massive body so that they take finer levels
    and add sub-steps of their own: no bit of the first 257 rows differs, and every massive row is active at the same times and goes on
    with the same levels.  (A tracer's terms are fma(d, +-0, sum): exact, and a block of sources behind the massive ones adds +-0 to a
    sum that is not -0.)  w = 1 everywhere is the unweighted statement bit for bit."""
    n, extra = 257, 40
    pos, vel = nb.make_bodies(n + extra, dtype=dtype)
    pos[:n, 3] = (1 + np.arange(n) % 4) * 0.25
    pos[n:, 3] = 0
    pos[n:n + 8, :3] = pos[:8, :3] + dtype(0.004)        # tracers in tight orbits about massive bodies: the finest levels
    run = dict(GPU_CASE, levels=8)
    alone = ref.run(pos[:n], vel[:n], dtype, mass=True, **run)
    both = ref.run(pos, vel, dtype, mass=True, **run)
    assert same((both[0][:n], both[1][:n]), alone[:2])
    assert row_traces(both[4], n) == row_traces(alone[4], n)
    assert both[2] > alone[2] and both[3] > alone[3]                  # the tracers did add sub-steps: the claim is not empty
    assert same(both[0][:, 3], pos[:, 3])
    ones = pos.copy()
    ones[:, 3] = 1
    assert same(ref.run(ones, vel, dtype, mass=True, trace=False, **run)[:2], ref.run(ones, vel, dtype, trace=False, **run)[:2])
    assert not same(ref.run(pos[:n], vel[:n], dtype, trace=False, **run)[0], alone[0])
