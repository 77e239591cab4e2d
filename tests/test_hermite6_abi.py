"""The sixth-order Hermite entry points (nbody_step_hermite6(_d), nbody_step_hermite6_adaptive(_d); include/nbody.h "sixth-order Hermite
integrator") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement
tests/hermite6_ref.c itself on the Kepler pair in binary64 — its order of convergence, which tells the scheme from the same scheme
without the crackle term, its energy error against the fourth-order statement's, its restart rule and its adaptive loop."""
import ctypes as C
import re

import numpy as np
import pytest

from field_common import ROOT
from hermite_common import PERIOD, HermiteRef, energy, kepler
from hermite_common import compile_ref as compile_hermite4
from hermite6_common import GAIN, MASS, NO_CRACKLE, ORDER_RATIO, Hermite6Ref, compile_ref, kepler_energy_error

NAMES = (("nbody_step_hermite6", 2), ("nbody_step_hermite6_d", 2), ("nbody_step_hermite6_adaptive", 7), ("nbody_step_hermite6_adaptive_d", 7))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Hermite6Ref(compile_ref(tmp_path_factory.mktemp("hermite6_ref")))


@pytest.fixture(scope="module")
def ref4(tmp_path_factory):
    return HermiteRef(compile_hermite4(tmp_path_factory.mktemp("hermite_ref")))


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_symbols_are_declared_exported_and_bound(nb):
    header = open(ROOT + "/include/nbody.h").read()
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs
    assert callable(nb.NBody.step_hermite6) and callable(nb.NBody.step_hermite6_adaptive)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    t, steps = C.c_double(7.0), C.c_int(7)
    assert lib.nbody_step_hermite6(0.01, 1) == nb._lib.ERR_NOT_INIT and lib.nbody_step_hermite6_d(0.01, 1) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite6_adaptive(0.04, 1.0, 1e-6, 1.0, 10, C.byref(t), C.byref(steps)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite6_adaptive_d(0.04, 1.0, 1e-6, 1.0, 10, C.byref(t), C.byref(steps)) == nb._lib.ERR_NOT_INIT
    assert (t.value, steps.value) == (7.0, 7)


def test_order_of_the_statement(ref):
    """Kepler e = 0.5 to t = 1, relative energy error: err(64) / err(128) >= 45 and err(128) / err(256) >= 45 (hermite6_common says
    where 45 comes from).  Measured: 64.9 and 64.5; the same scheme without the crackle term gives 32.9 and 32.5, which this also
    asserts lies below the bound — the test can tell the two apart."""
    err = [kepler_energy_error(lambda p, v, dt, n: ref.step(p, v, np.float64, dt, n), n) for n in (64, 128, 256)]
    ratios = [err[0] / err[1], err[1] / err[2]]
    print("energy errors %s, ratios %.2f %.2f" % (err, *ratios))
    assert all(r >= ORDER_RATIO for r in ratios), ratios
    wrong = [kepler_energy_error(lambda p, v, dt, n: ref.step(p, v, np.float64, dt, n, NO_CRACKLE), n) for n in (64, 128, 256)]
    wrong_ratios = [wrong[0] / wrong[1], wrong[1] / wrong[2]]
    print("without the crackle term %s, ratios %.2f %.2f" % (wrong, *wrong_ratios))
    assert all(r < ORDER_RATIO for r in wrong_ratios), wrong_ratios


def test_energy_against_the_fourth_order_statement(ref, ref4):
    """err6(128) <= err4(128) / 100.  Measured: 2.66e-10 against 1.838e-7, a ratio of 692."""
    err6 = kepler_energy_error(lambda p, v, dt, n: ref.step(p, v, np.float64, dt, n), 128)
    err4 = kepler_energy_error(lambda p, v, dt, n: ref4.step(p, v, np.float64, dt, n), 128)
    print("|dE|/|E| after 128 steps: sixth order %.3e, fourth order %.3e, ratio %.0f" % (err6, err4, err4 / err6))
    assert err6 <= err4 / GAIN


def test_restart_rule_and_carried_w(nb, ref):
    """two calls of one step are the statement restarted twice; one call of two steps differs from it (it carries the crackle and does
    not evaluate again); the fourth values of both words come through bit for bit"""
    pos, vel = nb.make_bodies(300)
    pos[:, 3] = np.arange(300, dtype=np.float32) - 7.5
    vel[:, 3] = np.float32(3.25)
    for dtype in (np.float32, np.float64):
        one = ref.step(pos, vel, dtype, 1.0 / 256, 1)
        twice = ref.step(*one, dtype, 1.0 / 256, 1)
        restarted = ref.restarted(pos, vel, dtype, 1.0 / 256, 2)
        carried = ref.step(pos, vel, dtype, 1.0 / 256, 2)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(twice, restarted))
        assert not all(np.array_equal(bits(a), bits(b)) for a, b in zip(carried, restarted))
        assert np.all(np.isfinite(carried[0])) and np.all(np.isfinite(restarted[0]))
        assert np.array_equal(bits(carried[0][:, 3]), bits(pos.astype(dtype)[:, 3])) and np.array_equal(bits(carried[1][:, 3]), bits(vel.astype(dtype)[:, 3]))


def test_first_step_is_independent_of_the_crackle_flag(nb, ref):
    """c0 = +0 in a call's first step: one step with and without the crackle term is the same step"""
    pos, vel = nb.make_bodies(300)
    for dtype in (np.float32, np.float64):
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(ref.step(pos, vel, dtype, 1.0 / 256, 1), ref.step(pos, vel, dtype, 1.0 / 256, 1, NO_CRACKLE)))


def test_adaptive_loop_of_the_statement(ref, ref4):
    """Kepler e = 0.9 over one period, eta = 0.04: the loop reaches t_end exactly and, step for step of the same rule, loses far less
    energy than the fourth-order statement; max_steps stops it early.  Measured: 352 steps both, |dE|/|E| 3.6e-9 against 1.2e-6."""
    pos, vel = kepler(0.9)
    e0 = energy(pos, vel)
    p, v, t, steps = ref.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0)
    p4, v4, t4, steps4 = ref4.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0)
    de, de4 = abs(energy(p, v) - e0) / abs(e0), abs(energy(p4, v4) - e0) / abs(e0)
    print("steps %d (fourth order %d), t %.17g, |dE|/|E| %.3e (fourth order %.3e)" % (steps, steps4, t, de, de4))
    assert t == PERIOD and abs(steps - steps4) <= 2
    assert de <= de4 / GAIN
    p5, v5, t5, s5 = ref.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0, max_steps=5)
    assert s5 == 5 and 0.0 < t5 < PERIOD


def test_masses_of_the_statement(ref):
    """masses_common's Kepler pair of masses 3/4 and 1/4, e = 0.5, 128 steps to t = 1, binary64: the weighted energy error is below the
    fourth-order statement's (tests/masses_ref.c) by the factor the unit-mass pair must reach, the masses are carried bit for bit, and
    the momentum — zero at the start — stays within the roundings of 128 steps: each step rounds a body's m v a few times (the
    corrector's three fma and its sums), which the two bodies do not share: 128 x 4 x 2^-53 of sum m |v|.
    Measured: |dE|/|E| 3.3e-11 against 4.7e-8; |P| / sum m |v| 3.9e-16."""
    import tempfile
    from masses_common import compile_masses_ref, kepler as kepler_masses, numpy_totals
    pos, vel = kepler_masses(0.75, 0.25, 0.5)
    e0, _, scale = numpy_totals(pos, vel)
    p, v = ref.step(pos, vel, np.float64, 1.0 / 128, 128, MASS)
    with tempfile.TemporaryDirectory() as tmp:
        p4, v4 = compile_masses_ref(tmp).hermite(pos, vel, np.float64, 1.0 / 128, 128)
    e6, mom, _ = numpy_totals(p, v)
    de, de4 = abs(e6 - e0) / abs(e0), abs(numpy_totals(p4, v4)[0] - e0) / abs(e0)
    print("masses 3/4 and 1/4: |dE|/|E| %.3e (fourth order %.3e), |P| / sum m |v| %.3e" % (de, de4, np.sqrt((mom ** 2).sum()) / scale))
    assert de <= de4 / GAIN
    assert np.sqrt((mom ** 2).sum()) / scale <= 128 * 4 * 2.0 ** -53
    assert np.array_equal(p[:, 3], pos[:, 3])
    unweighted = ref.step(pos, vel, np.float64, 1.0 / 128, 128)
    assert not np.array_equal(bits(unweighted[0]), bits(p))
