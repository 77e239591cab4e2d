"""The Hermite entry points (nbody_step_hermite(_d), nbody_min_aarseth, nbody_step_hermite_adaptive(_d); include/nbody.h "fourth-order
Hermite integrator") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU
statement tests/hermite_ref.c itself — against a plain numpy binary64 Hermite on the Kepler pair, its order of convergence, its restart
rule, its minimum and adaptive loop against numpy, and the binary32 statement's own error r_ref, on which the GPU test's bound rests."""
import ctypes as C
import re

import numpy as np
import pytest

from field_common import ROOT
from hermite_common import (PERIOD, R_REF, R_REF_MEDIAN, TIMED, HermiteRef, compile_ref, energy, kepler, numpy_aj, numpy_hermite, numpy_hermite_adaptive,
                            position_error, worst, worst_median)

NAMES = (("nbody_step_hermite", 2), ("nbody_step_hermite_d", 2), ("nbody_min_aarseth", 2), ("nbody_step_hermite_adaptive", 7),
         ("nbody_step_hermite_adaptive_d", 7))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return HermiteRef(compile_ref(tmp_path_factory.mktemp("hermite_ref")))


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_symbols_are_declared_exported_and_bound(nb):
    header = open(ROOT + "/include/nbody.h").read()
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs
    assert callable(nb.NBody.step_hermite) and callable(nb.NBody.min_aarseth) and callable(nb.NBody.step_hermite_adaptive)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    t, steps, q, row = C.c_double(7.0), C.c_int(7), C.c_double(7.0), C.c_int(7)
    assert lib.nbody_step_hermite(0.01, 1) == nb._lib.ERR_NOT_INIT and lib.nbody_step_hermite_d(0.01, 1) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_min_aarseth(C.byref(q), C.byref(row)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite_adaptive(0.04, 1.0, 1e-6, 1.0, 10, C.byref(t), C.byref(steps)) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_step_hermite_adaptive_d(0.04, 1.0, 1e-6, 1.0, 10, C.byref(t), C.byref(steps)) == nb._lib.ERR_NOT_INIT
    assert (t.value, steps.value, q.value, row.value) == (7.0, 7, 7.0, 7)


def test_hermite_ref_f64_is_the_numpy_hermite_on_the_kepler_pair(ref):
    for e in (0.0, 0.5, 0.9):
        pos, vel = kepler(e)
        for n in (1, 16, 128):
            p, v = ref.step(pos, vel, np.float64, 1.0 / n, n)
            wp, wv = numpy_hermite(pos, vel, 1.0 / n, n)
            err = worst(p, v, wp, wv)
            print("e=%.1f n=%d: hermite_f64 against numpy %.3e" % (e, n, err))
            assert err <= 1e-13
            assert np.array_equal(bits(p[:, 3]), bits(pos[:, 3])) and np.array_equal(bits(v[:, 3]), bits(vel[:, 3]))


def test_order_of_the_reference(ref):
    """Kepler e = 0.5 to t = 1: the position error against the numpy run of 8192 steps falls by 16 +- 1 per halving of dt.
    Measured: 15.90 and 15.96."""
    pos, vel = kepler(0.5)
    want = numpy_hermite(pos, vel, 1.0 / 8192, 8192)[0]
    err = [position_error(ref.step(pos, vel, np.float64, 1.0 / n, n)[0], want) for n in (64, 128, 256)]
    ratios = [err[0] / err[1], err[1] / err[2]]
    print("position errors %s, ratios %.2f %.2f" % (err, *ratios))
    assert all(15.0 <= r <= 17.0 for r in ratios), ratios


def test_energy_against_kick_drift_on_the_cpu(ref):
    """what the issue rests on: 128 Hermite steps of the Kepler pair lose far less energy than 128 kick-drift steps"""
    pos, vel = kepler(0.5)
    e0 = energy(pos, vel)
    p, v = ref.step(pos, vel, np.float64, 1.0 / 128, 128)
    r, u = pos[:, :3].copy(), vel[:, :3].copy()
    for _ in range(128):
        u = u + numpy_aj(r, u)[0] / 128
        r = r + u / 128
    de_h, de_e = abs(energy(p, v) - e0) / abs(e0), abs(energy(r, u) - e0) / abs(e0)
    print("|dE|/|E|: Hermite %.3e, kick-drift %.3e" % (de_h, de_e))
    assert de_h < 1e-3 * de_e


def test_restart_rule_and_carried_w(nb, ref):
    """two calls of one step are the reference restarted twice; one call of two steps differs from it in general; the fourth values of
    both words come through bit for bit"""
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
        assert np.array_equal(bits(carried[0][:, 3]), bits(pos.astype(dtype)[:, 3])) and np.array_equal(bits(carried[1][:, 3]), bits(vel.astype(dtype)[:, 3]))


def test_min_aarseth_of_the_reference(nb, ref):
    pos, vel = nb.make_bodies(700, dtype=np.float64)
    a, j = numpy_aj(pos[:, :3], vel[:, :3])
    q = (a * a).sum(1) / (j * j).sum(1)
    got_q, got_row = ref.min_aarseth(pos, vel, np.float64)
    assert got_row == int(np.argmin(q)) and abs(got_q - q.min()) <= 1e-10 * q.min()
    assert ref.min_aarseth(pos[:1], vel[:1], np.float64) == (np.inf, -1)
    assert ref.min_aarseth(pos[:1], vel[:1], np.float32) == (np.inf, -1)


def test_adaptive_loop_of_the_reference(ref):
    """Kepler e = 0.9 over one period, eta = 0.04: the numpy loop takes 352 steps, and the shared Aarseth step beats a constant dt with
    as many steps by far.  Measured: |dE|/|E| = 1.2e-6 adaptive against 0.37 constant."""
    pos, vel = kepler(0.9)
    e0 = energy(pos, vel)
    p, v, t, steps = ref.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0)
    wp, wv, wsteps = numpy_hermite_adaptive(pos, vel, 0.04, PERIOD, 1e-6, 1.0)
    de = abs(energy(p, v) - e0) / abs(e0)
    pc, vc = ref.step(pos, vel, np.float64, PERIOD / steps, steps)
    de_c = abs(energy(pc, vc) - e0) / abs(e0)
    print("steps %d (numpy %d), t %.17g, |dE|/|E| adaptive %.3e constant %.3e, against numpy %.3e" % (steps, wsteps, t, de, de_c, worst(p, v, wp, wv)))
    assert wsteps == 352 and steps == wsteps and t == PERIOD
    assert worst(p, v, wp, wv) <= 1e-9
    assert de < 1e-4 and de < 1e-3 * de_c
    p5, v5, t5, s5 = ref.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0, max_steps=5)
    assert s5 == 5 and 0.0 < t5 < PERIOD


def test_binary32_statement_against_binary64(nb, ref):
    """r_ref: strict binary32 hermite_ref against the numpy binary64 run at hermite_common.TIMED (N = 2100 make_bodies, 4 steps of
    1/256), the worst |delta| over position and velocity components relative to max(1, |value|).  The GPU test of the timed arithmetic
    is bounded by 2 r_ref + 6e-7 with r_ref = hermite_common.R_REF = 0.16, which this asserts.  Measured: 1.557e-1 in both d2 forms —
    one unresolved collision (hermite_common.R_REF says which); the median body keeps 6.0e-6, asserted against R_REF_MEDIAN = 1e-5."""
    n, steps, dt = TIMED
    pos, vel = nb.make_bodies(n)
    wp, wv = numpy_hermite(pos, vel, dt, steps)
    for r in (False, True):
        p, v = ref.step(pos, vel, np.float32, dt, steps, ref=r)
        err = worst(p, v, wp, wv)
        med = worst_median(p, v, wp, wv)
        print("binary32 hermite_ref (ref=%d) against binary64 numpy: worst %.3e, median body %.3e" % (r, err, med))
        assert err <= R_REF and med <= R_REF_MEDIAN, r
