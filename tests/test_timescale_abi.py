"""The pair time-scale entry points (nbody_timescale_rows, nbody_min_timescale, nbody_step_adaptive and their _d forms; include/nbody.h
"pair time scales and a shared adaptive time step") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT
without a context, the CPU statement tests/timescale_ref.c itself — against a plain Python restatement with an exact fma, against
tests/neighbors_ref.c for d2min, and on hand-made systems whose answers are known by construction — and the driver loop restated in
numpy on a two-body orbit."""
import ctypes as C
import math

import numpy as np
import pytest

import neighbors_common
from timescale_common import (adaptive_run, bits, kick_drift, make_ref, python_timescales, same, same_system, total_energy,
                              two_body_orbit)

SYMBOLS = {"nbody_timescale_rows": 5, "nbody_timescale_rows_d": 5, "nbody_min_timescale": 4, "nbody_min_timescale_d": 4,
           "nbody_step_adaptive": 7, "nbody_step_adaptive_d": 7}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("timescale_ref"))


@pytest.fixture(scope="module")
def nref(tmp_path_factory):
    return neighbors_common.make_ref(tmp_path_factory.mktemp("neighbors_ref_ts"))


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs, name
    assert callable(nb.NBody.timescales) and callable(nb.NBody.min_timescale) and callable(nb.NBody.step_adaptive)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for sfx, dt, ct in (("", np.float32, C.c_float), ("_d", np.float64, C.c_double)):
        fp = lambda a: a.ctypes.data_as(C.POINTER(ct))
        tau2, idx, d2 = np.full(4, 7, dt), np.full(4, 7, np.int32), np.full(4, 7, dt)
        t, steps = C.c_double(7.0), C.c_int(7)
        assert getattr(lib, "nbody_timescale_rows" + sfx)(0, 4, fp(tau2), ip(idx), fp(d2)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_min_timescale" + sfx)(fp(tau2), ip(idx), ip(idx[1:]), fp(d2)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_step_adaptive" + sfx)(0.02, 1.0, 1e-6, 0.1, 10, C.byref(t), C.byref(steps)) == nb._lib.ERR_NOT_INIT
        assert np.all(tau2 == 7) and np.all(idx == 7) and np.all(d2 == 7) and t.value == 7.0 and steps.value == 7


def test_timescale_ref_against_the_python_restatement(nb, ref):
    """binary64, the same IEEE operations in the same order (the fma computed exactly and rounded once): the integers equal, tau2 and
    d2min the same bits.  The binary32 statement against the binary64 one: q carries the three differences' roundings squared (2 u each
    on their term), one product and two fma per sum (u each) — at most 5 u on d2 and on v2 — and the quotient's own u: |q32 - q64| <=
    ((1 + u)^6 / (1 - u)^5 - 1) q64, 11 u to first order, u = 2^-24; the measured worst is printed."""
    n = 120
    pos32, vel32 = nb.make_bodies(n, seed=42)
    pos, vel = pos32.astype(np.float64), vel32.astype(np.float64)
    got = ref.rows(pos, vel)
    want = python_timescales(pos, vel)
    assert np.array_equal(got[1], want[1])
    assert same(got[0], want[0]) and same(got[2], want[2])
    assert same(ref.rows(pos, vel, 17, 50), tuple(g[17:67] for g in got))
    t32, i32, d32 = ref.rows(pos32, vel32)
    rel = np.abs(t32.astype(np.float64) - got[0]) / got[0]
    agree = i32 == got[1]
    u = 2.0 ** -24
    print("binary32 against binary64: worst relative difference of tau2 %.3g (bound %.3g) over %d of %d rows with the same partner"
          % (rel[agree].max(), (1 + u) ** 6 / (1 - u) ** 5 - 1, agree.sum(), n))
    assert agree.sum() >= n // 2 and rel[agree].max() <= ((1 + u) ** 6 / (1 - u) ** 5 - 1) * (1 + 1e-9)   # (1e-9: the binary64 side's own roundings)
    # the system form is the rows' best in ascending order
    tau2, i, j, d2min = ref.system(pos, vel)
    k = int(np.argmin(got[0]))
    assert (i, j) == (k, int(got[1][k])) and bits(tau2) == bits(got[0][k]) and bits(d2min) == bits(got[2].min())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_d2min_is_the_neighbour_statements_d2(nb, ref, nref, dtype):
    for n in (2, 65, 1100):
        pos, vel = nb.make_bodies(n, seed=9, dtype=dtype)
        if n > 1000:
            pos[70, :3] = pos[3, :3]   # a coincident pair: +0
        assert same(ref.rows(pos, vel)[2], nref.rows(pos)[1]), n
        assert bits(ref.system(pos, vel)[3]) == bits(nref.closest_pair(pos)[2]), n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_made_systems(ref, dtype):
    def system(p, v):
        pos, vel = np.zeros((len(p), 4), dtype), np.zeros((len(p), 4), dtype)
        pos[:, :3], vel[:, :3] = p, v
        return pos, vel

    inf = dtype(np.inf)
    # one body: nobody else
    pos, vel = system([[1, 2, 3]], [[1, 0, 0]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert idx[0] == -1 and tau2[0] == inf and d2[0] == inf
    assert same_system(ref.system(pos, vel), (inf, -1, -1, inf))
    # two bodies: d2 = 4, v2 = 16, each the other's partner; the system's i is the lower row
    pos, vel = system([[0, 0, 0], [2, 0, 0]], [[0, 2, 0], [0, -2, 0]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [1, 0] and np.all(tau2 == dtype(0.25)) and np.all(d2 == 4)
    assert same_system(ref.system(pos, vel), (dtype(0.25), 0, 1, dtype(4)))
    # two bodies at rest relative to each other: v2 = 0 with d2 > 0 gives q = +inf, which is never chosen; d2min is still there
    pos, vel = system([[0, 0, 0], [2, 0, 0]], [[1, 1, 1], [1, 1, 1]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [-1, -1] and np.all(tau2 == inf) and np.all(d2 == 4)
    assert same_system(ref.system(pos, vel), (inf, -1, -1, dtype(4)))
    # coincident and at relative rest: 0 / 0 is NaN, never chosen; d2min = +0
    pos, vel = system([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 0]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [-1, -1] and np.all(tau2 == inf) and np.all(bits(d2) == 0)
    # coincident and moving: q = +0, a legitimate answer
    pos, vel = system([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 3]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [1, 0] and np.all(bits(tau2) == 0)
    # three bodies, every pair at q = 1 (4 / 4, 4 / 4 and 8 / 8): the lowest j wins in every row
    pos, vel = system([[0, 0, 0], [2, 0, 0], [0, 2, 0]], [[0, 0, 0], [0, 2, 0], [2, 0, 0]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [1, 0, 0] and list(tau2) == [1, 1, 1] and list(d2) == [4, 4, 4]
    assert same_system(ref.system(pos, vel), (dtype(1), 0, 1, dtype(4)))   # all rows tie: the lowest row
    # a velocity whose square overflows: q = +0
    big = 1e30 if dtype is np.float32 else 1e200
    pos, vel = system([[0, 0, 0], [2, 0, 0], [0, 3, 0]], [[0, 0, 0], [big, 0, 0], [0, 1, 0]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [1, 0, 1] and np.all(bits(tau2) == 0) and list(d2) == [4, 4, 9]
    # a NaN velocity poisons only its own pairs
    pos, vel = system([[0, 0, 0], [2, 0, 0], [0, 3, 0]], [[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]])
    tau2, idx, d2 = ref.rows(pos, vel)
    assert list(idx) == [2, -1, 0] and tau2[1] == inf and list(tau2[[0, 2]]) == [9, 9] and list(d2) == [4, 4, 9]


def test_adaptive_driver_beats_a_fixed_step_on_an_eccentric_orbit():
    """The driver loop restated in numpy binary64 (timescale_common.adaptive_run) on two unit masses, a = 1, e = 0.9, from apocentre
    over one period (4.4429), eta = 0.02, dt in [1e-9, 1]: the adaptive run's worst |dE / E| is smaller than that of a fixed-step run
    of the same integrator with the same number of steps.  Measured on the CPU: 529 steps, worst |dE / E| 0.377 adaptive against 1.387
    fixed (at eta = 0.01: 1024 steps, 0.186 against 0.698).  Neither is small — a first-order kick-drift step through a pericentre at
    r = 0.1 — but the ordering is the claim, and only the ordering is asserted."""
    eta, dt_min, dt_max = 0.02, 1e-9, 1.0
    pos, vel, period = two_body_orbit(0.9)
    e0 = total_energy(pos, vel)
    worst = {"adaptive": 0.0, "fixed": 0.0}

    def watch(name):
        def observe(p, v):
            worst[name] = max(worst[name], abs((total_energy(p, v) - e0) / e0))
        return observe

    t, steps = adaptive_run(pos, vel, period, eta, dt_min, dt_max, observe=watch("adaptive"))
    assert t >= period and 100 < steps < 5000
    pos, vel, period = two_body_orbit(0.9)
    for _ in range(steps):
        kick_drift(pos, vel, period / steps)
        watch("fixed")(pos, vel)
    print("e = 0.9, eta = %g: %d steps, worst |dE/E| adaptive %.4g, fixed %.4g" % (eta, steps, worst["adaptive"], worst["fixed"]))
    assert worst["adaptive"] < worst["fixed"]
    # the cut-off: max_steps ends the loop early with t < t_end
    pos, vel, period = two_body_orbit(0.9)
    t, k = adaptive_run(pos, vel, period, eta, dt_min, dt_max, max_steps=7)
    assert k == 7 and 0 < t < period and math.isfinite(t)
