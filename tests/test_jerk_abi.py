"""The jerk entry points (nbody_jerk(_d), nbody_jerk_rows(_d); include/nbody.h "jerk") as far as no GPU is needed: the symbols and
their binding, NBODY_ERR_NOT_INIT without a context, aarseth_dt, and the CPU statement tests/jerk_ref.c itself — against a plain numpy
fp64 evaluation of the definition in the measure the GPU tests use, its acceleration against tests/field_ref.c bit for bit, zero
velocities, the antisymmetry of two bodies, the on-body query, and the jerk as the time derivative of tests/field_ref.c's acceleration."""
import ctypes as C

import numpy as np
import pytest

from field_common import EPS, FieldRef, compile_ref, make_points, make_skip
from jerk_common import TIMED_SHAPE, JerkRef, derivative_error, derivative_queries, numpy_jerk, worst
from tidal_common import GRADIENT_H

REF_F32 = 4.7e-6   # what jerk_ref.c's binary32 must keep against binary64 in the mag measure: the GPU test's bound rests on it
REF_F64 = 1e-13


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return JerkRef(compile_ref(tmp_path_factory.mktemp("jerk_ref"), "jerk_ref"))


@pytest.fixture(scope="module")
def field_ref(tmp_path_factory):
    return FieldRef(compile_ref(tmp_path_factory.mktemp("field_ref"), "field_ref"))


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in (("nbody_jerk", 6), ("nbody_jerk_d", 6), ("nbody_jerk_rows", 4), ("nbody_jerk_rows_d", 4)):
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs
    assert callable(nb.NBody.jerk) and callable(nb.NBody.jerk_at) and callable(nb.aarseth_dt)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    for pts_fn, rows_fn, dt, ct in ((lib.nbody_jerk, lib.nbody_jerk_rows, np.float32, C.c_float),
                                    (lib.nbody_jerk_d, lib.nbody_jerk_rows_d, np.float64, C.c_double)):
        pts, vel = np.zeros((4, 4), dt), np.zeros((4, 4), dt)
        a, j = np.full((4, 4), 7, dt), np.full((4, 4), 7, dt)
        p = lambda x: x.ctypes.data_as(C.POINTER(ct))
        assert pts_fn(p(pts), p(vel), 4, None, p(a), p(j)) == nb._lib.ERR_NOT_INIT
        assert rows_fn(0, 4, p(a), p(j)) == nb._lib.ERR_NOT_INIT
        assert np.all(a == 7) and np.all(j == 7)


def test_aarseth_dt(nb):
    a = np.array([[3, 4, 0, 9], [0, 0, 0, 0], [1, 2, 2, 0], [0, 0, 0, 5]], np.float32)
    j = np.array([[0, 0, 2, 9], [1, 0, 0, 0], [0, 0, 0, 7], [0, 0, 0, 5]], np.float32)
    dt = nb.aarseth_dt(a, j, 0.5)
    assert dt.dtype == np.float64 and dt.shape == (4,)
    assert dt[0] == 0.5 * 5.0 / 2.0 and dt[1] == 0.0 and dt[2] == np.inf and dt[3] == np.inf   # the fourth component never counts
    assert np.array_equal(nb.aarseth_dt(a[:, :3], j[:, :3], 0.5), dt)
    with pytest.raises(ValueError):
        nb.aarseth_dt(a, j[:3], 0.5)


def test_jerk_ref_against_numpy(nb, ref):
    """n = 2100, m = 300: three blocks, the last one short.  n = 65536, m = 512 (jerk_common.TIMED_SHAPE): the shape of the GPU test
    of the timed arithmetic, whose bound (TOL = 1e-5) is derived from the binary32 figure r asserted here, r <= 4.7e-6.
    Measured at (65536, 512), binary32: acceleration 4.5e-7, jerk r = 1.59e-6 (FMA3 form; 1.47e-6 in the reference's)."""
    assert TIMED_SHAPE == (65536, 512)
    for n, m in ((2100, 300), TIMED_SHAPE):
        pos, vel = nb.make_bodies(n)
        pts, on = make_points(nb, pos, m)
        pvel = nb.make_bodies(m, seed=78)[1]
        for skip in (None, make_skip(n, m, on)):
            wa, wj, mag_a, mag_j = numpy_jerk(pos, vel, pts, pvel, skip)
            for r in (False, True):
                a, j = ref.f32(pos, vel, pts, pvel, skip, ref=r)
                ea, ej = worst(a, wa, mag_a), worst(j, wj, mag_j)
                print("n=%d fp32 ref=%d skip=%s: accel %.3e jerk %.3e" % (n, r, skip is not None, ea, ej))
                assert max(ea, ej) <= REF_F32, (n, r)
            if n == 2100:
                a, j = ref.f64(pos, vel, pts, pvel, skip)
                ea, ej = worst(a, wa, mag_a), worst(j, wj, mag_j)
                print("n=%d fp64 skip=%s: accel %.3e jerk %.3e" % (n, skip is not None, ea, ej))
                assert max(ea, ej) <= REF_F64


def test_acceleration_is_field_refs_bit_for_bit(nb, ref, field_ref):
    n, m = 2100, 300
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    pvel = nb.make_bodies(m, seed=78)[1]
    for skip in (None, make_skip(n, m, on)):
        for r in (False, True):
            assert np.array_equal(bits(ref.f32(pos, vel, pts, pvel, skip, ref=r)[0]), bits(field_ref.f32(pos, pts, skip, ref=r)[0])), r
        p64, x64 = pos.astype(np.float64), pts.astype(np.float64)
        assert np.array_equal(bits(ref.f64(p64, vel, x64, pvel, skip)[0]), bits(field_ref.f64(p64, x64, skip)[0]))


def test_zero_velocities_give_a_jerk_of_plus_zero(nb, ref):
    n, m = 2100, 300
    pos = nb.make_bodies(n)[0]
    pts, on = make_points(nb, pos, m)
    zv, zu = np.zeros((n, 4), np.float32), np.zeros((m, 4), np.float32)
    for r in (False, True):
        assert not bits(ref.f32(pos, zv, pts, zu, None, ref=r)[1]).any()
    assert not bits(ref.f64(pos, zv, pts, zu, make_skip(n, m, on))[1]).any()


def test_two_bodies_have_opposite_jerks(nb, ref):
    """j_0 = -j_1 bit for bit: d -> -d and w -> -w leave rv and b as they are and negate t, and the sums have one term"""
    pos, vel = nb.make_bodies(2)
    sk = np.array([0, 1], np.int32)
    for r in (False, True):
        a, j = ref.f32(pos, vel, pos, vel, sk, ref=r)
        assert np.array_equal(bits(j[0, :3]), bits(-j[1, :3])) and np.all(j[:, :3] != 0)
        assert np.array_equal(bits(a[0, :3]), bits(-a[1, :3]))
    a, j = ref.f64(pos, vel, pos, vel, sk)
    assert np.array_equal(bits(j[0, :3]), bits(-j[1, :3])) and np.all(j[:, :3] != 0)


def test_a_query_on_a_body_without_skip(nb, ref):
    """with the body's own velocity the coincident body adds +0 to both outputs — what skipping it gives, bit for bit; with another
    velocity it adds w eps^(-3/2) to the jerk"""
    n = 2100
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, 3)
    own = vel[on]
    other = own.copy()
    other[:, :3] += np.float32(0.5)
    for f, cast in ((ref.f32, np.float32), (ref.f64, np.float64)):
        p, v, x = pos.astype(cast), vel.astype(cast), pts.astype(cast)
        a, j = f(p, v, x, own)
        a_sk, j_sk = f(p, v, x, own, np.array(on, np.int32))
        assert np.array_equal(bits(a), bits(a_sk)) and np.array_equal(bits(j), bits(j_sk))
        a2, j2 = f(p, v, x, other)
        a2_sk, j2_sk = f(p, v, x, other, np.array(on, np.int32))
        assert np.array_equal(bits(a2), bits(a2_sk))
        gap = j2[:, :3].astype(np.float64) - j2_sk[:, :3].astype(np.float64)
        assert np.all(np.abs(gap - (-0.5) * EPS ** -1.5) <= 1e-6 * 0.5 * EPS ** -1.5), gap


def test_jerk_ref_is_the_time_derivative_of_field_ref(nb, ref, field_ref):
    """the references alone, as tests/test_gpu_jerk.py asks of the device: the bound is the central difference's truncation error,
    estimated from the jerk itself at +-h, times 4, per query in the Euclidean norm"""
    n, h = 4099, GRADIENT_H
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    x, u = derivative_queries(nb, pos)
    err, trunc, scale = derivative_error(lambda b, p: field_ref.f64(b, p)[0], ref.f64, pos, vel, x, u, h)
    print("jerk_f64 / field_f64: worst error / |j| %.3e, worst error / bound %.3f" % ((err / scale).max(), (err / (4 * trunc)).max()))
    assert np.all(err <= 4 * trunc)
