"""The snap entry points (nbody_snap(_d), nbody_snap_rows(_d); include/nbody.h "snap") as far as no GPU is needed: the symbols and their
binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement tests/snap_ref.c itself — against a plain numpy fp64 evaluation of
the definition in the measure the GPU tests use, its acceleration and jerk against tests/jerk_ref.c bit for bit, the rows form against
the points form, and the snap as the time derivative of the jerk along the motion."""
import ctypes as C
import re

import numpy as np
import pytest

from field_common import ROOT, compile_ref, make_points, make_skip
from jerk_common import JerkRef, derivative_queries
from snap_common import R_REF, TIMED_BOUND, TIMED_SHAPE, SnapRef, derivative_error, numpy_snap, worst
from tidal_common import GRADIENT_H

REF_F64 = 1e-13
NAMES = (("nbody_snap", 8), ("nbody_snap_d", 8), ("nbody_snap_rows", 5), ("nbody_snap_rows_d", 5))


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SnapRef(compile_ref(tmp_path_factory.mktemp("snap_ref"), "snap_ref"))


@pytest.fixture(scope="module")
def jerk_ref(tmp_path_factory):
    return JerkRef(compile_ref(tmp_path_factory.mktemp("jerk_ref"), "jerk_ref"))


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def point_words(nb, m, dtype=np.float32):
    """the points' velocities (test_gpu_jerk.py's) and accelerations"""
    return nb.make_bodies(m, seed=78, dtype=dtype)[1], nb.make_bodies(m, seed=79, dtype=dtype)[1]


def test_symbols_are_declared_exported_and_bound(nb):
    header = open(ROOT + "/include/nbody.h").read()
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in NAMES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs
    assert callable(nb.NBody.snap) and callable(nb.NBody.snap_at)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    for pts_fn, rows_fn, dt, ct in ((lib.nbody_snap, lib.nbody_snap_rows, np.float32, C.c_float),
                                    (lib.nbody_snap_d, lib.nbody_snap_rows_d, np.float64, C.c_double)):
        x = np.zeros((4, 4), dt)
        a, j, s = (np.full((4, 4), 7, dt) for _ in range(3))
        p = lambda v: v.ctypes.data_as(C.POINTER(ct))
        assert pts_fn(p(x), p(x), p(x), 4, None, p(a), p(j), p(s)) == nb._lib.ERR_NOT_INIT
        assert rows_fn(0, 4, p(a), p(j), p(s)) == nb._lib.ERR_NOT_INIT
        assert np.all(a == 7) and np.all(j == 7) and np.all(s == 7)


def test_snap_ref_against_numpy(nb, ref):
    """n = 2100, m = 300: three blocks, the last one short.  n = 65536, m = 512 (jerk_common.TIMED_SHAPE): the shape of the GPU test of
    the timed arithmetic, whose bound (snap_common.TIMED_BOUND = 2 r + 7 * 2^-23) rests on the binary32 figure r asserted here,
    r <= snap_common.R_REF = 3e-6.  The sources' accelerations are the statement's own (the rows form's first pass).
    Measured at (65536, 512), binary32: acceleration 4.5e-7, jerk 1.59e-6, snap r = 2.49e-6 (FMA3 form; 2.68e-6 in the reference's)."""
    assert TIMED_SHAPE == (65536, 512) and R_REF == 3e-6 and TIMED_BOUND == 2 * R_REF + 7 * 2.0 ** -23
    for n, m in ((2100, 300), TIMED_SHAPE):
        pos, vel = nb.make_bodies(n)
        acc = ref.rows(pos, vel, np.float32)[0]
        pts, on = make_points(nb, pos, m)
        pvel, pacc = point_words(nb, m)
        for skip in (None, make_skip(n, m, on)):
            want = numpy_snap(pos, vel, acc, pts, pvel, pacc, skip)
            for r in (False, True):
                got = ref.f32(pos, vel, acc, pts, pvel, pacc, skip, ref=r)
                e = [worst(got[i], want[i], want[3 + i]) for i in range(3)]
                print("n=%d fp32 ref=%d skip=%s: accel %.3e jerk %.3e snap %.3e" % (n, r, skip is not None, *e))
                assert max(e) <= R_REF, (n, r)
            if n == 2100:
                got = ref.f64(pos, vel, acc, pts, pvel, pacc, skip)
                e = [worst(got[i], want[i], want[3 + i]) for i in range(3)]
                print("n=%d fp64 skip=%s: accel %.3e jerk %.3e snap %.3e" % (n, skip is not None, *e))
                assert max(e) <= REF_F64


def test_masses_of_the_statement_against_numpy(nb, ref):
    n, m = 2100, 300
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    pos[:, 3] = np.random.default_rng(3).uniform(0.25, 4.0, n)
    acc = ref.rows(pos, vel, np.float64, mass=True)[0]
    pts, on = make_points(nb, pos, m)
    pvel, pacc = point_words(nb, m, np.float64)
    skip = make_skip(n, m, on)
    want = numpy_snap(pos, vel, acc, pts, pvel, pacc, skip, mass=True)
    got = ref.f64(pos, vel, acc, pts, pvel, pacc, skip, mass=True)
    assert max(worst(got[i], want[i], want[3 + i]) for i in range(3)) <= REF_F64
    assert not np.array_equal(bits(got[2]), bits(ref.f64(pos, vel, acc, pts, pvel, pacc, skip)[2]))
    pos[:, 3] = 1.0   # unit masses weigh nothing: the unweighted bits
    unit = ref.f64(pos, vel, acc, pts, pvel, pacc, skip, mass=True)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(unit, ref.f64(pos, vel, acc, pts, pvel, pacc, skip)))


def test_acceleration_and_jerk_are_jerk_refs_bit_for_bit(nb, ref, jerk_ref):
    """whatever accelerations are brought"""
    n, m = 2100, 300
    pos, vel = nb.make_bodies(n)
    acc = ref.rows(pos, vel, np.float32)[0]
    pts, on = make_points(nb, pos, m)
    pvel, pacc = point_words(nb, m)
    for skip in (None, make_skip(n, m, on)):
        for r in (False, True):
            want = jerk_ref.f32(pos, vel, pts, pvel, skip, ref=r)
            for g_src, g_pt in ((acc, pacc), (np.zeros_like(acc), np.zeros_like(pacc))):
                got = ref.f32(pos, vel, g_src, pts, pvel, g_pt, skip, ref=r)
                assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1])), r
        p64, v64, x64, u64 = (a.astype(np.float64) for a in (pos, vel, pts, pvel))
        want = jerk_ref.f64(p64, v64, x64, u64, skip)
        got = ref.f64(p64, v64, acc, x64, u64, pacc, skip)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))


def test_rows_form_of_the_statement(nb, ref, jerk_ref):
    """row i is the query (r_i, v_i, a_i) with skip = i and a = the jerk pass's acceleration of every row; all fourth values are 0"""
    n = 1500
    self = np.arange(n, dtype=np.int32)
    for dtype in (np.float32, np.float64):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        rows = ref.rows(pos, vel, dtype)
        acc = (jerk_ref.f64 if dtype == np.float64 else jerk_ref.f32)(pos, vel, pos, vel, self)[0]
        assert np.array_equal(bits(rows[0]), bits(acc))
        pts = ref.of(dtype)(pos, vel, acc, pos, vel, acc, self)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(rows, pts))
        assert all(np.all(o[:, 3] == 0) for o in rows) and np.any(rows[2][:, :3] != 0)


def test_two_bodies_have_opposite_snaps(nb, ref):
    """s_0 = -s_1 bit for bit: d, w and g change sign together, which leaves rv, alpha, q and beta as they are and negates t and u"""
    pos, vel = nb.make_bodies(2)
    for dtype in (np.float32, np.float64):
        a, j, s = ref.rows(pos, vel, dtype)
        assert np.array_equal(bits(s[0, :3]), bits(-s[1, :3])) and np.all(s[:, :3] != 0)


def test_a_query_on_a_body_without_skip(nb, ref):
    """with the body's own velocity and acceleration the coincident body adds +0 to all three outputs — what skipping it gives, bit for
    bit; with another acceleration it adds g eps^(-3/2) to the snap alone"""
    from field_common import EPS
    n = 2100
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    acc = ref.rows(pos, vel, np.float64)[0]
    pts, on = make_points(nb, pos, 3)
    sk = np.array(on, np.int32)
    own = ref.f64(pos, vel, acc, pts, vel[on], acc[on])
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(own, ref.f64(pos, vel, acc, pts, vel[on], acc[on], sk)))
    other = acc[on].copy()
    other[:, :3] += 0.5
    got, got_sk = ref.f64(pos, vel, acc, pts, vel[on], other), ref.f64(pos, vel, acc, pts, vel[on], other, sk)
    assert np.array_equal(bits(got[0]), bits(got_sk[0])) and np.array_equal(bits(got[1]), bits(got_sk[1]))
    gap = got[2][:, :3] - got_sk[2][:, :3]
    assert np.all(np.abs(gap - (-0.5) * EPS ** -1.5) <= 1e-6 * 0.5 * EPS ** -1.5), gap


def test_snap_ref_is_the_time_derivative_of_its_jerk(nb, ref):
    """the central difference of the statement's jerk along x + h v + h^2 a / 2, v + h a (bodies and queries) against its snap: the
    bound is the difference's own truncation error, estimated from the snap itself at +-h, times 4, per query in the Euclidean norm,
    as jerk_common.derivative_error bounds the jerk.  Measured: worst error / bound 0.25 (error = 1.000 x the truncation estimate)."""
    n, h = 4099, GRADIENT_H
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    acc = ref.rows(pos, vel, np.float64)[0]
    x, u = derivative_queries(nb, pos)
    g = nb.make_bodies(len(x), seed=13, dtype=np.float64)[1]
    err, trunc, scale = derivative_error(ref.f64, pos, vel, acc, x, u, g, h)
    print("snap_f64: worst error / |s| %.3e, worst error / bound %.3f" % ((err / scale).max(), (err / (4 * trunc)).max()))
    assert np.all(err <= 4 * trunc) and np.all(scale > 0)
