"""What the jerk tests (test_jerk_abi.py, test_gpu_jerk.py) share: tests/jerk_ref.c compiled as the field tests compile theirs
(field_common.compile_ref), a plain numpy fp64 evaluation of the definition with the scale an error is measured against, and the
check that the jerk is the time derivative of the field.  The points and skip indices are field_common's."""
import ctypes as C

import numpy as np

from field_common import EPS

TIMED_SHAPE = (65536, 512)   # (n, m) of the timed binary32 test: test_jerk_abi.py asserts the reference's own error there


class JerkRef:
    """tests/jerk_ref.c: (accel, jerk), each (m, 4), in the documented order, IEEE 1/sqrt"""

    def __init__(self, lib):
        self.lib = lib

    def _run(self, fn, dtype, pos, vel, points, pvel, skip, *flags):
        pos, vel, points, pvel = (np.ascontiguousarray(a, dtype) for a in (pos, vel, points, pvel))
        m = len(points)
        assert len(pvel) == m and len(vel) == len(pos)
        acc, jerk = np.empty((m, 4), dtype), np.empty((m, 4), dtype)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            assert sk.shape == (m,)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        fn(p(pos), p(vel), len(pos), p(points), p(pvel), m, p(sk) if sk is not None else None, *flags, p(acc), p(jerk))
        return acc, jerk

    def f32(self, pos, vel, points, pvel, skip=None, ref=False):
        return self._run(self.lib.jerk_f32, np.float32, pos, vel, points, pvel, skip, int(ref))

    def f64(self, pos, vel, points, pvel, skip=None):
        return self._run(self.lib.jerk_f64, np.float64, pos, vel, points, pvel, skip)


def numpy_jerk(pos, vel, points, pvel, skip=None):
    """(accel, jerk, mag_a, mag_j), (m, 3) fp64 each: the definition in plain numpy over all j (skip left out, whatever it holds), no
    stated order, and the magnitude sums — the scale an error of a sum that cancels is measured against: the field's for the
    acceleration, mag_a = sum_j inv^3 (|w_a| + 3 (|dx wx| + |dy wy| + |dz wz|) inv^2 |d_a|) for the jerk"""
    p, v = pos[:, :3].astype(np.float64), vel[:, :3].astype(np.float64)
    x, u = points[:, :3].astype(np.float64), pvel[:, :3].astype(np.float64)
    m = len(x)
    acc, jerk, mag_a, mag_j = (np.zeros((m, 3)) for _ in range(4))
    with np.errstate(all="ignore"):
        for k in range(m):
            d, w = p - x[k], v - u[k]
            if skip is not None and skip[k] >= 0:
                d, w = np.delete(d, skip[k], 0), np.delete(w, skip[k], 0)
            inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
            inv2, inv3 = (inv * inv)[:, None], (inv ** 3)[:, None]
            ta = d * inv3
            tj = (w - 3.0 * (d * w).sum(1)[:, None] * inv2 * d) * inv3
            acc[k], jerk[k] = ta.sum(0), tj.sum(0)
            mag_a[k] = np.abs(ta).sum(0)
            mag_j[k] = ((np.abs(w) + 3.0 * np.abs(d * w).sum(1)[:, None] * inv2 * np.abs(d)) * inv3).sum(0)
    return acc, jerk, mag_a, mag_j


def worst(got, want, mag):
    """the worst |got - want| / mag over queries and the three components"""
    return float(np.max(np.abs(got[:, :3].astype(np.float64) - want) / mag))


def derivative_error(field_of, jerk_of, pos, vel, x, u, h):
    """Per query, in the Euclidean norm: |central difference of the acceleration in time with step h - jerk|, and the truncation error
    of that difference, h^2 |d^3 a / dt^3| / 6 with d^3 a / dt^3 = d^2 j / dt^2 estimated from the jerk itself at +-h:
    (j(+h) - 2 j(0) + j(-h)) / h^2.  Time moves every body and every query along its velocity: the state at +-h has the bodies at
    pos +- h vel and the queries at x +- h u, the velocities as they are — the motion of which the jerk is the derivative.
    field_of(bodies, points) -> (k, 4) accelerations; jerk_of(bodies, vel, points, pvel) -> (accel, jerk), (k, 4) each; all fp64 words.
    Returns (err, trunc, scale), (k,) each; scale = |j| of the query, for printing."""
    drift = lambda a, b, s: np.concatenate([a[:, :3] + s * b[:, :3], a[:, 3:]], axis=1)
    acc, jerk = {}, {}
    for s in (-h, 0.0, h):
        bodies, pts = drift(pos, vel, s), drift(x, u, s)
        jerk[s] = jerk_of(bodies, vel, pts, u)[1][:, :3]
        if s != 0.0:
            acc[s] = field_of(bodies, pts)[:, :3]
    norm = lambda a: np.sqrt((a ** 2).sum(1))
    err = norm((acc[h] - acc[-h]) / (2 * h) - jerk[0.0])
    trunc = norm(jerk[h] - 2 * jerk[0.0] + jerk[-h]) / 6     # h^2 |d2j / dt2| / 6
    return err, trunc, norm(jerk[0.0])


def derivative_queries(nb, pos):
    """tidal_common.gradient_points' 50 points (at least 0.05 from any body) as words, with velocities from make_bodies(50, seed=12)"""
    from tidal_common import gradient_points
    x3 = gradient_points(nb, pos)
    x = np.concatenate([x3, np.zeros((len(x3), 1))], axis=1)
    return x, nb.make_bodies(len(x), seed=12, dtype=np.float64)[1]
