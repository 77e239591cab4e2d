"""What the snap tests (test_snap_abi.py, test_gpu_snap.py) share: tests/snap_ref.c compiled as the field tests compile theirs
(field_common.compile_ref), a plain numpy fp64 evaluation of the definition with the scale an error is measured against, and the check
that the snap is the time derivative of the jerk along the motion.  The points and skip indices are field_common's."""
import ctypes as C

import numpy as np

from field_common import EPS
from jerk_common import TIMED_SHAPE  # noqa: F401  (the timed binary32 test's shape is the jerk's)

# What snap_ref.c's strict binary32 keeps against numpy binary64 at TIMED_SHAPE in the magnitude-sum measure (numpy_snap's mag_s; the
# acceleration and the jerk in jerk_common.numpy_jerk's); test_snap_abi.py asserts it.  Measured on the CPU at (65536, 512), worst of the
# FMA3 and the reference's d2 form, with and without skip: snap 2.49e-6 (FMA3) and 2.68e-6 (reference's), jerk 1.59e-6 and 1.47e-6,
# acceleration 4.5e-7 and 4.2e-7.
R_REF = 3e-6
# the GPU test of the timed arithmetic: the reference's own error doubled plus v_rsq_f32's 1 ulp through inv^7 (inv3 three-fold,
# alpha, beta and b two-fold each at most: DESIGN.md §3.20)
TIMED_BOUND = 2 * R_REF + 7 * 2.0 ** -23
# The same figure on the hostile system: specials_common.hostile_dynamic_system ("base", "overflow") at n = 70, 1100 and 2085 with
# hostile_points(…, 300, variant) and hostile_point_words, on the near queries; tests/test_specials_dynamic_reference.py measures and asserts it.
# Measured on the CPU, worst of both d2 forms, with and without skip: snap 4.931e-6 (n = 2085), jerk 3.356e-6 and acceleration 1.228e-6
# (n = 1100); the constant is the worst rounded up by 1.4 %.
R_REF_HOSTILE = 5.0e-6
TIMED_BOUND_HOSTILE = 2 * R_REF_HOSTILE + 7 * 2.0 ** -23


class SnapRef:
    """tests/snap_ref.c: (accel, jerk, snap), each (m, 4), in the documented order, IEEE 1/sqrt"""

    def __init__(self, lib):
        self.lib = lib

    def _run(self, suf, dtype, pos, vel, acc, points, pvel, pacc, skip, ref, mass):
        pos, vel, acc, points, pvel, pacc = (np.ascontiguousarray(a, dtype) for a in (pos, vel, acc, points, pvel, pacc))
        m = len(points)
        assert len(pvel) == m and len(pacc) == m and len(vel) == len(pos) and len(acc) == len(pos)
        out = [np.empty((m, 4), dtype) for _ in range(3)]
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            assert sk.shape == (m,)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        fn = getattr(self.lib, "snap_" + suf)
        fn.restype = None
        fn(p(pos), p(vel), p(acc), len(pos), p(points), p(pvel), p(pacc), m, p(sk) if sk is not None else None, int(ref), int(mass), *(p(o) for o in out))
        return tuple(out)

    def f32(self, pos, vel, acc, points, pvel, pacc, skip=None, ref=False, mass=False):
        return self._run("f32", np.float32, pos, vel, acc, points, pvel, pacc, skip, ref, mass)

    def f64(self, pos, vel, acc, points, pvel, pacc, skip=None, mass=False):
        return self._run("f64", np.float64, pos, vel, acc, points, pvel, pacc, skip, False, mass)

    def rows(self, pos, vel, dtype, ref=False, mass=False):
        """the rows form over all n rows: (accel, jerk, snap) with the sources' accelerations from the statement's own first pass"""
        pos, vel = np.ascontiguousarray(pos, dtype), np.ascontiguousarray(vel, dtype)
        out = [np.empty((len(pos), 4), dtype) for _ in range(3)]
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        fn = getattr(self.lib, "snap_rows_" + ("f64" if np.dtype(dtype) == np.float64 else "f32"))
        fn.restype = None
        fn(p(pos), p(vel), len(pos), int(ref), int(mass), *(p(o) for o in out))
        return tuple(out)

    def of(self, dtype):
        return self.f64 if np.dtype(dtype) == np.float64 else self.f32


def numpy_snap(pos, vel, acc, points, pvel, pacc, skip=None, mass=False):
    """(accel, jerk, snap, mag_a, mag_j, mag_s), (m, 3) fp64 each: the definition in plain numpy over all j (skip left out, whatever it
    holds), no stated order, and the magnitude sums — the scale an error of a sum that cancels is measured against: jerk_common's for the
    acceleration and the jerk, for the snap the sum over j of the absolute values of its terms,
    inv^3 (|g_a| + 6 |alpha| (|w_a| + 3 |alpha| |d_a|) + 3 (|w|^2 inv^2 + (|dx gx| + |dy gy| + |dz gz|) inv^2 + alpha^2) |d_a|)"""
    p, v, g = (a[:, :3].astype(np.float64) for a in (pos, vel, acc))
    x, u, gx = (a[:, :3].astype(np.float64) for a in (points, pvel, pacc))
    wgt = pos[:, 3].astype(np.float64) if mass else np.ones(len(pos))
    m = len(x)
    out = [np.zeros((m, 3)) for _ in range(6)]
    with np.errstate(all="ignore"):
        for k in range(m):
            d, w, h, mj = p - x[k], v - u[k], g - gx[k], wgt
            if skip is not None and skip[k] >= 0:
                d, w, h, mj = (np.delete(a, skip[k], 0) for a in (d, w, h, mj))
            inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
            inv2, inv3 = (inv * inv)[:, None], (mj * inv ** 3)[:, None]
            alpha = (d * w).sum(1)[:, None] * inv2
            beta = ((w * w).sum(1) + (d * h).sum(1))[:, None] * inv2 + alpha * alpha
            ta = d * inv3
            tj = (w - 3.0 * alpha * d) * inv3
            ts = h * inv3 - 6.0 * alpha * tj - 3.0 * beta * ta
            abs_alpha = np.abs(d * w).sum(1)[:, None] * inv2
            abs_beta = ((w * w).sum(1) + np.abs(d * h).sum(1))[:, None] * inv2 + abs_alpha * abs_alpha
            abs_j = np.abs(w) + 3.0 * abs_alpha * np.abs(d)
            out[0][k], out[1][k], out[2][k] = ta.sum(0), tj.sum(0), ts.sum(0)
            out[3][k] = np.abs(ta).sum(0)
            out[4][k] = (abs_j * inv3).sum(0)
            out[5][k] = ((np.abs(h) + 6.0 * abs_alpha * abs_j + 3.0 * abs_beta * np.abs(d)) * inv3).sum(0)
    return tuple(out)


def worst(got, want, mag):
    """the worst |got - want| / mag over queries and the three components"""
    return float(np.max(np.abs(got[:, :3].astype(np.float64) - want) / mag))


def advance(pos, vel, acc, s):
    """the words after time s along the motion the snap differentiates: x + s v + s^2 a / 2 and v + s a, accelerations as they are"""
    p, v = np.array(pos, np.float64), np.array(vel, np.float64)
    p[:, :3] = pos[:, :3] + s * vel[:, :3] + (0.5 * s * s) * acc[:, :3]
    v[:, :3] = vel[:, :3] + s * acc[:, :3]
    return p, v


def derivative_error(snap_of, pos, vel, acc, x, u, g, h):
    """Per query, in the Euclidean norm: |central difference of the jerk in time with step h - snap|, and the truncation error of that
    difference, h^2 |d^3 j / dt^3| / 6 with d^3 j / dt^3 = d^2 s / dt^2 estimated from the snap itself at +-h:
    (s(+h) - 2 s(0) + s(-h)) / h^2.  Time moves every body and every query by advance(): positions with velocity and acceleration,
    velocities with acceleration — the motion of which, at s = 0, the snap is the second derivative of the acceleration; the accelerations
    brought stay as they are (their own change enters the jerk's difference at O(h^2) only through the positions' h^3 term, inside the
    bound's factor).  snap_of(bodies, vel, acc, points, pvel, pacc) -> (accel, jerk, snap), (k, 4) each; all fp64 words.
    Returns (err, trunc, scale), (k,) each; scale = |s| of the query, for printing."""
    jerk, snap = {}, {}
    for s in (-h, 0.0, h):
        (bp, bv), (qp, qv) = advance(pos, vel, acc, s), advance(x, u, g, s)
        _, j, sn = snap_of(bp, bv, acc, qp, qv, g)
        jerk[s], snap[s] = j[:, :3], sn[:, :3]
    norm = lambda a: np.sqrt((a ** 2).sum(1))
    err = norm((jerk[h] - jerk[-h]) / (2 * h) - snap[0.0])
    trunc = norm(snap[h] - 2 * snap[0.0] + snap[-h]) / 6     # h^2 |d2s / dt2| / 6
    return err, trunc, norm(snap[0.0])
