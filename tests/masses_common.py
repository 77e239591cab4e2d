"""What the mass tests (test_masses_abi.py, test_gpu_masses.py) share: tests/masses_ref.c compiled as the field tests compile theirs
(field_common.compile_ref), the masses the tests put into the w of the position words, plain numpy binary64 evaluations of the weighted
definitions with the scales an error is measured against (field_common's, tidal_common's and jerk_common's with m_j in every term), the
Kepler pair of two unequal masses, and the energy and momentum of a weighted state."""
import ctypes as C

import numpy as np

from field_common import EPS, compile_ref
from tidal_common import DIAG

SIZES = (1, 2, 63, 257, 1025, 2100)   # one body, tails below a wave and a workgroup, one, two and three source blocks
RSQ_SHARE = 6e-7   # v_rsq_f32's share of a timed binary32 pair in the mag measure: 1 ulp in inv, three-fold in inv3, two-fold in b:
                   # <= 5 * 2^-23 (tests/test_gpu_jerk.py).  The weight is an exact factor of every term and of mag.
# What masses_ref.c's binary32 keeps against numpy binary64 in the mag measure with masses in [0.25, 4), at n = 2100 and at
# jerk_common.TIMED_SHAPE; test_masses_abi.py asserts it (measured there: 3.51e-6 at worst, the tidal tensor at TIMED_SHAPE) and the
# timed GPU bound 2 R_REF + RSQ_SHARE rests on it.  It is the budget tests/test_jerk_abi.py gives jerk_ref.c: the weight adds one
# rounding per pair, 2^-24 = 6e-8 of a term.
R_REF = 4.7e-6
# The same figure on specials_common.hostile_dynamic_system with hostile_masses ("base", "overflow") at n = 70, 1100 and 2085, on the near
# queries of hostile_points(…, 300, variant); tests/test_specials_dynamic_reference.py measures and asserts it.
# Measured on the CPU, worst of both d2 forms, with and without skip: 9.531e-3 (the acceleration at n = 70; 2.23e-4 at n = 1100, 2.02e-4
# at n = 2085; the jerk 4.5e-6 at the most) — the far body's figure, not the cloud's: its mass of 2^100 meets an inv^3 that binary32
# holds as one subnormal bit (9.4e-46 rounded to 1.4e-45), a term of 1.2 with an error of 0.6 on every query alike, against a magnitude
# sum of about 62 at n = 70.  No query's binary64 magnitude is non-finite, so the exclusion for that removes 0 of 300.  The constant is
# the worst rounded up by 4.9 %.
R_REF_HOSTILE = 1.0e-2


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def with_masses(pos, masses):
    """the position words with w = masses (a scalar or (n,)), in the words' precision"""
    out = np.array(pos, order="C")
    out[:, 3] = masses
    return out


def random_masses(n, seed=5, dtype=np.float32):
    """n masses in [0.25, 4), log-uniform, rounded to dtype"""
    return (0.25 * 16.0 ** np.random.default_rng(seed).random(n)).astype(dtype)


class MassesRef:
    """tests/masses_ref.c.  dtype float32 or float64 picks the statement; ref: the reference's d2 roundings (binary32 only)"""

    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def _suf(dtype):
        return "f64" if np.dtype(dtype) == np.float64 else "f32"

    def _fn(self, name, dtype):
        fn = getattr(self.lib, "m_%s_%s" % (name, self._suf(dtype)))
        fn.restype = C.c_int
        return fn

    @staticmethod
    def _skip(skip, m):
        if skip is None:
            return None
        sk = np.ascontiguousarray(skip, np.int32)
        assert sk.shape == (m,)
        return sk

    def field(self, pos, points, dtype, skip=None, ref=False):
        pos, points = np.ascontiguousarray(pos, dtype), np.ascontiguousarray(points, dtype)
        m = len(points)
        acc, phi, sk = np.empty((m, 4), dtype), np.empty(m, dtype), self._skip(skip, m)
        self._fn("field", dtype)(_p(pos), len(pos), _p(points), m, _p(sk), int(ref), _p(acc), _p(phi))
        return acc, phi

    def tidal(self, pos, points, dtype, skip=None, ref=False):
        pos, points = np.ascontiguousarray(pos, dtype), np.ascontiguousarray(points, dtype)
        m = len(points)
        t, sk = np.empty((m, 6), dtype), self._skip(skip, m)
        self._fn("tidal", dtype)(_p(pos), len(pos), _p(points), m, _p(sk), int(ref), _p(t))
        return t

    def jerk(self, pos, vel, points, pvel, dtype, skip=None, ref=False):
        pos, vel, points, pvel = (np.ascontiguousarray(a, dtype) for a in (pos, vel, points, pvel))
        m = len(points)
        assert len(pvel) == m and len(vel) == len(pos)
        acc, jerk, sk = np.empty((m, 4), dtype), np.empty((m, 4), dtype), self._skip(skip, m)
        self._fn("jerk", dtype)(_p(pos), _p(vel), len(pos), _p(points), _p(pvel), m, _p(sk), int(ref), _p(acc), _p(jerk))
        return acc, jerk

    def jerk_rows(self, pos, vel, dtype, ref=False):
        return self.jerk(pos, vel, pos, vel, dtype, np.arange(len(pos), dtype=np.int32), ref)

    def potential(self, pos, dtype, ref=False):
        pos = np.ascontiguousarray(pos, dtype)
        phi = np.empty(len(pos), dtype)
        self._fn("potential", dtype)(_p(pos), len(pos), 0, len(pos), int(ref), _p(phi))
        return phi

    def totals(self, pos, vel, dtype, slices=None, ref=False):
        """the eight values {T, U, Px, Py, Pz, Lx, Ly, Lz}; slices: [(first, count), ...] of the ranks (default: one)"""
        pos, vel = np.ascontiguousarray(pos, dtype), np.ascontiguousarray(vel, dtype)
        sl = np.ascontiguousarray(slices if slices is not None else [(0, len(pos))], np.int32)
        out = np.zeros(8, np.float64)
        assert self._fn("energy_totals", dtype)(_p(pos), _p(vel), len(pos), _p(sl), len(sl), int(ref), _p(out)) == 0
        return out

    def hermite(self, pos, vel, dtype, dt, nsteps, ref=False):
        """one call of nsteps steps of dt: new (pos, vel) words"""
        p, v = np.array(pos, dtype, order="C"), np.array(vel, dtype, order="C")
        fn = self._fn("hermite", dtype)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double if np.dtype(dtype) == np.float64 else C.c_float, C.c_int, C.c_int]
        fn.restype = None
        fn(p.ctypes.data, v.ctypes.data, len(p), float(dt), int(nsteps), int(ref))
        return p, v

    def hermite_block(self, pos, vel, dtype, eta, dt_max, levels, nblocks, ref=False):
        """(pos, vel, substeps, row_evals)"""
        p, v = np.array(pos, dtype, order="C"), np.array(vel, dtype, order="C")
        fn = self._fn("hermite_block", dtype)
        ct = C.c_double if np.dtype(dtype) == np.float64 else C.c_float
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, ct, ct, C.c_int, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
        steps, evals = C.c_longlong(), C.c_longlong()
        rc = fn(p.ctypes.data, v.ctypes.data, len(p), int(ref), float(dtype(eta)), float(dtype(dt_max)), levels, nblocks, C.byref(steps), C.byref(evals))
        assert rc == 0, "masses_ref hermite_block: %d" % rc
        return p, v, steps.value, evals.value


def compile_masses_ref(tmp_dir):
    return MassesRef(compile_ref(tmp_dir, "masses_ref"))


def numpy_field(pos, points, skip=None):
    """(acc (m, 3), phi (m,), mag (m, 3)): field_common.numpy_field with m_j = pos[:, 3] in every term"""
    p, mj, x = pos[:, :3].astype(np.float64), pos[:, 3].astype(np.float64), points[:, :3].astype(np.float64)
    acc, phi, mag = np.zeros((len(x), 3)), np.zeros(len(x)), np.zeros((len(x), 3))
    for k in range(len(x)):
        d = p - x[k]
        inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
        w = mj.copy()
        if skip is not None and skip[k] >= 0:
            w[skip[k]] = 0.0
        term = d * (w * inv ** 3)[:, None]
        acc[k], mag[k], phi[k] = term.sum(0), np.abs(term).sum(0), -(w * inv).sum()
    return acc, phi, mag


def numpy_tidal(pos, points, skip=None):
    """(T, mag), (m, 6) each: tidal_common.numpy_tidal with m_j in every term"""
    p, mj, x = pos[:, :3].astype(np.float64), pos[:, 3].astype(np.float64), points[:, :3].astype(np.float64)
    t, mag = np.zeros((len(x), 6)), np.zeros((len(x), 6))
    for k in range(len(x)):
        d = p - x[k]
        inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
        w = mj.copy()
        if skip is not None and skip[k] >= 0:
            w[skip[k]] = 0.0
        inv3, inv5 = w * inv ** 3, w * inv ** 5
        for q, (a, b) in enumerate(DIAG):
            term = 3.0 * d[:, a] * d[:, b] * inv5
            t[k, q] = term.sum() - (inv3.sum() if a == b else 0.0)
            mag[k, q] = np.abs(term).sum() + (np.abs(inv3).sum() if a == b else 0.0)
    return t, mag


def numpy_jerk(pos, vel, points, pvel, skip=None):
    """(accel, jerk, mag_a, mag_j), (m, 3) each: jerk_common.numpy_jerk with m_j in every term"""
    p, mj, v = pos[:, :3].astype(np.float64), pos[:, 3].astype(np.float64), vel[:, :3].astype(np.float64)
    x, u = points[:, :3].astype(np.float64), pvel[:, :3].astype(np.float64)
    m = len(x)
    acc, jerk, mag_a, mag_j = (np.zeros((m, 3)) for _ in range(4))
    for k in range(m):
        d, w = p - x[k], v - u[k]
        wt = mj.copy()
        if skip is not None and skip[k] >= 0:
            wt[skip[k]] = 0.0
        inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
        inv2, inv3 = (inv * inv)[:, None], (wt * inv ** 3)[:, None]
        ta = d * inv3
        tj = (w - 3.0 * (d * w).sum(1)[:, None] * inv2 * d) * inv3
        acc[k], jerk[k] = ta.sum(0), tj.sum(0)
        mag_a[k] = np.abs(ta).sum(0)
        mag_j[k] = ((np.abs(w) + 3.0 * np.abs(d * w).sum(1)[:, None] * inv2 * np.abs(d)) * np.abs(inv3)).sum(0)
    return acc, jerk, mag_a, mag_j


def worst(got, want, mag):
    """the worst |got - want| / mag over queries and the components `want` has"""
    return float(np.max(np.abs(np.asarray(got, np.float64)[:, :want.shape[1]] - want) / mag))


def numpy_totals(pos, vel):
    """(E, P (3,), sum m |v|): T + U, the momentum and its scale of a weighted state in plain numpy binary64"""
    r, mj, v = np.asarray(pos, np.float64)[:, :3], np.asarray(pos, np.float64)[:, 3], np.asarray(vel, np.float64)[:, :3]
    d = r[None, :, :] - r[:, None, :]
    inv = 1.0 / np.sqrt((d * d).sum(2) + EPS)
    np.fill_diagonal(inv, 0.0)
    e = 0.5 * (mj * (v * v).sum(1)).sum() - 0.5 * (mj[:, None] * mj[None, :] * inv).sum()
    return e, (mj[:, None] * v).sum(0), (mj * np.sqrt((v * v).sum(1))).sum()


def kepler(m1, m2, e, dtype=np.float64):
    """(pos, vel) words of masses m1 and m2 (m1 + m2 = 1, in w) on a relative orbit of semi-major axis 1 and eccentricity e, started at
    pericentre on the x axis with the centre of mass at rest in the origin; the period is 2 pi"""
    assert m1 + m2 == 1.0
    rp, vp = 1.0 - e, np.sqrt((1.0 + e) / (1.0 - e))
    pos = np.array([[-m2 * rp, 0, 0, m1], [m1 * rp, 0, 0, m2]], dtype)
    vel = np.array([[0, -m2 * vp, 0, 0], [0, m1 * vp, 0, 0]], dtype)
    return pos, vel
