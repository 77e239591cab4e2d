"""What the Hermite tests (test_hermite_abi.py, test_gpu_hermite.py) share: tests/hermite_ref.c compiled together with tests/jerk_ref.c
as jerk_common compiles its own (-ffp-contract=off), a plain numpy binary64 Hermite with no stated order, the Kepler pair, the energy of
a state and the measure the timed binary32 test uses."""
import ctypes as C
import os
import subprocess

import numpy as np

from field_common import EPS, ROOT

# What hermite_ref.c's strict binary32 keeps against the numpy binary64 run at TIMED, in worst()'s measure; test_hermite_abi.py asserts it.
# Measured on the CPU: 1.557e-1 in both d2 forms, at rows 1608 and 588 (the third worst row keeps 3.2e-2).  It is that large because
# a shared dt of 1/256 does not resolve make_bodies(2100)'s close encounters (min |a|^2 / |j|^2 = 4.1e-6 at t = 0, an Aarseth step of
# 8e-5 at eta = 0.04): rows 588 and 1608 start 0.040 apart and closing, are 0.029 and 0.022 apart after one and two steps, and the
# third step takes them through an all but unsoftened collision that throws them 3.6e3 apart in the binary64 run too.  The
# thrown values amplify the two bodies' rounding differences to 0.16 of themselves, while the median body keeps 6e-6 in velocity and
# 1e-7 in position (R_REF_MEDIAN, worst_median()).
R_REF = 0.16
R_REF_MEDIAN = 1.0e-5
TIMED = (2100, 4, 1.0 / 256)   # (n, steps, dt) of the timed binary32 test
TIMED_BOUND = 2 * R_REF + 6e-7   # the reference's own error doubled, plus v_rsq_f32's share
PERIOD = 2 * np.pi / np.sqrt(2.0)


def compile_ref(tmp_dir):
    """tests/hermite_ref.c + tests/jerk_ref.c as one shared library"""
    so = os.path.join(str(tmp_dir), "hermite_ref.so")
    srcs = [os.path.join(ROOT, "tests", f) for f in ("hermite_ref.c", "jerk_ref.c")]
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], []):   # every operation is IEEE-exact: vector width and threads change no bit
        r = subprocess.run(["gcc", "-std=c11", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"] + extra + ["-o", so] + srcs + ["-lm"],
                           capture_output=True, timeout=180)
        if r.returncode == 0:
            return C.CDLL(so)
    raise RuntimeError("cannot compile tests/hermite_ref.c: %s" % r.stderr.decode()[-2000:])


class HermiteRef:
    """tests/hermite_ref.c.  dtype float32 or float64 picks the statement; every method returns new (pos, vel) words, (n, 4) each"""

    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def _words(pos, vel, dtype):
        p, v = np.array(pos, dtype, order="C"), np.array(vel, dtype, order="C")
        assert p.shape == v.shape and p.shape[1] == 4
        return p, v

    @staticmethod
    def _suf(dtype):
        return "f64" if np.dtype(dtype) == np.float64 else "f32"

    def _stepper(self, name, pos, vel, dtype, dt, count, ref):
        p, v = self._words(pos, vel, dtype)
        fn = getattr(self.lib, name + "_" + self._suf(dtype))
        ct = C.c_double if np.dtype(dtype) == np.float64 else C.c_float
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ct, C.c_int, C.c_int]
        fn.restype = None
        fn(p.ctypes.data, v.ctypes.data, len(p), float(dt), int(count), int(ref))
        return p, v

    def step(self, pos, vel, dtype, dt, nsteps, ref=False):
        """one call of nsteps steps (the carried form)"""
        return self._stepper("hermite", pos, vel, dtype, dt, nsteps, ref)

    def restarted(self, pos, vel, dtype, dt, ncalls, ref=False):
        """ncalls calls of one step each"""
        return self._stepper("hermite_restarted", pos, vel, dtype, dt, ncalls, ref)

    def min_aarseth(self, pos, vel, dtype, ref=False):
        p, v = self._words(pos, vel, dtype)
        fn = getattr(self.lib, "min_aarseth_" + self._suf(dtype))
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        fn.restype = None
        q, row = C.c_double(), C.c_int()
        fn(p.ctypes.data, v.ctypes.data, len(p), int(ref), C.byref(q), C.byref(row))
        return q.value, row.value

    def adaptive(self, pos, vel, dtype, eta, t_end, dt_min, dt_max, max_steps=1000000, ref=False):
        """(pos, vel, t_reached, steps)"""
        p, v = self._words(pos, vel, dtype)
        fn = getattr(self.lib, "hermite_adaptive_" + self._suf(dtype))
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                       C.POINTER(C.c_double), C.POINTER(C.c_int)]
        fn.restype = None
        t, steps = C.c_double(), C.c_int()
        fn(p.ctypes.data, v.ctypes.data, len(p), int(ref), eta, t_end, dt_min, dt_max, int(max_steps), C.byref(t), C.byref(steps))
        return p, v, t.value, steps.value


def numpy_aj(r, v, chunk=256):
    """(a, j), (n, 3) binary64 each: the definition over all other bodies in plain numpy, no stated order"""
    n = len(r)
    a, j = np.empty((n, 3)), np.empty((n, 3))
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        d = r[None, :, :] - r[i0:i1, None, :]
        w = v[None, :, :] - v[i0:i1, None, :]
        inv = 1.0 / np.sqrt((d * d).sum(2) + EPS)
        inv[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
        inv2 = inv * inv
        inv3 = inv * inv2
        a[i0:i1] = (d * inv3[:, :, None]).sum(1)
        rv = (d * w).sum(2)
        j[i0:i1] = ((w - 3.0 * (rv * inv2)[:, :, None] * d) * inv3[:, :, None]).sum(1)
    return a, j


def numpy_hermite(pos, vel, dt, nsteps):
    """one call of nsteps steps in plain numpy binary64; (pos, vel) words with the fourth values carried"""
    p, u = np.array(pos, np.float64), np.array(vel, np.float64)
    r, v = p[:, :3].copy(), u[:, :3].copy()
    a0, j0 = numpy_aj(r, v)
    for _ in range(nsteps):
        rp = r + v * dt + a0 * (dt * dt / 2) + j0 * (dt ** 3 / 6)
        vp = v + a0 * dt + j0 * (dt * dt / 2)
        a1, j1 = numpy_aj(rp, vp)
        v1 = v + (a0 + a1) * (dt / 2) + (j0 - j1) * (dt * dt / 12)
        r1 = r + (v + v1) * (dt / 2) + (a0 - a1) * (dt * dt / 12)
        r, v, a0, j0 = r1, v1, a1, j1
    p[:, :3], u[:, :3] = r, v
    return p, u


def numpy_hermite_adaptive(pos, vel, eta, t_end, dt_min, dt_max):
    """(pos, vel, steps): the adaptive loop in plain numpy binary64"""
    p, u = np.array(pos, np.float64), np.array(vel, np.float64)
    r, v = p[:, :3].copy(), u[:, :3].copy()
    a0, j0 = numpy_aj(r, v)
    t, n = 0.0, 0
    while t < t_end:
        q = ((a0 * a0).sum(1) / (j0 * j0).sum(1)).min()
        dt = max(min(eta * np.sqrt(q), dt_max), dt_min)
        if t + dt > t_end:
            dt = t_end - t
        rp = r + v * dt + a0 * (dt * dt / 2) + j0 * (dt ** 3 / 6)
        vp = v + a0 * dt + j0 * (dt * dt / 2)
        a1, j1 = numpy_aj(rp, vp)
        v1 = v + (a0 + a1) * (dt / 2) + (j0 - j1) * (dt * dt / 12)
        r1 = r + (v + v1) * (dt / 2) + (a0 - a1) * (dt * dt / 12)
        r, v, a0, j0 = r1, v1, a1, j1
        t += dt
        n += 1
    p[:, :3], u[:, :3] = r, v
    return p, u, n


def kepler(e, dtype=np.float64):
    """(pos, vel) words of two unit masses on a relative orbit of semi-major axis 1 and eccentricity e, started at pericentre on the x
    axis; the period is PERIOD = 2 pi / sqrt(2)"""
    rp, vp = 1.0 - e, np.sqrt(2.0 * (1.0 + e) / (1.0 - e))
    pos = np.array([[-rp / 2, 0, 0, 0], [rp / 2, 0, 0, 0]], dtype)
    vel = np.array([[0, -vp / 2, 0, 0], [0, vp / 2, 0, 0]], dtype)
    return pos, vel


def energy(pos, vel):
    """T + U of unit masses with the force's softening, binary64"""
    r, v = np.asarray(pos, np.float64)[:, :3], np.asarray(vel, np.float64)[:, :3]
    d = r[None, :, :] - r[:, None, :]
    inv = 1.0 / np.sqrt((d * d).sum(2) + EPS)
    np.fill_diagonal(inv, 0.0)
    return 0.5 * (v * v).sum() - 0.5 * inv.sum()


def worst(pos, vel, want_pos, want_vel):
    """the worst |got - want| over the position and velocity components, relative to max(1, |want|)"""
    out = 0.0
    for got, want in ((pos, want_pos), (vel, want_vel)):
        g, w = np.asarray(got, np.float64)[:, :3], np.asarray(want, np.float64)[:, :3]
        out = max(out, float(np.max(np.abs(g - w) / np.maximum(1.0, np.abs(w)))))
    return out


def worst_median(pos, vel, want_pos, want_vel):
    """the median over the bodies of each body's worst component error in worst()'s measure: what the typical body keeps"""
    per = np.zeros(len(want_pos))
    for got, want in ((pos, want_pos), (vel, want_vel)):
        g, w = np.asarray(got, np.float64)[:, :3], np.asarray(want, np.float64)[:, :3]
        per = np.maximum(per, (np.abs(g - w) / np.maximum(1.0, np.abs(w))).max(1))
    return float(np.median(per))


def position_error(pos, want_pos):
    return float(np.max(np.abs(np.asarray(pos, np.float64)[:, :3] - np.asarray(want_pos, np.float64)[:, :3])))
