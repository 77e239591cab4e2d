"""What the pair time-scale tests (test_timescale_abi.py, test_gpu_timescale.py) share: tests/timescale_ref.c compiled as the field
tests compile field_ref.c, bit comparison (bits and same, from pass_common), a plain restatement of the definition in Python binary64
with an exact fma, and a plain numpy restatement of the driver loop of nbody_step_adaptive and of the step it drives."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from field_common import EPS, compile_ref
from pass_common import bits, same  # noqa: F401


class TimescaleRef:
    """tests/timescale_ref.c: (tau2, idx, d2min) per row by one ascending scan; the system form by a scan of its own"""

    def __init__(self, lib):
        self.lib = lib

    def rows(self, pos, vel, first=0, m=None):
        """rows first .. first + m of the system (dtype of pos), each leaving itself out"""
        dtype = pos.dtype.type
        pos, vel = np.ascontiguousarray(pos), np.ascontiguousarray(vel, dtype)
        m = len(pos) - first if m is None else m
        fn = self.lib.timescale_f64 if dtype == np.float64 else self.lib.timescale_f32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        fn.restype = None
        tau2, idx, d2min = np.empty(m, dtype), np.empty(m, np.int32), np.empty(m, dtype)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        fn(vp(pos), vp(vel), len(pos), int(first), int(m), vp(tau2), vp(idx), vp(d2min))
        return tau2, idx, d2min

    def system(self, pos, vel):
        """(tau2, i, j, d2min) of the whole system"""
        dtype = pos.dtype.type
        pos, vel = np.ascontiguousarray(pos), np.ascontiguousarray(vel, dtype)
        fn = self.lib.min_timescale_f64 if dtype == np.float64 else self.lib.min_timescale_f32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        fn.restype = None
        tau2, out, d2min = np.empty(1, dtype), np.empty(2, np.int32), np.empty(1, dtype)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        fn(vp(pos), vp(vel), len(pos), vp(tau2), vp(out), vp(d2min))
        return tau2[0], int(out[0]), int(out[1]), d2min[0]


def make_ref(tmp_dir):
    return TimescaleRef(compile_ref(tmp_dir, "timescale_ref"))


def same_system(got, want):
    """(tau2, i, j, d2min) against (tau2, i, j, d2min): the indices equal, the floats the same bits and the same type"""
    return (got[1], got[2]) == (want[1], want[2]) and same((np.asarray(got[0]), np.asarray(got[3])), (np.asarray(want[0]), np.asarray(want[3])))


def exact_fma(a, b, c):
    """fma(a, b, c) of finite binary64 values, rounded once: the exact rational value, which float() rounds correctly"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def python_timescales(pos, vel):
    """The definition restated in plain Python binary64 for FINITE inputs, the fma order of include/nbody.h: (tau2, idx, d2min)"""
    n = len(pos)
    p, v = pos[:, :3].astype(np.float64).tolist(), vel[:, :3].astype(np.float64).tolist()
    tau2, idx, d2min = np.full(n, np.inf), np.full(n, -1, np.int32), np.full(n, np.inf)
    for i in range(n):
        for j in range(n):
            if j == i:
                continue
            dx, dy, dz = p[j][0] - p[i][0], p[j][1] - p[i][1], p[j][2] - p[i][2]
            ux, uy, uz = v[j][0] - v[i][0], v[j][1] - v[i][1], v[j][2] - v[i][2]
            d2 = exact_fma(dx, dx, exact_fma(dy, dy, dz * dz))
            v2 = exact_fma(ux, ux, exact_fma(uy, uy, uz * uz))
            q = d2 / v2 if v2 != 0.0 else (math.nan if d2 == 0.0 else math.inf)
            if q < tau2[i]:
                tau2[i], idx[i] = q, j
            if d2 < d2min[i]:
                d2min[i] = d2
    return tau2, idx, d2min


def step_size(tau2, d2min, eta, dt_min, dt_max, t, t_end):
    """h of nbody_step_adaptive before it is rounded to the context precision: everything in binary64"""
    s = float(d2min) + EPS
    tff2 = s * math.sqrt(s) / 2.0
    h = float(eta) * math.sqrt(min(float(tau2), tff2))
    h = max(float(dt_min), min(h, float(dt_max)))
    if t + h > t_end:
        h = t_end - t
    return h


# ---- the driver restated in numpy binary64 on a system small enough for plain sums ----
def accel(pos):
    d = pos[None, :, :3] - pos[:, None, :3]
    inv3 = ((d * d).sum(2) + EPS) ** -1.5
    return (d * inv3[:, :, None]).sum(1)


def kick_drift(pos, vel, dt):
    """one step of the engine's integrator: v += a dt, then x += v dt"""
    vel[:, :3] += accel(pos) * dt
    pos[:, :3] += vel[:, :3] * dt


def total_energy(pos, vel):
    d = pos[None, :, :3] - pos[:, None, :3]
    inv = ((d * d).sum(2) + EPS) ** -0.5
    return 0.5 * float((vel[:, :3] ** 2).sum()) - float(np.triu(inv, 1).sum())


def numpy_min_timescale(pos, vel):
    """(tau2, d2min) of the whole system in plain numpy binary64 (no fma: the driver's ordering claim does not hang on a bit)"""
    n = len(pos)
    d = pos[None, :, :3] - pos[:, None, :3]
    u = vel[None, :, :3] - vel[:, None, :3]
    d2, v2 = (d * d).sum(2), (u * u).sum(2)
    off = ~np.eye(n, dtype=bool)
    with np.errstate(all="ignore"):
        q = d2 / v2
    q = q[off]
    q = q[np.isfinite(q)]
    return (float(q.min()) if len(q) else math.inf), float(d2[off].min()) if n > 1 else math.inf


def adaptive_run(pos, vel, t_end, eta, dt_min, dt_max, max_steps=1000000, observe=None):
    """the loop of nbody_step_adaptive on (pos, vel), in place -> (t_reached, steps); observe(pos, vel) after every step"""
    t, steps = 0.0, 0
    while t < t_end and steps < max_steps:
        tau2, d2min = numpy_min_timescale(pos, vel)
        h = step_size(tau2, d2min, eta, dt_min, dt_max, t, t_end)
        kick_drift(pos, vel, h)
        t += h
        steps += 1
        if observe:
            observe(pos, vel)
    return t, steps


def two_body_orbit(e, dtype=np.float64):
    """(pos, vel, period): two unit masses (G = 1, so mu = 2) on an orbit of semi-major axis 1 and eccentricity e, at apocentre, the
    centre of mass at rest at the origin"""
    mu, a = 2.0, 1.0
    r, v = a * (1.0 + e), math.sqrt(mu * (1.0 - e) / (a * (1.0 + e)))
    pos, vel = np.zeros((2, 4), dtype), np.zeros((2, 4), dtype)
    pos[0, 0], pos[1, 0] = -r / 2, r / 2
    vel[0, 1], vel[1, 1] = -v / 2, v / 2
    return pos, vel, 2.0 * math.pi * math.sqrt(a ** 3 / mu)


def worst_drift(run):
    """max |E - E0| / |E0| over the steps of run(observe)"""
    state = {"e0": None, "worst": 0.0}

    def observe(pos, vel):
        state["worst"] = max(state["worst"], abs((total_energy(pos, vel) - state["e0"]) / state["e0"]))

    def start(pos, vel):
        state["e0"] = total_energy(pos, vel)

    run(start, observe)
    return state["worst"]
