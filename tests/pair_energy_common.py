"""What the pair binding-energy tests (test_pair_energy_abi.py, test_gpu_pair_energy.py) share: tests/pair_energy_ref.c compiled as the
field tests compile field_ref.c, a plain restatement of the definition and of the elements in Python binary64 with timescale_common's
exact fma, and the builders of the systems whose binaries are known by construction."""
import ctypes as C
import decimal
import math

import numpy as np

from field_common import EPS, compile_ref
from pass_common import bits, same  # noqa: F401
from timescale_common import exact_fma, two_body_orbit

ANALYTIC = (-1.0, 1.0, 0.5, math.pi * math.sqrt(2.0))   # {E, a, ecc, period} of two unit masses on an orbit with a = 1, ecc = 0.5


class PairEnergyRef:
    """tests/pair_energy_ref.c: (e, idx) per row by one ascending scan; the system form and the elements"""

    def __init__(self, lib):
        self.lib = lib

    def rows(self, pos, vel, first=0, m=None):
        """rows first .. first + m of the system (dtype of pos), each leaving itself out"""
        dtype = pos.dtype.type
        pos, vel = np.ascontiguousarray(pos), np.ascontiguousarray(vel, dtype)
        m = len(pos) - first if m is None else m
        fn = self.lib.pair_energy_f64 if dtype == np.float64 else self.lib.pair_energy_f32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        fn.restype = None
        e, idx = np.empty(m, dtype), np.empty(m, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        fn(vp(pos), vp(vel), len(pos), int(first), int(m), vp(e), vp(idx))
        return e, idx

    def pair(self, pos, vel, i, j):
        """e of row i against body j alone, in the dtype of pos"""
        dtype = pos.dtype.type
        pos, vel = np.ascontiguousarray(pos), np.ascontiguousarray(vel, dtype)
        fn = self.lib.pair_e_f64 if dtype == np.float64 else self.lib.pair_e_f32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        fn.restype = C.c_double if dtype == np.float64 else C.c_float
        return dtype(fn(pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p), int(i), int(j)))

    def binaries(self, pos, vel, e_max=0.0, max_pairs=None):
        """(found, i, j, elements) of the whole system: the first min(found, max_pairs) pairs (None: all of them)"""
        dtype = pos.dtype.type
        pos, vel = np.ascontiguousarray(pos), np.ascontiguousarray(vel, dtype)
        fn = self.lib.binaries_f64 if dtype == np.float64 else self.lib.binaries_f32
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        fn.restype = C.c_int
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        k = len(pos) if max_pairs is None else int(max_pairs)
        i, j, el = np.empty(k, np.int32), np.empty(k, np.int32), np.empty((k, 4), np.float64)
        found = fn(vp(pos), vp(vel), len(pos), float(e_max), k, vp(i), vp(j), vp(el))
        got = min(found, k)
        return found, i[:got], j[:got], el[:got]


def make_ref(tmp_dir):
    return PairEnergyRef(compile_ref(tmp_dir, "pair_energy_ref"))


def python_pair_energy(pos, vel):
    """The definition restated in plain Python binary64 for FINITE inputs, the operations of include/nbody.h in their order: (e, idx)"""
    n = len(pos)
    p, v = pos[:, :3].astype(np.float64).tolist(), vel[:, :3].astype(np.float64).tolist()
    e, idx = np.full(n, np.inf), np.full(n, -1, np.int32)
    for i in range(n):
        for j in range(n):
            if j == i:
                continue
            dx, dy, dz = p[j][0] - p[i][0], p[j][1] - p[i][1], p[j][2] - p[i][2]
            ux, uy, uz = v[j][0] - v[i][0], v[j][1] - v[i][1], v[j][2] - v[i][2]
            d2 = exact_fma(dx, dx, exact_fma(dy, dy, dz * dz))
            v2 = exact_fma(ux, ux, exact_fma(uy, uy, uz * uz))
            inv = 1.0 / math.sqrt(d2 + EPS)
            q = exact_fma(0.5, v2, -2.0 * inv)
            if q < e[i]:
                e[i], idx[i] = q, j
    return e, idx


def python_elements(pos, vel, i, j):
    """{E, a, ecc, period} of the pair (i, j) in plain Python binary64 from the state converted exactly, the header's order"""
    ri, rj, vi, vj = (np.asarray(a[k, :3], np.float64).tolist() for a, k in ((pos, i), (pos, j), (vel, i), (vel, j)))
    dx, dy, dz = rj[0] - ri[0], rj[1] - ri[1], rj[2] - ri[2]
    ux, uy, uz = vj[0] - vi[0], vj[1] - vi[1], vj[2] - vi[2]
    s = ((dx * dx + dy * dy) + dz * dz) + EPS
    r = math.sqrt(s)
    v2 = (ux * ux + uy * uy) + uz * uz
    E = 0.5 * v2 - 2.0 / r
    a = -1.0 / E
    cx, cy, cz = dy * uz - dz * uy, dz * ux - dx * uz, dx * uy - dy * ux
    L2 = (cx * cx + cy * cy) + cz * cz
    ecc = math.sqrt(max(0.0, 1.0 + (0.5 * E) * L2))
    a3 = ((2.0 * a) * a) * a
    period = math.pi * math.sqrt(a3) if a3 >= 0.0 else math.nan   # (an unbound pair: a < 0)
    return np.array([E, a, ecc, period])


def softened_orbit(dtype=np.float64):
    """two_body_orbit(0.5) — two unit masses at apocentre, a = 1 — with the separation r and the speed v corrected for the softening, so
    that the SOFTENED pair of include/nbody.h has E = -1, a = 1 and ecc = 0.5 exactly in real arithmetic:
        v^2 / 2 - 2 / sqrt(r^2 + eps) = -1   and   r^2 v^2 = 3 / 2   (d is perpendicular to u at apocentre, so L2 = r^2 v^2 and
                                                                     ecc^2 = 1 + E L2 / 2 = 1 / 4).
    Plain two_body_orbit(0.5) (r = 3 / 2, v^2 = 2 / 3) has these only for eps = 0: with the force's eps = 1e-9 its softened energy is
    -1 + eps / r^3 = -1 + 3.0e-10 (test_pair_energy_abi.py shows it), beyond the 1e-12 the elements are held to.  S = r^2 + eps solves
    f(S) = 3 / (4 (S - eps)) - 2 / sqrt(S) + 1 = 0 near 9 / 4: Newton's iteration in 50-digit decimals, then one rounding of r / 2 and
    of v / 2 to binary64."""
    pos, vel, _ = two_body_orbit(0.5, dtype=np.float64)
    with decimal.localcontext() as ctx:
        ctx.prec = 50
        D = decimal.Decimal
        eps, S = D(EPS), D(9) / D(4)
        for _ in range(60):
            f = D(3) / (4 * (S - eps)) - 2 / S.sqrt() + 1
            df = -D(3) / (4 * (S - eps) ** 2) + 1 / (S * S.sqrt())
            S -= f / df
        assert abs(D(3) / (4 * (S - eps)) - 2 / S.sqrt() + 1) < D(10) ** -45
        r = (S - eps).sqrt()
        v = (D(3) / D(2)).sqrt() / r
        half_r, half_v = float(r / 2), float(v / 2)
    assert abs(half_r - 0.75) < 1e-9 and abs(half_v - math.sqrt(2.0 / 3.0) / 2) < 1e-9   # the correction is of the order of eps
    pos[0, 0], pos[1, 0] = -half_r, half_r
    vel[0, 1], vel[1, 1] = -half_v, half_v
    return pos.astype(dtype), vel.astype(dtype)


# six bodies ten lengths away on the axes, each moving at speed 3 across its radius, no two alike
FIELD_BODIES = (((10, 0, 0), (0, 3, 0)), ((-10, 0, 0), (0, -3, 0)), ((0, 10, 0), (0, 0, 3)), ((0, -10, 0), (0, 0, -3)),
                ((0, 0, 10), (3, 0, 0)), ((0, 0, -10), (-3, 0, 0)))


def binary_fixture(dtype=np.float64):
    """(pos, vel) of 8 bodies: softened_orbit() as bodies 0 and 1, then FIELD_BODIES.  Every pair but (0, 1) is at least 9 apart
    (2 / r <= 0.23) with a relative speed of at least 2.5 (v2 / 2 >= 3): e > 0, checked here in binary64 on every pair."""
    pos, vel = np.zeros((8, 4), np.float64), np.zeros((8, 4), np.float64)
    pos[:2], vel[:2] = softened_orbit()
    for k, (p, v) in enumerate(FIELD_BODIES):
        pos[2 + k, :3], vel[2 + k, :3] = p, v
    for i in range(8):
        for j in range(8):
            if i != j and (i, j) not in ((0, 1), (1, 0)):
                d, u = pos[j, :3] - pos[i, :3], vel[j, :3] - vel[i, :3]
                assert 0.5 * float(u @ u) - 2.0 / math.sqrt(float(d @ d) + EPS) > 2.0, (i, j)
    return pos.astype(dtype), vel.astype(dtype)


def place(parts, dtype=np.float64):
    """one system of several: parts = ((pos, vel, offset), ...), each moved by its offset (3 numbers), in order"""
    pos = np.concatenate([p + np.array(list(off) + [0.0]) for p, _, off in parts]).astype(dtype)
    vel = np.concatenate([v for _, v, _ in parts]).astype(dtype)
    return pos, vel
