"""What the field tests (test_field_abi.py, test_gpu_field.py) share: tests/field_ref.c and tests/potential_ref.c compiled as the
energy tests compile the latter, the family of test points and a plain numpy fp64 evaluation of the definition."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.array([0x3089705F], np.uint32).view(np.float32)[0])


def compile_ref(tmp_dir, name):
    """tests/<name>.c as a shared library (-ffp-contract=off: products are fused only where the source says fma)"""
    so = os.path.join(str(tmp_dir), name + ".so")
    src = os.path.join(ROOT, "tests", name + ".c")
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], []):   # every operation is IEEE-exact: vector width and threads change no bit
        r = subprocess.run(["gcc", "-std=c11", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"] + extra + ["-o", so, src, "-lm"],
                           capture_output=True, timeout=180)
        if r.returncode == 0:
            return C.CDLL(so)
    raise RuntimeError("cannot compile tests/%s.c: %s" % (name, r.stderr.decode()[-2000:]))


class FieldRef:
    """tests/field_ref.c: (accel, phi) in the documented order, IEEE 1/sqrt"""

    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def _skip(skip, m):
        if skip is None:
            return None, None
        sk = np.ascontiguousarray(skip, np.int32)
        assert sk.shape == (m,)
        return sk, sk.ctypes.data_as(C.c_void_p)

    def f32(self, pos, points, skip=None, ref=False):
        pos, points = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(points, np.float32)
        m = len(points)
        acc, phi = np.empty((m, 4), np.float32), np.empty(m, np.float32)
        keep, sk = self._skip(skip, m)
        self.lib.field_f32(pos.ctypes.data_as(C.c_void_p), len(pos), points.ctypes.data_as(C.c_void_p), m, sk, int(ref),
                           acc.ctypes.data_as(C.c_void_p), phi.ctypes.data_as(C.c_void_p))
        return acc, phi

    def f64(self, pos, points, skip=None):
        pos, points = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(points, np.float64)
        m = len(points)
        acc, phi = np.empty((m, 4), np.float64), np.empty(m, np.float64)
        keep, sk = self._skip(skip, m)
        self.lib.field_f64(pos.ctypes.data_as(C.c_void_p), len(pos), points.ctypes.data_as(C.c_void_p), m, sk,
                           acc.ctypes.data_as(C.c_void_p), phi.ctypes.data_as(C.c_void_p))
        return acc, phi


def make_points(nb, pos, m, seed=7):
    """m points 1.5 x the positions of an m-body system (so some lie outside the cube the bodies fill), the first three set onto bodies
    0, 5 and N - 1 (clipped to the bodies there are).  Returns (points, the on-body indices)."""
    n = len(pos)
    pts = (1.5 * nb.make_bodies(m, seed=seed)[0].astype(np.float64)).astype(pos.dtype)   # 1.5 x is exact in either precision
    on = [0, min(5, n - 1), n - 1][:m]
    for k, i in enumerate(on):
        pts[k] = pos[i]
    return pts, on


def make_skip(n, m, on):
    """-1, the matching body for the on-body points, and arbitrary indices for every third of the others"""
    sk = np.full(m, -1, np.int32)
    for p in range(len(on), m):
        if p % 3 == 1:
            sk[p] = (p * 7919) % n
    sk[:len(on)] = on
    return sk


def numpy_field(pos, points, skip=None, mags=False):
    """the definition in plain numpy fp64: sums over all j (skip left out, whatever it holds), no stated order.  mags: also the sums
    of the magnitudes of the acceleration's terms, (m, 3) — the scale an error of a sum that cancels is measured against"""
    p, x = pos[:, :3].astype(np.float64), points[:, :3].astype(np.float64)
    acc, phi, mag = np.zeros((len(x), 4)), np.zeros(len(x)), np.zeros((len(x), 3))
    with np.errstate(all="ignore"):
        for k in range(len(x)):
            d = p - x[k]
            inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
            term = d * (inv ** 3)[:, None]
            if skip is not None and skip[k] >= 0:
                inv[skip[k]] = 0.0
                term[skip[k]] = 0.0
            acc[k, :3] = term.sum(0)
            mag[k] = np.abs(term).sum(0)
            phi[k] = -inv.sum()
    return (acc, phi, mag) if mags else (acc, phi)


def row_rel(got, want):
    """max over points of |got - want|_2 / |want|_2 of the three components (the project's force measure)"""
    g, w = got[:, :3].astype(np.float64), want[:, :3].astype(np.float64)
    return float(np.max(np.linalg.norm(g - w, axis=1) / np.linalg.norm(w, axis=1)))
