"""What the tidal tests (test_tidal_abi.py, test_gpu_tidal.py) share: tests/tidal_ref.c compiled as the field tests compile theirs
(field_common.compile_ref), a plain numpy fp64 evaluation of the definition with the scale an error is measured against, and the
check that T is the gradient of the field.  The points and skip indices are field_common's."""
import ctypes as C

import numpy as np

from field_common import EPS

DIAG = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))   # (a, b) of the six values {xx, yy, zz, xy, xz, yz}


class TidalRef:
    """tests/tidal_ref.c: (m, 6) in the documented order, IEEE 1/sqrt"""

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
        t = np.empty((m, 6), np.float32)
        keep, sk = self._skip(skip, m)
        self.lib.tidal_f32(pos.ctypes.data_as(C.c_void_p), len(pos), points.ctypes.data_as(C.c_void_p), m, sk, int(ref), t.ctypes.data_as(C.c_void_p))
        return t

    def f64(self, pos, points, skip=None):
        pos, points = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(points, np.float64)
        m = len(points)
        t = np.empty((m, 6), np.float64)
        keep, sk = self._skip(skip, m)
        self.lib.tidal_f64(pos.ctypes.data_as(C.c_void_p), len(pos), points.ctypes.data_as(C.c_void_p), m, sk, t.ctypes.data_as(C.c_void_p))
        return t


def numpy_tidal(pos, points, skip=None):
    """(T, mag), both (m, 6) fp64: the definition in plain numpy, T_ab = sum_j (3 d_a d_b inv^5 - delta_ab inv^3) over all j (skip left
    out, whatever it holds), no stated order, and the magnitude sums mag_ab = sum_j (3 |d_a d_b| inv^5 + delta_ab inv^3) — the scale an
    error of a sum that cancels is measured against"""
    p, x = pos[:, :3].astype(np.float64), points[:, :3].astype(np.float64)
    t, mag = np.zeros((len(x), 6)), np.zeros((len(x), 6))
    with np.errstate(all="ignore"):
        for k in range(len(x)):
            d = p - x[k]
            inv = 1.0 / np.sqrt((d * d).sum(1) + EPS)
            inv3, inv5 = inv ** 3, inv ** 5
            if skip is not None and skip[k] >= 0:
                d, inv3, inv5 = np.delete(d, skip[k], 0), np.delete(inv3, skip[k]), np.delete(inv5, skip[k])
            for q, (a, b) in enumerate(DIAG):
                term = 3.0 * d[:, a] * d[:, b] * inv5
                t[k, q] = term.sum() - (inv3.sum() if a == b else 0.0)
                mag[k, q] = np.abs(term).sum() + (inv3.sum() if a == b else 0.0)
    return t, mag


def worst(got, want, mag):
    """the worst |got - want| / mag over points and the six values"""
    return float(np.max(np.abs(got.astype(np.float64) - want) / mag))


def gradient_error(tidal, field, x, h):
    """Per point and (a, b), a, b in 0..2: |central difference of a_a along b with step h - T_ab|, and the truncation error of that
    difference, h^2 |d^3 a_a / dx_b^3| / 6 with d^3 a_a / dx_b^3 = d^2 T_ab / dx_b^2 estimated from T itself at +-h:
    (T_ab(x + h e_b) - 2 T_ab(x) + T_ab(x - h e_b)) / h^2.  tidal(points) -> (m, 6), field(points) -> (m, 4) accelerations, fp64.
    Returns (err, trunc, scale), (k, 3, 3) each; scale = |T| (Frobenius) of the point, for printing."""
    k = len(x)
    shifts = [np.zeros(3)] + [s * np.eye(3)[ax] for ax in range(3) for s in (h, -h)]
    pts = np.zeros((k * len(shifts), 4))
    for q, d in enumerate(shifts):
        pts[q * k:(q + 1) * k, :3] = x + d
    t6 = tidal(pts).reshape(len(shifts), k, 6)
    acc = field(pts).reshape(len(shifts), k, 4)
    full = t6[..., [[0, 3, 4], [3, 1, 5], [4, 5, 2]]]   # (shift, k, 3, 3)
    err, trunc = np.zeros((k, 3, 3)), np.zeros((k, 3, 3))
    for b in range(3):
        ph, mh = 1 + 2 * b, 2 + 2 * b
        for a in range(3):
            err[:, a, b] = np.abs((acc[ph, :, a] - acc[mh, :, a]) / (2 * h) - full[0, :, a, b])
            d2t = (full[ph, :, a, b] - 2 * full[0, :, a, b] + full[mh, :, a, b]) / (h * h)
            trunc[:, a, b] = h * h * np.abs(d2t) / 6
    scale = np.sqrt((full[0] ** 2).sum((1, 2)))
    return err, trunc, scale


GRADIENT_H = 1e-4   # the truncation error is 1e-5 of |T| there, the references' round-off (1e-16 |a| / h) six orders below it


def gradient_points(nb, pos):
    """50 points at least 0.05 from any body"""
    cand = nb.make_bodies(200, seed=11, dtype=np.float64)[0][:, :3]
    near = np.array([np.sqrt(((pos[:, :3] - c) ** 2).sum(1).min()) for c in cand])
    x = cand[near >= 0.05]
    assert len(x) >= 50, len(x)
    return x[:50]
