"""What the neighbour tests (test_neighbors_abi.py, test_gpu_neighbors.py) share: tests/neighbors_ref.c compiled as the field tests
compile field_ref.c, bit comparison (bits and same, from pass_common), a plain numpy fp64 brute force and the planted systems
(duplicates, ties, a NaN body)."""
import ctypes as C

import numpy as np

from field_common import compile_ref
from pass_common import bits, same  # noqa: F401


class NeighborsRef:
    """tests/neighbors_ref.c: (idx, d2, count-or-None) per query by one ascending scan; the closest pair by a scan of its own"""

    def __init__(self, lib):
        self.lib = lib

    def _run(self, dtype, pos, points, first, m, skip, r2):
        pos = np.ascontiguousarray(pos, dtype)
        fn = self.lib.neighbors_f64 if dtype == np.float64 else self.lib.neighbors_f32
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_double if dtype == np.float64 else C.c_float,
                       C.c_void_p, C.c_void_p, C.c_void_p]
        fn.restype = None
        pts = None
        if points is not None:
            pts = np.ascontiguousarray(points, dtype)
            m = len(pts)
        sk = np.ascontiguousarray(skip, np.int32) if skip is not None else None
        assert sk is None or sk.shape == (m,)
        idx, d2 = np.empty(m, np.int32), np.empty(m, dtype)
        cnt = np.empty(m, np.int32) if r2 is not None else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        fn(vp(pos), len(pos), vp(pts), int(first), m, vp(sk), float(dtype(0 if r2 is None else r2)), vp(idx), vp(d2), vp(cnt))
        return idx, d2, cnt

    def rows(self, pos, first=0, m=None, r2=None):
        """the bodies first .. first + m as queries, each leaving itself out (dtype of pos)"""
        return self._run(pos.dtype.type, pos, None, first, len(pos) - first if m is None else m, None, r2)

    def points(self, pos, points, skip=None, r2=None):
        return self._run(pos.dtype.type, pos, points, 0, None, skip, r2)

    def closest_pair(self, pos):
        dtype = pos.dtype.type
        pos = np.ascontiguousarray(pos)
        out = np.empty(2, np.int32)
        d2 = np.empty(1, dtype)
        fn = self.lib.closest_pair_f64 if dtype == np.float64 else self.lib.closest_pair_f32
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        fn.restype = None
        fn(pos.ctypes.data_as(C.c_void_p), len(pos), out.ctypes.data_as(C.c_void_p), d2.ctypes.data_as(C.c_void_p))
        return int(out[0]), int(out[1]), d2[0]


def make_ref(tmp_dir):
    return NeighborsRef(compile_ref(tmp_dir, "neighbors_ref"))


def numpy_neighbors(pos, queries, skip):
    """plain numpy fp64: per query (index of the smallest squared distance, that distance, the second smallest), skip left out"""
    p, x = pos[:, :3].astype(np.float64), queries[:, :3].astype(np.float64)
    idx, best, second = np.empty(len(x), np.int64), np.empty(len(x)), np.empty(len(x))
    for k in range(len(x)):
        d = ((p - x[k]) ** 2).sum(1)
        if skip is not None and skip[k] >= 0:
            d[skip[k]] = np.inf
        o = np.argsort(d, kind="stable")
        idx[k], best[k], second[k] = o[0], d[o[0]], d[o[1]] if len(d) > 1 else np.inf
    return idx, best, second


def r2_for(pos, fraction):
    """a radius (squared, in the dtype of pos) that holds about `fraction` of the bodies around body 0"""
    dtype = pos.dtype.type
    d = ((pos[:, :3].astype(np.float64) - pos[0, :3].astype(np.float64)) ** 2).sum(1)
    return dtype(np.sort(d)[min(len(d) - 1, int(fraction * len(d)))])


def planted(nb, n, dtype=np.float32, seed=2):
    """an n-body system (n >= 1100) with: bodies 70 and 900 on body 3's position (duplicates: d2 = +0, lowest index); body 63's
    nearest at exactly the same d2 — bodies 64 (the other side of a 64-source window edge), 500 and 1024 (the other side of a block,
    hence a chunk, edge) one step up along x, y and z, and body 65 (64's window) one step down along x; and body 200 all NaN"""
    pos = nb.make_bodies(n, seed=seed, dtype=dtype)[0].copy()
    pos[70, :3] = pos[3, :3]
    pos[900, :3] = pos[3, :3]
    h = dtype(2.0 ** -12)
    c = np.array([4.0, 4.0, 4.0], dtype)   # away from the cube the bodies fill: exact sums, nobody else near
    pos[63, :3] = c
    for j, ax in ((1024, 2), (500, 1), (64, 0)):
        pos[j, :3] = c
        pos[j, ax] += h
    pos[65, :3] = c
    pos[65, 0] -= h
    pos[200, :3] = np.nan
    return pos
