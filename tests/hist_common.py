"""What the radial-count tests (test_hist_abi.py, test_gpu_hist.py) share: tests/hist_ref.c compiled as the field tests compile
field_ref.c, the edge sets and a plain numpy fp64 brute force.  bits and same come from pass_common, planted and r2_for from
neighbors_common, make_points and make_skip from field_common."""
import ctypes as C

import numpy as np

from field_common import compile_ref, make_points, make_skip  # noqa: F401
from neighbors_common import planted, r2_for  # noqa: F401
from pass_common import bits, same  # noqa: F401

BINS = (1, 2, 4, 5, 8, 9, 16, 17, 31, 32)   # both sides of every capacity the kernels are built for (4, 8, 16, 32)


def geom_edges(n_bins, dtype):
    """n_bins + 1 squared radii from 0 (then 1e-3) to 16, geometrically spaced, in dtype"""
    e = np.geomspace(1e-3, 16, n_bins + 1).astype(dtype)
    e[0] = 0
    return e


def radius_edges(pos):
    """{0, a radius that holds 1 % of the bodies around body 0, one that holds 30 %, 12.5, +inf}: counts from none to all"""
    dtype = pos.dtype.type
    return np.array([0, r2_for(pos, 0.01), r2_for(pos, 0.3), 12.5, np.inf], dtype)


def count_edges(r2, dtype):
    """the edges whose one bin is the neighbour pass's count at r2: d2 < nextafter(r2, +inf) is d2 <= r2"""
    return np.array([0, np.nextafter(dtype(r2), dtype(np.inf))], dtype)


class HistRef:
    """tests/hist_ref.c: counts (m, n_bins) int32 per query by one ascending scan; the pair histogram by a scan of its own"""

    def __init__(self, lib):
        self.lib = lib

    def _run(self, dtype, pos, points, first, m, skip, edges2):
        pos = np.ascontiguousarray(pos, dtype)
        e = np.ascontiguousarray(edges2, dtype)
        nb = len(e) - 1
        assert e.ndim == 1 and 1 <= nb <= 32
        fn = self.lib.hist_f64 if dtype == np.float64 else self.lib.hist_f32
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        fn.restype = None
        pts = None
        if points is not None:
            pts = np.ascontiguousarray(points, dtype)
            m = len(pts)
        sk = np.ascontiguousarray(skip, np.int32) if skip is not None else None
        assert sk is None or sk.shape == (m,)
        counts = np.empty((m, nb), np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        fn(vp(pos), len(pos), vp(pts), int(first), m, vp(sk), vp(e), nb, vp(counts))
        return counts

    def rows(self, pos, edges2, first=0, m=None):
        """the bodies first .. first + m as queries, each leaving itself out (dtype of pos)"""
        return self._run(pos.dtype.type, pos, None, first, len(pos) - first if m is None else m, None, edges2)

    def points(self, pos, points, edges2, skip=None):
        return self._run(pos.dtype.type, pos, points, 0, None, skip, edges2)

    def pairs(self, pos, edges2):
        dtype = pos.dtype.type
        pos = np.ascontiguousarray(pos)
        e = np.ascontiguousarray(edges2, dtype)
        out = np.empty(len(e) - 1, np.int64)
        fn = self.lib.pair_hist_f64 if dtype == np.float64 else self.lib.pair_hist_f32
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        fn.restype = None
        fn(pos.ctypes.data_as(C.c_void_p), len(pos), e.ctypes.data_as(C.c_void_p), len(e) - 1, out.ctypes.data_as(C.c_void_p))
        return out


def make_ref(tmp_dir):
    return HistRef(compile_ref(tmp_dir, "hist_ref"))


def numpy_d2(pos, queries, skip):
    """plain numpy fp64: the (m, N) squared distances, NaN where the body is the query's skipped one"""
    p, x = pos[:, :3].astype(np.float64), queries[:, :3].astype(np.float64)
    v = ((p[None, :, :] - x[:, None, :]) ** 2).sum(2)
    if skip is not None:
        rows = np.flatnonzero(np.asarray(skip) >= 0)
        v[rows, np.asarray(skip)[rows]] = np.nan
    return v
