"""What the knn tests (test_knn_abi.py, test_gpu_knn.py) share: tests/knn_ref.c compiled as the field tests compile field_ref.c, bit
comparison of (idx, d2) pairs and a plain numpy fp64 brute force.  bits and same come from pass_common, planted from neighbors_common,
make_points and make_skip from field_common."""
import ctypes as C

import numpy as np

from field_common import compile_ref, make_points, make_skip  # noqa: F401
from neighbors_common import planted  # noqa: F401
from pass_common import bits, same  # noqa: F401

KS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32)   # both sides of every list capacity the kernels are built for (4, 8, 16, 32)


class KnnRef:
    """tests/knn_ref.c: (idx, d2), each (m, k), per query by one ascending scan with a stable insertion list"""

    def __init__(self, lib):
        self.lib = lib

    def _run(self, dtype, pos, points, first, m, skip, k):
        pos = np.ascontiguousarray(pos, dtype)
        fn = self.lib.knn_f64 if dtype == np.float64 else self.lib.knn_f32
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        fn.restype = None
        pts = None
        if points is not None:
            pts = np.ascontiguousarray(points, dtype)
            m = len(pts)
        sk = np.ascontiguousarray(skip, np.int32) if skip is not None else None
        assert sk is None or sk.shape == (m,)
        assert 1 <= k <= 32
        idx, d2 = np.empty((m, k), np.int32), np.empty((m, k), dtype)
        vp = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        fn(vp(pos), len(pos), vp(pts), int(first), m, vp(sk), int(k), vp(idx), vp(d2))
        return idx, d2

    def rows(self, pos, k, first=0, m=None):
        """the bodies first .. first + m as queries, each leaving itself out (dtype of pos)"""
        return self._run(pos.dtype.type, pos, None, first, len(pos) - first if m is None else m, None, k)

    def points(self, pos, points, k, skip=None):
        return self._run(pos.dtype.type, pos, points, 0, None, skip, k)


def make_ref(tmp_dir):
    return KnnRef(compile_ref(tmp_dir, "knn_ref"))


def numpy_knn(pos, queries, skip, k):
    """plain numpy fp64: per query the indices of the k + 1 smallest squared distances and those distances, skip left out ((m, k + 1)
    each; +inf where the bodies run out)"""
    p, x = pos[:, :3].astype(np.float64), queries[:, :3].astype(np.float64)
    idx, d = np.full((len(x), k + 1), -1, np.int64), np.full((len(x), k + 1), np.inf)
    for q in range(len(x)):
        v = ((p - x[q]) ** 2).sum(1)
        if skip is not None and skip[q] >= 0:
            v[skip[q]] = np.inf
        o = np.argsort(v, kind="stable")[:k + 1]
        idx[q, :len(o)], d[q, :len(o)] = o, v[o]
    return idx, d
