"""The k-nearest-neighbour entry points (nbody_knn_rows, nbody_knn and their _d forms; include/nbody.h "k nearest neighbours") as far
as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement tests/knn_ref.c itself
— against a plain numpy fp64 brute force, against tests/neighbors_ref.c at k = 1, its prefix property, and on planted systems whose
answers are known by construction (duplicates, exact ties, a NaN body, fewer than k candidates)."""
import ctypes as C

import numpy as np
import pytest

import neighbors_common
from knn_common import bits, make_ref, numpy_knn, planted, same

SYMBOLS = {"nbody_knn_rows": 5, "nbody_knn_rows_d": 5, "nbody_knn": 6, "nbody_knn_d": 6}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("knn_ref"))


@pytest.fixture(scope="module")
def nref(tmp_path_factory):
    return neighbors_common.make_ref(tmp_path_factory.mktemp("neighbors_ref"))


def queries_n300(nb, dtype):
    n = 300
    pos32 = nb.make_bodies(n, seed=42)[0]
    pts32 = (1.5 * nb.make_bodies(n, seed=7)[0].astype(np.float64)).astype(np.float32)
    return pos32.astype(dtype), pts32.astype(dtype)


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs, name
    assert callable(nb.NBody.knn) and callable(nb.NBody.knn_at)
    hdr = open(nb._lib.HERE + "/../include/nbody.h").read()
    assert "#define NBODY_KNN_MAX 32" in hdr and nb._lib.KNN_MAX == 32


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for sfx, dt, ct in (("", np.float32, C.c_float), ("_d", np.float64, C.c_double)):
        fp = lambda a: a.ctypes.data_as(C.POINTER(ct))
        pts = np.zeros((4, 4), dt)
        idx, d2 = np.full((4, 3), 7, np.int32), np.full((4, 3), 7, dt)
        assert getattr(lib, "nbody_knn_rows" + sfx)(0, 4, 3, ip(idx), fp(d2)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_knn" + sfx)(fp(pts), 4, None, 3, ip(idx), fp(d2)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_knn" + sfx)(None, 4, None, 99, None, None) == nb._lib.ERR_NOT_INIT
        assert np.all(idx == 7) and np.all(d2 == 7)


@pytest.mark.parametrize("k", [1, 4, 5, 8, 16, 32])
def test_knn_ref_against_numpy(nb, ref, k):
    """Identical index lists wherever the order of the k + 1 smallest fp64 distances is beyond the rounding of d2.  The statement's d2
    carries at most five roundings relative to the exact value (tests/test_neighbors_abi.py derives it: |d2 - exact| <= 5 u d2,
    u = 2^-24 or 2^-53), so two candidates a < b keep their order when b - a exceeds 5 u (a + b), twice over for the numpy side's own
    roundings.  A row is compared only when every consecutive gap among its k + 1 smallest fp64 distances exceeds that — the gap
    behind entry k - 1 decides who is the last one in.  With these seeds that leaves out 0 of the 300 rows in either precision, rows
    form and points form, for every k here, which is asserted."""
    n = 300
    for dtype, u in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -53)):
        pos, pts = queries_n300(nb, dtype)
        for name, got, queries, sk in (("rows", ref.rows(pos, k), pos, np.arange(n)), ("points", ref.points(pos, pts, k), pts, None)):
            idx, d2 = got
            assert idx.shape == (n, k) and d2.shape == (n, k) and idx.dtype == np.int32 and d2.dtype == dtype
            widx, wd = numpy_knn(pos, queries, sk, k)
            a, b = wd[:, :-1], wd[:, 1:]
            clear = np.all(b - a > 2 * 5 * u * (a + b), axis=1)
            print("%s %s k=%d: %d of %d rows left out" % (np.dtype(dtype).name, name, k, int((~clear).sum()), n))
            assert int((~clear).sum()) == 0, (name, np.flatnonzero(~clear))
            assert np.array_equal(idx, widx[:, :k]), name
            assert np.all(np.abs(d2.astype(np.float64) - wd[:, :k]) <= 5 * u * wd[:, :k]), name
            assert np.all(np.diff(d2.astype(np.float64), axis=1) >= 0), name


def test_knn_ref_is_neighbors_ref_at_k1_and_a_prefix_of_every_larger_k(nb, ref, nref):
    n = 300
    skip = np.full(n, -1, np.int32)
    skip[:3] = (0, 5, n - 1)
    skip[10::3] = (np.arange(10, n, 3) * 7919) % n
    for dtype in (np.float32, np.float64):
        pos, pts = queries_n300(nb, dtype)
        pts[:3] = pos[[0, 5, n - 1]]
        forms = ((lambda k: ref.rows(pos, k), nref.rows(pos)), (lambda k: ref.rows(pos, k, 17, 100), nref.rows(pos, 17, 100)),
                 (lambda k: ref.points(pos, pts, k), nref.points(pos, pts)), (lambda k: ref.points(pos, pts, k, skip), nref.points(pos, pts, skip)))
        for call, near in forms:
            one = call(1)
            assert same((one[0][:, 0], one[1][:, 0]), near[:2])   # bit for bit
            full = call(32)
            for k in (1, 2, 3, 4, 5, 8, 9, 16, 17, 31):
                assert same(call(k), (full[0][:, :k], full[1][:, :k])), k


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_cases(nb, ref, dtype):
    n = 1100
    pos = planted(nb, n, dtype)
    h2 = dtype(2.0 ** -24)
    for k in (4, 5, 32):
        idx, d2 = ref.rows(pos, k)
        # 64, 65, 500 and 1024 are all exactly h away from 63: ascending j among equal d2
        assert list(idx[63, :4]) == [64, 65, 500, 1024] and np.all(bits(d2[63, :4]) == bits(h2))
        assert k == 4 or d2[63, 4] > h2
        # two bodies on body 3's position: +0, the lower index first
        assert list(idx[3, :2]) == [70, 900] and np.all(bits(d2[3, :2]) == 0) and d2[3, 2] > 0
        assert list(idx[70, :2]) == [3, 900] and list(idx[900, :2]) == [3, 70]
        # the NaN body is in no list, and its own list is empty
        assert not np.any(idx == 200) and np.all(idx[200] == -1) and np.all(np.isposinf(d2[200]))
        others = np.delete(np.arange(n), 200)
        assert np.all(idx[others] >= 0) and np.all(np.isfinite(d2[others]))
    # the points form: a point on a body lists it first at +0 unless it is skipped
    pts = pos[[3, 63, 200]].copy()
    pts[2, :3] = 4.0   # body 63's position again
    pi, pd = ref.points(pos, pts, 5)
    assert list(pi[0, :3]) == [3, 70, 900] and list(pi[1]) == [63, 64, 65, 500, 1024] and list(pi[2]) == [63, 64, 65, 500, 1024]
    assert np.all(bits(pd[0, :3]) == 0) and list(pd[1]) == [0, h2, h2, h2, h2]
    pi, pd = ref.points(pos, pts, 3, np.array([3, 64, -1], np.int32))
    assert list(pi[0, :2]) == [70, 900] and list(pi[1]) == [63, 65, 500] and list(pi[2]) == [63, 64, 65]
    # fewer than k candidates: padded with (-1, +inf)
    one = pos[:1]
    idx, d2 = ref.rows(one, 3)
    assert np.all(idx == -1) and np.all(np.isposinf(d2))
    idx, d2 = ref.points(one, one, 2)
    assert list(idx[0]) == [0, -1] and bits(d2[0, 0]) == 0 and np.isposinf(d2[0, 1])
    assert np.all(ref.points(one, one, 2, np.zeros(1, np.int32))[0] == -1)
    five = pos[:5]
    idx, d2 = ref.rows(five, 8)
    assert np.all(idx[:, :4] >= 0) and np.all(idx[:, 4:] == -1) and np.all(np.isfinite(d2[:, :4])) and np.all(np.isposinf(d2[:, 4:]))
    assert all(sorted(idx[i, :4]) == [j for j in range(5) if j != i] for i in range(5))
