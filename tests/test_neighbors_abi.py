"""The neighbour entry points (nbody_neighbors_rows, nbody_nearest, nbody_closest_pair and their _d forms; include/nbody.h "nearest
neighbour, radius count, closest pair") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a
context, and the CPU statement tests/neighbors_ref.c itself — against a plain numpy fp64 brute force, and on planted systems whose
answers are known by construction (duplicates, an exact tie, a NaN body, N = 1)."""
import ctypes as C

import numpy as np
import pytest

from neighbors_common import bits, make_ref, numpy_neighbors, planted, same

SYMBOLS = {"nbody_neighbors_rows": 6, "nbody_neighbors_rows_d": 6, "nbody_nearest": 7, "nbody_nearest_d": 7, "nbody_closest_pair": 3,
           "nbody_closest_pair_d": 3}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("neighbors_ref"))


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs, name
    assert callable(nb.NBody.neighbors) and callable(nb.NBody.nearest) and callable(nb.NBody.closest_pair)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for sfx, dt, ct in (("", np.float32, C.c_float), ("_d", np.float64, C.c_double)):
        fp = lambda a: a.ctypes.data_as(C.POINTER(ct))
        pts = np.zeros((4, 4), dt)
        idx, d2, cnt = np.full(4, 7, np.int32), np.full(4, 7, dt), np.full(4, 7, np.int32)
        assert getattr(lib, "nbody_neighbors_rows" + sfx)(0, 4, ip(idx), fp(d2), 1.0, ip(cnt)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_nearest" + sfx)(fp(pts), 4, None, ip(idx), fp(d2), 1.0, ip(cnt)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_closest_pair" + sfx)(ip(idx), ip(idx[1:]), fp(d2)) == nb._lib.ERR_NOT_INIT
        assert np.all(idx == 7) and np.all(d2 == 7) and np.all(cnt == 7)


def test_neighbors_ref_against_numpy(nb, ref):
    """Identical indices wherever the fp64 gap between the best and the second best exceeds the rounding of d2.  The statement's d2
    carries at most five roundings relative to the exact value (the three differences enter squared: 2 u each on their term; one
    product and two fma: u each), so |d2 - exact| <= 5 u d2, u = 2^-24 (2^-53); a row is compared when second - best exceeds
    5 u (best + second), twice over for the numpy side's own roundings.  With this seed that leaves out 0 of the 300 rows in either
    precision, rows form and points form, which is asserted."""
    n = 300
    pos32 = nb.make_bodies(n, seed=42)[0]
    pts32 = (1.5 * nb.make_bodies(n, seed=7)[0].astype(np.float64)).astype(np.float32)
    pts32[:3] = pos32[[0, 5, n - 1]]
    skip = np.full(n, -1, np.int32)
    skip[:3] = (0, 5, n - 1)
    skip[10::3] = (np.arange(10, n, 3) * 7919) % n
    for dtype, u in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -53)):
        pos, pts = pos32.astype(dtype), pts32.astype(dtype)
        for name, got, queries, sk in (("rows", ref.rows(pos), pos, np.arange(n)), ("points", ref.points(pos, pts), pts, None),
                                       ("points+skip", ref.points(pos, pts, skip), pts, skip)):
            idx, d2, none = got
            assert none is None
            widx, best, second = numpy_neighbors(pos, queries, sk)
            clear = second - best > 2 * 5 * u * (best + second)
            print("%s %s: %d of %d rows left out" % (np.dtype(dtype).name, name, int((~clear).sum()), n))
            assert clear.all(), (name, np.flatnonzero(~clear))
            assert np.array_equal(idx, widx), name
            assert np.all(np.abs(d2.astype(np.float64) - best) <= 5 * u * best), name
        # counts: every body whose fp64 distance is clear of r2 by the same margin is counted or not as numpy says
        r2 = dtype(0.3)
        cnt = ref.rows(pos, r2=r2)[2]
        d = ((pos[:, None, :3].astype(np.float64) - pos[None, :, :3].astype(np.float64)) ** 2).sum(2)
        np.fill_diagonal(d, np.inf)
        lo, hi = (d <= float(r2) * (1 - 10 * u)).sum(1), (d <= float(r2) * (1 + 10 * u)).sum(1)
        assert np.all((lo <= cnt) & (cnt <= hi)) and cnt.min() < 10 and cnt.max() > 30, (cnt.min(), cnt.max())
        i, j, dmin = ref.closest_pair(pos)
        flat = int(np.argmin(d))
        full = ref.rows(pos)
        assert (i, j) == (flat // n, flat % n) and i < j and bits(dmin) == bits(full[1].min())
        assert same(ref.rows(pos, 17, 100), (full[0][17:117], full[1][17:117], None))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_cases(nb, ref, dtype):
    n = 1100
    pos = planted(nb, n, dtype)
    h2 = dtype(2.0 ** -24)
    r2 = dtype(1e30)   # everything that has a distance
    idx, d2, cnt = ref.rows(pos, r2=r2)
    # two bodies on body 3's position: +0 and the lowest index
    assert (idx[3], idx[70], idx[900]) == (70, 3, 3)
    assert all(bits(d2[[3, 70, 900]]) == 0)
    # 64, 65, 500 and 1024 are all exactly h away from 63: the lowest j
    assert idx[63] == 64 and d2[63] == h2 and idx[64] == 63 and idx[65] == 63 and idx[500] == 63 and idx[1024] == 63
    assert np.all(d2[[64, 65, 500, 1024]] == h2)
    assert np.array_equal(ref.rows(pos, r2=h2)[2][[63, 64, 65, 500, 1024]], [4, 1, 1, 1, 1])
    # the NaN body is never chosen or counted, and finds nobody
    assert not np.any(idx == 200) and idx[200] == -1 and np.isposinf(d2[200]) and cnt[200] == 0
    assert np.all(np.delete(cnt, 200) == n - 2)
    assert ref.closest_pair(pos)[:2] == (3, 70) and bits(ref.closest_pair(pos)[2]) == 0
    # the points form: a point on a body finds it at +0 unless it is skipped
    pts = pos[[3, 63, 200]].copy()
    pts[2, :3] = 4.0   # body 63's position again
    pi, pd, pc = ref.points(pos, pts, r2=h2)
    assert list(pi) == [3, 63, 63] and np.all(bits(pd) == 0) and list(pc) == [3, 5, 5]
    pi, pd, pc = ref.points(pos, pts, np.array([3, 63, -1], np.int32), r2=h2)
    assert list(pi) == [70, 64, 63] and list(pd) == [0, h2, 0] and list(pc) == [2, 4, 5]
    # N = 1: nobody else
    one = pos[:1]
    assert [int(v[0]) for v in ref.rows(one, r2=r2)[::2]] == [-1, 0] and np.isposinf(ref.rows(one)[1][0])
    assert ref.closest_pair(one)[:2] == (-1, -1) and np.isposinf(ref.closest_pair(one)[2])
    assert ref.points(one, one)[0][0] == 0 and ref.points(one, one, np.zeros(1, np.int32))[0][0] == -1
