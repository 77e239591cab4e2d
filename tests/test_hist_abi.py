"""The radial-count entry points (nbody_radial_counts_rows, nbody_radial_counts, nbody_pair_histogram and their _d forms;
include/nbody.h "radial counts, pair histogram") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without
a context, and the CPU statement tests/hist_ref.c itself — against a plain numpy fp64 brute force, against tests/neighbors_ref.c's
radius count, the merging of bins, the pair histogram against the rows form, and planted systems whose answers are known by
construction (duplicates, exact ties on an edge, a NaN body)."""
import ctypes as C

import numpy as np
import pytest

import neighbors_common
from hist_common import count_edges, geom_edges, make_ref, numpy_d2, planted, r2_for, same
from test_knn_abi import queries_n300

SYMBOLS = {"nbody_radial_counts_rows": 5, "nbody_radial_counts_rows_d": 5, "nbody_radial_counts": 6, "nbody_radial_counts_d": 6,
           "nbody_pair_histogram": 3, "nbody_pair_histogram_d": 3}

# pairs that may stand too close to an edge to be compared (see test_hist_ref_against_numpy): of the 44 850 body-body pairs at most 1,
# of the 90 000 point-body pairs at most 2 (what is left out is 0 in every case but the ones the docstring names)
ROWS_CAP, POINTS_CAP = 1, 2


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("hist_ref"))


@pytest.fixture(scope="module")
def nref(tmp_path_factory):
    return neighbors_common.make_ref(tmp_path_factory.mktemp("neighbors_ref"))


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs, name
    assert callable(nb.NBody.radial_counts) and callable(nb.NBody.radial_counts_at) and callable(nb.NBody.pair_histogram)
    hdr = open(nb._lib.HERE + "/../include/nbody.h").read()
    assert "#define NBODY_HIST_MAX_BINS 32" in hdr and nb._lib.HIST_MAX_BINS == 32


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for sfx, dt, ct in (("", np.float32, C.c_float), ("_d", np.float64, C.c_double)):
        fp = lambda a: a.ctypes.data_as(C.POINTER(ct))
        pts, edges = np.zeros((4, 4), dt), np.array([0, 1, 2, 3], dt)
        counts, pairs = np.full((4, 3), 7, np.int32), np.full(3, 7, np.int64)
        assert getattr(lib, "nbody_radial_counts_rows" + sfx)(0, 4, fp(edges), 3, ip(counts)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_radial_counts" + sfx)(fp(pts), 4, None, fp(edges), 3, ip(counts)) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_pair_histogram" + sfx)(fp(edges), 3, pairs.ctypes.data_as(C.POINTER(C.c_longlong))) == nb._lib.ERR_NOT_INIT
        assert getattr(lib, "nbody_radial_counts" + sfx)(None, 4, None, None, 99, None) == nb._lib.ERR_NOT_INIT
        assert np.all(counts == 7) and np.all(pairs == 7)


@pytest.mark.parametrize("n_bins", [1, 4, 5, 8, 9, 16, 17, 31, 32])
def test_hist_ref_against_numpy(nb, ref, n_bins):
    """The statement's d2 carries at most five roundings relative to the exact value (tests/test_neighbors_abi.py derives it:
    |d2 - exact| <= 5 u d2, u = 2^-24 or 2^-53), so a pair whose fp64 d2 v is further than 10 u max(v, e) from an edge e — twice the
    bound, for the numpy side's own roundings — stands on the same side of e in both.  A pair takes part only if that holds for every
    edge; per bin the statement and numpy may then differ by at most the number of pairs left out at the bin's two edges.  The number
    left out is a condition, not a measurement: at most 1 of the 44 850 body-body pairs (0 in every case except fp32 at 31 bins, which
    loses 1) and at most 2 of the 90 000 point-body pairs (0 in every case except fp32 at 31 bins, which loses 2), printed and
    asserted."""
    n = 300
    for dtype, u in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -53)):
        pos, pts = queries_n300(nb, dtype)
        edges = geom_edges(n_bins, dtype)
        e64 = edges.astype(np.float64)
        for name, got, queries, sk, cap in (("rows", ref.rows(pos, edges), pos, np.arange(n), ROWS_CAP),
                                            ("points", ref.points(pos, pts, edges), pts, None, POINTS_CAP)):
            assert got.shape == (n, n_bins) and got.dtype == np.int32
            v = numpy_d2(pos, queries, sk)   # NaN where skipped: in no bin, near no edge
            with np.errstate(invalid="ignore"):
                near = np.stack([np.abs(v - e) <= 10 * u * np.maximum(v, e) for e in e64])   # (edges, m, N)
                unclear = near.any(0)
                left_out = int(np.triu(unclear, 1).sum()) if name == "rows" else int(unclear.sum())
                print("%s %s n_bins=%d: %d pairs left out" % (np.dtype(dtype).name, name, n_bins, left_out))
                assert left_out <= cap, (name, dtype, left_out)
                want = np.stack([((v >= e64[b]) & (v < e64[b + 1]) & ~unclear).sum(1) for b in range(n_bins)], axis=1)
            slack = np.stack([near[b].sum(1) + near[b + 1].sum(1) for b in range(n_bins)], axis=1)
            assert np.all(np.abs(got.astype(np.int64) - want) <= slack), (name, dtype)


def test_hist_ref_is_the_radius_count_of_neighbors_ref(nb, ref, nref):
    n = 300
    skip = np.full(n, -1, np.int32)
    skip[:3] = (0, 5, n - 1)
    skip[10::3] = (np.arange(10, n, 3) * 7919) % n
    for dtype in (np.float32, np.float64):
        pos, pts = queries_n300(nb, dtype)
        pts[:3] = pos[[0, 5, n - 1]]
        for r2 in (dtype(0), r2_for(pos, 0.01), r2_for(pos, 0.3), dtype(12.5)):
            e = count_edges(r2, dtype)
            assert same(ref.rows(pos, e)[:, 0], nref.rows(pos, r2=r2)[2]), r2
            assert same(ref.rows(pos, e, 17, 100)[:, 0], nref.rows(pos, 17, 100, r2=r2)[2]), r2
            assert same(ref.points(pos, pts, e)[:, 0], nref.points(pos, pts, r2=r2)[2]), r2
            assert same(ref.points(pos, pts, e, skip)[:, 0], nref.points(pos, pts, skip, r2=r2)[2]), r2


def test_a_bin_that_merges_bins_holds_their_sum(nb, ref):
    n = 300
    for dtype in (np.float32, np.float64):
        pos, pts = queries_n300(nb, dtype)
        edges = geom_edges(32, dtype)
        for call in (lambda e: ref.rows(pos, e), lambda e: ref.points(pos, pts, e), lambda e: ref.pairs(pos, e)):
            fine = call(edges)
            for keep in [np.arange(0, 33, s) for s in (2, 4, 8, 16, 32)] + [np.array([0, 1, 2, 7, 8, 19, 31, 32])]:
                merged = np.stack([fine[..., a:b].sum(-1) for a, b in zip(keep[:-1], keep[1:])], axis=-1)
                assert same(call(edges[keep]), merged.astype(fine.dtype)), keep


def test_pair_hist_is_half_the_column_sums_of_the_rows(nb, ref):
    n = 300
    for dtype in (np.float32, np.float64):
        pos = queries_n300(nb, dtype)[0]
        for edges in (geom_edges(32, dtype), geom_edges(5, dtype), np.array([0, np.inf], dtype)):
            twice = ref.rows(pos, edges).astype(np.int64).sum(0)
            assert np.all(twice % 2 == 0)
            assert same(ref.pairs(pos, edges), twice // 2)
        assert list(ref.pairs(pos, np.array([0, np.inf], dtype))) == [n * (n - 1) // 2]


def check_planted(rows, at, pos):
    """the assertions on a planted system, for the statement (here) and the device (test_gpu_hist.py): rows(edges) and
    at(points, edges, skip) give the counts"""
    n, dtype = len(pos), pos.dtype.type
    h2 = dtype(2.0 ** -24)
    edges = np.array([0, h2, np.nextafter(h2, dtype(np.inf)), 1, np.inf], dtype)
    c = rows(edges)
    assert list(c[63, :2]) == [0, 4]           # 64, 65, 500 and 1024 are exactly h away: in [h2, next), not in [0, h2)
    for i in (3, 70, 900):
        assert c[i, 0] == 2                    # the two other bodies on body 3's position, at +0
    assert np.all(c[200] == 0)                 # the NaN body counts nobody
    others = np.delete(np.arange(n), 200)
    assert np.all(c[others].sum(1) == n - 2)   # and nobody counts it
    pts = pos[[3]].copy()
    assert at(pts, edges, None)[0, 0] == 3                         # a point on body 3: 3, 70 and 900 at +0
    assert at(pts, edges, np.array([3], np.int32))[0, 0] == 2      # without body 3


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_cases(nb, ref, dtype):
    pos = planted(nb, 1100, dtype)
    check_planted(lambda e: ref.rows(pos, e), lambda pts, e, sk: ref.points(pos, pts, e, sk), pos)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_small_and_degenerate_cases(nb, ref, dtype):
    pos = queries_n300(nb, dtype)[0]
    one = pos[:1]
    e = geom_edges(5, dtype)
    assert np.all(ref.rows(one, e) == 0) and np.all(ref.pairs(one, e) == 0)
    assert np.all(ref.points(one, one, np.array([0, np.inf], dtype)) == 1)
    # equal edges: an empty bin between them, the others as without it
    a = ref.rows(pos, np.array([0, 0.5, 0.5, 2], dtype))
    b = ref.rows(pos, np.array([0, 0.5, 2], dtype))
    assert np.all(a[:, 1] == 0) and same(a[:, [0, 2]], b) and b.sum() > 0
    # edges entirely below and entirely above every distance
    assert np.all(ref.rows(pos, np.array([-3, -2, -1, -0.0], dtype)) == 0)
    assert np.all(ref.rows(pos, np.array([100, 200, np.inf], dtype)) == 0)
    assert np.all(ref.pairs(pos, np.array([100, 200, np.inf], dtype)) == 0)
