"""Radial counts and the pair histogram on the device (nbody_radial_counts_rows, nbody_radial_counts, nbody_pair_histogram and their _d
forms; include/nbody.h "radial counts, pair histogram"): every case bit for bit against tests/hist_ref.c — integers equal — in both
precisions, for n_bins on both sides of every capacity, in both loop forms, however the work is laid out (source split, batches,
windows of rows, force configuration, device and process count); one bin is the neighbour pass's radius count; 64-bit totals known by
construction; no effect on the step; the guards; the C host program's line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hist_common import BINS, count_edges, geom_edges, make_points, make_ref, make_skip, planted, r2_for, radius_edges, same
from pass_common import FORCE_CONFIGS, check_step_untouched
from ranks_common import ROOT, run_ranks, shared_gpu_env, worker_source
from specials_common import (HOSTILE_BINS, POINT_COUNTS, SIZES, VARIANTS, hand_made_distances, hostile_distance_system, hostile_edges,
                             hostile_points, hostile_radii)
from test_gpu_neighbors import windows
from test_hist_abi import check_planted

pytestmark = pytest.mark.gpu
ENV = ("NBODY_HIST_SPLIT", "NBODY_HIST_SCRATCH_MB", "NBODY_HIST_LOOP", "NBODY_NEIGHBORS_SPLIT", "NBODY_NEIGHBORS_SCRATCH_MB",
       "NBODY_NEIGHBORS_LOOP")
LOOPS = ("1", "2")   # NBODY_HIST_LOOP: the scan, the gated form


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("hist_ref"))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def edge_sets(pos):
    """the geometric edges for every n_bins of BINS — both sides of every capacity — and the edges from the radii of the neighbour tests"""
    dtype = pos.dtype.type
    return [geom_edges(b, dtype) for b in BINS] + [radius_edges(pos)]


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("fp64", [False, True])
def test_rows_and_pairs_bit_for_bit(nb, ref, monkeypatch, fp64, loop):
    monkeypatch.setenv("NBODY_HIST_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    for n in (1, 2, 63, 64, 65, 257, 1000, 1025, 2100):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for edges in edge_sets(pos):
                want = ref.rows(pos, edges)
                for first, cnt in windows(n):
                    assert same(eng.radial_counts(edges, first, cnt), want[first:first + cnt]), (n, len(edges), first, cnt)
                assert same(eng.pair_histogram(edges), ref.pairs(pos, edges)), (n, len(edges))
            if n > 1:
                assert np.all(eng.radial_counts(radius_edges(pos)).sum(1) == n - 1)   # [0, +inf) holds every other body


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("fp64", [False, True])
def test_points_form(nb, ref, monkeypatch, fp64, loop):
    monkeypatch.setenv("NBODY_HIST_LOOP", loop)
    n = 2100
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        for m in (1, 255, 256, 257):
            pts, on = make_points(nb, pos, m)   # on bodies 0, 5, N - 1; between the bodies; 1.5 x: outside the cube
            pts[-1, :3] = 50.0                  # and far outside
            spread = ((np.arange(m) * 997) % n).astype(np.int32)   # skip indices across all blocks: the compare window spans the sources
            for skip in (None, make_skip(n, m, on), spread):
                for edges in (geom_edges(1, dtype), geom_edges(5, dtype), geom_edges(32, dtype), radius_edges(pos)):
                    assert same(eng.radial_counts_at(pts, edges, skip), ref.points(pos, pts, edges, skip)), (m, skip is not None, len(edges))
            e9 = geom_edges(9, dtype)
            assert same(eng.radial_counts_at(np.ascontiguousarray(pts[:, :3]), e9), ref.points(pos, pts, e9))   # (m, 3) points are padded
        e17 = geom_edges(17, dtype)
        assert same(eng.radial_counts_at(pos, e17, np.arange(n, dtype=np.int32)), eng.radial_counts(e17))
        with pytest.raises(ValueError):
            eng.radial_counts_at(pts[:, :2], e9)
        with pytest.raises(ValueError):
            eng.radial_counts_at(pts, e9, spread[:-1])
        for bad in ([1.0], np.arange(34.0), [0.0, np.nan], [0.0, 2.0, 1.0]):
            for call in (eng.radial_counts, eng.pair_histogram, lambda e: eng.radial_counts_at(pts, e)):
                with pytest.raises(ValueError):
                    call(bad)


@pytest.mark.parametrize("fp64", [False, True])
def test_one_bin_is_the_neighbour_pass_count(nb, monkeypatch, fp64):
    dtype = np.float64 if fp64 else np.float32
    n, m = 2100, 257
    pos = nb.make_bodies(n, dtype=dtype)[0]
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, np.zeros_like(pos))
        for loop in LOOPS:
            monkeypatch.setenv("NBODY_HIST_LOOP", loop)
            for r2 in (dtype(0), r2_for(pos, 0.01), r2_for(pos, 0.3), dtype(12.5)):
                e = count_edges(r2, dtype)
                assert same(eng.radial_counts(e)[:, 0], eng.neighbors(r2=r2)[2]), (loop, r2)
                for sk in (None, skip):
                    assert same(eng.radial_counts_at(pts, e, sk)[:, 0], eng.nearest(pts, sk, r2=r2)[2]), (loop, r2)


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system(nb, ref, monkeypatch, fp64, loop):
    """specials_common.hostile_distance_system integer for integer against hist_ref.c with the edges of hostile_edges — a first edge of
    -inf or 0, an empty bin at 0, a subnormal edge between the planted pair's d2 and its d2 to the bodies at zero, the smallest normal,
    the largest finite (which a d2 that overflowed is not below) and +inf (nor below that) — at 3, 9, 17 and 32 bins (binary32: the
    edges in SGPRs and in VGPRs), in both loop forms, every split (3 puts 1023 and 1024 in different chunks), windows of rows, the
    points form; the pair histogram is half the rows' sums; one bin is the neighbour pass's count at every finite radius."""
    monkeypatch.setenv("NBODY_HIST_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_distance_system(nb, n, dtype, variant)
            edges = [hostile_edges(pos, b) for b in HOSTILE_BINS]
            want_rows = [ref.rows(pos, e) for e in edges]
            want_pairs = [ref.pairs(pos, e) for e in edges]
            queries = [(pts, sk) for m in POINT_COUNTS for pts, skip in [hostile_points(nb, pos, m, variant)] for sk in (skip, None)]
            want_points = [[ref.points(pos, pts, e, sk) for e in edges] for pts, sk in queries]
            for e, rows, pairs in zip(edges, want_rows, want_pairs):
                assert np.array_equal(rows.astype(np.int64).sum(0), 2 * pairs) and not np.any(rows[:, e[:-1] == e[1:]])
                if variant in ("overflow", "inf"):
                    assert rows[0].sum() < n - 1 and not np.any(rows[63, :-2])   # a +inf d2 is in no bin, not even one that ends at +inf
            with nb.NBody(n, fp64=fp64) as eng:
                eng.upload(pos, vel)
                for split in (None, "1", "2", "3"):
                    if split:
                        monkeypatch.setenv("NBODY_HIST_SPLIT", split)
                    tag = (n, variant, split)
                    for e, rows, pairs in zip(edges, want_rows, want_pairs):
                        for first, cnt in windows(n):
                            assert same(eng.radial_counts(e, first, cnt), rows[first:first + cnt]), tag + (len(e), first)
                        assert same(eng.pair_histogram(e), pairs), tag + (len(e),)
                    for (pts, sk), wants in zip(queries, want_points):
                        for e, want in zip(edges, wants):
                            assert same(eng.radial_counts_at(pts, e, sk), want), tag + (len(e), len(pts), sk is not None)
                monkeypatch.delenv("NBODY_HIST_SPLIT")
                pts, skip = queries[-2]
                for r2 in hostile_radii(pos)[:-1]:   # every finite one: 0, a subnormal, the smallest normal, an ordinary one, the largest
                    with np.errstate(over="ignore"):   # the largest finite radius: the edge above it is +inf
                        e = count_edges(r2, dtype)
                    assert same(eng.radial_counts(e)[:, 0], eng.neighbors(r2=r2)[2]), (n, variant, r2)
                    for sk in (None, skip):
                        assert same(eng.radial_counts_at(pts, e, sk)[:, 0], eng.nearest(pts, sk, r2=r2)[2]), (n, variant, r2)
                if variant in ("overflow", "inf"):   # ... and at r2 = +inf the count takes the +inf d2 that no edge does
                    assert eng.neighbors(0, 1, r2=dtype(np.inf))[2][0] == n - 1 > eng.radial_counts(edges[-1], 0, 1).sum()


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("fp64", [False, True])
def test_hand_made_specials(nb, ref, monkeypatch, fp64, loop):
    """two- and three-body systems whose counts are known by construction (specials_common.hand_made_distances)"""
    monkeypatch.setenv("NBODY_HIST_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    systems, v = hand_made_distances(dtype)
    inf, above = v.inf, lambda x: np.nextafter(dtype(x), dtype(np.inf))
    cases = {   # name: (edges, counts per row)
        "alone": ([-inf, 0, v.max, inf], [[0, 0, 0]]),
        "coincident": ([-inf, 0, v.sub, inf], [[0, 1, 0]] * 2),            # +0 is in the bin that holds 0
        "underflow": ([0, 0, v.sub, inf], [[0, 1, 0]] * 2),
        "subnormal": ([0, v.sub, v.h2, above(v.h2), inf], [[0, 0, 1, 0]] * 2),   # not below its own value, below the next one
        "overflow": ([0, 9, above(9), v.max, inf], [[0, 1, 0, 0], [0, 0, 0, 0], [0, 1, 0, 0]]),
        "nan": ([-inf, 0, 9, above(9), inf], [[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, 0]]),
        "inf": ([0, above(9), v.max, inf], [[1, 0, 0], [0, 0, 0], [1, 0, 0]]),
        "two_inf": ([-inf, v.max, inf], [[0, 0]] * 3),
        "tied": ([0, 2, above(2)], [[0, 2]] * 3)}
    assert set(cases) == set(systems)
    for name, (edges, counts) in cases.items():
        pos = systems[name]
        e, want = np.array(edges, dtype), np.array(counts, np.int32)
        with nb.NBody(len(pos), fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            got = eng.radial_counts(e)
            assert same(got, want) and same(got, ref.rows(pos, e)), name
            assert same(eng.radial_counts_at(pos, e, np.arange(len(pos), dtype=np.int32)), want), name
            assert same(eng.radial_counts_at(pos, e), ref.points(pos, pos, e)), name
            pairs = eng.pair_histogram(e)
            assert same(pairs, want.astype(np.int64).sum(0) // 2) and same(pairs, ref.pairs(pos, e)), name


@pytest.mark.parametrize("loop", LOOPS)
@pytest.mark.parametrize("fp64", [False, True])
def test_planted_system(nb, ref, monkeypatch, fp64, loop):
    monkeypatch.setenv("NBODY_HIST_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    n = 2100
    pos = planted(nb, n, dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, np.zeros_like(pos))
        for split in (None, "3"):   # three chunks of one block: the tie at 1024 sits in another chunk than 63's other ties
            if split:
                monkeypatch.setenv("NBODY_HIST_SPLIT", split)
            check_planted(eng.radial_counts, eng.radial_counts_at, pos)
            for edges in (geom_edges(32, dtype), radius_edges(pos)):
                assert same(eng.radial_counts(edges), ref.rows(pos, edges)), split
                assert same(eng.pair_histogram(edges), ref.pairs(pos, edges)), split


def test_values_do_not_follow_the_arithmetic(nb, ref):
    n = 2100
    pos, vel = nb.make_bodies(n)
    edges = geom_edges(9, np.float32)
    want = ref.rows(pos, edges)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for arith in (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT):
            eng.set_option(nb.OPT_ARITH, arith)
            assert same(eng.radial_counts(edges), want), arith
            assert same(eng.pair_histogram(edges), ref.pairs(pos, edges)), arith


@pytest.mark.parametrize("loop", LOOPS)
def test_values_do_not_depend_on_the_source_split_or_the_batches(nb, ref, monkeypatch, loop):
    monkeypatch.setenv("NBODY_HIST_LOOP", loop)
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for n_bins in (5, 32):
            e = geom_edges(n_bins, np.float32)
            want = (ref.points(pos, pts, e), ref.points(pos, pts, e, skip), ref.rows(pos, e, 100, m), ref.pairs(pos, e))
            calls = lambda: (eng.radial_counts_at(pts, e), eng.radial_counts_at(pts, e, skip), eng.radial_counts(e, 100, m), eng.pair_histogram(e))
            for split in (None, "1", "2", "3", "64"):
                if split:
                    monkeypatch.setenv("NBODY_HIST_SPLIT", split)
                for g_, w in zip(calls(), want):
                    assert same(g_, w), (n_bins, split)
            # a bound of 6000 n_bins bytes.  Queries: 5 chunks x n_bins x 4 B = 20 n_bins B a query, 300 fit, whole workgroups: batches
            # of 256 + 256 + 188.  Pair histogram: n_bins x 4 B a row, 1500 fit, 1280 rows a batch: four batches through the reduction,
            # each of them split again into launches of 256 queries.
            monkeypatch.setenv("NBODY_HIST_SCRATCH_MB", repr(6000.0 * n_bins / 1048576.0))
            for split in ("5", None):
                if split:
                    monkeypatch.setenv("NBODY_HIST_SPLIT", split)
                else:
                    monkeypatch.delenv("NBODY_HIST_SPLIT")
                for g_, w in zip(calls(), want):
                    assert same(g_, w), (n_bins, "batches", split)
            monkeypatch.setenv("NBODY_HIST_SPLIT", "5")
            monkeypatch.setenv("NBODY_HIST_SCRATCH_MB", "0")   # not even one workgroup's queries fit: no split; 256 rows a reduction
            for g_, w in zip(calls(), want):
                assert same(g_, w), (n_bins, "no scratch")
            monkeypatch.delenv("NBODY_HIST_SPLIT")
            monkeypatch.delenv("NBODY_HIST_SCRATCH_MB")


def test_values_do_not_depend_on_the_queries_beside_a_query_or_the_force_configuration(nb, ref):
    n, m = 5000, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    e = geom_edges(9, np.float32)
    perm = np.random.default_rng(5).permutation(m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        a, rows, pairs = eng.radial_counts_at(pts, e, skip), eng.radial_counts(e), eng.pair_histogram(e)
        assert same(a, ref.points(pos, pts, e, skip)) and same(rows, ref.rows(pos, e)) and same(pairs, ref.pairs(pos, e))
        for sel in (slice(0, 1), slice(100, 357), slice(699, 700), slice(63, 129), perm):
            assert same(eng.radial_counts_at(pts[sel], e, skip[sel]), a[sel]), sel
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            assert same(eng.radial_counts_at(pts, e, skip), a) and same(eng.radial_counts(e), rows) and same(eng.pair_histogram(e), pairs), (key, val)
            eng.set_option(key, default)


def test_values_do_not_depend_on_the_device_count(nb, ref, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n, m = 1500, 300   # 1500 = 500 x 3: slices that end inside a 64-source window and inside a workgroup's rows
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    e = geom_edges(9, np.float32)
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            res[ngpus] = (eng.radial_counts(e), eng.radial_counts(e, 450, 600), eng.radial_counts_at(pts, e, skip), eng.pair_histogram(e),
                          eng.download()[0])
    now = res[1][4]
    assert same(now, res[3][4]) and not same(now, pos), "the two states differ, or no drift happened"
    want = ref.rows(now, e)
    for g in (1, 3):
        assert same(res[g][0], want), g
        assert same(res[g][1], want[450:1050]), g   # a window across both device boundaries
        assert same(res[g][2], ref.points(now, pts, e, skip)), g
        assert same(res[g][3], ref.pairs(now, e)), g


WORKER = """
    from field_common import make_points, make_skip
    from hist_common import geom_edges
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m, n_bins = (300, 41)[rank], (5, 32)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    counts = eng.radial_counts_at(pts, geom_edges(n_bins, np.float32), make_skip(n, m, on))
    rows = eng.radial_counts(geom_edges(9, np.float32))          # this rank's own rows
    pairs = eng.pair_histogram(geom_edges(17, np.float32))       # collective: the same values on every rank
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, counts=counts, rows=rows, pairs=pairs,
             first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p)
"""


def test_two_processes_host_transport_equal_one_process(nb, ref, tmp_path):
    n, world = 1500, 2
    out = str(tmp_path / "hist")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now = got[0]["pos"]
    assert same(now, got[1]["pos"])
    pos, vel = nb.make_bodies(n, seed=33)
    want_rows = ref.rows(now, geom_edges(9, np.float32))
    covered = 0
    for r, (m, n_bins) in enumerate(((300, 5), (41, 32))):
        g_ = got[r]
        pts, on = make_points(nb, pos, m, seed=50 + r)
        assert same(g_["counts"], ref.points(now, pts, geom_edges(n_bins, np.float32), make_skip(n, m, on))), r
        first, cnt = (int(v) for v in g_["first"])
        assert same(g_["rows"], want_rows[first:first + cnt]), r
        covered += cnt
    assert covered == n
    e17 = geom_edges(17, np.float32)
    with nb.NBody(n) as eng:
        eng.upload(now, vel)   # the ranks' state: the steps of two ranks sum the forces in another order than one process does
        one = eng.pair_histogram(e17)
    assert same(got[0]["pairs"], got[1]["pairs"]) and same(got[0]["pairs"], one) and same(one, ref.pairs(now, e17))


def test_totals_beyond_32_bits(nb):
    """known by construction, no CPU reference: N = 70 000 has 2 449 965 000 pairs, more than 2^31, and the rows' sum before the halving
    is more than 2^32"""
    n = 70000
    pos, vel = nb.make_bodies(n)
    total = n * (n - 1) // 2
    assert total > 2 ** 31 and 2 * total > 2 ** 32
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        pairs = eng.pair_histogram([0, np.inf])
        assert pairs.dtype == np.int64 and list(pairs) == [total]
        x = r2_for(pos, 0.3)
        two = eng.pair_histogram([0, x, np.inf])
        assert int(two.sum()) == total and 0 < two[0] < total
        for first in (0, 35000, n - 1):
            assert int(eng.radial_counts([0, x, np.inf], first, 1).sum()) == n - 1


def test_hist_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, on = make_points(nb, nb.make_bodies(n)[0], 300)
    e5, e17 = geom_edges(5, np.float32), geom_edges(17, np.float32)
    probe = lambda eng: (eng.radial_counts(e5), eng.radial_counts_at(pts, e17, make_skip(n, 300, on)), eng.pair_histogram(e5))
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_HIST_SPLIT")


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_longlong))
    pts, pts64 = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float64)
    e32, e64 = np.array([0, 1, 2, 3], np.float32), np.array([0, 1, 2, 3], np.float64)
    counts, pairs = np.full((4, 3), 7, np.int32), np.full(3, 7, np.int64)
    sk = np.array([-1, 0, 3, 2], np.int32)
    calls32 = (lambda: lib.nbody_radial_counts_rows(0, 4, e32.ctypes.data_as(f32), 3, ip(counts)),
               lambda: lib.nbody_radial_counts(pts.ctypes.data_as(f32), 4, ip(sk), e32.ctypes.data_as(f32), 3, ip(counts)),
               lambda: lib.nbody_pair_histogram(e32.ctypes.data_as(f32), 3, lp(pairs)))
    calls64 = (lambda: lib.nbody_radial_counts_rows_d(0, 4, e64.ctypes.data_as(f64), 3, ip(counts)),
               lambda: lib.nbody_radial_counts_d(pts64.ctypes.data_as(f64), 4, ip(sk), e64.ctypes.data_as(f64), 3, ip(counts)),
               lambda: lib.nbody_pair_histogram_d(e64.ctypes.data_as(f64), 3, lp(pairs)))
    untouched = lambda: np.all(counts == 7) and np.all(pairs == 7)
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [c() for c in calls32 + calls64] == [E.ERR_STATE] * 6
        finally:
            mb.serve(False)
        assert untouched()
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        assert [c() for c in calls64] == [E.ERR_STATE] * 3 and untouched()
        c_, x, e_ = ip(counts), pts.ctypes.data_as(f32), e32.ctypes.data_as(f32)
        # a NULL output, edges2 or points
        assert lib.nbody_radial_counts_rows(0, 4, e_, 3, None) == E.ERR_ARG
        assert lib.nbody_radial_counts_rows(0, 4, None, 3, c_) == E.ERR_ARG
        assert lib.nbody_radial_counts(x, 4, None, e_, 3, None) == E.ERR_ARG
        assert lib.nbody_radial_counts(x, 4, None, None, 3, c_) == E.ERR_ARG
        assert lib.nbody_radial_counts(None, 4, None, e_, 3, c_) == E.ERR_ARG
        assert lib.nbody_pair_histogram(e_, 3, None) == E.ERR_ARG
        assert lib.nbody_pair_histogram(None, 3, lp(pairs)) == E.ERR_ARG
        # n_bins outside 1 .. 32 (the edges are not read)
        for b in (0, -1, 33, 1 << 30):
            assert lib.nbody_radial_counts_rows(0, 4, e_, b, c_) == E.ERR_ARG, b
            assert lib.nbody_radial_counts(x, 4, None, e_, b, c_) == E.ERR_ARG, b
            assert lib.nbody_pair_histogram(e_, b, lp(pairs)) == E.ERR_ARG, b
        # a NaN or a descending edge
        for bad in ((0, np.nan, 2, 3), (np.nan, 1, 2, 3), (0, 1, 2, np.nan), (0, 2, 1, 3), (1, 0, 2, 3), (0, 1, 3, 2), (np.inf, 1, 2, 3)):
            b32 = np.array(bad, np.float32)
            b_ = b32.ctypes.data_as(f32)
            assert lib.nbody_radial_counts_rows(0, 4, b_, 3, c_) == E.ERR_ARG, bad
            assert lib.nbody_radial_counts(x, 4, None, b_, 3, c_) == E.ERR_ARG, bad
            assert lib.nbody_pair_histogram(b_, 3, lp(pairs)) == E.ERR_ARG, bad
        # a bad row range, m < 1, a skip value outside [-1, N)
        for first, rows in ((-1, 4), (0, 0), (0, -2), (97, 4), (100, 1), (0, 101), (1 << 30, 1 << 30)):
            assert lib.nbody_radial_counts_rows(first, rows, e_, 3, c_) == E.ERR_ARG, (first, rows)
        assert lib.nbody_radial_counts(x, 0, None, e_, 3, c_) == E.ERR_ARG
        assert lib.nbody_radial_counts(x, -3, None, e_, 3, c_) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_radial_counts(x, 4, ip(sk), e_, 3, c_) == E.ERR_ARG, bad
        assert untouched()
        # legal: equal edges, a last edge of +inf, -inf first
        sk[:] = (-1, 0, n - 1, n - 1)
        ok = np.array([-np.inf, 0, 0, np.inf], np.float32)
        assert lib.nbody_radial_counts(x, 4, ip(sk), ok.ctypes.data_as(f32), 3, c_) == 0 and not np.any(counts == 7)
        assert np.all(counts[:, :2] == 0) and list(counts[:, 2]) == [n, n - 1, n - 1, n - 1]
        assert lib.nbody_radial_counts_rows(96, 4, e_, 3, c_) == 0 and same(counts, eng.radial_counts(e32)[96:])
        assert lib.nbody_pair_histogram(e_, 3, lp(pairs)) == 0 and same(pairs, eng.pair_histogram(e32))
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert [c() for c in calls32] == [E.ERR_STATE] * 3 and [c() for c in calls64] == [0] * 3


def test_c_host_program_pair_histogram_line(nb, ref):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters, bins = 4096, 3, 8
    for flags, fp64 in (([], False), (["--fp64"], True)):
        r = subprocess.run([exe, str(n), str(iters), "--pair-histogram", str(bins)] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = re.findall(r"^pair histogram:((?: \d+)+)$", r.stdout, flags=re.M)
        assert len(lines) == 1, r.stdout
        plain = subprocess.run([exe, str(n), str(iters)] + flags, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0 and "histogram" not in plain.stdout
        strip = lambda text: [ln for ln in text.splitlines() if "Billion Interactions" not in ln and not ln.startswith("pair histogram")]
        assert strip(r.stdout) == strip(plain.stdout)   # nothing else changes (the rate line carries a time)
        dtype = np.float64 if fp64 else np.float32
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            eng.step(float(np.float32(0.01)), iters)   # the program's dt is the binary32 0.01 in fp64 contexts too
            now = eng.download()[0]
        edges = np.array([0] + [2.0 ** (2 * (b - bins) + 4) for b in range(1, bins + 1)], dtype)
        assert edges[-1] == 16
        assert [int(v) for v in lines[0].split()] == list(ref.pairs(now, edges))
    assert subprocess.run([exe, str(n), str(iters), "--pair-histogram", "33"], capture_output=True, text=True, timeout=60).returncode == 2
