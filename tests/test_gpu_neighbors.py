"""Nearest neighbour, radius count and closest pair on the device (nbody_neighbors_rows, nbody_nearest, nbody_closest_pair and their
_d forms; include/nbody.h "nearest neighbour, radius count, closest pair"): every case bit for bit against tests/neighbors_ref.c — idx
and count equal, d2 the same bits — in both precisions, in every arithmetic, both loop forms, however the work is laid out (source
split, batches, windows of rows, force configuration, device and process count); no effect on the step; the guards; the C host
program's --closest-pair line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from field_common import make_points, make_skip
from neighbors_common import bits, make_ref, planted, r2_for, same
from pass_common import FORCE_CONFIGS, check_step_untouched
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import (POINT_COUNTS, SIZES, VARIANTS, hand_made_distances, hostile_distance_system, hostile_points, hostile_radii,
                             same_nan)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("NBODY_NEIGHBORS_SPLIT", "NBODY_NEIGHBORS_SCRATCH_MB", "NBODY_NEIGHBORS_LOOP")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("neighbors_ref"))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def windows(n):
    """(first_row, n_rows): everything, a window across a 64 boundary and across a 256 boundary, the last row alone"""
    w = [(0, n), (n - 1, 1)]
    if n > 70:
        w.append((50, 20))
    if n > 300:
        w.append((200, 100))
    return w


@pytest.mark.parametrize("loop", ["1", "2"])
@pytest.mark.parametrize("fp64", [False, True])
def test_rows_bit_for_bit(nb, ref, monkeypatch, fp64, loop):
    monkeypatch.setenv("NBODY_NEIGHBORS_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    for n in (1, 2, 63, 64, 65, 257, 1000, 1025, 2100):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for r2 in (None, dtype(0), r2_for(pos, 0.01), r2_for(pos, 0.3), dtype(12.5)):   # counts from 0 to all of the others
                want = ref.rows(pos, r2=r2)
                if r2 is not None and r2 == 12.5:
                    assert np.all(want[2] == n - 1)
                for first, cnt in windows(n):
                    got = eng.neighbors(first, cnt, r2=r2)
                    assert same(got, tuple(None if w is None else w[first:first + cnt] for w in want)), (n, first, cnt, r2)
            assert same(eng.neighbors(), ref.rows(pos))
            assert eng.closest_pair()[:2] == ref.closest_pair(pos)[:2] and bits(eng.closest_pair()[2]) == bits(ref.closest_pair(pos)[2]), n


def test_bits_do_not_follow_the_arithmetic(nb, ref):
    n = 2100
    pos, vel = nb.make_bodies(n)
    r2 = r2_for(pos, 0.1)
    want = ref.rows(pos, r2=r2)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT):
            eng.set_option(nb.OPT_ARITH, mode)
            assert same(eng.neighbors(r2=r2), want), mode


@pytest.mark.parametrize("fp64", [False, True])
def test_points_form(nb, ref, fp64):
    n = 2100
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    r2 = r2_for(pos, 0.05)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        for m in (1, 255, 256, 257):
            pts, on = make_points(nb, pos, m)   # on bodies 0, 5, N - 1; between the bodies; 1.5 x: outside the cube
            pts[-1, :3] = 50.0                  # and far outside
            spread = ((np.arange(m) * 997) % n).astype(np.int32)   # skip indices across all blocks: the compare window spans the sources
            for skip in (None, make_skip(n, m, on), spread):
                for rr in (None, r2):
                    assert same(eng.nearest(pts, skip, r2=rr), ref.points(pos, pts, skip, r2=rr)), (m, skip is not None, rr)
            assert same(eng.nearest(np.ascontiguousarray(pts[:, :3])), ref.points(pos, pts))   # (m, 3) points are padded to words
        got = eng.nearest(pts[:3])
        assert list(got[0]) == on and np.all(bits(got[1]) == 0)   # a point on a body without a skip: that body at +0
        assert same(eng.nearest(pos, np.arange(n, dtype=np.int32), r2=r2), eng.neighbors(r2=r2))


@pytest.mark.parametrize("loop", ["1", "2"])
@pytest.mark.parametrize("fp64", [False, True])
def test_ties_and_specials(nb, ref, monkeypatch, fp64, loop):
    monkeypatch.setenv("NBODY_NEIGHBORS_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    n = 2100
    pos = planted(nb, n, dtype)
    vel = np.zeros_like(pos)
    h2 = dtype(2.0 ** -24)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        for split in (None, "3"):   # three chunks of one block: the tie at 1024 sits in another chunk than 63's other ties
            if split:
                monkeypatch.setenv("NBODY_NEIGHBORS_SPLIT", split)
            idx, d2, cnt = got = eng.neighbors(r2=h2)
            assert same(got, ref.rows(pos, r2=h2)), split
            assert (idx[3], idx[70], idx[900]) == (70, 3, 3) and np.all(bits(d2[[3, 70, 900]]) == 0)
            assert idx[63] == 64 and d2[63] == h2 and list(cnt[[63, 64, 65, 500, 1024]]) == [4, 1, 1, 1, 1]
            assert idx[200] == -1 and np.isposinf(d2[200]) and cnt[200] == 0 and not np.any(idx == 200)
            pts = pos[[3, 63, 200, 63]].copy()
            pts[2, :3] = 4.0
            sk = np.array([3, 63, -1, 64], np.int32)
            assert same(eng.nearest(pts, sk, r2=h2), ref.points(pos, pts, sk, r2=h2)), split
            assert list(eng.nearest(pts, sk)[0]) == [70, 64, 63, 63]
            assert eng.closest_pair()[:2] == (3, 70) and bits(eng.closest_pair()[2]) == 0
    one = pos[:1]
    with nb.NBody(1, fp64=fp64) as eng:
        eng.upload(one, vel[:1])
        idx, d2, cnt = eng.neighbors(r2=dtype(1e30))
        assert idx[0] == -1 and np.isposinf(d2[0]) and cnt[0] == 0
        i, j, d = eng.closest_pair()
        assert (i, j) == (-1, -1) and np.isposinf(d)
        assert eng.nearest(one)[0][0] == 0 and eng.nearest(one, np.zeros(1, np.int32))[0][0] == -1


def agree(got, want):
    """(idx, d2, count) against the reference's: the integers equal, the floats with the same NaN mask and the same bits elsewhere"""
    return np.array_equal(got[0], want[0]) and same_nan(got[1], want[1]) and np.array_equal(got[2], want[2])


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system(nb, ref, monkeypatch, fp64):
    """specials_common.hostile_distance_system — a subnormal d2 across the 63 | 64 window edge, d2 = +0 between distinct bodies, d2
    that overflows for all partners but one, inf - inf, the NaN body, the coincident group across the 1023 | 1024 edge — bit for bit
    against neighbors_ref.c: both loop forms, every split (3 puts 1023 and 1024 in different chunks), windows of rows, the points
    form with and without skip, every radius of hostile_radii (0, a subnormal, the smallest normal, an ordinary one, the largest finite,
    +inf), the closest pair.  What the reference itself is worth there: tests/test_specials_distance_reference.py."""
    dtype = np.float64 if fp64 else np.float32
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_distance_system(nb, n, dtype, variant)
            radii = hostile_radii(pos)
            want_rows = [ref.rows(pos, r2=r2) for r2 in radii]
            queries = [(pts, sk) for m in POINT_COUNTS for pts, skip in [hostile_points(nb, pos, m, variant)] for sk in (skip, None)]
            want_points = [[ref.points(pos, pts, sk, r2=r2) for r2 in radii] for pts, sk in queries]
            want_pair = ref.closest_pair(pos)
            idx, d2, cnt = want_rows[-1]
            assert not np.any(np.isnan(d2)) and (idx[62], idx[65]) == (65, 62) and 0 < d2[62] < np.finfo(dtype).tiny   # a NaN is never chosen
            if variant == "overflow":
                assert (idx[63], idx[66]) == (66, 63) and np.isfinite(d2[63]) and cnt[0] == n - 1
            if variant == "inf":
                assert idx[63] == idx[66] == -1 and cnt[63] == n - 2 and cnt[0] == n - 1
            with nb.NBody(n, fp64=fp64) as eng:
                eng.upload(pos, vel)
                for loop in ("1", "2"):
                    monkeypatch.setenv("NBODY_NEIGHBORS_LOOP", loop)
                    for split in (None, "1", "2", "3"):
                        if split:
                            monkeypatch.setenv("NBODY_NEIGHBORS_SPLIT", split)
                        tag = (n, variant, loop, split)
                        for r2, want in zip(radii, want_rows):
                            for first, rows in windows(n):
                                assert agree(eng.neighbors(first, rows, r2=r2), tuple(w[first:first + rows] for w in want)), tag + (r2, first)
                        for (pts, sk), wants in zip(queries, want_points):
                            for r2, want in zip(radii, wants):
                                assert agree(eng.nearest(pts, sk, r2=r2), want), tag + (r2, len(pts), sk is not None)
                        i, j, d = eng.closest_pair()
                        assert (i, j) == want_pair[:2] == (10, 11) and bits(d) == bits(want_pair[2]) == 0, tag
                    monkeypatch.delenv("NBODY_NEIGHBORS_SPLIT")


@pytest.mark.parametrize("loop", ["1", "2"])
@pytest.mark.parametrize("fp64", [False, True])
def test_hand_made_specials(nb, ref, monkeypatch, fp64, loop):
    """two- and three-body systems whose answers are known by construction (specials_common.hand_made_distances): the constructed
    (idx, d2, count at each r2, closest pair), and the reference's"""
    monkeypatch.setenv("NBODY_NEIGHBORS_LOOP", loop)
    dtype = np.float64 if fp64 else np.float32
    systems, v = hand_made_distances(dtype)
    inf, below = v.inf, lambda x: np.nextafter(x, dtype(0))
    cases = {   # name: (idx, d2, {r2: count}, closest pair)
        "alone": ([-1], [inf], {v.max: [0], inf: [0]}, (-1, -1, inf)),
        "coincident": ([1, 0], [0, 0], {0: [1, 1]}, (0, 1, 0)),
        "underflow": ([1, 0], [0, 0], {0: [1, 1]}, (0, 1, 0)),
        "subnormal": ([1, 0], [v.h2, v.h2], {0: [0, 0], below(v.h2): [0, 0], v.h2: [1, 1], inf: [1, 1]}, (0, 1, v.h2)),
        "overflow": ([2, -1, 0], [9, inf, 9], {9: [1, 0, 1], v.max: [1, 0, 1], inf: [2, 2, 2]}, (0, 2, 9)),
        "nan": ([2, -1, 0], [9, inf, 9], {v.max: [1, 0, 1], inf: [1, 0, 1]}, (0, 2, 9)),
        "inf": ([2, -1, 0], [9, inf, 9], {v.max: [1, 0, 1], inf: [2, 2, 2]}, (0, 2, 9)),
        "two_inf": ([-1, -1, -1], [inf, inf, inf], {v.max: [0, 0, 0], inf: [1, 1, 2]}, (-1, -1, inf)),
        "tied": ([1, 0, 0], [2, 2, 2], {below(dtype(2)): [0, 0, 0], 2: [2, 2, 2]}, (0, 1, 2))}
    assert set(cases) == set(systems)
    for name, (idx, d2, counts, pair) in cases.items():
        pos = systems[name]
        with nb.NBody(len(pos), fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            for r2, cnt in counts.items():
                want = (np.array(idx, np.int32), np.array(d2, dtype), np.array(cnt, np.int32))
                got = eng.neighbors(r2=dtype(r2))
                assert same(got, want) and same(got, ref.rows(pos, r2=dtype(r2))), (name, r2)
                # the same queries as points that skip their own body, and without a skip: the body itself at +0 (or nothing, where
                # it is not at a distance from itself: NaN - NaN, inf - inf)
                assert same(eng.nearest(pos, np.arange(len(pos), dtype=np.int32), r2=dtype(r2)), want), (name, r2)
                own = eng.nearest(pos, r2=dtype(r2))
                assert same(own, ref.points(pos, pos, r2=dtype(r2))), (name, r2)
                finite = np.all(np.isfinite(pos[:, :3]), axis=1)
                assert np.all(bits(own[1][finite]) == 0) and np.all(own[0][~finite] == want[0][~finite]), (name, r2)
            i, j, d = eng.closest_pair()
            assert (i, j) == pair[:2] == ref.closest_pair(pos)[:2] and bits(d) == bits(dtype(pair[2])) == bits(ref.closest_pair(pos)[2]), name


def test_bits_do_not_depend_on_the_source_split_or_the_batches(nb, ref, monkeypatch):
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    r2 = r2_for(pos, 0.1)
    want = (ref.points(pos, pts, r2=r2), ref.points(pos, pts, skip, r2=r2), ref.rows(pos, 100, m, r2=r2))
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        calls = lambda: (eng.nearest(pts, r2=r2), eng.nearest(pts, skip, r2=r2), eng.neighbors(100, m, r2=r2))
        for loop in ("1", "2"):
            monkeypatch.setenv("NBODY_NEIGHBORS_LOOP", loop)
            for split in (None, "1", "2", "3", "64"):
                if split:
                    monkeypatch.setenv("NBODY_NEIGHBORS_SPLIT", split)
                for g_, w in zip(calls(), want):
                    assert same(g_, w), (loop, split)
                assert same(eng.nearest(pts, skip), want[1][:2] + (None,)), (loop, split)
            # 700 queries x 5 chunks x 12 B = 42 kB against a bound of 0.02 MB: batches of 256 queries
            monkeypatch.setenv("NBODY_NEIGHBORS_SCRATCH_MB", "0.02")
            for split in ("5", None):
                if split:
                    monkeypatch.setenv("NBODY_NEIGHBORS_SPLIT", split)
                else:
                    monkeypatch.delenv("NBODY_NEIGHBORS_SPLIT")
                for g_, w in zip(calls(), want):
                    assert same(g_, w), (loop, "batches", split)
            monkeypatch.setenv("NBODY_NEIGHBORS_SPLIT", "5")
            monkeypatch.setenv("NBODY_NEIGHBORS_SCRATCH_MB", "0")   # not even one workgroup's queries fit: no split
            assert same(calls()[1], want[1]), loop
            monkeypatch.delenv("NBODY_NEIGHBORS_SPLIT")
            monkeypatch.delenv("NBODY_NEIGHBORS_SCRATCH_MB")


def test_bits_do_not_depend_on_the_queries_beside_a_query_or_the_force_configuration(nb, ref):
    n, m = 5000, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    r2 = r2_for(pos, 0.1)
    perm = np.random.default_rng(5).permutation(m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        a = eng.nearest(pts, skip, r2=r2)
        rows = eng.neighbors(r2=r2)
        assert same(a, ref.points(pos, pts, skip, r2=r2)) and same(rows, ref.rows(pos, r2=r2))
        for sel in (slice(0, 1), slice(100, 357), slice(699, 700), slice(63, 129), perm):
            assert same(eng.nearest(pts[sel], skip[sel], r2=r2), tuple(v[sel] for v in a)), sel
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            assert same(eng.nearest(pts, skip, r2=r2), a) and same(eng.neighbors(r2=r2), rows), (key, val)
            eng.set_option(key, default)


def test_bits_do_not_depend_on_the_device_count(nb, ref, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n, m = 1500, 300   # 1500 = 500 x 3: slices that end inside a 64-source window and inside a workgroup's rows
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    r2 = r2_for(pos, 0.1)
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            res[ngpus] = (eng.neighbors(r2=r2), eng.neighbors(450, 600, r2=r2), eng.nearest(pts, skip, r2=r2), eng.closest_pair(),
                          eng.download()[0])
    now = res[1][4]
    assert same((now,), (res[3][4],)) and not same((now,), (pos,)), "the two states differ, or no drift happened"
    want = ref.rows(now, r2=r2)
    assert same(res[1][0], want)
    for k in (1, 3):
        assert same(res[k][0], want), k
        assert same(res[k][1], tuple(w[450:1050] for w in want)), k   # a window across both device boundaries: global indices
        assert same(res[k][2], ref.points(now, pts, skip, r2=r2)), k
        assert res[k][3][:2] == ref.closest_pair(now)[:2] and bits(res[k][3][2]) == bits(ref.closest_pair(now)[2]), k


WORKER = """
    from field_common import make_points, make_skip
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m = (300, 41)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    r2 = np.float32(0.05)
    idx, d2, cnt = eng.nearest(pts, make_skip(n, m, on), r2=r2)
    ridx, rd2, rcnt = eng.neighbors(r2=r2)                      # this rank's own rows
    pair = eng.closest_pair()
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, idx=idx, d2=d2, cnt=cnt, ridx=ridx, rd2=rd2, rcnt=rcnt, pair_ij=np.array(pair[:2]),
             pair_d2=np.array([pair[2]], np.float32), first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p)
"""


def test_two_processes_host_transport_equal_one_process(nb, ref, tmp_path):
    n, world = 1500, 2
    out = str(tmp_path / "nbr")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now = got[0]["pos"]
    assert same((now,), (got[1]["pos"],))
    pos = nb.make_bodies(n, seed=33)[0]
    r2 = np.float32(0.05)
    want_rows = ref.rows(now, r2=r2)
    want_pair = ref.closest_pair(now)
    covered = 0
    for r, m in enumerate((300, 41)):
        g_ = got[r]
        pts, on = make_points(nb, pos, m, seed=50 + r)
        assert same((g_["idx"], g_["d2"], g_["cnt"]), ref.points(now, pts, make_skip(n, m, on), r2=r2)), r
        first, cnt = (int(v) for v in g_["first"])
        assert same((g_["ridx"], g_["rd2"], g_["rcnt"]), tuple(w[first:first + cnt] for w in want_rows)), r   # global indices
        covered += cnt
        assert tuple(int(v) for v in g_["pair_ij"]) == want_pair[:2] and bits(g_["pair_d2"][0]) == bits(want_pair[2]), r
    assert covered == n
    with nb.NBody(n) as one:   # ... and equal to one GPU
        one.upload(now, np.zeros_like(now))
        i, j, d = one.closest_pair()
        assert (i, j) == want_pair[:2] and bits(d) == bits(want_pair[2])


@pytest.mark.parametrize("fp64", [False, True])
def test_closest_pair_n16384(nb, ref, fp64):
    n = 16384
    pos, vel = nb.make_bodies(n, dtype=np.float64 if fp64 else np.float32)
    wi, wj, wd = ref.closest_pair(pos)
    rows = ref.rows(pos)
    assert rows[0][wi] == wj and bits(rows[1].min()) == bits(wd)   # the pair scan and the rows scan agree
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        i, j, d = eng.closest_pair()
        assert (i, j) == (wi, wj) and bits(d) == bits(wd)
        assert same(eng.neighbors(), rows)


def test_rows_n65536(nb, ref, monkeypatch):
    """the window re-walk and many workgroups are live here"""
    n = 65536
    pos, vel = nb.make_bodies(n)
    r2 = np.float32(1e-3)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for first in (0, n // 2 - 256, n - 512):
            want = ref.rows(pos, first, 512, r2=r2)
            for loop in ("1", "2"):
                monkeypatch.setenv("NBODY_NEIGHBORS_LOOP", loop)
                assert same(eng.neighbors(first, 512, r2=r2), want), (first, loop)
                assert same(eng.neighbors(first, 512), want[:2] + (None,)), (first, loop)


def test_neighbor_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, on = make_points(nb, nb.make_bodies(n)[0], 300)
    probe = lambda eng: (eng.neighbors(r2=np.float32(0.01)), eng.nearest(pts, make_skip(n, 300, on)), eng.closest_pair())
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_NEIGHBORS_SPLIT")


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pts, pts64 = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float64)
    idx, cnt = np.full(4, 7, np.int32), np.full(4, 7, np.int32)
    d2, d264 = np.full(4, 7, np.float32), np.full(4, 7, np.float64)
    sk = np.array([-1, 0, 3, 2], np.int32)
    calls32 = (lambda: lib.nbody_neighbors_rows(0, 4, ip(idx), d2.ctypes.data_as(f32), 1.0, ip(cnt)),
               lambda: lib.nbody_nearest(pts.ctypes.data_as(f32), 4, ip(sk), ip(idx), d2.ctypes.data_as(f32), 1.0, ip(cnt)),
               lambda: lib.nbody_closest_pair(ip(idx), ip(idx[1:]), d2.ctypes.data_as(f32)))
    calls64 = (lambda: lib.nbody_neighbors_rows_d(0, 4, ip(idx), d264.ctypes.data_as(f64), 1.0, ip(cnt)),
               lambda: lib.nbody_nearest_d(pts64.ctypes.data_as(f64), 4, ip(sk), ip(idx), d264.ctypes.data_as(f64), 1.0, ip(cnt)),
               lambda: lib.nbody_closest_pair_d(ip(idx), ip(idx[1:]), d264.ctypes.data_as(f64)))
    untouched = lambda: np.all(idx == 7) and np.all(cnt == 7) and np.all(d2 == 7) and np.all(d264 == 7)
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
        i_, d_, c_, x = ip(idx), d2.ctypes.data_as(f32), ip(cnt), pts.ctypes.data_as(f32)
        assert lib.nbody_neighbors_rows(0, 4, None, None, 1.0, None) == E.ERR_ARG
        for first, rows in ((-1, 4), (0, 0), (0, -2), (97, 4), (100, 1), (0, 101), (1 << 30, 1 << 30)):
            assert lib.nbody_neighbors_rows(first, rows, i_, d_, 1.0, c_) == E.ERR_ARG, (first, rows)
        assert lib.nbody_nearest(None, 4, None, i_, d_, 1.0, c_) == E.ERR_ARG
        assert lib.nbody_nearest(x, 0, None, i_, d_, 1.0, c_) == E.ERR_ARG
        assert lib.nbody_nearest(x, -3, None, i_, d_, 1.0, c_) == E.ERR_ARG
        assert lib.nbody_nearest(x, 4, None, None, None, 1.0, None) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_nearest(x, 4, ip(sk), i_, d_, 1.0, c_) == E.ERR_ARG, bad
        assert lib.nbody_closest_pair(None, None, None) == E.ERR_ARG
        assert untouched()
        sk[:] = (-1, 0, n - 1, n - 1)
        assert lib.nbody_nearest(x, 4, ip(sk), i_, None, 1.0, None) == 0 and not np.any(idx == 7) and np.all(d2 == 7) and np.all(cnt == 7)
        assert lib.nbody_neighbors_rows(96, 4, None, d_, 1.0, None) == 0 and not np.any(d2 == 7) and np.all(cnt == 7)
        assert lib.nbody_neighbors_rows(96, 4, None, None, 100.0, c_) == 0 and np.all(cnt == n - 1)
        assert lib.nbody_closest_pair(None, i_, None) == 0 and idx[0] == eng.closest_pair()[1]
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert [c() for c in calls32] == [E.ERR_STATE] * 3 and [c() for c in calls64] == [0] * 3


def test_c_host_program_closest_pair_line(nb, ref):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters = 4096, 3
    for flags, fp64 in (([], False), (["--fp64"], True)):
        r = subprocess.run([exe, str(n), str(iters), "--closest-pair"] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = re.findall(r"^closest pair: (-?\d+) (-?\d+) d2 (\S+)$", r.stdout, flags=re.M)
        assert len(lines) == 1, r.stdout
        plain = subprocess.run([exe, str(n), str(iters)] + flags, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0 and "closest" not in plain.stdout
        strip = lambda text: [ln for ln in text.splitlines() if "Billion Interactions" not in ln and not ln.startswith("closest pair")]
        assert strip(r.stdout) == strip(plain.stdout)   # nothing else changes (the rate line carries a time)
        dtype = np.float64 if fp64 else np.float32
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            eng.step(float(np.float32(0.01)), iters)   # the program's dt is the binary32 0.01 in fp64 contexts too
            now = eng.download()[0]
        wi, wj, wd = ref.closest_pair(now)
        assert (int(lines[0][0]), int(lines[0][1])) == (wi, wj) and dtype(float(lines[0][2])) == wd


@pytest.mark.parametrize("fp64", [False, True])
def test_interleaved_with_the_field_pass(nb, monkeypatch, fp64):
    """The neighbour and the field pass keep their points, skip indices and split scratch in the same buffers of the context: on one
    context (one device), twice over — nearest at 700 points over three chunks against 0.02 MB = 20971 B of scratch (fp32: 36 B a
    query, 582 fit, batches of 512 + 188; fp64: 48 B, 436 fit, batches of 256 + 256 + 188), the field at 257 points, nearest at 5000
    points — every result the bits of the same call on a fresh context that never ran the other pass.  N = 2100: three blocks, a
    tail that is no multiple of 64."""
    for k in ("NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"):
        monkeypatch.delenv(k, raising=False)
    n = 2100
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    r2 = r2_for(pos, 0.05)
    pts = {m: make_points(nb, pos, m)[0] for m in (257, 700, 5000)}
    skip = {m: ((np.arange(m) * 997) % n).astype(np.int32) for m in pts}

    def nearest_small(eng):
        monkeypatch.setenv("NBODY_NEIGHBORS_SPLIT", "3")
        monkeypatch.setenv("NBODY_NEIGHBORS_SCRATCH_MB", "0.02")
        got = eng.nearest(pts[700], skip[700], r2=r2)
        monkeypatch.delenv("NBODY_NEIGHBORS_SPLIT")
        monkeypatch.delenv("NBODY_NEIGHBORS_SCRATCH_MB")
        return got

    calls = (nearest_small, lambda eng: eng.field(pts[257], skip[257]), lambda eng: eng.nearest(pts[5000], skip[5000], r2=r2))

    def run(which):
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            return [calls[k](eng) if k in which else None for _ in range(2) for k in range(3)]

    mixed, only_nearest, only_field = run((0, 1, 2)), run((0, 2)), run((1,))
    for k in (0, 2, 3, 5):
        assert same(mixed[k], only_nearest[k]), k
    for k in (1, 4):
        assert same(mixed[k], only_field[k]), k   # (accel, phi): the same bits
        assert np.all(np.isfinite(mixed[k][0])) and np.all(np.isfinite(mixed[k][1]))
    assert np.all(mixed[0][0] >= 0) and np.all(mixed[2][0] >= 0) and np.all(mixed[0][0] != skip[700])
