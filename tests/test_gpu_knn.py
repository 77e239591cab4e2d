"""The k nearest neighbours on the device (nbody_knn_rows, nbody_knn and their _d forms; include/nbody.h "k nearest neighbours"): every
case bit for bit against tests/knn_ref.c — idx equal, d2 the same bits — in both precisions, for k on both sides of every list
capacity, however the work is laid out (source split, batches, windows of rows, force configuration, device and process count);
column 0 is the neighbour pass and shorter lists are prefixes of longer ones; no effect on the step; the guards."""
import ctypes as C

import numpy as np
import pytest

import neighbors_common
from knn_common import KS, bits, make_points, make_ref, make_skip, planted, same
from pass_common import FORCE_CONFIGS, check_step_untouched
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import POINT_COUNTS, SIZES, VARIANTS, hand_made_distances, hostile_distance_system, hostile_points, same_nan
from test_gpu_neighbors import windows

pytestmark = pytest.mark.gpu
ENV = ("NBODY_KNN_SPLIT", "NBODY_KNN_SCRATCH_MB", "NBODY_NEIGHBORS_SPLIT", "NBODY_NEIGHBORS_SCRATCH_MB", "NBODY_NEIGHBORS_LOOP",
       "NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("knn_ref"))


@pytest.fixture(scope="module")
def nref(tmp_path_factory):
    return neighbors_common.make_ref(tmp_path_factory.mktemp("neighbors_ref"))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def ks_for(n):
    """every k at the sizes that decide something (one body, fewer bodies than k, a window edge, a block edge, two blocks and a tail);
    elsewhere one k on each side of a capacity boundary"""
    return KS if n in (1, 5, 65, 1025, 2100) else (1, 4, 5, 17, 32)


@pytest.mark.parametrize("fp64", [False, True])
def test_rows_bit_for_bit(nb, ref, fp64):
    dtype = np.float64 if fp64 else np.float32
    for n in (1, 2, 5, 63, 64, 65, 257, 1000, 1025, 2100):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for k in ks_for(n):
                want = ref.rows(pos, k)
                for first, cnt in windows(n):
                    got = eng.knn(k, first, cnt)
                    assert same(got, tuple(w[first:first + cnt] for w in want)), (n, k, first, cnt)
                assert same(eng.knn(k), want), (n, k)


@pytest.mark.parametrize("fp64", [False, True])
def test_k1_is_the_neighbour_pass_and_shorter_lists_are_prefixes(nb, monkeypatch, fp64):
    dtype = np.float64 if fp64 else np.float32
    n, m = 2100, 257
    for pos in (nb.make_bodies(n, dtype=dtype)[0], planted(nb, n, dtype)):
        pts, on = make_points(nb, pos, m)
        skip = make_skip(n, m, on)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            for split in (None, "3"):
                if split:
                    monkeypatch.setenv("NBODY_KNN_SPLIT", split)
                idx, d2 = eng.knn(1)
                assert same((idx[:, 0], d2[:, 0]), eng.neighbors()[:2]), split
                for sk in (None, skip):
                    idx, d2 = eng.knn_at(pts, 1, sk)
                    assert same((idx[:, 0], d2[:, 0]), eng.nearest(pts, sk)[:2]), split
                rows32, at32 = eng.knn(32), eng.knn_at(pts, 32, skip)
                for k in KS:
                    assert same(eng.knn(k), (rows32[0][:, :k], rows32[1][:, :k])), (k, split)
                    assert same(eng.knn_at(pts, k, skip), (at32[0][:, :k], at32[1][:, :k])), (k, split)
            monkeypatch.delenv("NBODY_KNN_SPLIT")


@pytest.mark.parametrize("fp64", [False, True])
def test_points_form(nb, ref, fp64):
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
                for k in (1, 5, 8, 32):
                    assert same(eng.knn_at(pts, k, skip), ref.points(pos, pts, k, skip)), (m, skip is not None, k)
            assert same(eng.knn_at(np.ascontiguousarray(pts[:, :3]), 9), ref.points(pos, pts, 9))   # (m, 3) points are padded to words
        idx, d2 = eng.knn_at(pts[:3], 2)
        assert list(idx[:, 0]) == on and np.all(bits(d2[:, 0]) == 0)   # a point on a body without a skip: that body first, at +0
        assert same(eng.knn_at(pos, 17, np.arange(n, dtype=np.int32)), eng.knn(17))
        with pytest.raises(ValueError):
            eng.knn_at(pts[:, :2], 3)
        with pytest.raises(ValueError):
            eng.knn_at(pts, 3, spread[:-1])
        for bad in (0, 33, -1):
            with pytest.raises(ValueError):
                eng.knn(bad)


def agree(got, want):
    """(idx, d2) against the reference's: idx equal, d2 with the same NaN mask and the same bits elsewhere"""
    return np.array_equal(got[0], want[0]) and same_nan(got[1], want[1])


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system(nb, ref, monkeypatch, fp64):
    """specials_common.hostile_distance_system bit for bit against knn_ref.c: lists that run through +0 ties in ascending index and
    then through two distinct subnormal values (rows 22, 23), lists of one entry and padding (rows 63, 66 of "overflow"), empty lists
    (the NaN body; rows 63, 66 of "inf"), for k on both sides of the smallest capacity and at the largest, every split (3 puts 1023
    and 1024 in different chunks), windows of rows and the points form; column 0 is the neighbour pass, k = 5 a prefix of k = 32."""
    dtype = np.float64 if fp64 else np.float32
    ks = (1, 4, 5, 32)
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_distance_system(nb, n, dtype, variant)
            want_rows = {k: ref.rows(pos, k) for k in ks}
            queries = [(pts, sk) for m in POINT_COUNTS for pts, skip in [hostile_points(nb, pos, m, variant)] for sk in (skip, None)]
            want_points = [{k: ref.points(pos, pts, k, sk) for k in ks} for pts, sk in queries]
            idx, d2 = want_rows[32]
            assert not np.any(np.isnan(d2)) and idx[62, 0] == 65 and idx[65, 0] == 62
            for i, other in ((22, 23), (23, 22)):
                assert list(idx[i, :6]) == sorted((10, 11, 64, other)) + [62, 65] and np.all(bits(d2[i, :4]) == 0)
                assert 0 < d2[i, 4] < d2[i, 5] < np.finfo(dtype).tiny
            if variant == "overflow":
                assert list(idx[63, :2]) == [66, -1] and list(idx[66, :2]) == [63, -1] and np.isfinite(d2[63, 0]) and np.isposinf(d2[63, 1])
            if variant == "inf":
                assert np.all(idx[[63, 66]] == -1) and np.all(np.isposinf(d2[[63, 66]]))
            with nb.NBody(n, fp64=fp64) as eng:
                eng.upload(pos, vel)
                for split in (None, "1", "2", "3"):
                    if split:
                        monkeypatch.setenv("NBODY_KNN_SPLIT", split)
                    tag = (n, variant, split)
                    got = {}
                    for k in ks:
                        for first, rows in windows(n):
                            got[k, first] = eng.knn(k, first, rows)
                            assert agree(got[k, first], tuple(w[first:first + rows] for w in want_rows[k])), tag + (k, first)
                    assert agree((got[5, 0][0], got[5, 0][1]), (got[32, 0][0][:, :5], got[32, 0][1][:, :5])), tag
                    near = eng.neighbors()
                    assert np.array_equal(got[1, 0][0][:, 0], near[0]) and same_nan(got[1, 0][1][:, 0], near[1]), tag
                    for (pts, sk), wants in zip(queries, want_points):
                        at = {k: eng.knn_at(pts, k, sk) for k in ks}
                        for k in ks:
                            assert agree(at[k], wants[k]), tag + (k, len(pts), sk is not None)
                        assert agree(at[5], (at[32][0][:, :5], at[32][1][:, :5])), tag
                        near = eng.nearest(pts, sk)
                        assert np.array_equal(at[1][0][:, 0], near[0]) and same_nan(at[1][1][:, 0], near[1]), tag
                monkeypatch.delenv("NBODY_KNN_SPLIT")


@pytest.mark.parametrize("fp64", [False, True])
def test_hand_made_specials(nb, ref, fp64):
    """two- and three-body systems whose answers are known by construction (specials_common.hand_made_distances): the constructed
    lists at k = 2 (k = 1, 4 and 32 are their prefix and their padding), and the reference's"""
    dtype = np.float64 if fp64 else np.float32
    systems, v = hand_made_distances(dtype)
    inf = v.inf
    cases = {   # name: (idx, d2) at k = 2
        "alone": ([[-1, -1]], [[inf, inf]]),
        "coincident": ([[1, -1], [0, -1]], [[0, inf], [0, inf]]),
        "underflow": ([[1, -1], [0, -1]], [[0, inf], [0, inf]]),
        "subnormal": ([[1, -1], [0, -1]], [[v.h2, inf], [v.h2, inf]]),
        "overflow": ([[2, -1], [-1, -1], [0, -1]], [[9, inf], [inf, inf], [9, inf]]),
        "nan": ([[2, -1], [-1, -1], [0, -1]], [[9, inf], [inf, inf], [9, inf]]),
        "inf": ([[2, -1], [-1, -1], [0, -1]], [[9, inf], [inf, inf], [9, inf]]),
        "two_inf": ([[-1, -1]] * 3, [[inf, inf]] * 3),
        "tied": ([[1, 2], [0, 2], [0, 1]], [[2, 2]] * 3)}
    assert set(cases) == set(systems)
    for name, (idx, d2) in cases.items():
        pos = systems[name]
        want = (np.array(idx, np.int32), np.array(d2, dtype))
        with nb.NBody(len(pos), fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            for k in (1, 2, 4, 32):
                pad = max(0, k - 2)
                made = (np.pad(want[0], ((0, 0), (0, pad)), constant_values=-1)[:, :k], np.pad(want[1], ((0, 0), (0, pad)), constant_values=inf)[:, :k])
                got = eng.knn(k)
                assert same(got, made) and same(got, ref.rows(pos, k)), (name, k)
                assert same(eng.knn_at(pos, k, np.arange(len(pos), dtype=np.int32)), made), (name, k)
                assert same(eng.knn_at(pos, k), ref.points(pos, pos, k)), (name, k)


@pytest.mark.parametrize("fp64", [False, True])
def test_ties_and_specials(nb, ref, monkeypatch, fp64):
    dtype = np.float64 if fp64 else np.float32
    n = 2100
    pos = planted(nb, n, dtype)
    vel = np.zeros_like(pos)
    h2 = dtype(2.0 ** -24)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        for split in (None, "3"):   # three chunks of one block: the tie at 1024 sits in another chunk than 63's other ties
            if split:
                monkeypatch.setenv("NBODY_KNN_SPLIT", split)
            for k in (1, 3, 4, 5, 32):
                idx, d2 = got = eng.knn(k)
                assert same(got, ref.rows(pos, k)), (split, k)
                assert list(idx[63, :4]) == [64, 65, 500, 1024][:k] and np.all(bits(d2[63, :4]) == bits(h2))
                assert list(idx[3, :2]) == [70, 900][:k] and np.all(bits(d2[3, :2]) == 0)
                assert np.all(idx[200] == -1) and np.all(np.isposinf(d2[200])) and not np.any(idx == 200)
            pts = pos[[3, 63, 200, 63]].copy()
            pts[2, :3] = 4.0
            sk = np.array([3, 63, -1, 64], np.int32)
            assert same(eng.knn_at(pts, 5, sk), ref.points(pos, pts, 5, sk)), split
            assert [list(r) for r in eng.knn_at(pts, 3, sk)[0]] == [[70, 900, eng.knn(3, 3, 1)[0][0, 2]], [64, 65, 500], [63, 64, 65], [63, 65, 500]]
    for few in (1, 5):   # fewer than k candidates: padded with (-1, +inf)
        with nb.NBody(few, fp64=fp64) as eng:
            eng.upload(pos[:few], vel[:few])
            for k in (1, 4, 8, 32):
                idx, d2 = got = eng.knn(k)
                assert same(got, ref.rows(pos[:few], k)), (few, k)
                assert np.all(idx[:, few - 1:] == -1) and np.all(np.isposinf(d2[:, few - 1:])) and np.all(idx[:, :min(k, few - 1)] >= 0)
            idx, d2 = eng.knn_at(pos[:1], 2)
            assert list(idx[0]) == ([0, -1] if few == 1 else [0, eng.knn(1, 0, 1)[0][0, 0]])
            assert np.all(eng.knn_at(pos[:1], 2, np.zeros(1, np.int32))[0][0, few - 1:] == -1)


def test_values_do_not_depend_on_the_source_split_or_the_batches(nb, ref, monkeypatch):
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for k in (1, 5, 32):
            want = (ref.points(pos, pts, k), ref.points(pos, pts, k, skip), ref.rows(pos, k, 100, m))
            calls = lambda: (eng.knn_at(pts, k), eng.knn_at(pts, k, skip), eng.knn(k, 100, m))
            for split in (None, "1", "2", "3", "1000"):
                if split:
                    monkeypatch.setenv("NBODY_KNN_SPLIT", split)
                for g_, w in zip(calls(), want):
                    assert same(g_, w), (k, split)
            # 700 queries x 5 chunks x k x 8 B = 28 k kB against a bound of 0.02 k MB = 20971 k B: 524 queries fit, batches of 512 + 188
            monkeypatch.setenv("NBODY_KNN_SCRATCH_MB", repr(0.02 * k))
            for split in ("5", None):
                if split:
                    monkeypatch.setenv("NBODY_KNN_SPLIT", split)
                else:
                    monkeypatch.delenv("NBODY_KNN_SPLIT")
                for g_, w in zip(calls(), want):
                    assert same(g_, w), (k, "batches", split)
            monkeypatch.setenv("NBODY_KNN_SPLIT", "5")
            monkeypatch.setenv("NBODY_KNN_SCRATCH_MB", "0")   # not even one workgroup's queries fit: no split
            assert same(calls()[1], want[1]), k
            monkeypatch.delenv("NBODY_KNN_SPLIT")
            monkeypatch.delenv("NBODY_KNN_SCRATCH_MB")
        # one output at a time, split or not
        want = ref.points(pos, pts, 9, skip)
        lib, ip = nb._lib.load(), C.POINTER(C.c_int)
        for split in (None, "3"):
            if split:
                monkeypatch.setenv("NBODY_KNN_SPLIT", split)
            idx, d2 = np.full((m, 9), 7, np.int32), np.full((m, 9), 7, np.float32)
            args = (pts.ctypes.data_as(C.POINTER(C.c_float)), m, skip.ctypes.data_as(ip), 9)
            assert lib.nbody_knn(*args, idx.ctypes.data_as(ip), None) == 0 and np.all(d2 == 7) and same((idx,), want[:1])
            idx[:] = 7
            assert lib.nbody_knn(*args, None, d2.ctypes.data_as(C.POINTER(C.c_float))) == 0 and np.all(idx == 7) and same((d2,), want[1:])


def test_values_do_not_depend_on_the_queries_beside_a_query_or_the_force_configuration(nb, ref):
    n, m, k = 5000, 700, 9
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    perm = np.random.default_rng(5).permutation(m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        a = eng.knn_at(pts, k, skip)
        rows = eng.knn(k)
        assert same(a, ref.points(pos, pts, k, skip)) and same(rows, ref.rows(pos, k))
        for sel in (slice(0, 1), slice(100, 357), slice(699, 700), slice(63, 129), perm):
            assert same(eng.knn_at(pts[sel], k, skip[sel]), tuple(v[sel] for v in a)), sel
        for key, val, default in FORCE_CONFIGS + ((nb.OPT_ARITH, nb.ARITH_REFERENCE, nb.ARITH_FMA3), (nb.OPT_ARITH, nb.ARITH_STRICT, nb.ARITH_FMA3),
                                                  (nb.OPT_ARITH, nb.ARITH_REFERENCE_STRICT, nb.ARITH_FMA3)):
            eng.set_option(key, val)
            assert same(eng.knn_at(pts, k, skip), a) and same(eng.knn(k), rows), (key, val)
            eng.set_option(key, default)


def test_values_do_not_depend_on_the_device_count(nb, ref, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n, m, k = 1500, 300, 9   # 1500 = 500 x 3: slices that end inside a 64-source window and inside a workgroup's rows
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            res[ngpus] = (eng.knn(k), eng.knn(k, 450, 600), eng.knn_at(pts, k, skip), eng.download()[0])
    now = res[1][3]
    assert same((now,), (res[3][3],)) and not same((now,), (pos,)), "the two states differ, or no drift happened"
    want = ref.rows(now, k)
    for g in (1, 3):
        assert same(res[g][0], want), g
        assert same(res[g][1], tuple(w[450:1050] for w in want)), g   # a window across both device boundaries: global indices
        assert same(res[g][2], ref.points(now, pts, k, skip)), g


WORKER = """
    from field_common import make_points, make_skip
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m = (300, 41)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    idx, d2 = eng.knn_at(pts, 9, make_skip(n, m, on))
    ridx, rd2 = eng.knn(5)                                      # this rank's own rows
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, idx=idx, d2=d2, ridx=ridx, rd2=rd2,
             first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p)
"""


def test_two_processes_host_transport_equal_one_process(nb, ref, tmp_path):
    n, world = 1500, 2
    out = str(tmp_path / "knn")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now = got[0]["pos"]
    assert same((now,), (got[1]["pos"],))
    pos = nb.make_bodies(n, seed=33)[0]
    want_rows = ref.rows(now, 5)
    covered = 0
    for r, m in enumerate((300, 41)):
        g_ = got[r]
        pts, on = make_points(nb, pos, m, seed=50 + r)
        assert same((g_["idx"], g_["d2"]), ref.points(now, pts, 9, make_skip(n, m, on))), r
        first, cnt = (int(v) for v in g_["first"])
        assert same((g_["ridx"], g_["rd2"]), tuple(w[first:first + cnt] for w in want_rows)), r   # global indices
        covered += cnt
    assert covered == n


def test_rows_n65536_k32(nb, ref):
    """every row of a mid-size system (4 x 10^9 pairs) at the largest k: many workgroups, the second walk live in early windows and
    rare in late ones"""
    n = 65536
    pos, vel = nb.make_bodies(n)
    want = ref.rows(pos, 32)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        assert same(eng.knn(32), want)


def test_knn_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, on = make_points(nb, nb.make_bodies(n)[0], 300)
    probe = lambda eng: (eng.knn(5), eng.knn_at(pts, 17, make_skip(n, 300, on)))
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_KNN_SPLIT")


@pytest.mark.parametrize("fp64", [False, True])
def test_interleaved_with_the_field_and_the_neighbour_pass(nb, ref, nref, monkeypatch, fp64):
    """The three point passes keep their points, skip indices and split scratch in the same buffers of the context: on one context,
    twice over — knn_at at 700 points over three chunks in batches, the field at 257 points, nearest at 5000 points, knn_at at 5000
    points — the knn and nearest results equal their references, the field's the bits of a context that ran nothing else."""
    n = 2100
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    pts = {m: make_points(nb, pos, m)[0] for m in (257, 700, 5000)}
    skip = {m: ((np.arange(m) * 997) % n).astype(np.int32) for m in pts}

    def knn_small(eng):
        monkeypatch.setenv("NBODY_KNN_SPLIT", "3")
        monkeypatch.setenv("NBODY_KNN_SCRATCH_MB", "0.06")   # 62914 B against 3 x 5 x 8 (fp64: 12) B a query: 524 (349) fit, batches of 512 (256)
        got = eng.knn_at(pts[700], 5, skip[700])
        monkeypatch.delenv("NBODY_KNN_SPLIT")
        monkeypatch.delenv("NBODY_KNN_SCRATCH_MB")
        return got

    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        field_alone = eng.field(pts[257], skip[257])
    want_small, want_big = ref.points(pos, pts[700], 5, skip[700]), ref.points(pos, pts[5000], 32, skip[5000])
    want_near = nref.points(pos, pts[5000], skip[5000])
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        for _ in range(2):
            assert same(knn_small(eng), want_small)
            assert same(eng.field(pts[257], skip[257]), field_alone)
            assert same(eng.nearest(pts[5000], skip[5000])[:2], want_near[:2])
            assert same(eng.knn_at(pts[5000], 32, skip[5000]), want_big)


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pts, pts64 = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float64)
    idx = np.full((4, 3), 7, np.int32)
    d2, d264 = np.full((4, 3), 7, np.float32), np.full((4, 3), 7, np.float64)
    sk = np.array([-1, 0, 3, 2], np.int32)
    calls32 = (lambda: lib.nbody_knn_rows(0, 4, 3, ip(idx), d2.ctypes.data_as(f32)),
               lambda: lib.nbody_knn(pts.ctypes.data_as(f32), 4, ip(sk), 3, ip(idx), d2.ctypes.data_as(f32)))
    calls64 = (lambda: lib.nbody_knn_rows_d(0, 4, 3, ip(idx), d264.ctypes.data_as(f64)),
               lambda: lib.nbody_knn_d(pts64.ctypes.data_as(f64), 4, ip(sk), 3, ip(idx), d264.ctypes.data_as(f64)))
    untouched = lambda: np.all(idx == 7) and np.all(d2 == 7) and np.all(d264 == 7)
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [c() for c in calls32 + calls64] == [E.ERR_STATE] * 4
        finally:
            mb.serve(False)
        assert untouched()
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        assert [c() for c in calls64] == [E.ERR_STATE] * 2 and untouched()
        i_, d_, x = ip(idx), d2.ctypes.data_as(f32), pts.ctypes.data_as(f32)
        assert lib.nbody_knn_rows(0, 4, 3, None, None) == E.ERR_ARG
        for k in (0, -1, 33, 1 << 30):
            assert lib.nbody_knn_rows(0, 4, k, i_, d_) == E.ERR_ARG, k
            assert lib.nbody_knn(x, 4, None, k, i_, d_) == E.ERR_ARG, k
        for first, rows in ((-1, 4), (0, 0), (0, -2), (97, 4), (100, 1), (0, 101), (1 << 30, 1 << 30)):
            assert lib.nbody_knn_rows(first, rows, 3, i_, d_) == E.ERR_ARG, (first, rows)
        assert lib.nbody_knn(None, 4, None, 3, i_, d_) == E.ERR_ARG
        assert lib.nbody_knn(x, 0, None, 3, i_, d_) == E.ERR_ARG
        assert lib.nbody_knn(x, -3, None, 3, i_, d_) == E.ERR_ARG
        assert lib.nbody_knn(x, 4, None, 3, None, None) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_knn(x, 4, ip(sk), 3, i_, d_) == E.ERR_ARG, bad
        assert untouched()
        sk[:] = (-1, 0, n - 1, n - 1)
        assert lib.nbody_knn(x, 4, ip(sk), 3, i_, None) == 0 and not np.any(idx == 7) and np.all(d2 == 7)
        assert lib.nbody_knn_rows(96, 4, 3, None, d_) == 0 and not np.any(d2 == 7)
        assert same(eng.knn(3, 96, 4), (eng.knn(3)[0][96:], d2))
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert [c() for c in calls32] == [E.ERR_STATE] * 2 and [c() for c in calls64] == [0] * 2
