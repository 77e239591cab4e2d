"""Friends-of-friends groups on the device (nbody_fof and its _d form; include/nbody.h "friends-of-friends groups"): every case
integer for integer against tests/fof_ref.c in both precisions, on planted ties and chains whose groups are known by construction,
however the work is laid out (source split, batches, the active-row list, force configuration, device and process count); against the
neighbour pass with no CPU statement involved; no effect on the step or on the passes that share the query buffers; the guards."""
import ctypes as C

import numpy as np
import pytest

import knn_common
import neighbors_common
from fof_common import CHAIN_N, b2_for, chain, make_ref, planted, round_bound
from field_common import make_points, make_skip
from pass_common import PLANS, check_step_untouched
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import VARIANTS, hand_made_distances, hostile_b2, hostile_distance_system, nan_row
from specials_common import SIZES as HOSTILE_SIZES

pytestmark = pytest.mark.gpu
ENV = ("NBODY_FOF_SPLIT", "NBODY_FOF_SCRATCH_MB", "NBODY_FOF_ALL_ROWS", "NBODY_KNN_SPLIT", "NBODY_KNN_SCRATCH_MB", "NBODY_NEIGHBORS_SPLIT",
       "NBODY_NEIGHBORS_SCRATCH_MB", "NBODY_NEIGHBORS_LOOP", "NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB")
SIZES = (1, 2, 5, 63, 64, 65, 257, 1000, 1025, 2100)   # one body, a window edge, a block edge, two blocks with a tail
RATIOS = (0.0, 0.3, 0.7, 0.9, 1.5, np.inf)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("fof_ref"))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def check(eng, ref, pos, b2, what, want=None):
    """one call against the statement (want: ref.groups(pos, b2) where the caller has it already): the same group array and count, the
    round bound; returns (group, rounds)"""
    n = len(pos)
    group, n_groups = eng.fof(b2)
    want, want_groups = want or ref.groups(pos, b2)
    assert group.dtype == np.int32 and group.shape == (n,), what
    assert np.array_equal(group, want), what
    assert n_groups == want_groups == int((group == np.arange(n)).sum()), what
    assert 1 <= eng.fof_rounds <= round_bound(n), (what, eng.fof_rounds)
    return group, eng.fof_rounds


@pytest.mark.parametrize("fp64", [False, True])
def test_bit_for_bit(nb, ref, fp64):
    dtype = np.float64 if fp64 else np.float32
    for n in SIZES:
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for ratio in RATIOS:
                group, rounds = check(eng, ref, pos, b2_for(n, ratio, dtype), (n, ratio))
                if ratio == 0.0:
                    assert np.array_equal(group, np.arange(n)) and rounds == 1
                if np.isinf(ratio):
                    assert np.all(group == 0) and rounds == (1 if n == 1 else 2)   # everybody reports 0 (body 0 reports 1) in round 1


@pytest.mark.parametrize("fp64", [False, True])
def test_planted_ties_coincident_bodies_and_a_nan_body(nb, ref, monkeypatch, fp64):
    dtype = np.float64 if fp64 else np.float32
    n = 2100
    pos = planted(nb, n, dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, np.zeros_like(pos))
        seen = []
        for split in (None, "3"):   # three chunks of one block: 1024 sits in another chunk than 63's other friends
            if split:
                monkeypatch.setenv("NBODY_FOF_SPLIT", split)
            group, rounds = check(eng, ref, pos, dtype(2.0 ** -24), split)
            assert all(group[i] == 63 for i in (63, 64, 65, 500, 1024)) and int((group == 63).sum()) == 5   # d2 == b2 exactly: linked
            assert all(group[i] == 3 for i in (3, 70, 900)) and group[200] == 200 and int((group == 200).sum()) == 1
            seen.append((group, rounds))
            for b2 in (0.0, 2.0 ** -40):   # coincident bodies are linked at any b2 >= 0
                group, _ = check(eng, ref, pos, dtype(b2), (split, b2))
                assert all(group[i] == 3 for i in (3, 70, 900)) and group[63] == 63 and group[64] == 64 and group[200] == 200
            group, _ = check(eng, ref, pos, dtype(np.inf), (split, "inf"))
            assert group[200] == 200 and int((group == 0).sum()) == n - 1
        assert np.array_equal(seen[0][0], seen[1][0]) and seen[0][1] == seen[1][1]


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system(nb, ref, monkeypatch, fp64):
    """specials_common.hostile_distance_system integer for integer against fof_ref.c at every linking length of hostile_b2 — 0, which
    links the distinct bodies whose d2 underflows to +0; a subnormal between the planted pair's d2 and its d2 to the bodies at zero,
    which links that pair and nothing else to it; the smallest normal; an ordinary one; the largest finite, which a d2 that overflowed
    is not within; +inf, which it is, while a NaN is not — every split (3 puts 1023 and 1024 in different chunks), with the active-row
    list and with every row in every round, the round bound, and against the neighbour pass: a body is alone iff nobody is within b2."""
    dtype = np.float64 if fp64 else np.float32
    for n in HOSTILE_SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_distance_system(nb, n, dtype, variant)
            nans = int(variant == "nan")
            with nb.NBody(n, fp64=fp64) as eng:
                eng.upload(pos, vel)
                for b2 in hostile_b2(pos):
                    seen, want = set(), ref.groups(pos, b2)
                    for all_rows in (None, "1"):
                        if all_rows:
                            monkeypatch.setenv("NBODY_FOF_ALL_ROWS", all_rows)
                        for split in (None, "1", "2", "3"):
                            if split:
                                monkeypatch.setenv("NBODY_FOF_SPLIT", split)
                            group, rounds = check(eng, ref, pos, b2, (n, variant, b2, all_rows, split), want)
                            seen.add(rounds)
                        monkeypatch.delenv("NBODY_FOF_SPLIT")
                    monkeypatch.delenv("NBODY_FOF_ALL_ROWS")
                    assert len(seen) == 1, (n, variant, b2, seen)   # the same rounds for every launch shape
                    idx, d2, count = eng.neighbors(r2=b2)
                    alone = np.bincount(group, minlength=n)[group] == 1
                    with np.errstate(invalid="ignore"):   # the +inf of a body without a candidate is no distance
                        assert np.array_equal(alone, count == 0) and np.array_equal(alone[idx >= 0], ~(d2 <= b2)[idx >= 0]), (n, variant, b2)
                    if b2 == 0:
                        assert all(group[i] == 10 for i in (10, 11, 22, 23, 64)) and int((group == 10).sum()) == 5 and group[62] == 62
                        if n > 1028:
                            members = [i for i in range(1023, 1029) if not (nans and i == 1024)]
                            assert all(group[i] == 1023 for i in members) and int((group == 1023).sum()) == len(members)
                    if 0 < b2 < np.finfo(dtype).tiny:
                        assert group[62] == group[65] == 62 and int((group == 62).sum()) == 2 and int((group == 10).sum()) == 5
                    if b2 == np.finfo(dtype).max and variant == "overflow":
                        assert group[63] == group[66] == 63 and int((group == 63).sum()) == 2
                    if b2 == np.finfo(dtype).max and variant == "inf":
                        assert group[63] == 63 and group[66] == 66
                    if np.isposinf(b2):
                        assert int((group == 0).sum()) == n - nans and (not nans or group[nan_row(n)] == nan_row(n))


@pytest.mark.parametrize("fp64", [False, True])
def test_hand_made_specials(nb, ref, fp64):
    """two- and three-body systems whose groups are known by construction (specials_common.hand_made_distances)"""
    dtype = np.float64 if fp64 else np.float32
    systems, v = hand_made_distances(dtype)
    below = lambda x: np.nextafter(x, dtype(0))
    cases = {   # name: {b2: group}
        "alone": {0: [0], v.inf: [0]},
        "coincident": {0: [0, 0], v.sub: [0, 0]},
        "underflow": {0: [0, 0]},
        "subnormal": {0: [0, 1], below(v.h2): [0, 1], v.h2: [0, 0]},
        "overflow": {below(dtype(9)): [0, 1, 2], 9: [0, 1, 0], v.max: [0, 1, 0], v.inf: [0, 0, 0]},
        "nan": {9: [0, 1, 0], v.inf: [0, 1, 0]},
        "inf": {9: [0, 1, 0], v.max: [0, 1, 0], v.inf: [0, 0, 0]},
        "two_inf": {v.max: [0, 1, 2], v.inf: [0, 0, 0]},   # inf - inf = NaN links nothing: the two meet through the finite body
        "tied": {below(dtype(2)): [0, 1, 2], 2: [0, 0, 0]}}
    assert set(cases) == set(systems)
    for name, by_b2 in cases.items():
        pos = systems[name]
        with nb.NBody(len(pos), fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            for b2, want in by_b2.items():
                group, rounds = check(eng, ref, pos, dtype(b2), (name, b2))
                assert list(group) == want, (name, b2)


@pytest.mark.parametrize("fp64", [False, True])
def test_chains(nb, ref, monkeypatch, fp64):
    dtype = np.float64 if fp64 else np.float32
    for cut in (False, True):
        pos, b2, want = chain(dtype, cut=cut)
        with nb.NBody(CHAIN_N, fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            rounds = set()
            for split in (None, "3"):
                if split:
                    monkeypatch.setenv("NBODY_FOF_SPLIT", split)
                group, r = check(eng, ref, pos, b2, (cut, split))
                assert np.array_equal(group, want), (cut, split)
                assert eng.fof(b2)[1] == (8 if cut else 1)
                rounds.add(r)
            monkeypatch.delenv("NBODY_FOF_SPLIT")
            print("chain cut=%s: %d rounds (bound %d)" % (cut, r, round_bound(CHAIN_N)))
            assert len(rounds) == 1 and r > 2   # a long component does take several rounds, the same however the sources are split


def test_layout_independence(nb, ref, monkeypatch):
    n = 5000   # five blocks
    pos, vel = nb.make_bodies(n)
    chain_pos, chain_b2, chain_want = chain()
    for p, b2s in ((pos, [b2_for(n, r) for r in (0.7, 0.9, 1.5)]), (chain_pos, [chain_b2])):
        with nb.NBody(len(p)) as eng:
            eng.upload(p, np.zeros_like(p))
            for b2 in b2s:
                want = check(eng, ref, p, b2, "plain")

                def same(what):
                    group, _ = eng.fof(b2)
                    assert np.array_equal(group, want[0]) and eng.fof_rounds == want[1], (what, eng.fof_rounds, want[1])

                for split in ("1", "2", "3", "64"):
                    monkeypatch.setenv("NBODY_FOF_SPLIT", split)
                    same(("split", split))
                # 5 chunks x 4 B a row against 0.005 MB = 5242 B: 262 rows fit, batches of one workgroup
                monkeypatch.setenv("NBODY_FOF_SCRATCH_MB", "0.005")
                for split in ("5", None):
                    if split:
                        monkeypatch.setenv("NBODY_FOF_SPLIT", split)
                    else:
                        monkeypatch.delenv("NBODY_FOF_SPLIT")
                    same(("batches", split))
                monkeypatch.delenv("NBODY_FOF_SCRATCH_MB")
                monkeypatch.setenv("NBODY_FOF_ALL_ROWS", "1")
                for split in (None, "3"):
                    if split:
                        monkeypatch.setenv("NBODY_FOF_SPLIT", split)
                    same(("all rows", split))
                monkeypatch.delenv("NBODY_FOF_SPLIT")
                monkeypatch.delenv("NBODY_FOF_ALL_ROWS")
            b2 = b2s[0]
            want = eng.fof(b2)[0]
            for key, val, default in ((nb.OPT_VARIANT, nb.VARIANT_SMEM, nb.VARIANT_AUTO), (nb.OPT_ARITH, nb.ARITH_REFERENCE_STRICT, nb.ARITH_FMA3)):
                eng.set_option(key, val)
                assert np.array_equal(eng.fof(b2)[0], want), (key, val)
                eng.set_option(key, default)


def test_values_do_not_depend_on_the_device_count(nb, ref, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n = 2100
    pos, vel = nb.make_bodies(n)
    b2s = [b2_for(n, r) for r in (0.7, 1.5)]
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            res[ngpus] = [eng.fof(b2) + (eng.fof_rounds,) for b2 in b2s] + [eng.download()[0]]
    now = res[1][-1]
    assert np.array_equal(now.view(np.uint32), res[3][-1].view(np.uint32)) and not np.array_equal(now, pos)
    for k, b2 in enumerate(b2s):
        want = ref.groups(now, b2)
        for g in (1, 3):
            group, n_groups, rounds = res[g][k]
            assert np.array_equal(group, want[0]) and n_groups == want[1], (g, k)
        assert res[1][k][2] == res[3][k][2]


WORKER = """
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    group, n_groups = eng.fof(np.float32({b2!r}))
    rounds = eng.fof_rounds
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, group=group, meta=np.array([n_groups, rounds]), pos=p)
"""


def test_two_processes_host_transport_equal_one_process(nb, ref, tmp_path):
    n, world = 1500, 2
    b2 = float(b2_for(n, 0.9))
    out = str(tmp_path / "fof")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out, b2=b2), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now = got[0]["pos"]
    assert np.array_equal(now.view(np.uint32), got[1]["pos"].view(np.uint32))
    want, want_groups = ref.groups(now, np.float32(b2))
    with nb.NBody(n) as eng:   # one process at the same state: the rounds every rank must report
        eng.upload(now, np.zeros_like(now))
        one = eng.fof(np.float32(b2))
        one_rounds = eng.fof_rounds
    assert np.array_equal(one[0], want) and one[1] == want_groups
    for r in range(world):   # every rank returns the one-process values over ALL N bodies
        assert got[r]["group"].shape == (n,) and np.array_equal(got[r]["group"], want), r
        assert list(got[r]["meta"]) == [want_groups, one_rounds], r


@pytest.mark.parametrize("fp64", [False, True])
def test_cross_checks_against_the_neighbour_pass(nb, fp64):
    dtype = np.float64 if fp64 else np.float32
    n = 2100
    for pos in (nb.make_bodies(n, dtype=dtype)[0], planted(nb, n, dtype)):
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, np.zeros_like(pos))
            for b2 in [b2_for(n, r, dtype) for r in (0.3, 0.7, 1.5)] + [dtype(2.0 ** -24)]:
                group, n_groups = eng.fof(b2)
                idx, d2, count = eng.neighbors(r2=b2)
                me = np.arange(n)
                sizes = np.bincount(group, minlength=n)
                assert np.array_equal(count == 0, sizes[group] == 1)        # nobody within b: a group of one, and only then
                near = d2 <= b2
                assert np.array_equal(group[idx[near]], group[near])        # the nearest body, if within b, is in the same group
                assert np.all(group <= me) and np.array_equal(group[group], group)
                assert n_groups == int((group == me).sum())


def test_fof_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    b2 = b2_for(n, 0.9)
    check_step_untouched(nb, monkeypatch, n, lambda eng: eng.fof(b2), "NBODY_FOF_SPLIT", (([1] * 6, 0, False),) + PLANS[1:])


def test_interleaved_with_knn_neighbors_and_field(nb, ref, tmp_path_factory, monkeypatch):
    """fof takes its split scratch from the buffer the point passes share (q_scratch): on one context, twice over — fof over three
    chunks in batches, knn_at, nearest, the field, fof unsplit — everything equals its reference, the field the bits of a context that
    ran nothing else."""
    n, m = 2100, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    kref = knn_common.make_ref(tmp_path_factory.mktemp("knn_ref"))
    nref = neighbors_common.make_ref(tmp_path_factory.mktemp("neighbors_ref"))
    b2 = b2_for(n, 0.9)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        field_alone = eng.field(pts, skip)
    want_knn, want_near, want_fof = kref.points(pos, pts, 5, skip), nref.points(pos, pts, skip), ref.groups(pos, b2)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for _ in range(2):
            monkeypatch.setenv("NBODY_FOF_SPLIT", "3")
            monkeypatch.setenv("NBODY_FOF_SCRATCH_MB", "0.007")   # 7340 B against 3 x 4 B a row: 611 fit, batches of 512
            assert np.array_equal(eng.fof(b2)[0], want_fof[0])
            monkeypatch.delenv("NBODY_FOF_SPLIT")
            monkeypatch.delenv("NBODY_FOF_SCRATCH_MB")
            monkeypatch.setenv("NBODY_KNN_SPLIT", "3")
            assert knn_common.same(eng.knn_at(pts, 5, skip), want_knn)
            monkeypatch.delenv("NBODY_KNN_SPLIT")
            assert neighbors_common.same(eng.nearest(pts, skip)[:2], want_near[:2])
            assert knn_common.same(eng.field(pts, skip), field_alone)
            group, n_groups = eng.fof(b2)
            assert np.array_equal(group, want_fof[0]) and n_groups == want_fof[1]


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    n = 100
    group, out = np.full(n, 7, np.int32), np.full(2, 7, np.int32)
    untouched = lambda: np.all(group == 7) and np.all(out == 7)
    calls = (lambda: lib.nbody_fof(0.25, ip(group), ip(out[:1]), ip(out[1:])), lambda: lib.nbody_fof_d(0.25, ip(group), ip(out[:1]), ip(out[1:])))
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [c() for c in calls] == [E.ERR_STATE] * 2
        finally:
            mb.serve(False)
        assert untouched()
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        assert calls[1]() == E.ERR_STATE and untouched()
        assert lib.nbody_fof(0.25, None, None, None) == E.ERR_ARG
        assert lib.nbody_fof(0.25, None, None, ip(out[1:])) == E.ERR_ARG
        for bad in (float("nan"), -1.0, -1e-30, float("-inf")):
            assert lib.nbody_fof(bad, ip(group), ip(out[:1]), ip(out[1:])) == E.ERR_ARG, bad
            with pytest.raises(ValueError):
                eng.fof(bad)
        assert untouched() and eng.fof_rounds is None
        want, want_groups = eng.fof(0.25)
        assert lib.nbody_fof(0.25, ip(group), None, None) == 0 and np.array_equal(group, want) and np.all(out == 7)
        group[:] = 7
        assert lib.nbody_fof(0.25, None, ip(out[:1]), None) == 0 and np.all(group == 7) and out[0] == want_groups and out[1] == 7
        assert lib.nbody_fof(float("inf"), ip(group), ip(out[:1]), ip(out[1:])) == 0 and np.all(group == 0) and list(out) == [1, 2]
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert calls[0]() == E.ERR_STATE and calls[1]() == 0


def test_n65536(nb, ref):
    """a mid-size system (4 x 10^9 pairs a round) at 0.7 mean spacings with the split automatic: many workgroups, most windows
    walked once, several rounds over a shrinking list of active rows"""
    n = 65536
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        check(eng, ref, pos, b2_for(n, 0.7), n)
