"""The snap at rows and at phase-space points (nbody_snap(_d), nbody_snap_rows(_d); include/nbody.h "snap"): bit for bit against
tests/snap_ref.c in the strict modes, within the derived bound in the timed arithmetic, the acceleration and the jerk against the jerk
pass in every arithmetic, the rows form against the points form, the same bits however the work is laid out (source split, batches,
device and process count), the masses, hand-made special systems, no effect on the step, and the guards."""
import ctypes as C

import numpy as np
import pytest

from field_common import compile_ref, make_points, make_skip
from pass_common import bits, check_step_untouched, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from snap_common import TIMED_BOUND, TIMED_BOUND_HOSTILE, TIMED_SHAPE, SnapRef, numpy_snap, worst
from specials_common import POINT_COUNTS as HOSTILE_POINT_COUNTS
from specials_common import SIZES as HOSTILE_SIZES
from specials_common import VARIANTS, hostile_dynamic_system, hostile_point_words, hostile_points, nan_row, near, same_nan, special_row

pytestmark = pytest.mark.gpu
SIZES = (1, 2, 63, 257, 1025, 2100)   # one body, a pair, a tail below a wave, a block edge, two blocks, three blocks with a tail
POINT_COUNTS = (1, 255, 256, 257)     # a lane, a workgroup less one, a workgroup, a workgroup and a tail
F32_MODES = ("ARITH_FMA3", "ARITH_REFERENCE", "ARITH_STRICT", "ARITH_REFERENCE_STRICT")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return SnapRef(compile_ref(tmp_path_factory.mktemp("snap_ref"), "snap_ref"))


def point_words(nb, m, dtype=np.float32):
    """the points' velocities (test_gpu_jerk.py's) and accelerations"""
    return nb.make_bodies(m, seed=78, dtype=dtype)[1], nb.make_bodies(m, seed=79, dtype=dtype)[1]


def queries(nb, pos, m):
    pts, on = make_points(nb, pos, m)
    pvel, pacc = point_words(nb, m, pos.dtype.type)
    return pts, pvel, pacc, make_skip(len(pos), m, on)


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_strict_bit_for_bit(nb, ref, arith):
    """rows and points, with and without skip; the sources' accelerations of the points form are the statement's own first pass, which
    the device's opening jerk pass must reproduce for any later bit to agree"""
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    r = mode == nb.ARITH_REFERENCE_STRICT
    for n in SIZES:
        pos, vel = nb.make_bodies(n, dtype=dtype)
        want_rows = ref.rows(pos, vel, dtype, ref=r)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            eng.upload(pos, vel)
            rows = eng.snap()
            assert same(rows, want_rows), (n, [int((bits(g) != bits(w)).any(1).sum()) for g, w in zip(rows, want_rows)])
            assert all(np.all(o[:, 3] == 0) for o in rows)
            for m in POINT_COUNTS:
                pts, pvel, pacc, sk = queries(nb, pos, m)
                for skip in (None, sk):
                    want = ref.f64(pos, vel, want_rows[0], pts, pvel, pacc, skip) if fp64 else ref.f32(pos, vel, want_rows[0], pts, pvel, pacc, skip, ref=r)
                    assert same(eng.snap_at(pts, pvel, pacc, skip), want), (n, m, skip is not None)


@pytest.mark.parametrize("fp64", [False, True])
def test_acceleration_and_jerk_are_the_jerk_pass_bit_for_bit(nb, fp64):
    """in all four binary32 arithmetics and both binary64 ones, the timed ones included: rows and points"""
    dtype = np.float64 if fp64 else np.float32
    modes = ("ARITH_FMA3", "ARITH_STRICT") if fp64 else F32_MODES
    for n in (63, 2100):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        pts, pvel, pacc, sk = queries(nb, pos, 257)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for mode in modes:
                eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
                a, j, s = eng.snap()
                assert same((a, j), eng.jerk()) and np.any(s[:, :3] != 0), (n, mode)
                for skip in (None, sk):
                    a, j, s = eng.snap_at(pts, pvel, pacc, skip)
                    assert same((a, j), eng.jerk_at(pts, pvel, skip)), (n, mode, skip is not None)


@pytest.mark.parametrize("form", ["fma3", "strict", "fp64"])
def test_rows_form_is_the_points_form(nb, form):
    """row i is the query (r_i, v_i, a_i) with skip = i and a_i the jerk pass's acceleration, bit for bit, on windows inside a wave,
    across a wave's edge, across a block's edge and over every row"""
    n = 2100
    fp64 = form == "fp64"
    pos, vel = nb.make_bodies(n, dtype=np.float64 if fp64 else np.float32)
    with nb.NBody(n, fp64=fp64) as eng:
        if form == "strict":
            eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos, vel)
        acc = eng.jerk()[0]
        every = eng.snap()
        for first, last in ((0, 1), (63, 66), (1000, 1100), (0, n)):
            rows = eng.snap(first, last - first)
            assert same(rows, eng.snap_at(pos[first:last], vel[first:last], acc[first:last], np.arange(first, last, dtype=np.int32))), (first, last)
            assert same(rows, tuple(o[first:last] for o in every))


def test_bits_do_not_depend_on_the_source_split_or_the_batches(nb, monkeypatch):
    """timed binary32 and strict binary64; NBODY_SNAP_SPLIT unset, 1, 2, 3, 7 (more than the three blocks there are); a scratch bound
    that cuts the queries into batches; and the opening jerk pass's own split"""
    n, m = 2100, 700   # three blocks
    for fp64 in (False, True):
        dtype = np.float64 if fp64 else np.float32
        pos, vel = nb.make_bodies(n, dtype=dtype)
        big, on = make_points(nb, pos, 40000)
        big_vel, big_acc = point_words(nb, 40000, dtype)
        pts, pvel, pacc, skip = big[:m], big_vel[:m], big_acc[:m], make_skip(n, m, on)
        with nb.NBody(n, fp64=fp64) as eng:
            if fp64:
                eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
            eng.upload(pos, vel)
            for env in ("NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB", "NBODY_JERK_SPLIT"):
                monkeypatch.delenv(env, raising=False)
            base, base_sk, base_rows = eng.snap_at(pts, pvel, pacc), eng.snap_at(pts, pvel, pacc, skip), eng.snap(900, 700)
            assert not same(base, base_sk)
            for split in ("1", "2", "3", "7"):
                monkeypatch.setenv("NBODY_SNAP_SPLIT", split)
                assert same(eng.snap_at(pts, pvel, pacc), base) and same(eng.snap_at(pts, pvel, pacc, skip), base_sk) and same(eng.snap(900, 700), base_rows), split
            monkeypatch.setenv("NBODY_JERK_SPLIT", "2")
            assert same(eng.snap_at(pts, pvel, pacc, skip), base_sk) and same(eng.snap(900, 700), base_rows)
            monkeypatch.delenv("NBODY_JERK_SPLIT")
            # 40000 queries x 3 blocks x 9 sums x 4 (8) B = 4.3 (8.6) MB of per-block sums against a bound of 1 MB: consecutive batches
            monkeypatch.delenv("NBODY_SNAP_SPLIT")
            monkeypatch.setenv("NBODY_SNAP_SCRATCH_MB", "1")
            s_big = eng.snap_at(big, big_vel, big_acc)
            monkeypatch.setenv("NBODY_SNAP_SPLIT", "1")
            s_one = eng.snap_at(big, big_vel, big_acc)
            assert same(s_big, s_one) and same(tuple(o[:m] for o in s_big), base)
            monkeypatch.setenv("NBODY_SNAP_SPLIT", "3")
            assert same(eng.snap_at(big, big_vel, big_acc), s_one)
            monkeypatch.setenv("NBODY_SNAP_SCRATCH_MB", "0")   # not even one workgroup's queries fit: no split
            assert same(eng.snap_at(pts, pvel, pacc, skip), base_sk) and same(eng.snap(900, 700), base_rows)
            monkeypatch.delenv("NBODY_SNAP_SPLIT")
            monkeypatch.delenv("NBODY_SNAP_SCRATCH_MB")


def test_bits_do_not_depend_on_the_device_count(nb, monkeypatch):
    """three oversubscribed devices after a step — each holds only its own slice's new positions and velocities and computes only its
    own rows' accelerations; the pass brings the rest first — against one device that is given the same state; timed binary32"""
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n, m = 2100, 257
    pos, vel = nb.make_bodies(n)
    pts, pvel, pacc, skip = queries(nb, pos, m)
    probe = lambda eng: (eng.snap_at(pts, pvel, pacc, skip), eng.snap_at(pts[:2], pvel[:2], pacc[:2]), eng.snap(), eng.snap(600, 900))
    with nb.NBody(n, ngpus=3) as eng:
        eng.upload(pos, vel)
        eng.step(0.01, 1)
        three = probe(eng)
        now, vnow = eng.download()
    assert not same(now, pos) and not same(vnow, vel), "no step happened"
    with nb.NBody(n) as eng:
        eng.upload(now, vnow)
        one = probe(eng)
    for k in range(4):
        assert same(three[k], one[k]), k
    assert same(three[3], tuple(o[600:1500] for o in three[2]))   # a window across both device boundaries


WORKER = """
    from field_common import make_points, make_skip
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m = (257, 41)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    pvel, pacc = nb.make_bodies(m, seed=78 + rank)[1], nb.make_bodies(m, seed=90 + rank)[1]
    a, j, s = eng.snap_at(pts, pvel, pacc, make_skip(n, m, on))
    ra, rj, rs = eng.snap()                                   # this rank's own rows
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, a=a, j=j, s=s, ra=ra, rj=rj, rs=rs, first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p, vel=v)
"""


def test_two_processes_host_transport_equal_one_process(nb, tmp_path):
    """after three steps each rank holds only its own velocities and computes only its own rows' accelerations: both must really be
    gathered, and the velocities again after the accelerations have passed through the same buffer"""
    n, world = 2100, 2
    out = str(tmp_path / "sn")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now, vnow = got[0]["pos"], got[0]["vel"]
    assert same((now, vnow), (got[1]["pos"], got[1]["vel"]))
    pos, vel = nb.make_bodies(n, seed=33)
    assert not same(vnow, vel)
    covered = 0
    with nb.NBody(n) as one:
        one.upload(now, vnow)
        rows = one.snap()
        for r, m in enumerate((257, 41)):
            pts, on = make_points(nb, pos, m, seed=50 + r)
            pvel, pacc = nb.make_bodies(m, seed=78 + r)[1], nb.make_bodies(m, seed=90 + r)[1]
            assert same((got[r]["a"], got[r]["j"], got[r]["s"]), one.snap_at(pts, pvel, pacc, make_skip(n, m, on))), r
            first, cnt = (int(v) for v in got[r]["first"])
            assert same((got[r]["ra"], got[r]["rj"], got[r]["rs"]), tuple(o[first:first + cnt] for o in rows)), r
            covered += cnt
    assert covered == n


def test_timed_fp32_within_tolerance(nb, ref):
    """n = 65536, m = 512 (jerk_common.TIMED_SHAPE), with skip indices, |got - want64| / mag, all three outputs, bound
    snap_common.TIMED_BOUND = 2 r + 7 * 2^-23 = 6.83e-6: the rounding paths differ by no more than the statement's own error r (asserted
    on the CPU at this shape: r <= 3e-6, tests/test_snap_abi.py); the timed form differs from the strict one by v_rsq_f32's <= 1 ulp,
    which enters a snap term through inv3 three-fold and through alpha, beta or b two-fold each, inv^7 at the most.  want64 takes the
    accelerations the device's own opening pass gives the sources in the same arithmetic: numpy binary64 for the FMA3 form, which also
    gives the magnitude sums, and tests/snap_ref.c's binary64 (within 1e-13 of numpy in this measure, asserted on the CPU) for the
    reference's form — one numpy evaluation of 512 x 65536 pairs, not two.
    Measured on an MI355X: snap 2.49e-6 (FMA3) and 2.68e-6 (REFERENCE), jerk 1.59e-6 and 1.47e-6, acceleration 4.4e-7 and 4.2e-7 — the
    strict statement's own figures."""
    n, m = TIMED_SHAPE
    pos, vel = nb.make_bodies(n)
    pts, pvel, pacc, skip = queries(nb, pos, m)
    mag = None
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
            eng.set_option(nb.OPT_ARITH, mode)
            acc = eng.jerk()[0]
            got = eng.snap_at(pts, pvel, pacc, skip)
            if mag is None:
                full = numpy_snap(pos, vel, acc, pts, pvel, pacc, skip)
                want, mag = full[:3], full[3:]
            else:
                want = [w[:, :3] for w in ref.f64(pos, vel, acc, pts, pvel, pacc, skip)]
            e = [worst(got[i], want[i], mag[i]) for i in range(3)]
            print("timed fp32 arith %d: accel %.3e jerk %.3e snap %.3e (bound %.3e)" % (mode, *e, TIMED_BOUND))
            assert max(e) <= TIMED_BOUND, mode


@pytest.mark.parametrize("fp64", [False, True])
def test_masses(nb, ref, fp64):
    """every w = 1 gives the unweighted bits; the weighted strict bits are the statement's; masses x 4 together with velocities x 2 give
    accel x 4, jerk x 8 and snap x 16 exactly (every operation scales by a power of two); appended w = +0 tracers change no bit of the
    first N rows.  Timed binary32 and timed binary64 for the identities, the strict mode for the statement."""
    dtype = np.float64 if fp64 else np.float32
    n, extra = 2100, 70
    pos, vel = nb.make_bodies(n + extra, dtype=dtype)
    pos[:, 3] = (0.25 * 16.0 ** np.random.default_rng(5).random(n + extra)).astype(dtype)
    unit = pos[:n].copy()
    unit[:, 3] = 1
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(unit, vel[:n])
        plain = eng.snap()
        eng.use_masses()
        assert same(eng.snap(), plain)
        eng.upload(pos[:n], vel[:n])
        base = eng.snap()
        assert not same(base, plain)
        heavy, fast = pos[:n].copy(), vel[:n].copy()
        heavy[:, 3] *= 4
        fast[:, :3] *= 2
        eng.upload(heavy, fast)
        scaled = eng.snap()
        for k, factor in enumerate((4, 8, 16)):
            assert same(scaled[k], (base[k] * dtype(factor)).astype(dtype)), factor
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos[:n], vel[:n])
        assert same(eng.snap(), ref.rows(pos[:n], vel[:n], dtype, mass=True))
        eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
    tracers = pos.copy()
    tracers[n:, 3] = 0.0
    with nb.NBody(n + extra, fp64=fp64) as eng:
        eng.use_masses()
        eng.upload(tracers, vel)
        with_tracers = eng.snap()
    assert same(tuple(o[:n] for o in with_tracers), base)
    assert np.any(with_tracers[2][n:, :3] != 0)   # a tracer is accelerated and moves no one


def hand_made(dtype):
    """{name: (pos, vel)}: two- and three-body systems whose answers the DOMAIN paragraph states.  on_body: rows 0 and 1 coincide and
    move together; overflow: row 2 is so far that d2 overflows, inv = 0, and slow enough that no product with it does; nan: row 1 is NaN"""
    big = dtype(np.sqrt(float(np.finfo(dtype).max)) * 4)
    z = lambda rows: np.array(rows, dtype)
    return {
        "on_body": (z([[0.25, -0.5, 0.125, 1], [0.25, -0.5, 0.125, 1], [1, 1, 0.5, 1]]), z([[0.5, 0.25, 0, 0], [0.5, 0.25, 0, 0], [-0.25, 0, 0.5, 0]])),
        "overflow": (z([[0, 0, 0, 1], [0.5, 0.25, -0.125, 1], [big, 0, 0, 1]]), z([[0.25, 0, 0, 0], [0, -0.5, 0.25, 0], [0, 2.0 ** -80, 0, 0]])),
        "nan": (z([[0, 0, 0, 1], [np.nan, 0.25, 0, 1], [0.5, 0.5, 0.5, 1]]), z([[0.25, 0, 0, 0], [0, 0.5, 0, 0], [0, 0, -0.25, 0]])),
        "pair": (z([[0, 0, 0, 1], [0.5, 0.25, -0.125, 1]]), z([[0.25, 0, 0, 0], [0, -0.5, 0.25, 0]])),
    }


@pytest.mark.parametrize("fp64", [False, True])
def test_hand_made_specials_bit_for_bit(nb, ref, fp64):
    """the systems of hand_made() in the strict modes against the statement, NaN for NaN and bit for bit elsewhere, and what
    include/nbody.h's DOMAIN paragraph says of each, directly"""
    dtype = np.float64 if fp64 else np.float32
    for name, (pos, vel) in hand_made(dtype).items():
        n = len(pos)
        with nb.NBody(n, fp64=fp64) as eng:
            for mode in ((nb.ARITH_STRICT,) if fp64 else (nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)):
                eng.set_option(nb.OPT_ARITH, mode)
                eng.upload(pos, vel)
                got = eng.snap()
                want = ref.rows(pos, vel, dtype, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                assert all(same_nan(g, w) for g, w in zip(got, want)), (name, mode)
                a, j, s = got
                if name == "on_body":   # the twin adds +0 to all three: rows 0 and 1 get what row 2 alone gives them, identical bits
                    assert all(same(o[0], o[1]) for o in got) and np.all(np.isfinite(s))
                    alone = eng.snap_at(pos[:1], vel[:1], a[:1], np.array([1], np.int32))
                    assert same(tuple(o[:1] for o in got), alone)
                if name == "overflow":   # the far body contributes +0 and receives +0: rows 0 and 1 are the pair's
                    pair_pos, pair_vel = hand_made(dtype)["pair"]
                    assert np.all(np.isfinite(s)) and not bits(np.stack([o[2] for o in got])).any()
                    assert same(tuple(o[:2] for o in got), ref.rows(pair_pos, pair_vel, dtype, ref=(mode == nb.ARITH_REFERENCE_STRICT)))
                if name == "nan":   # the NaN body poisons every row: directly, and through the accelerations beside it
                    assert all(np.all(np.isnan(o[:, :3])) for o in got)


def test_snap_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, pvel, pacc, sk = queries(nb, nb.make_bodies(n)[0], 257)
    probe = lambda eng: (eng.snap_at(pts, pvel, pacc), eng.snap_at(pts, pvel, pacc, sk), eng.snap(), eng.snap(700, 7))
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_SNAP_SPLIT", plans=(([1] * 6, 0, False), ([64, 6, 64], 1, False), ([3, 2], 0, True)))


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64 = C.POINTER(C.c_float), C.POINTER(C.c_double)
    w32, w64 = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float64)
    o32, o64 = [np.full((4, 4), 7, np.float32) for _ in range(3)], [np.full((4, 4), 7, np.float64) for _ in range(3)]
    sk = np.array([-1, 0, 3, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    p32, p64 = (lambda a: a.ctypes.data_as(f32)), (lambda a: a.ctypes.data_as(f64))
    call32 = lambda: lib.nbody_snap(p32(w32), p32(w32), p32(w32), 4, ip(sk), *(p32(o) for o in o32))
    call64 = lambda: lib.nbody_snap_d(p64(w64), p64(w64), p64(w64), 4, ip(sk), *(p64(o) for o in o64))
    rows32 = lambda: lib.nbody_snap_rows(0, 4, *(p32(o) for o in o32))
    rows64 = lambda: lib.nbody_snap_rows_d(0, 4, *(p64(o) for o in o64))
    untouched = lambda outs: all(np.all(o == 7) for o in outs)

    def reset():
        for o in o32 + o64:
            o[...] = 7

    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [call32(), call64(), rows32(), rows64()] == [E.ERR_STATE] * 4
        finally:
            mb.serve(False)
        assert untouched(o32) and untouched(o64)
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        x, (a, j, s) = p32(w32), (p32(o) for o in o32)
        assert lib.nbody_snap(None, x, x, 4, None, a, j, s) == E.ERR_ARG
        assert lib.nbody_snap(x, None, x, 4, None, a, j, s) == E.ERR_ARG
        assert lib.nbody_snap(x, x, None, 4, None, a, j, s) == E.ERR_ARG
        assert lib.nbody_snap(x, x, x, 4, None, None, None, None) == E.ERR_ARG
        assert lib.nbody_snap(x, x, x, 0, None, a, j, s) == E.ERR_ARG
        assert lib.nbody_snap(x, x, x, -3, None, a, j, s) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_snap(x, x, x, 4, ip(sk), a, j, s) == E.ERR_ARG, bad
        assert lib.nbody_snap_rows(0, 4, None, None, None) == E.ERR_ARG
        for first, cnt in ((-1, 4), (0, 0), (0, -1), (n, 1), (n - 3, 4), (0, n + 1)):
            assert lib.nbody_snap_rows(first, cnt, a, j, s) == E.ERR_ARG, (first, cnt)
        assert untouched(o32)
        assert [call64(), rows64()] == [E.ERR_STATE] * 2 and untouched(o64)
        sk[:] = (-1, 0, n - 1, n - 1)
        full = eng.snap_at(w32, w32, w32, sk)
        full_rows = eng.snap(n - 4, 4)
        for keep in range(3):   # each output alone, and each output NULL in turn
            for only in (True, False):
                reset()
                ptrs = [p32(o) if (k == keep) == only else None for k, o in enumerate(o32)]
                assert lib.nbody_snap(x, x, x, 4, ip(sk), *ptrs) == 0
                for k, o in enumerate(o32):
                    assert (same(o, full[k]) if ptrs[k] is not None else np.all(o == 7)), (keep, only, k)
                reset()
                assert lib.nbody_snap_rows(n - 4, 4, *ptrs) == 0
                for k, o in enumerate(o32):
                    assert (same(o, full_rows[k]) if ptrs[k] is not None else np.all(o == 7)), (keep, only, k)
    with nb.NBody(n, fp64=True) as eng:
        sk[:] = (-1, 0, 3, 2)
        reset()
        assert [call32(), rows32()] == [E.ERR_STATE] * 2 and untouched(o32)
        assert [call64(), rows64()] == [0, 0] and not untouched(o64)


# ---- the hostile system (specials_common.py): what a uniform cloud never shows the pass ----

def check_specials_directly(got, pts, skip, n, variant, what, planted=0):
    """What include/nbody.h promises without any reference (test_gpu_jerk.py's check, extended to the snap): a skipped body leaves no
    trace in the nine sums, so a finite query that skips the NaN, inf or overflow body has a finite acceleration (planted: how many such
    queries there must be); a NaN body poisons the acceleration and the jerk of every query that does not skip it and, through the a_j
    of the bodies beside it, the snap of EVERY query; and in the finite variants point 1, which sits on body 0 with that body's own
    velocity and acceleration and does not skip it, gets +0 from it in all three outputs: the bits of point 0, which does skip it."""
    a, j, s = got
    special = special_row(n, variant)
    sk = np.full(len(pts), -1, np.int32) if skip is None else skip
    if special is not None:
        clean = near(pts) & (sk == special)
        assert clean.sum() >= planted, what
        assert np.all(np.isfinite(a[clean])), what
    if variant == "nan":
        hit = sk != nan_row(n)
        assert np.all(np.isnan(a[hit][:, :3])) and np.all(np.isnan(j[hit][:, :3])) and np.all(np.isnan(s[:, :3])), what
    if variant in ("base", "overflow") and len(pts) > 1:
        assert all(same(o[0], o[1]) and np.all(np.isfinite(o[:2])) for o in got), what


def hostile_queries(nb, pos, vel, acc, m, variant):
    pts, skip = hostile_points(nb, pos, m, variant)
    pvel, pacc = hostile_point_words(nb, m, pos.dtype.type, vel, acc)
    return pts, pvel, pacc, skip


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_hostile_system_strict_bit_for_bit(nb, ref, arith, monkeypatch):
    """hostile_dynamic_system in every variant and size, every query count, with and without the hostile skip, the one-launch form and
    the scratch + combine form (NBODY_SNAP_SPLIT unset, 1, 2, 3), and the rows form: all three outputs bit for bit tests/snap_ref.c (NaN
    for NaN), whose `continue` on j == skip is the definition.  The sources' accelerations are the statement's own first pass, which
    the device's opening pass must reproduce; points 0 and 1 carry body 0's own velocity and acceleration."""
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    r = mode == nb.ARITH_REFERENCE_STRICT
    differ = []
    for n in HOSTILE_SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            for variant in VARIANTS:
                pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
                with np.errstate(all="ignore"):
                    want_rows = ref.rows(pos, vel, dtype, ref=r)
                eng.upload(pos, vel)
                for m in HOSTILE_POINT_COUNTS:
                    pts, pvel, pacc, hsk = hostile_queries(nb, pos, vel, want_rows[0], m, variant)
                    for skip in (None, hsk):
                        with np.errstate(all="ignore"):
                            want = ref.f64(pos, vel, want_rows[0], pts, pvel, pacc, skip) if fp64 else ref.f32(pos, vel, want_rows[0], pts, pvel, pacc, skip, ref=r)
                        what = (n, variant, m, skip is not None)
                        planted = 2 if skip is not None and m >= 65 else 0
                        check_specials_directly(want, pts, skip, n, variant, what, planted)     # the statement itself keeps the promise
                        for split in (None, "1", "2", "3"):
                            if split is None:
                                monkeypatch.delenv("NBODY_SNAP_SPLIT", raising=False)
                            else:
                                monkeypatch.setenv("NBODY_SNAP_SPLIT", split)
                            got = eng.snap_at(pts, pvel, pacc, skip)
                            if not all(same_nan(g, w) for g, w in zip(got, want)):
                                differ.append(what + (split, [int((bits(g) != bits(w)).any(1).sum()) for g, w in zip(got, want)]))
                            check_specials_directly(got, pts, skip, n, variant, what + (split,), planted)
                monkeypatch.delenv("NBODY_SNAP_SPLIT", raising=False)
                rows = eng.snap()
                if not all(same_nan(g, w) for g, w in zip(rows, want_rows)):
                    differ.append((n, variant, "rows", [int((bits(g) != bits(w)).any(1).sum()) for g, w in zip(rows, want_rows)]))
    assert not differ, differ   # every input where the device and the statement differ, none dropped


def skipped_special_leaves_no_trace(nb, ref, eng, pos, vel, acc, queries_, n, variant, got, strict, is_ref):
    """The queries that skip the variant's special body get, bit for bit, what they get once that body is an ordinary one: nothing of
    it reaches their nine sums.  The acceleration and the jerk: against the device's own run with the body at (0.25, 0.25, 0.25) moving
    with (0.5, 0.5, 0.5).  The snap cannot be compared that way — an ordinary body changes the a_j of every other source (include/nbody.h:
    a NaN body reaches every snap through them) — so it is compared (a) in the strict modes against the statement on that ordinary body
    with the device's own a_j and 0.75 in the body's acceleration word, and (b) in "overflow", in every arithmetic, against the device's
    run with the body at another position whose square overflows and with another velocity: it gives every other source +0 as before."""
    pts, pvel, pacc, skip = queries_
    special = special_row(n, variant)
    if special is None or skip is None or not np.any(skip == special):
        return []
    sel, differ = skip == special, []
    tame_p, tame_v, tame_a = pos.copy(), vel.copy(), acc.copy()
    tame_p[special, :3], tame_v[special, :3], tame_a[special, :3] = 0.25, 0.5, 0.75
    eng.upload(tame_p, tame_v)
    tame = eng.snap_at(pts, pvel, pacc, skip)
    if not (same_nan(got[0][sel], tame[0][sel]) and same_nan(got[1][sel], tame[1][sel])):
        differ.append("ordinary body: acceleration or jerk")
    if strict:
        with np.errstate(all="ignore"):
            want = ref.of(pos.dtype)(tame_p, tame_v, tame_a, pts, pvel, pacc, skip, **({"ref": True} if is_ref else {}))
        if not all(same_nan(g[sel], w[sel]) for g, w in zip(got, want)):
            differ.append("ordinary body, its acceleration word included: the statement")
    if variant == "overflow":
        moved_p = pos.copy()
        moved_p[special, :3] = -pos[special, [1, 2, 0]]
        eng.upload(moved_p, tame_v)
        moved = eng.snap_at(pts, pvel, pacc, skip)
        if not all(same_nan(g[sel], w[sel]) for g, w in zip(got, moved)):
            differ.append("moved body")
    eng.upload(pos, vel)
    return differ


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system_every_arithmetic(nb, ref, fp64):
    """Every arithmetic — the timed ones (v_rsq_f32; the v_rsq_f64 seed + one third-order step) and the strict ones — on
    hostile_dynamic_system: all three outputs finite and NaN exactly where the strict statement of the same d2 form is, given the
    accelerations the device's own opening pass gives the sources, in every variant, with and without skip; a skipped NaN, inf or
    overflow body leaves no trace (skipped_special_leaves_no_trace); a NaN body poisons every query that does not skip it."""
    dtype = np.float64 if fp64 else np.float32
    modes = (nb.ARITH_FMA3, nb.ARITH_STRICT) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)
    differ = []
    for n in HOSTILE_SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            for variant in VARIANTS:
                pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                for mode in modes:
                    eng.set_option(nb.OPT_ARITH, mode)
                    is_ref = mode in (nb.ARITH_REFERENCE, nb.ARITH_REFERENCE_STRICT)
                    strict = mode in (nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)
                    acc = eng.jerk()[0]
                    pts, pvel, pacc, hsk = hostile_queries(nb, pos, vel, acc, 300, variant)
                    for skip in (hsk, None):
                        what = (n, variant, mode, skip is not None)
                        with np.errstate(all="ignore"):
                            want = ref.f64(pos, vel, acc, pts, pvel, pacc, skip) if fp64 else ref.f32(pos, vel, acc, pts, pvel, pacc, skip, ref=is_ref)
                        got = eng.snap_at(pts, pvel, pacc, skip)
                        for k, (g_, w) in enumerate(zip(got, want)):
                            if not (np.array_equal(np.isfinite(g_), np.isfinite(w)) and np.array_equal(np.isnan(g_), np.isnan(w))):
                                differ.append(what + (k, np.flatnonzero((np.isfinite(g_) != np.isfinite(w)).any(1) | (np.isnan(g_) != np.isnan(w)).any(1))[:8]))
                        check_specials_directly(got, pts, skip, n, variant, what, 2 if skip is not None else 0)
                        differ += [what + (d,) for d in skipped_special_leaves_no_trace(nb, ref, eng, pos, vel, acc, (pts, pvel, pacc, skip), n, variant, got,
                                                                                        strict, is_ref)]
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
    assert not differ, differ   # an input where the patterns differ is reported, not dropped


def test_hostile_system_timed_fp32_within_tolerance(nb):
    """ "base" and "overflow", every size, 300 hostile queries with and without skip, both timed binary32 arithmetics: |got - want64| / mag
    of the snap, the jerk and the acceleration on the near queries that are finite in binary64 (at least 290 of 300, asserted) within
    snap_common.TIMED_BOUND_HOSTILE = 2 R_REF_HOSTILE + 7 * 2^-23 = 1.08e-5 — TIMED_BOUND's rule with the statement's own figure on this
    system (4.93e-6, tests/test_specials_dynamic_reference.py).  want64 is numpy binary64 with the accelerations the device's own
    opening pass gives the sources in the same arithmetic.
    Measured on an MI355X, worst over sizes, variants and skip: see the printed lines."""
    worst_of = {}
    for n in HOSTILE_SIZES:
        with nb.NBody(n) as eng:
            for variant in ("base", "overflow"):
                pos, vel, far = hostile_dynamic_system(nb, n, np.float32, variant)
                eng.upload(pos, vel)
                for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                    eng.set_option(nb.OPT_ARITH, mode)
                    acc = eng.jerk()[0]
                    pts, pvel, pacc, hsk = hostile_queries(nb, pos, vel, acc, 300, variant)
                    for skip in (hsk, None):
                        got = eng.snap_at(pts, pvel, pacc, skip)
                        full = numpy_snap(pos, vel, acc, pts, pvel, pacc, skip)
                        keep = near(pts) & np.all([np.isfinite(o).all(1) for o in full], axis=0)
                        assert keep.sum() >= 290, (n, variant, mode)
                        e = [worst(got[i][keep], full[i][keep], full[3 + i][keep]) for i in range(3)]
                        worst_of[(n, mode)] = [max(a, b) for a, b in zip(worst_of.get((n, mode), [0.0] * 3), e)]
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
    for (n, mode), e in sorted(worst_of.items()):
        print("hostile timed fp32 n=%d arith %d: accel %.3e jerk %.3e snap %.3e (bound %.3e)" % (n, mode, *e, TIMED_BOUND_HOSTILE))
    assert all(max(e) <= TIMED_BOUND_HOSTILE for e in worst_of.values()), worst_of
