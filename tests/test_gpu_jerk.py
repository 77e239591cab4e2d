"""The jerk at rows and at phase-space points (nbody_jerk(_d), nbody_jerk_rows(_d); include/nbody.h "jerk"): bit for bit against
tests/jerk_ref.c in the strict modes, within derived bounds in the timed arithmetic, the rows form against the points form, the
acceleration against the field pass, all of it again on the hostile system of specials_common.py, the same bits however the work is laid
out (source split, batches, sub-ranges, force configuration, device and process count), no effect on the step, the jerk as the time
derivative of the field, the guards and the C host program's --jerk line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from field_common import FieldRef, compile_ref, make_points, make_skip
from jerk_common import TIMED_SHAPE, JerkRef, derivative_error, derivative_queries, numpy_jerk, worst
from pass_common import FORCE_CONFIGS, bits, check_step_untouched, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import POINT_COUNTS, SIZES, VARIANTS, hostile_points, hostile_system, nan_row, near, same_nan, special_row
from tidal_common import GRADIENT_H

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5   # the project's north_star tolerance (TOL in tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return JerkRef(compile_ref(tmp_path_factory.mktemp("jerk_ref"), "jerk_ref"))


@pytest.fixture(scope="module")
def field_ref(tmp_path_factory):
    return FieldRef(compile_ref(tmp_path_factory.mktemp("field_ref"), "field_ref"))


def point_velocities(nb, m, dtype=np.float32):
    return nb.make_bodies(m, seed=78, dtype=dtype)[1]


@pytest.mark.parametrize("arith", ["strict", "reference_strict"])
def test_strict_fp32_bit_for_bit(nb, ref, arith):
    mode = {"strict": nb.ARITH_STRICT, "reference_strict": nb.ARITH_REFERENCE_STRICT}[arith]
    for n in (1, 2, 63, 64, 65, 1000, 1025, 4099):
        pos, vel = nb.make_bodies(n)
        with nb.NBody(n) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            eng.upload(pos, vel)
            for m in (1, 64, 65, 257, 1000):
                pts, on = make_points(nb, pos, m)
                pvel = point_velocities(nb, m)
                for skip in (None, make_skip(n, m, on)):
                    want = ref.f32(pos, vel, pts, pvel, skip, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                    got = eng.jerk_at(pts, pvel, skip)
                    assert same(got, want), (n, m, skip is not None, int((got[1] != want[1]).any(1).sum()))


def test_fp64(nb, ref):
    """strict: tests/jerk_ref.c bit for bit.  Timed (the v_rsq_f64 seed refined to full precision): <= 1e-12 of mag against numpy
    binary64, the field's and the tidal's bound."""
    m = 257
    for n in (2, 1025, 4099):
        pos, vel = nb.make_bodies(n, dtype=np.float64)
        pts, on = make_points(nb, pos, m)
        pvel = point_velocities(nb, m, np.float64)
        with nb.NBody(n, fp64=True) as eng:
            eng.upload(pos, vel)
            for skip in (None, make_skip(n, m, on)):
                wa, wj, mag_a, mag_j = numpy_jerk(pos, vel, pts, pvel, skip)
                a, j = eng.jerk_at(pts, pvel, skip)
                ea, ej = worst(a, wa, mag_a), worst(j, wj, mag_j)
                print("fp64 timed n=%d skip=%s: accel %.3e jerk %.3e" % (n, skip is not None, ea, ej))
                assert max(ea, ej) <= 1e-12, n
                eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
                assert same(eng.jerk_at(pts, pvel, skip), ref.f64(pos, vel, pts, pvel, skip)), (n, skip is not None)
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)


@pytest.mark.parametrize("form", ["fma3", "strict", "fp64"])
def test_rows_form_is_the_points_form(nb, form):
    """row i is the query (r_i, v_i) with skip = i, bit for bit, on windows inside a wave, across a wave's edge, across a block's edge
    and over every row"""
    n = 4099
    fp64 = form == "fp64"
    pos, vel = nb.make_bodies(n, dtype=np.float64 if fp64 else np.float32)
    with nb.NBody(n, fp64=fp64) as eng:
        if form == "strict":
            eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos, vel)
        for first, last in ((0, 1), (63, 66), (1000, 1100), (0, n)):
            rows = eng.jerk(first, last - first)
            pts = eng.jerk_at(pos[first:last], vel[first:last], np.arange(first, last, dtype=np.int32))
            assert same(rows, pts), (first, last)
            assert np.all(rows[0][:, 3] == 0) and np.all(rows[1][:, 3] == 0)
        assert same(eng.jerk(), eng.jerk(0, n))


def test_acceleration_is_the_field_pass_bit_for_bit(nb):
    """in all four binary32 arithmetics and both binary64 ones; and zero velocities everywhere give a jerk of +0"""
    n, m = 4099, 300
    for fp64, modes in ((False, (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)), (True, (nb.ARITH_FMA3, nb.ARITH_STRICT))):
        dtype = np.float64 if fp64 else np.float32
        pos, vel = nb.make_bodies(n, dtype=dtype)
        pts, on = make_points(nb, pos, m)
        pvel = point_velocities(nb, m, dtype)
        skip = make_skip(n, m, on)
        with nb.NBody(n, fp64=fp64) as eng:
            for mode in modes:
                eng.set_option(nb.OPT_ARITH, mode)
                eng.upload(pos, vel)
                for sk in (None, skip):
                    a, j = eng.jerk_at(pts, pvel, sk)
                    assert same(a, eng.field(pts, sk, potential=False)[0]), (fp64, mode, sk is not None)
                    assert np.any(j[:, :3] != 0)
                eng.upload(pos, np.zeros_like(vel))
                a0, j0 = eng.jerk_at(pts, np.zeros_like(pvel), skip)
                assert same(a0, a) and not bits(j0).any(), (fp64, mode)
                assert not bits(eng.jerk(1000, 200)[1]).any(), (fp64, mode)


def test_timed_fp32_within_tolerance(nb):
    """n = 65536, m = 512 (jerk_common.TIMED_SHAPE, fixed in tests/test_jerk_abi.py), |got - want64| / mag against numpy binary64, both
    outputs, bound TOL = 1e-5, derived: the timed form differs from the strict one by v_rsq_f32's <= 1 ulp, which enters inv3
    three-fold and b two-fold: <= 5 * 2^-23 = 6e-7 of mag; the rounding paths differ by no more than the reference's own error r
    (asserted on the CPU at this shape: r <= 4.7e-6, tests/test_jerk_abi.py); 2 r + 6e-7 < 1e-5.
    Measured on an MI355X: jerk 1.587e-6 (FMA3) and 1.470e-6 (REFERENCE), acceleration 4.41e-7 and 4.16e-7, with and without skip —
    the strict reference's own figures (r = 1.59e-6)."""
    n, m = TIMED_SHAPE
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    pvel = point_velocities(nb, m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for skip in (None, make_skip(n, m, on)):
            wa, wj, mag_a, mag_j = numpy_jerk(pos, vel, pts, pvel, skip)
            for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                eng.set_option(nb.OPT_ARITH, mode)
                a, j = eng.jerk_at(pts, pvel, skip)
                ea, ej = worst(a, wa, mag_a), worst(j, wj, mag_j)
                print("timed fp32 arith %d skip=%s: accel %.3e jerk %.3e" % (mode, skip is not None, ea, ej))
                assert max(ea, ej) <= TOL, (mode, skip is not None)


def test_the_jerk_is_the_time_derivative_of_the_acceleration(nb, ref, field_ref):
    """The jerk against the central difference in time of eng.field's acceleration, binary64: the bodies uploaded at pos +- h vel, the
    50 queries (at least 0.05 from any body) at x +- h u.  The bound is a property of the references: the truncation error of the
    difference, estimated from the jerk itself at +-h, times 4, per query in the Euclidean norm; tests/jerk_ref.c and
    tests/field_ref.c must meet it (tests/test_jerk_abi.py asserts that too) before the device is asked, in both binary64 arithmetics."""
    n, h = 4099, GRADIENT_H
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    x, u = derivative_queries(nb, pos)
    err, trunc, scale = derivative_error(lambda b, p: field_ref.f64(b, p)[0], ref.f64, pos, vel, x, u, h)
    print("references: worst error / |j| %.3e, worst error / bound %.3f" % ((err / scale).max(), (err / (4 * trunc)).max()))
    assert np.all(err <= 4 * trunc)
    with nb.NBody(n, fp64=True) as eng:
        def field_of(bodies, p):
            eng.upload(bodies, vel)
            return eng.field(p, potential=False)[0]

        def jerk_of(bodies, v, p, pv):
            eng.upload(bodies, v)
            return eng.jerk_at(p, pv)

        for mode in (nb.ARITH_FMA3, nb.ARITH_STRICT):
            eng.set_option(nb.OPT_ARITH, mode)
            err, trunc, scale = derivative_error(field_of, jerk_of, pos, vel, x, u, h)
            print("device arith %d: worst error / |j| %.3e, worst error / bound %.3f" % (mode, (err / scale).max(), (err / (4 * trunc)).max()))
            assert np.all(err <= 4 * trunc), mode


def test_bits_do_not_depend_on_the_source_split_or_the_batches(nb, monkeypatch):
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    big, on = make_points(nb, pos, 70000)
    big_vel = point_velocities(nb, 70000)
    pts, pvel = big[:m], big_vel[:m]
    skip = make_skip(n, m, on)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        monkeypatch.delenv("NBODY_JERK_SPLIT", raising=False)
        base, base_sk, base_rows = eng.jerk_at(pts, pvel), eng.jerk_at(pts, pvel, skip), eng.jerk(900, 700)
        assert not same(base, base_sk)
        for split in ("1", "2", "3", "5", "64"):
            monkeypatch.setenv("NBODY_JERK_SPLIT", split)
            assert same(eng.jerk_at(pts, pvel), base) and same(eng.jerk_at(pts, pvel, skip), base_sk) and same(eng.jerk(900, 700), base_rows), split
        # 70000 queries x 5 blocks x 24 B = 8.4 MB of per-block sums against a bound of 1 MB: consecutive batches of 8704 queries
        monkeypatch.delenv("NBODY_JERK_SPLIT")
        monkeypatch.setenv("NBODY_JERK_SCRATCH_MB", "1")
        j_big = eng.jerk_at(big, big_vel)
        monkeypatch.setenv("NBODY_JERK_SPLIT", "1")
        j_one = eng.jerk_at(big, big_vel)
        assert same(j_big, j_one) and same(tuple(o[:m] for o in j_big), base)
        monkeypatch.setenv("NBODY_JERK_SPLIT", "4")
        assert same(eng.jerk_at(big, big_vel), j_one)
        monkeypatch.setenv("NBODY_JERK_SCRATCH_MB", "0")   # not even one workgroup's queries fit: no split
        assert same(eng.jerk_at(pts, pvel, skip), base_sk) and same(eng.jerk(900, 700), base_rows)


def test_bits_do_not_depend_on_the_queries_beside_a_query_or_the_force_configuration(nb):
    n, m = 5000, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    pvel = point_velocities(nb, m)
    skip = make_skip(n, m, on)
    perm = np.random.default_rng(5).permutation(m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        got = eng.jerk_at(pts, pvel, skip)
        rows = eng.jerk()
        for sel in (slice(0, 1), slice(100, 357), slice(699, 700), slice(63, 129), perm):
            assert same(eng.jerk_at(pts[sel], pvel[sel], skip[sel]), tuple(o[sel] for o in got)), sel
        assert same(eng.jerk(1000, 100), tuple(o[1000:1100] for o in rows))
        assert same(eng.jerk_at(np.ascontiguousarray(pts[:, :3]), np.ascontiguousarray(pvel[:, :3]), skip), got)   # (m, 3) arrays are padded to words
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            assert same(eng.jerk_at(pts, pvel, skip), got) and same(eng.jerk(), rows), (key, val)
            eng.set_option(key, default)


def test_bits_do_not_depend_on_the_device_count(nb, monkeypatch):
    """three oversubscribed devices after a step — each holds only its own slice's new positions and velocities, the pass brings the
    rest first — against one device that is given the same state"""
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n, m = 3001, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    pvel = point_velocities(nb, m)
    skip = make_skip(n, m, on)
    probe = lambda eng: (eng.jerk_at(pts, pvel, skip), eng.jerk_at(pts[:2], pvel[:2]), eng.jerk(), eng.jerk(900, 1200))
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
    assert same(three[3], tuple(o[900:2100] for o in three[2]))   # a window across both device boundaries


WORKER = """
    from field_common import make_points, make_skip
    eng.set_option(nb.OPT_JSUB, 2)
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m = (300, 41)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    pvel = nb.make_bodies(m, seed=78 + rank)[1]
    a, j = eng.jerk_at(pts, pvel, make_skip(n, m, on))
    ra, rj = eng.jerk()                                       # this rank's own rows
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, a=a, j=j, ra=ra, rj=rj, first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p, vel=v)
"""


def test_two_processes_host_transport_equal_one_process(nb, tmp_path):
    """after three steps the velocities differ from the upload, and each rank holds only its own: they must really be gathered"""
    n, world = 6007, 2
    out = str(tmp_path / "jk")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now, vnow = got[0]["pos"], got[0]["vel"]
    assert same((now, vnow), (got[1]["pos"], got[1]["vel"]))
    pos, vel = nb.make_bodies(n, seed=33)
    assert not same(vnow, vel)
    covered = 0
    with nb.NBody(n) as one:
        one.upload(now, vnow)
        rows = one.jerk()
        for r, m in enumerate((300, 41)):
            pts, on = make_points(nb, pos, m, seed=50 + r)
            pvel = nb.make_bodies(m, seed=78 + r)[1]
            assert same((got[r]["a"], got[r]["j"]), one.jerk_at(pts, pvel, make_skip(n, m, on))), r
            first, cnt = (int(v) for v in got[r]["first"])
            assert same((got[r]["ra"], got[r]["rj"]), tuple(o[first:first + cnt] for o in rows)), r
            covered += cnt
    assert covered == n


def test_jerk_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, on = make_points(nb, nb.make_bodies(n)[0], 300)
    pvel = point_velocities(nb, 300)
    probe = lambda eng: (eng.jerk_at(pts, pvel), eng.jerk_at(pts, pvel, make_skip(n, 300, on)), eng.jerk(), eng.jerk(700, 7))
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_JERK_SPLIT")


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64 = C.POINTER(C.c_float), C.POINTER(C.c_double)
    pts, pv = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
    pts64, pv64 = np.zeros((4, 4), np.float64), np.zeros((4, 4), np.float64)
    oa, oj = np.full((4, 4), 7, np.float32), np.full((4, 4), 7, np.float32)
    oa64, oj64 = np.full((4, 4), 7, np.float64), np.full((4, 4), 7, np.float64)
    sk = np.array([-1, 0, 3, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    p32, p64 = (lambda a: a.ctypes.data_as(f32)), (lambda a: a.ctypes.data_as(f64))
    call32 = lambda: lib.nbody_jerk(p32(pts), p32(pv), 4, ip(sk), p32(oa), p32(oj))
    call64 = lambda: lib.nbody_jerk_d(p64(pts64), p64(pv64), 4, ip(sk), p64(oa64), p64(oj64))
    rows32 = lambda: lib.nbody_jerk_rows(0, 4, p32(oa), p32(oj))
    rows64 = lambda: lib.nbody_jerk_rows_d(0, 4, p64(oa64), p64(oj64))
    untouched32 = lambda: np.all(oa == 7) and np.all(oj == 7)
    untouched64 = lambda: np.all(oa64 == 7) and np.all(oj64 == 7)
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [call32(), call64(), rows32(), rows64()] == [E.ERR_STATE] * 4
        finally:
            mb.serve(False)
        assert untouched32() and untouched64()
        assert [call32(), call64()] == [0, E.ERR_STATE]       # served no more: an fp32 context again
        assert untouched64() and not np.any(oa == 7) and not np.any(oj == 7)
        oa[...] = 7
        oj[...] = 7
        assert [rows32(), rows64()] == [0, E.ERR_STATE]
        assert untouched64() and not np.any(oa == 7) and not np.any(oj == 7)
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        oa[...] = 7
        oj[...] = 7
        a, j, x, u = p32(oa), p32(oj), p32(pts), p32(pv)
        assert lib.nbody_jerk(None, u, 4, None, a, j) == E.ERR_ARG
        assert lib.nbody_jerk(x, None, 4, None, a, j) == E.ERR_ARG
        assert lib.nbody_jerk(x, u, 4, None, None, None) == E.ERR_ARG
        assert lib.nbody_jerk(x, u, 0, None, a, j) == E.ERR_ARG
        assert lib.nbody_jerk(x, u, -3, None, a, j) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_jerk(x, u, 4, ip(sk), a, j) == E.ERR_ARG, bad
        assert lib.nbody_jerk_rows(0, 4, None, None) == E.ERR_ARG
        for first, cnt in ((-1, 4), (0, 0), (0, -1), (n, 1), (n - 3, 4), (0, n + 1)):
            assert lib.nbody_jerk_rows(first, cnt, a, j) == E.ERR_ARG, (first, cnt)
        assert untouched32()
        sk[:] = (-1, 0, n - 1, n - 1)
        assert lib.nbody_jerk(x, u, 4, ip(sk), a, None) == 0 and not np.any(oa == 7) and np.all(oj == 7)      # either output alone
        assert lib.nbody_jerk(x, u, 4, ip(sk), None, j) == 0 and not np.any(oj == 7)
        oa[...] = 7
        oj[...] = 7
        assert lib.nbody_jerk_rows(n - 4, 4, None, j) == 0 and np.all(oa == 7) and not np.any(oj[:, :3] == 7)
        assert lib.nbody_jerk_rows(n - 4, 4, a, None) == 0 and not np.any(oa[:, :3] == 7)
        assert [call64(), rows64()] == [E.ERR_STATE] * 2 and untouched64()
    with nb.NBody(n, fp64=True) as eng:
        sk[:] = (-1, 0, 3, 2)
        assert [call32(), rows32()] == [E.ERR_STATE] * 2
        assert [call64(), rows64()] == [0, 0]


def test_c_host_program_jerk_line(nb):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters, m = 4096, 3, 1000
    r = subprocess.run([exe, str(n), str(iters), "--jerk", str(m)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^jerk of (\d+) rows: a_sum (\S+) (\S+) (\S+) j_sum (\S+) (\S+) (\S+)$", r.stdout, flags=re.M)
    assert len(lines) == 1 and int(lines[0][0]) == m, r.stdout
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        eng.step(0.01, iters)
        a, j = eng.jerk(0, m)
    want = [0.0] * 6
    for k in range(m):   # plain ascending fp64 sums
        for c in range(3):
            want[c] += float(a[k, c])
            want[3 + c] += float(j[k, c])
    got = [float(v) for v in lines[0][1:]]
    for g_, w in zip(got, want):
        assert abs(g_ - w) <= 1e-12 * abs(w), (got, want)


# ---- the hostile system (specials_common.py): what a uniform cloud never shows the pass ----

def check_specials_directly(got, pts, skip, n, variant, what, planted=0):
    """What include/nbody.h promises without any reference: a skipped body leaves no trace ("for j == skip[p] all six keep their
    values"), so a finite query that skips the NaN, inf or overflow body has a finite acceleration (planted: how many such queries there
    must be) — its jerk as well unless another far body's 3 rv overflows, which the reference decides; and a NaN body poisons the
    acceleration and the jerk of every query that does not skip it."""
    a, j = got
    special = special_row(n, variant)
    sk = np.full(len(pts), -1, np.int32) if skip is None else skip
    if special is not None:
        clean = near(pts) & (sk == special)
        assert clean.sum() >= planted, what
        assert np.all(np.isfinite(a[clean])), what
    if variant == "nan":
        hit = sk != nan_row(n)
        assert np.all(np.isnan(a[hit][:, :3])) and np.all(np.isnan(j[hit][:, :3])), what


def skipped_special_leaves_no_trace(nb, eng, pos, vel, pts, pvel, skip, n, variant, got):
    """the queries that skip the variant's special body get, bit for bit, what they get once that body is an ordinary one: nothing of
    it — neither its position nor its velocity — reaches their sums"""
    special = special_row(n, variant)
    if special is None or skip is None or not np.any(skip == special):
        return
    tame_p, tame_v = pos.copy(), vel.copy()
    tame_p[special, :3] = 0.25
    tame_v[special, :3] = 0.5
    eng.upload(tame_p, tame_v)
    tame = eng.jerk_at(pts, pvel, skip)
    eng.upload(pos, vel)
    sel = skip == special
    assert same_nan(got[0][sel], tame[0][sel]) and same_nan(got[1][sel], tame[1][sel]), (n, variant)


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_hostile_system_strict_bit_for_bit(nb, ref, arith, monkeypatch):
    """every variant, size and query count, with and without skip, the one-launch form and the scratch + combine form
    (NBODY_JERK_SPLIT unset, 1, 2, 3): bit for bit tests/jerk_ref.c, whose `continue` on j == skip is the definition"""
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    differ = []
    for n in SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                for m in POINT_COUNTS:
                    pts, hsk = hostile_points(nb, pos, m, variant)
                    pvel = point_velocities(nb, m, dtype)
                    for skip in (None, hsk):
                        want = ref.f64(pos, vel, pts, pvel, skip) if fp64 else ref.f32(pos, vel, pts, pvel, skip, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                        what = (n, variant, m, skip is not None)
                        planted = 2 if skip is not None and m >= 65 else 0
                        check_specials_directly(want, pts, skip, n, variant, what, planted)     # the reference itself keeps the promise
                        for split in (None, "1", "2", "3"):
                            if split is None:
                                monkeypatch.delenv("NBODY_JERK_SPLIT", raising=False)
                            else:
                                monkeypatch.setenv("NBODY_JERK_SPLIT", split)
                            got = eng.jerk_at(pts, pvel, skip)
                            if not (same_nan(got[0], want[0]) and same_nan(got[1], want[1])):
                                differ.append(what + (split, np.flatnonzero((bits(got[1]) != bits(want[1])).any(1))[:8]))
                            check_specials_directly(got, pts, skip, n, variant, what + (split,), planted)
                monkeypatch.delenv("NBODY_JERK_SPLIT", raising=False)
                rows = eng.jerk()
                want = ref.f64(pos, vel, pos, vel, np.arange(n, dtype=np.int32)) if fp64 else \
                    ref.f32(pos, vel, pos, vel, np.arange(n, dtype=np.int32), ref=(mode == nb.ARITH_REFERENCE_STRICT))
                if not (same_nan(rows[0], want[0]) and same_nan(rows[1], want[1])):
                    differ.append((n, variant, "rows"))
    assert not differ, differ   # every input where the device and the reference differ, none dropped


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system_every_arithmetic(nb, ref, fp64):
    """Every arithmetic — the timed ones (v_rsq_f32; the v_rsq_f64 seed + one third-order step) and the strict ones — on the hostile
    system: NaN and finite exactly where the strict reference of the same d2 form is, in every variant, with and without skip; a
    skipped NaN, inf or overflow body leaves no trace; a NaN body poisons every query that does not skip it."""
    dtype = np.float64 if fp64 else np.float32
    modes = (nb.ARITH_FMA3, nb.ARITH_STRICT) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)
    differ = []
    for n in SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                pts, hsk = hostile_points(nb, pos, 300, variant)
                pvel = point_velocities(nb, 300, dtype)
                for skip in (hsk, None):
                    for mode in modes:
                        eng.set_option(nb.OPT_ARITH, mode)
                        what = (n, variant, mode, skip is not None)
                        is_ref = mode in (nb.ARITH_REFERENCE, nb.ARITH_REFERENCE_STRICT)
                        want = ref.f64(pos, vel, pts, pvel, skip) if fp64 else ref.f32(pos, vel, pts, pvel, skip, ref=is_ref)
                        got = eng.jerk_at(pts, pvel, skip)
                        for g_, w in zip(got, want):
                            if not (np.array_equal(np.isfinite(g_), np.isfinite(w)) and np.array_equal(np.isnan(g_), np.isnan(w))):
                                differ.append(what + (np.flatnonzero((np.isfinite(g_) != np.isfinite(w)).any(1) | (np.isnan(g_) != np.isnan(w)).any(1))[:8],))
                        check_specials_directly(got, pts, skip, n, variant, what, 2 if skip is not None else 0)
                        skipped_special_leaves_no_trace(nb, eng, pos, vel, pts, pvel, skip, n, variant, got)
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
    assert not differ, differ   # an input where the patterns differ is reported, not dropped
