"""Acceleration and potential at arbitrary points (nbody_field(_d); include/nbody.h "field at arbitrary points"): bit for bit against
tests/field_ref.c in the strict modes, within the project's tolerances in the timed arithmetic, phi with the point's own body skipped
equal to nbody_potential_rows in EVERY arithmetic, all of it again on the hostile system of specials_common.py (coincident bodies on
the window and block edges, underflow, overflow, subnormal cubes, signed zeros, infinity, NaN, skip indices on every loop edge), the
same bits however the work is laid out (source split, batches, sub-ranges,
force configuration, device and process count), no effect on the step, the force as the gradient of the potential, the guards and the
C host program's --field line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from field_common import FieldRef, compile_ref, make_points, make_skip, numpy_field, row_rel
from pass_common import FORCE_CONFIGS, bits, check_step_untouched, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import POINT_COUNTS, SIZES, VARIANTS, hostile_points, hostile_system, nan_row, near, same_nan, special_row, within

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5   # the project's north_star tolerance (TOL in tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return FieldRef(compile_ref(tmp_path_factory.mktemp("field_ref"), "field_ref"))


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
                for skip in (None, make_skip(n, m, on)):
                    wa, wp = ref.f32(pos, pts, skip, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                    a, p = eng.field(pts, skip)
                    assert same(a, wa), (n, m, skip is not None, int((a != wa).any(1).sum()))
                    assert same(p, wp), (n, m, skip is not None, int((p != wp).sum()))
                    assert np.all(a[:, 3].view(np.uint32) == 0)
                    a1, none = eng.field(pts, skip, potential=False)
                    assert none is None and same(a1, wa), (n, m)
                    none, p1 = eng.field(pts, skip, accel=False)
                    assert none is None and same(p1, wp), (n, m)


def test_fp64(nb, ref):
    m = 257
    for n in (2, 1025, 4099):
        pos, vel = nb.make_bodies(n, dtype=np.float64)
        pts, on = make_points(nb, pos, m)
        with nb.NBody(n, fp64=True) as eng:
            eng.upload(pos, vel)
            for skip in (None, make_skip(n, m, on)):
                wa, wp = ref.f64(pos, pts, skip)
                a, p = eng.field(pts, skip)
                ep, ea = float(np.max(np.abs(p - wp) / np.abs(wp))), row_rel(a, wa)
                print("fp64 n=%d skip=%s: phi %.3e accel %.3e" % (n, skip is not None, ep, ea))
                assert ep < 1e-12 and ea < 1e-11, n
                eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
                a, p = eng.field(pts, skip)
                assert same(a, wa) and same(p, wp), (n, skip is not None)
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)


def test_timed_fp32_within_tolerance(nb, ref):
    n, m = 65536, 512
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    for skip in (None, make_skip(n, m, on)):
        wa, wp = ref.f64(pos.astype(np.float64), pts.astype(np.float64), skip)
        with nb.NBody(n) as eng:
            eng.upload(pos, vel)
            a, p = eng.field(pts, skip)
        ea, ep = row_rel(a, wa), float(np.max(np.abs(p - wp) / np.abs(wp)))
        print("timed fp32 skip=%s: accel %.3e phi %.3e" % (skip is not None, ea, ep))
        assert ea < TOL and ep < TOL


@pytest.mark.parametrize("fp64", [False, True])
def test_phi_with_self_skipped_is_potential_rows(nb, ref, fp64):
    """needs no CPU statement: holds in the timed arithmetic too"""
    dtype = np.float64 if fp64 else np.float32
    modes = (nb.ARITH_FMA3, nb.ARITH_STRICT) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)
    for n in (65, 1025, 5000):
        pos, vel = nb.make_bodies(n, dtype=dtype)
        sk = np.arange(n, dtype=np.int32)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for mode in modes:
                eng.set_option(nb.OPT_ARITH, mode)
                a, p = eng.field(pos, sk)
                assert same(p, eng.potential_rows(0, n)), (n, mode)
                if mode in (nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT):
                    wa, wp = ref.f64(pos, pos, sk) if fp64 else ref.f32(pos, pos, sk, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                    assert same(a, wa) and same(p, wp), (n, mode)


def test_bits_do_not_depend_on_the_source_split_or_the_batches(nb, monkeypatch):
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    big, on = make_points(nb, pos, 70000)
    pts = big[:m]
    skip = make_skip(n, m, on)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        monkeypatch.delenv("NBODY_FIELD_SPLIT", raising=False)
        base, base_sk = eng.field(pts), eng.field(pts, skip)
        for split in ("1", "2", "3", "5", "64"):
            monkeypatch.setenv("NBODY_FIELD_SPLIT", split)
            for got, want in ((eng.field(pts), base), (eng.field(pts, skip), base_sk)):
                assert same(got[0], want[0]) and same(got[1], want[1]), split
            assert same(eng.field(pts, potential=False)[0], base[0]) and same(eng.field(pts, accel=False)[1], base[1]), split
        # 70000 points x 5 blocks x 16 B = 5.6 MB of per-block sums against a bound of 1 MB: consecutive batches of 13056 points
        monkeypatch.delenv("NBODY_FIELD_SPLIT")
        monkeypatch.setenv("NBODY_FIELD_SCRATCH_MB", "1")
        a_big, p_big = eng.field(big)
        monkeypatch.setenv("NBODY_FIELD_SPLIT", "1")
        a_one, p_one = eng.field(big)
        assert same(a_big, a_one) and same(p_big, p_one)
        assert same(a_big[:m], base[0]) and same(p_big[:m], base[1])
        monkeypatch.setenv("NBODY_FIELD_SPLIT", "4")
        a_big, p_big = eng.field(big)
        assert same(a_big, a_one) and same(p_big, p_one)
        monkeypatch.setenv("NBODY_FIELD_SCRATCH_MB", "0")   # not even one workgroup's points fit: no split
        a0, p0 = eng.field(pts, skip)
        assert same(a0, base_sk[0]) and same(p0, base_sk[1])


def test_bits_do_not_depend_on_the_points_beside_a_point_or_the_force_configuration(nb):
    n, m = 5000, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    perm = np.random.default_rng(5).permutation(m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        a, p = eng.field(pts, skip)
        for sel in (slice(0, 1), slice(100, 357), slice(699, 700), slice(63, 129), perm):
            a1, p1 = eng.field(pts[sel], skip[sel])
            assert same(a1, a[sel]) and same(p1, p[sel]), sel
        a3, p3 = eng.field(np.ascontiguousarray(pts[:, :3]), skip)   # (m, 3) points are padded to words
        assert same(a3, a) and same(p3, p)
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            a1, p1 = eng.field(pts, skip)
            assert same(a1, a) and same(p1, p), (key, val)
            eng.set_option(key, default)


def test_bits_do_not_depend_on_the_device_count(nb, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n, m = 3001, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            res[ngpus] = eng.field(pts, skip) + eng.field(pts[:2]) + (eng.download()[0],)
    assert same(res[1][4], res[3][4]), "the two states differ"
    assert not same(res[1][4], pos), "no drift happened"
    for k in range(4):
        assert same(res[1][k], res[3][k]), k


WORKER = """
    from field_common import make_points, make_skip
    eng.set_option(nb.OPT_JSUB, 2)
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m = (300, 41)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    a, phi = eng.field(pts, make_skip(n, m, on))
    p, v = eng.download()
    np.save({out!r} + "_%d_accel.npy" % rank, a)
    np.save({out!r} + "_%d_phi.npy" % rank, phi)
    if rank == 0:
        np.save({out!r} + "_pos.npy", p)
        open({out!r} + "_wsplit.txt", "w").write(str(eng.config["wsplit"]))
"""


def test_two_processes_host_transport_equal_one_process(nb, tmp_path, monkeypatch):
    n, world = 6007, 2
    out = str(tmp_path / "fd")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    pos, vel = nb.make_bodies(n, seed=33)
    with nb.NBody(n, ngpus=world) as one:
        one.set_option(nb.OPT_JSUB, 2)
        one.set_option(nb.OPT_WSPLIT, int(open(out + "_wsplit.txt").read()))
        one.upload(pos, vel)
        one.step(0.01, 3)
        wp, _ = one.download()
        assert np.array_equal(np.load(out + "_pos.npy").view(np.uint32), wp.view(np.uint32)), "the two runs' states differ"
        for r, m in enumerate((300, 41)):
            pts, on = make_points(nb, pos, m, seed=50 + r)
            a, phi = one.field(pts, make_skip(n, m, on))
            assert same(np.load(out + "_%d_accel.npy" % r), a), r
            assert same(np.load(out + "_%d_phi.npy" % r), phi), r


def test_field_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, on = make_points(nb, nb.make_bodies(n)[0], 300)
    probe = lambda eng: (eng.field(pts), eng.field(pts, make_skip(n, 300, on)), eng.field(pts[:7], accel=False))
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_FIELD_SPLIT")


def gradient_error(field, x, h):
    """Per point: |central difference of phi with step h + a|_2, |a|_2 and the truncation error of the difference, h^2 |d^3 phi / dx_k^3| / 6
    per axis as a vector norm, with d^3 phi / dx_k^3 = -d^2 a_k / dx_k^2 estimated from a at +-2h.  field(points) -> (accel, phi), fp64."""
    k = len(x)
    shifts = [np.zeros(3)] + [s * np.eye(3)[ax] for ax in range(3) for s in (h, -h, 2 * h, -2 * h)]
    pts = np.zeros((k * len(shifts), 4))
    for q, d in enumerate(shifts):
        pts[q * k:(q + 1) * k, :3] = x + d
    a, phi = field(pts)
    a, phi = a.reshape(len(shifts), k, 4), phi.reshape(len(shifts), k)
    err, trunc = np.zeros((k, 3)), np.zeros((k, 3))
    for ax in range(3):
        ph, mh, p2, m2 = (1 + 4 * ax + q for q in range(4))
        err[:, ax] = (phi[ph] - phi[mh]) / (2 * h) + a[0, :, ax]
        d3 = (a[p2, :, ax] - 2 * a[0, :, ax] + a[m2, :, ax]) / (2 * h) ** 2
        trunc[:, ax] = h * h * np.abs(d3) / 6
    return np.linalg.norm(err, axis=1), np.linalg.norm(a[0, :, :3], axis=1), np.linalg.norm(trunc, axis=1)


def test_acceleration_is_minus_the_gradient_of_the_potential(nb, ref):
    """The bound is a property of the reference: the truncation error of the central difference, estimated from field_f64 itself, with
    a factor 4 on top for round-off and the estimate's own error; field_f64 must meet it before the device is asked."""
    n, h = 4099, 1e-4
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    cand = nb.make_bodies(200, seed=11, dtype=np.float64)[0][:, :3]
    near = np.array([np.sqrt(((pos[:, :3] - c) ** 2).sum(1).min()) for c in cand])
    x = cand[near >= 0.05]
    assert len(x) >= 50, len(x)
    x = x[:50]
    e, an, tr = gradient_error(lambda pts: ref.f64(pos, pts), x, h)
    print("field_f64: worst error / |a| %.3e, worst error / bound %.3f" % ((e / an).max(), (e / (4 * tr)).max()))
    assert np.all(e / an <= 4 * tr / an)
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos, vel)
        for mode in (nb.ARITH_FMA3, nb.ARITH_STRICT):
            eng.set_option(nb.OPT_ARITH, mode)
            e, an, tr = gradient_error(eng.field, x, h)
            print("device arith %d: worst error / |a| %.3e, worst error / bound %.3f" % (mode, (e / an).max(), (e / (4 * tr)).max()))
            assert np.all(e / an <= 4 * tr / an), mode


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64 = C.POINTER(C.c_float), C.POINTER(C.c_double)
    pts = np.zeros((4, 4), np.float32)
    pts64 = np.zeros((4, 4), np.float64)
    acc, phi = np.full((4, 4), 7, np.float32), np.full(4, 7, np.float32)
    acc64, phi64 = np.full((4, 4), 7, np.float64), np.full(4, 7, np.float64)
    sk = np.array([-1, 0, 3, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    call32 = lambda: lib.nbody_field(pts.ctypes.data_as(f32), 4, ip(sk), acc.ctypes.data_as(f32), phi.ctypes.data_as(f32))
    call64 = lambda: lib.nbody_field_d(pts64.ctypes.data_as(f64), 4, ip(sk), acc64.ctypes.data_as(f64), phi64.ctypes.data_as(f64))
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [call32(), call64()] == [E.ERR_STATE] * 2
        finally:
            mb.serve(False)
        assert np.all(acc == 7) and np.all(phi == 7)
        assert [call32(), call64()] == [0, E.ERR_STATE]       # served no more: an fp32 context again
        assert np.all(acc64 == 7) and np.all(phi64 == 7) and not np.any(phi == 7)
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        acc[...] = 7
        phi[...] = 7
        a, p, x = acc.ctypes.data_as(f32), phi.ctypes.data_as(f32), pts.ctypes.data_as(f32)
        assert lib.nbody_field(None, 4, None, a, p) == E.ERR_ARG
        assert lib.nbody_field(x, 0, None, a, p) == E.ERR_ARG
        assert lib.nbody_field(x, -3, None, a, p) == E.ERR_ARG
        assert lib.nbody_field(x, 4, None, None, None) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_field(x, 4, ip(sk), a, p) == E.ERR_ARG, bad
        assert np.all(acc == 7) and np.all(phi == 7)
        sk[:] = (-1, 0, n - 1, n - 1)
        assert lib.nbody_field(x, 4, ip(sk), a, p) == 0 and not np.any(phi == 7)
        assert call64() == E.ERR_STATE
    with nb.NBody(n, fp64=True) as eng:
        assert call32() == E.ERR_STATE and call64() == 0


def test_c_host_program_field_line(nb):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters, m = 4096, 3, 1000
    r = subprocess.run([exe, str(n), str(iters), "--field", str(m)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^field of (\d+) points: phi_sum (\S+) a_sum (\S+) (\S+) (\S+)$", r.stdout, flags=re.M)
    assert len(lines) == 1 and int(lines[0][0]) == m, r.stdout
    plain = subprocess.run([exe, str(n), str(iters)], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "field" not in plain.stdout
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        eng.step(0.01, iters)
        a, phi = eng.field(nb.make_bodies(m, seed=4242)[0])
    want = [0.0, 0.0, 0.0, 0.0]
    for k in range(m):   # plain ascending fp64 sums
        want[0] += float(phi[k])
        for c in range(3):
            want[1 + c] += float(a[k, c])
    got = [float(v) for v in lines[0][1:]]
    for g_, w in zip(got, want):
        assert abs(g_ - w) <= 1e-12 * abs(w), (got, want)


# ---- the hostile system (specials_common.py): what a uniform cloud never shows the pass ----

def check_specials_directly(a, p, pts, skip, n, variant, what, planted=0):
    """What include/nbody.h promises without any reference: a skipped body leaves no trace ("for j == skip[p] all four keep their
    values"), so a finite point that skips the NaN, inf or overflow body has a finite field (planted: how many such points there must
    be); and a NaN body poisons every point that does not skip it."""
    special = special_row(n, variant)
    sk = np.full(len(pts), -1, np.int32) if skip is None else skip
    if special is not None:
        clean = near(pts) & (sk == special)
        assert clean.sum() >= planted, what
        for out in (a[:, :3] if a is not None else None, p):
            assert out is None or np.all(np.isfinite(out[clean])), what
    if variant == "nan":
        dirty = sk != nan_row(n)
        for out in (a[:, :3] if a is not None else None, p):
            assert out is None or np.all(np.isnan(out[dirty])), what


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_hostile_system_strict_bit_for_bit(nb, ref, arith, monkeypatch):
    """every variant, size and point count, with and without skip, both outputs and each alone, the one-launch form and the scratch +
    combine form (NBODY_FIELD_SPLIT unset, 1, 2, 3): bit for bit tests/field_ref.c, whose `continue` on j == skip is the definition"""
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    for n in SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                for m in POINT_COUNTS:
                    pts, hsk = hostile_points(nb, pos, m, variant)
                    for skip in (None, hsk):
                        wa, wp = ref.f64(pos, pts, skip) if fp64 else ref.f32(pos, pts, skip, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                        what = (n, variant, m, skip is not None)
                        planted = 2 if skip is not None and m >= 65 else 0
                        check_specials_directly(wa, wp, pts, skip, n, variant, what, planted)     # the reference itself keeps the promise
                        for split in (None, "1", "2", "3"):
                            if split is None:
                                monkeypatch.delenv("NBODY_FIELD_SPLIT", raising=False)
                            else:
                                monkeypatch.setenv("NBODY_FIELD_SPLIT", split)
                            a, p = eng.field(pts, skip)
                            assert same_nan(a, wa), what + (split, np.flatnonzero((bits(a) != bits(wa)).any(1))[:8])
                            assert same_nan(p, wp), what + (split, np.flatnonzero(bits(p) != bits(wp))[:8])
                            assert np.all(bits(a[:, 3]) == 0)
                            check_specials_directly(a, p, pts, skip, n, variant, what + (split,), planted)
                            a1, none = eng.field(pts, skip, potential=False)
                            assert none is None and same_nan(a1, wa), what + (split,)
                            none, p1 = eng.field(pts, skip, accel=False)
                            assert none is None and same_nan(p1, wp), what + (split,)


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system_timed_arithmetic(nb, ref, fp64):
    """The timed arithmetic (v_rsq_f32; the v_rsq_f64 seed + one third-order step) on the hostile system:
    (a) finite exactly where the strict reference is finite, in every variant — rows, points, with and without skip;
    (b) phi of points = pos, skip = arange(n) is potential_rows(0, n), NaN for NaN and bit for bit elsewhere, in every arithmetic;
    (c) on the near rows and points (every |coordinate| <= 2, not a far-away body): |a - a64| <= TOL sum_j |term_j| per component and
        |phi - phi64| <= TOL |phi64| against the plain numpy binary64 evaluation, TOL = 1e-5 (binary32) or 1e-12 (binary64).
    The far-away rows are held to (a) and (b) only: there the strict binary32 arithmetic is itself tens of percent off binary64 (a cube
    of one or two bits).  The strict references sit at <= 1.6e-6 (binary32) and <= 4.7e-15 (binary64) in the measure of (c), worst over
    sizes and variants (tests/test_specials_reference.py, which requires 3e-6 and 1e-13).  Measured on an MI355X, worst over sizes,
    variants and point sets: binary32 accel 1.6e-6, phi 1.6e-6; binary64 accel 4.7e-15, phi 2.8e-15."""
    dtype = np.float64 if fp64 else np.float32
    tol = 1e-12 if fp64 else TOL
    modes = (nb.ARITH_FMA3, nb.ARITH_STRICT) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT)
    for n in SIZES:
        rows_skip = np.arange(n, dtype=np.int32)
        with nb.NBody(n, fp64=fp64) as eng:
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                for mode in modes:                                                   # (b)
                    eng.set_option(nb.OPT_ARITH, mode)
                    a, p = eng.field(pos, rows_skip)
                    assert same_nan(p, eng.potential_rows(0, n)), (n, variant, mode)
                pts, hsk = hostile_points(nb, pos, 300, variant)
                for x, skip, keep in ((pos, rows_skip, near(pos, far)), (pts, hsk, near(pts)), (pts, None, near(pts))):
                    a64, p64, mag = numpy_field(pos, x, skip, mags=True)
                    for mode in (nb.ARITH_FMA3,) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                        eng.set_option(nb.OPT_ARITH, mode)
                        what = (n, variant, mode, len(x), skip is not None)
                        wa, wp = ref.f64(pos, x, skip) if fp64 else ref.f32(pos, x, skip, ref=(mode == nb.ARITH_REFERENCE))
                        a, p = eng.field(x, skip)
                        assert np.array_equal(np.isfinite(a), np.isfinite(wa)), what + (np.flatnonzero((np.isfinite(a) != np.isfinite(wa)).any(1))[:8],)   # (a)
                        assert np.array_equal(np.isfinite(p), np.isfinite(wp)), what + (np.flatnonzero(np.isfinite(p) != np.isfinite(wp))[:8],)
                        check_specials_directly(a, p, x, skip, n, variant, what, 2 if x is pts and skip is not None else 0)
                        with np.errstate(all="ignore"):                              # (c)
                            ea = np.nanmax(np.abs(a[keep, :3] - a64[keep, :3]) / mag[keep], initial=0.0)
                            ep = np.nanmax(np.abs(p[keep] - p64[keep]) / np.abs(p64[keep]), initial=0.0)
                        print("timed %s n=%d %s arith %d, %d of %d near, skip=%s: accel %.3e phi %.3e"
                              % (np.dtype(dtype).name, n, variant, mode, keep.sum(), len(x), skip is not None, ea, ep))
                        assert within(a[keep, :3], a64[keep, :3], tol * mag[keep]), what
                        assert within(p[keep], p64[keep], tol * np.abs(p64[keep])), what
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
