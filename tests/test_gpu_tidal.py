"""The tidal tensor at arbitrary points (nbody_tidal(_d); include/nbody.h "tidal tensor at arbitrary points"): bit for bit against
tests/tidal_ref.c in the strict modes, within derived bounds in the timed arithmetic, all of it again on the hostile system of
specials_common.py, the same bits however the work is laid out (source split, batches, sub-ranges, force configuration, device and
process count), no effect on the step, T as the gradient of the field, the guards and the C host program's --tidal line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from field_common import FieldRef, compile_ref, make_points, make_skip
from pass_common import FORCE_CONFIGS, bits, check_step_untouched, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import POINT_COUNTS, SIZES, VARIANTS, hostile_points, hostile_system, nan_row, near, same_nan, special_row
from tidal_common import GRADIENT_H, TidalRef, gradient_error, gradient_points, numpy_tidal, worst

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-5   # the project's north_star tolerance (TOL in tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return TidalRef(compile_ref(tmp_path_factory.mktemp("tidal_ref"), "tidal_ref"))


@pytest.fixture(scope="module")
def field_ref(tmp_path_factory):
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
                    want = ref.f32(pos, pts, skip, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                    t = eng.tidal(pts, skip)
                    assert same(t, want), (n, m, skip is not None, int((t != want).any(1).sum()))


def test_fp64(nb, ref):
    """strict: tests/tidal_ref.c bit for bit.  Timed (the v_rsq_f64 seed refined to full precision): <= 1e-12 of mag against numpy
    binary64, the field test's bound."""
    m = 257
    for n in (2, 1025, 4099):
        pos, vel = nb.make_bodies(n, dtype=np.float64)
        pts, on = make_points(nb, pos, m)
        with nb.NBody(n, fp64=True) as eng:
            eng.upload(pos, vel)
            for skip in (None, make_skip(n, m, on)):
                want64, mag = numpy_tidal(pos, pts, skip)
                t = eng.tidal(pts, skip)
                e = worst(t, want64, mag)
                print("fp64 timed n=%d skip=%s: %.3e" % (n, skip is not None, e))
                assert e <= 1e-12, n
                eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
                assert same(eng.tidal(pts, skip), ref.f64(pos, pts, skip)), (n, skip is not None)
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)


def test_timed_fp32_within_tolerance(nb, ref):
    """n = 65536, m = 512, |T - T64| / mag against numpy binary64, bound TOL = 1e-5, derived: the timed form differs from the strict
    one by v_rsq_f32's <= 1 ulp, which enters inv5 five-fold: <= 5 * 2^-23 = 6e-7 of mag; the rounding paths differ by no more than the
    reference's own error r <= 5e-6 (asserted on the CPU at this shape: tests/test_tidal_abi.py, measured 3.7e-6); r + r + 6e-7 < 1e-5
    needs r <= 4.7e-6.  Measured on an MI355X: 3.718e-6 (FMA3) and 3.550e-6 (REFERENCE), with and without skip."""
    n, m = 65536, 512
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for skip in (None, make_skip(n, m, on)):
            want64, mag = numpy_tidal(pos, pts, skip)
            for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                eng.set_option(nb.OPT_ARITH, mode)
                e = worst(eng.tidal(pts, skip), want64, mag)
                print("timed fp32 arith %d skip=%s: %.3e" % (mode, skip is not None, e))
                assert e <= TOL, (mode, skip is not None)


def test_bits_do_not_depend_on_the_source_split_or_the_batches(nb, monkeypatch):
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    big, on = make_points(nb, pos, 70000)
    pts = big[:m]
    skip = make_skip(n, m, on)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        monkeypatch.delenv("NBODY_TIDAL_SPLIT", raising=False)
        base, base_sk = eng.tidal(pts), eng.tidal(pts, skip)
        assert not same(base, base_sk)
        for split in ("1", "2", "3", "5", "64"):
            monkeypatch.setenv("NBODY_TIDAL_SPLIT", split)
            assert same(eng.tidal(pts), base) and same(eng.tidal(pts, skip), base_sk), split
        # 70000 points x 5 blocks x 28 B = 9.8 MB of per-block sums against a bound of 1 MB: consecutive batches of 7424 points
        monkeypatch.delenv("NBODY_TIDAL_SPLIT")
        monkeypatch.setenv("NBODY_TIDAL_SCRATCH_MB", "1")
        t_big = eng.tidal(big)
        monkeypatch.setenv("NBODY_TIDAL_SPLIT", "1")
        t_one = eng.tidal(big)
        assert same(t_big, t_one) and same(t_big[:m], base)
        monkeypatch.setenv("NBODY_TIDAL_SPLIT", "4")
        assert same(eng.tidal(big), t_one)
        monkeypatch.setenv("NBODY_TIDAL_SCRATCH_MB", "0")   # not even one workgroup's points fit: no split
        assert same(eng.tidal(pts, skip), base_sk)


def test_bits_do_not_depend_on_the_points_beside_a_point_or_the_force_configuration(nb):
    n, m = 5000, 700
    pos, vel = nb.make_bodies(n)
    pts, on = make_points(nb, pos, m)
    skip = make_skip(n, m, on)
    perm = np.random.default_rng(5).permutation(m)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        t = eng.tidal(pts, skip)
        for sel in (slice(0, 1), slice(100, 357), slice(699, 700), slice(63, 129), perm):
            assert same(eng.tidal(pts[sel], skip[sel]), t[sel]), sel
        assert same(eng.tidal(np.ascontiguousarray(pts[:, :3]), skip), t)   # (m, 3) points are padded to words
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            assert same(eng.tidal(pts, skip), t), (key, val)
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
            res[ngpus] = (eng.tidal(pts, skip), eng.tidal(pts[:2]), eng.download()[0])
    assert same(res[1][2], res[3][2]), "the two states differ"
    assert not same(res[1][2], pos), "no drift happened"
    for k in range(2):
        assert same(res[1][k], res[3][k]), k


WORKER = """
    from field_common import make_points, make_skip
    eng.set_option(nb.OPT_JSUB, 2)
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    m = (300, 41)[rank]
    pts, on = make_points(nb, pos, m, seed=50 + rank)
    t = eng.tidal(pts, make_skip(n, m, on))
    p, v = eng.download()
    np.save({out!r} + "_%d_tidal.npy" % rank, t)
    if rank == 0:
        np.save({out!r} + "_pos.npy", p)
        open({out!r} + "_wsplit.txt", "w").write(str(eng.config["wsplit"]))
"""


def test_two_processes_host_transport_equal_one_process(nb, tmp_path, monkeypatch):
    n, world = 6007, 2
    out = str(tmp_path / "td")
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
            assert same(np.load(out + "_%d_tidal.npy" % r), one.tidal(pts, make_skip(n, m, on))), r


def test_tidal_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    pts, on = make_points(nb, nb.make_bodies(n)[0], 300)
    probe = lambda eng: (eng.tidal(pts), eng.tidal(pts, make_skip(n, 300, on)), eng.tidal(pts[:7]))
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_TIDAL_SPLIT")


def test_the_tensor_is_the_gradient_of_the_acceleration(nb, ref, field_ref):
    """T_ab against the central difference of eng.field's a_a along b, binary64, 50 points at least 0.05 from any body.  The bound is a
    property of the references: the truncation error of the difference, estimated from T itself at +-h, times 4, per point in the
    Frobenius norm; tests/tidal_ref.c and tests/field_ref.c must meet it (tests/test_tidal_abi.py asserts that too) before the device is
    asked, in both binary64 arithmetics."""
    n, h = 4099, GRADIENT_H
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    x = gradient_points(nb, pos)
    norms = lambda err, trunc: (np.sqrt((err ** 2).sum((1, 2))), np.sqrt((trunc ** 2).sum((1, 2))))
    err, trunc, scale = gradient_error(lambda p: ref.f64(pos, p), lambda p: field_ref.f64(pos, p)[0], x, h)
    e, tr = norms(err, trunc)
    print("references: worst error / |T| %.3e, worst error / bound %.3f" % ((e / scale).max(), (e / (4 * tr)).max()))
    assert np.all(e <= 4 * tr)
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos, vel)
        for mode in (nb.ARITH_FMA3, nb.ARITH_STRICT):
            eng.set_option(nb.OPT_ARITH, mode)
            err, trunc, scale = gradient_error(eng.tidal, lambda p: eng.field(p, potential=False)[0], x, h)
            e, tr = norms(err, trunc)
            print("device arith %d: worst error / |T| %.3e, worst error / bound %.3f" % (mode, (e / scale).max(), (e / (4 * tr)).max()))
            assert np.all(e <= 4 * tr), mode


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64 = C.POINTER(C.c_float), C.POINTER(C.c_double)
    pts = np.zeros((4, 4), np.float32)
    pts64 = np.zeros((4, 4), np.float64)
    out, out64 = np.full((4, 6), 7, np.float32), np.full((4, 6), 7, np.float64)
    sk = np.array([-1, 0, 3, 2], np.int32)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    call32 = lambda: lib.nbody_tidal(pts.ctypes.data_as(f32), 4, ip(sk), out.ctypes.data_as(f32))
    call64 = lambda: lib.nbody_tidal_d(pts64.ctypes.data_as(f64), 4, ip(sk), out64.ctypes.data_as(f64))
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [call32(), call64()] == [E.ERR_STATE] * 2
        finally:
            mb.serve(False)
        assert np.all(out == 7)
        assert [call32(), call64()] == [0, E.ERR_STATE]       # served no more: an fp32 context again
        assert np.all(out64 == 7) and not np.any(out == 7)
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        out[...] = 7
        t, x = out.ctypes.data_as(f32), pts.ctypes.data_as(f32)
        assert lib.nbody_tidal(None, 4, None, t) == E.ERR_ARG
        assert lib.nbody_tidal(x, 4, None, None) == E.ERR_ARG
        assert lib.nbody_tidal(x, 0, None, t) == E.ERR_ARG
        assert lib.nbody_tidal(x, -3, None, t) == E.ERR_ARG
        for bad in (n, -2, 1 << 30):
            sk[:] = (-1, 0, bad, n - 1)
            assert lib.nbody_tidal(x, 4, ip(sk), t) == E.ERR_ARG, bad
        assert np.all(out == 7)
        sk[:] = (-1, 0, n - 1, n - 1)
        assert lib.nbody_tidal(x, 4, ip(sk), t) == 0 and not np.any(out == 7)
        assert call64() == E.ERR_STATE
    with nb.NBody(n, fp64=True) as eng:
        assert call32() == E.ERR_STATE and call64() == 0


def test_c_host_program_tidal_line(nb):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters, m = 4096, 3, 1000
    r = subprocess.run([exe, str(n), str(iters), "--tidal", str(m)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"^tidal of (\d+) points: trace_sum (\S+) t_sum (\S+) (\S+) (\S+) (\S+) (\S+) (\S+)$", r.stdout, flags=re.M)
    assert len(lines) == 1 and int(lines[0][0]) == m, r.stdout
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        eng.step(0.01, iters)
        t = eng.tidal(nb.make_bodies(m, seed=4242)[0])
    want = [0.0] * 7
    for k in range(m):   # plain ascending fp64 sums
        want[0] += (float(t[k, 0]) + float(t[k, 1])) + float(t[k, 2])
        for c in range(6):
            want[1 + c] += float(t[k, c])
    got = [float(v) for v in lines[0][1:]]
    for g_, w in zip(got, want):
        assert abs(g_ - w) <= 1e-12 * abs(w), (got, want)


# ---- the hostile system (specials_common.py): what a uniform cloud never shows the pass ----

def check_specials_directly(t, pts, skip, n, variant, what, planted=0):
    """What include/nbody.h promises without any reference: a skipped body leaves no trace ("for j == skip[p] all seven keep their
    values"), so a finite point that skips the NaN, inf or overflow body has a finite tensor (planted: how many such points there must
    be); and a NaN body poisons all six values of every point that does not skip it."""
    special = special_row(n, variant)
    sk = np.full(len(pts), -1, np.int32) if skip is None else skip
    if special is not None:
        clean = near(pts) & (sk == special)
        assert clean.sum() >= planted, what
        assert np.all(np.isfinite(t[clean])), what
    if variant == "nan":
        assert np.all(np.isnan(t[sk != nan_row(n)])), what


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_hostile_system_strict_bit_for_bit(nb, ref, arith, monkeypatch):
    """every variant, size and point count, with and without skip, the one-launch form and the scratch + combine form
    (NBODY_TIDAL_SPLIT unset, 1, 2, 3): bit for bit tests/tidal_ref.c, whose `continue` on j == skip is the definition"""
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
                        want = ref.f64(pos, pts, skip) if fp64 else ref.f32(pos, pts, skip, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                        what = (n, variant, m, skip is not None)
                        planted = 2 if skip is not None and m >= 65 else 0
                        check_specials_directly(want, pts, skip, n, variant, what, planted)     # the reference itself keeps the promise
                        for split in (None, "1", "2", "3"):
                            if split is None:
                                monkeypatch.delenv("NBODY_TIDAL_SPLIT", raising=False)
                            else:
                                monkeypatch.setenv("NBODY_TIDAL_SPLIT", split)
                            t = eng.tidal(pts, skip)
                            assert same_nan(t, want), what + (split, np.flatnonzero((bits(t) != bits(want)).any(1))[:8])
                            check_specials_directly(t, pts, skip, n, variant, what + (split,), planted)


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system_timed_arithmetic(nb, ref, fp64):
    """The timed arithmetic (v_rsq_f32; the v_rsq_f64 seed + one third-order step) on the hostile system: finite exactly where the
    strict reference of the same d2 form is finite, in every variant, with and without skip; a skipped NaN, inf or overflow body leaves
    no trace; a NaN body poisons every point that does not skip it."""
    dtype = np.float64 if fp64 else np.float32
    for n in SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                pts, hsk = hostile_points(nb, pos, 300, variant)
                for skip in (hsk, None):
                    for mode in (nb.ARITH_FMA3,) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                        eng.set_option(nb.OPT_ARITH, mode)
                        what = (n, variant, mode, skip is not None)
                        want = ref.f64(pos, pts, skip) if fp64 else ref.f32(pos, pts, skip, ref=(mode == nb.ARITH_REFERENCE))
                        t = eng.tidal(pts, skip)
                        assert np.array_equal(np.isfinite(t), np.isfinite(want)), what + (np.flatnonzero((np.isfinite(t) != np.isfinite(want)).any(1))[:8],)
                        assert np.array_equal(np.isnan(t), np.isnan(want)), what
                        check_specials_directly(t, pts, skip, n, variant, what, 2 if skip is not None else 0)
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
