"""Pair time scales and the shared adaptive step on the device (nbody_timescale_rows, nbody_min_timescale, nbody_step_adaptive and
their _d forms; include/nbody.h "pair time scales and a shared adaptive time step"): every case bit for bit against
tests/timescale_ref.c — idx equal, tau2 and d2min the same bits — in both precisions, on the hostile system, however the work is laid
out (source split, batches, windows of rows, force configuration, device and process count); d2min against the neighbour pass; no effect
on the step; the driver against a Python loop of its stated formula; the guards; the C host program's --adaptive line."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from field_common import EPS
from pass_common import FORCE_CONFIGS, check_step_untouched
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import SIZES, VARIANTS, hostile_system, same_nan
from timescale_common import bits, make_ref, same, same_system, step_size, two_body_orbit

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("NBODY_TIMESCALE_SPLIT", "NBODY_TIMESCALE_SCRATCH_MB")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("timescale_ref"))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def windows(n):
    """(first_row, n_rows): everything, the last row alone, a window across a 64 boundary and across a 256 boundary"""
    w = [(0, n), (n - 1, 1)]
    if n > 70:
        w.append((50, 20))
    if n > 300:
        w.append((200, 100))
    return w


@pytest.mark.parametrize("fp64", [False, True])
def test_rows_and_system_bit_for_bit(nb, ref, fp64):
    dtype = np.float64 if fp64 else np.float32
    for n in (1, 2, 63, 64, 65, 1000, 1025, 4099):   # window and block edges, ragged tails, the lone body
        pos, vel = nb.make_bodies(n, dtype=dtype)
        want = ref.rows(pos, vel)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for first, cnt in windows(n):
                assert same(eng.timescales(first, cnt), tuple(w[first:first + cnt] for w in want)), (n, first, cnt)
            assert same(eng.timescales(), want), n
            assert same_system(eng.min_timescale(), ref.system(pos, vel)), n
        if n > 1:
            assert np.all(want[1] >= 0) and np.all(np.isfinite(want[0])) and np.all(want[0] > 0), n


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system(nb, ref, monkeypatch, fp64):
    """NaN and inf positions, a NaN velocity, a 1e18 (1e150) velocity whose square is finite and leaves the quotients of its pairs
    tiny — in binary32 around the smallest normal number, subnormal ones among them — coincident groups across the 1023 | 1024 edge, signed zeros: the
    floats with the same NaN mask and the same bits elsewhere, idx equal, for every split.  (A v2 that does overflow is in
    test_hand_made_specials.)"""
    dtype = np.float64 if fp64 else np.float32
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_system(nb, n, dtype, variant)
            want = ref.rows(pos, vel)
            wsys = ref.system(pos, vel)
            assert not np.any(np.isnan(want[0])) and not np.any(np.isnan(want[2]))   # a NaN is never chosen
            with nb.NBody(n, fp64=fp64) as eng:
                eng.upload(pos, vel)
                for split in (None, "1", "2", "3"):
                    if split:
                        monkeypatch.setenv("NBODY_TIMESCALE_SPLIT", split)
                    tau2, idx, d2min = eng.timescales()
                    assert same_nan(tau2, want[0]) and np.array_equal(idx, want[1]) and same_nan(d2min, want[2]), (n, variant, split)
                    got = eng.min_timescale()
                    assert (got[1], got[2]) == (wsys[1], wsys[2]), (n, variant, split)
                    assert same_nan(np.array([got[0], got[3]]), np.array([wsys[0], wsys[3]])), (n, variant, split)
                monkeypatch.delenv("NBODY_TIMESCALE_SPLIT")
            if n > 1024:
                assert np.all(bits(want[2][[1023, 1025]]) == 0), (n, variant)   # the coincident group (1024 is the NaN body of "nan"): d2min = +0
            assert 0 < want[0][6] < (1e-295 if fp64 else 1e-35)   # body 6's 1e18 (1e150): v2 = 1e36 (1e300); binary32: quotients at the subnormal edge


@pytest.mark.parametrize("fp64", [False, True])
def test_hand_made_specials(nb, ref, fp64):
    """the systems of tests/test_timescale_abi.py whose answers are known by construction, on the device"""
    dtype = np.float64 if fp64 else np.float32
    big = 1e30 if dtype is np.float32 else 1e200
    cases = (([[1, 2, 3]], [[1, 0, 0]]),                                                          # nobody else
             ([[0, 0, 0], [2, 0, 0]], [[0, 2, 0], [0, -2, 0]]),                                   # q = 4 / 16
             ([[0, 0, 0], [2, 0, 0]], [[1, 1, 1], [1, 1, 1]]),                                    # v2 = 0: +inf, never chosen
             ([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 0]]),                                    # 0 / 0: NaN, never chosen; d2min = +0
             ([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 3]]),                                    # coincident and moving: +0
             ([[0, 0, 0], [2, 0, 0], [0, 2, 0]], [[0, 0, 0], [0, 2, 0], [2, 0, 0]]),              # every pair ties: the lowest j, the lowest row
             ([[0, 0, 0], [2, 0, 0], [0, 3, 0]], [[0, 0, 0], [big, 0, 0], [0, 1, 0]]),            # v2 overflows: q = +0
             ([[0, 0, 0], [2, 0, 0], [0, 3, 0]], [[0, 0, 0], [np.nan, 0, 0], [0, 1, 0]]),         # a NaN velocity poisons its own pairs only
             ([[0, 0, 0], [big, 0, 0], [0, 3, 0]], [[0, 0, 0], [1, 0, 0], [0, 1, 0]]))            # d2 overflows: +inf, never chosen
    for p, v in cases:
        pos, vel = np.zeros((len(p), 4), dtype), np.zeros((len(p), 4), dtype)
        pos[:, :3], vel[:, :3] = p, v
        with nb.NBody(len(p), fp64=fp64) as eng:
            eng.upload(pos, vel)
            assert same(eng.timescales(), ref.rows(pos, vel)), (p, v)
            assert same_system(eng.min_timescale(), ref.system(pos, vel)), (p, v)


@pytest.mark.parametrize("fp64", [False, True])
def test_d2min_is_the_neighbour_pass_d2(nb, fp64):
    dtype = np.float64 if fp64 else np.float32
    for n in (2, 65, 2100):
        pos, vel = nb.make_bodies(n, seed=9, dtype=dtype)
        if n > 1000:
            pos[70, :3] = pos[3, :3]
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            assert same(eng.timescales()[2], eng.neighbors()[1]), n
            assert bits(eng.min_timescale()[3]) == bits(eng.closest_pair()[2]), n


def test_values_do_not_depend_on_the_source_split_or_the_batches(nb, ref, monkeypatch):
    n, m = 5000, 700   # five blocks
    pos, vel = nb.make_bodies(n)
    want = ref.rows(pos, vel)
    wsys = ref.system(pos, vel)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)

        def check(tag):
            assert same(eng.timescales(), want), tag
            assert same(eng.timescales(100, m), tuple(w[100:100 + m] for w in want)), tag
            assert same_system(eng.min_timescale(), wsys), tag

        for split in (None, "1", "2", "3", "4", "5", "64"):
            if split:
                monkeypatch.setenv("NBODY_TIMESCALE_SPLIT", split)
            check(split)
        # 5000 rows x 5 chunks x 12 B = 300 kB against 1 MB: one batch; against 0.02 MB = 20971 B: batches of 256 rows
        for mb in ("1", "0.02"):
            monkeypatch.setenv("NBODY_TIMESCALE_SCRATCH_MB", mb)
            for split in ("5", None):
                if split:
                    monkeypatch.setenv("NBODY_TIMESCALE_SPLIT", split)
                else:
                    monkeypatch.delenv("NBODY_TIMESCALE_SPLIT")
                check(("batches", mb, split))
        monkeypatch.setenv("NBODY_TIMESCALE_SPLIT", "5")
        monkeypatch.setenv("NBODY_TIMESCALE_SCRATCH_MB", "0")   # not even one workgroup's rows fit: no split
        check("no scratch")


def test_values_do_not_depend_on_the_rows_beside_a_row_or_the_force_configuration(nb, ref):
    n = 5000
    pos, vel = nb.make_bodies(n)
    want = ref.rows(pos, vel)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for first, cnt in ((0, 1), (100, 257), (4999, 1), (63, 66), (1000, 3000)):
            assert same(eng.timescales(first, cnt), tuple(w[first:first + cnt] for w in want)), (first, cnt)
        for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT):
            eng.set_option(nb.OPT_ARITH, mode)
            assert same(eng.timescales(), want), mode
        eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            assert same(eng.timescales(), want) and same_system(eng.min_timescale(), ref.system(pos, vel)), (key, val)
            eng.set_option(key, default)


def test_values_do_not_depend_on_the_device_count(nb, ref, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n = 1500   # 1500 = 500 x 3: slices that end inside a 64-source window and inside a workgroup's rows
    pos, vel = nb.make_bodies(n)
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            drift = (eng.timescales(), eng.download())
            # ... and after steps only its own new velocities as well
            eng.step(0.01, 2)
            res[ngpus] = drift + (eng.timescales(), eng.timescales(450, 600), eng.min_timescale(), eng.download())
    assert same(res[1][1], res[3][1]), "a drift is the same on one device and on three"
    assert not same((res[1][1][0],), (pos,)) and same((res[1][1][1],), (vel,)), "no drift happened"
    for g_ in (1, 3):
        assert same(res[g_][0], ref.rows(*res[g_][1])), g_
        now, vnow = res[g_][5]   # (the timed arithmetic's sums follow the device count: each state against its own reference)
        assert not same((vnow,), (vel,)), "the velocities did not change"
        want = ref.rows(now, vnow)
        assert same(res[g_][2], want), g_
        assert same(res[g_][3], tuple(w[450:1050] for w in want)), g_   # a window across both device boundaries: global indices
        assert same_system(res[g_][4], ref.system(now, vnow)), g_


WORKER = """
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    tau2, idx, d2min = eng.timescales()                         # this rank's own rows
    best = eng.min_timescale()
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, tau2=tau2, idx=idx, d2min=d2min, best_ij=np.array(best[1:3]),
             best_f=np.array([best[0], best[3]], np.float32), first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p, vel=v)
"""


def test_two_processes_host_transport_equal_the_reference(nb, ref, tmp_path):
    """after three steps the velocities differ from the upload, and each rank holds only its own: they must really be gathered"""
    n, world = 6007, 2
    out = str(tmp_path / "ts")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now, vnow = got[0]["pos"], got[0]["vel"]
    assert same((now, vnow), (got[1]["pos"], got[1]["vel"]))
    assert not same((vnow,), (nb.make_bodies(n, seed=33)[1],))
    want = ref.rows(now, vnow)
    wsys = ref.system(now, vnow)
    covered = 0
    for r in range(world):
        g_ = got[r]
        first, cnt = (int(v) for v in g_["first"])
        assert same((g_["tau2"], g_["idx"], g_["d2min"]), tuple(w[first:first + cnt] for w in want)), r   # global indices
        covered += cnt
        assert tuple(int(v) for v in g_["best_ij"]) == wsys[1:3], r
        assert bits(g_["best_f"][0]) == bits(wsys[0]) and bits(g_["best_f"][1]) == bits(wsys[3]), r
    assert covered == n


def test_timescale_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    probe = lambda eng: (eng.timescales(), eng.min_timescale())
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_TIMESCALE_SPLIT")


def python_adaptive(eng, t_end, eta, dt_min, dt_max, max_steps, after=None):
    """the loop of nbody_step_adaptive in Python: min_timescale() + step(dt, 1) with the stated formula"""
    t, steps = 0.0, 0
    while t < t_end and steps < max_steps:
        tau2, i, j, d2min = eng.min_timescale()
        h = step_size(tau2, d2min, eta, dt_min, dt_max, t, t_end)
        dt = h if eng.fp64 else float(np.float32(h))
        eng.step(dt, 1)
        t += dt
        steps += 1
        if after:
            after(eng, dt)
    return t, steps


@pytest.mark.parametrize("fp64", [False, True])
def test_step_adaptive_is_the_python_loop_bit_for_bit(nb, fp64):
    n = 300
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    eta, dt_min, dt_max = 2.0 ** -5, 2.0 ** -20, 2.0 ** -4   # exact in either precision

    def run(driver, t_end, max_steps):
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
            eng.upload(pos, vel)
            out = driver(eng, t_end, max_steps)
            return out, eng.download()

    dts = []
    (t20, k20), state20 = run(lambda eng, te, ms: python_adaptive(eng, te, eta, dt_min, dt_max, ms, after=lambda e, dt: dts.append(dt)), 1e9, 20)
    assert k20 == 20 and 0 < t20 < 1e9 and all(dt_min <= dt <= dt_max for dt in dts) and len(set(dts)) > 1, dts
    # the cut-off: max_steps ends the call with t_reached < t_end
    (t, k), state = run(lambda eng, te, ms: eng.step_adaptive(te, eta, dt_min, dt_max, ms), 1e9, 20)
    assert (t, k) == (t20, 20) and same(state, state20)
    # t_end inside the 13th step: the last step is the rest of the way
    t_end = float(np.float32(sum(dts[:12]) + dts[12] / 2))
    want, wstate = run(lambda eng, te, ms: python_adaptive(eng, te, eta, dt_min, dt_max, ms), t_end, 1000)
    (t, k), state = run(lambda eng, te, ms: eng.step_adaptive(te, eta, dt_min, dt_max, ms), t_end, 1000)
    assert (t, k) == want and k >= 13 and t >= t_end and same(state, wstate)
    assert not same(state, state20)


def test_adaptive_beats_a_fixed_step_on_an_eccentric_orbit_fp64(nb):
    """two unit masses, a = 1, e = 0.9, one period from apocentre, eta = 0.02, on the device in fp64: the worst |dE / E| (nbody_energy
    after every step) of the adaptive run is below that of a fixed-step run with the same number of steps, as the numpy restatement
    shows on the CPU (tests/test_timescale_abi.py: 529 steps, 0.377 against 1.387).  Only the ordering is asserted."""
    eta, dt_min, dt_max = 0.02, 1e-9, 1.0
    pos, vel, period = two_body_orbit(0.9)
    worst = {"adaptive": 0.0, "fixed": 0.0}
    with nb.NBody(2, fp64=True) as eng:
        eng.upload(pos, vel)
        e0 = eng.energy()["total"]

        def watch(name):
            def after(e, dt):
                worst[name] = max(worst[name], abs((e.energy()["total"] - e0) / e0))
            return after

        t, steps = python_adaptive(eng, period, eta, dt_min, dt_max, 100000, after=watch("adaptive"))
        loop_state = eng.download()
        assert t >= period and 100 < steps < 5000
        eng.upload(pos, vel)
        for _ in range(steps):
            eng.step(period / steps, 1)
            watch("fixed")(eng, None)
        eng.upload(pos, vel)
        assert eng.step_adaptive(period, eta, dt_min, dt_max) == (t, steps) and same(eng.download(), loop_state)
    print("e = 0.9, eta = %g on the device: %d steps, worst |dE/E| adaptive %.4g, fixed %.4g" % (eta, steps, worst["adaptive"], worst["fixed"]))
    assert worst["adaptive"] < worst["fixed"]


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    f32, f64, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    idx = np.full(4, 7, np.int32)
    t32, d32, t64, d64 = np.full(4, 7, np.float32), np.full(4, 7, np.float32), np.full(4, 7, np.float64), np.full(4, 7, np.float64)
    tr, st = C.c_double(7.0), C.c_int(7)
    calls32 = (lambda: lib.nbody_timescale_rows(0, 4, t32.ctypes.data_as(f32), ip(idx), d32.ctypes.data_as(f32)),
               lambda: lib.nbody_min_timescale(t32.ctypes.data_as(f32), ip(idx), ip(idx[1:]), d32.ctypes.data_as(f32)),
               lambda: lib.nbody_step_adaptive(0.5, 0.25, 0.125, 0.125, 3, C.byref(tr), C.byref(st)))
    calls64 = (lambda: lib.nbody_timescale_rows_d(0, 4, t64.ctypes.data_as(f64), ip(idx), d64.ctypes.data_as(f64)),
               lambda: lib.nbody_min_timescale_d(t64.ctypes.data_as(f64), ip(idx), ip(idx[1:]), d64.ctypes.data_as(f64)),
               lambda: lib.nbody_step_adaptive_d(0.5, 0.25, 0.125, 0.125, 3, C.byref(tr), C.byref(st)))
    untouched = lambda: (np.all(idx == 7) and np.all(t32 == 7) and np.all(d32 == 7) and np.all(t64 == 7) and np.all(d64 == 7)
                         and tr.value == 7.0 and st.value == 7)
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
        t_, i_, d_ = t32.ctypes.data_as(f32), ip(idx), d32.ctypes.data_as(f32)
        assert lib.nbody_timescale_rows(0, 4, None, None, None) == E.ERR_ARG
        for first, rows in ((-1, 4), (0, 0), (0, -2), (97, 4), (100, 1), (0, 101), (1 << 30, 1 << 30)):
            assert lib.nbody_timescale_rows(first, rows, t_, i_, d_) == E.ERR_ARG, (first, rows)
        assert lib.nbody_min_timescale(None, None, None, None) == E.ERR_ARG
        inf, nan = math.inf, math.nan
        for eta, t_end, lo, hi, ms in ((0.0, 1.0, 0.1, 0.2, 5), (-0.5, 1.0, 0.1, 0.2, 5), (0.5, 0.0, 0.1, 0.2, 5), (0.5, -1.0, 0.1, 0.2, 5),
                                       (0.5, 1.0, 0.0, 0.2, 5), (0.5, 1.0, -0.1, 0.2, 5), (0.5, 1.0, 0.3, 0.2, 5), (0.5, 1.0, 0.1, 0.2, 0),
                                       (0.5, 1.0, 0.1, 0.2, -1), (inf, 1.0, 0.1, 0.2, 5), (0.5, inf, 0.1, 0.2, 5), (0.5, 1.0, inf, inf, 5),
                                       (0.5, 1.0, 0.1, inf, 5), (nan, 1.0, 0.1, 0.2, 5), (0.5, nan, 0.1, 0.2, 5), (0.5, 1.0, nan, 0.2, 5),
                                       (0.5, 1.0, 0.1, nan, 5)):
            assert lib.nbody_step_adaptive(eta, t_end, lo, hi, ms, C.byref(tr), C.byref(st)) == E.ERR_ARG, (eta, t_end, lo, hi, ms)
        assert untouched()
        p0 = eng.download()
        assert same(p0, (pos, vel))   # ... and nothing was stepped
        assert lib.nbody_timescale_rows(96, 4, None, i_, None) == 0 and not np.any(idx == 7) and np.all(t32 == 7) and np.all(d32 == 7)
        assert lib.nbody_timescale_rows(96, 4, t_, None, None) == 0 and not np.any(t32 == 7) and np.all(d32 == 7)
        assert lib.nbody_min_timescale(None, None, i_, None) == 0 and idx[0] == eng.min_timescale()[2]
        assert calls32[2]() == 0 and (tr.value, st.value) == (0.25, 2)
        assert lib.nbody_step_adaptive(0.5, 0.25, 0.125, 0.125, 3, None, None) == 0
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert [c() for c in calls32] == [E.ERR_STATE] * 3 and [c() for c in calls64] == [0] * 3


def test_c_host_program_adaptive_line(nb, ref):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters, eta = 4096, 3, 0.02
    for flags, fp64 in (([], False), (["--fp64"], True)):
        r = subprocess.run([exe, str(n), str(iters), "--adaptive", repr(eta)] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = re.findall(r"^min timescale: tau2 (\S+) pair (-?\d+) (-?\d+) d2min (\S+) dt (\S+)$", r.stdout, flags=re.M)
        assert len(lines) == 1, r.stdout
        plain = subprocess.run([exe, str(n), str(iters)] + flags, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0 and "timescale" not in plain.stdout
        strip = lambda text: [ln for ln in text.splitlines() if "Billion Interactions" not in ln and not ln.startswith("min timescale")]
        assert strip(r.stdout) == strip(plain.stdout)   # nothing else changes (the rate line carries a time)
        dtype = np.float64 if fp64 else np.float32
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            eng.step(float(np.float32(0.01)), iters)   # the program's dt is the binary32 0.01 in fp64 contexts too
            got = eng.min_timescale()
            now, vnow = eng.download()
        assert same_system(got, ref.system(now, vnow))
        tau2, i, j, d2min, dt = lines[0]
        assert (int(i), int(j)) == (got[1], got[2]) and dtype(float(tau2)) == got[0] and dtype(float(d2min)) == got[3]
        s = float(got[3]) + EPS
        assert float(dt) == eta * math.sqrt(min(float(got[0]), s * math.sqrt(s) / 2.0))
    assert subprocess.run([exe, str(n), str(iters), "--adaptive", "0"], capture_output=True, text=True, timeout=60).returncode == 2
