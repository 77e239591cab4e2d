"""The sixth-order Hermite integrator (nbody_step_hermite6(_d), nbody_step_hermite6_adaptive(_d); include/nbody.h "sixth-order Hermite
integrator"): bit for bit against tests/hermite6_ref.c in the strict modes, the restart rule, the same bits however the work is laid out
(devices, processes, source split), the adaptive loop against the statement's, the Kepler pair's energy errors through the device, the
masses, NBODY_INFO_STEPS_DONE, the guards and the C host program's --hermite6 lines."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hermite_common import PERIOD, HermiteRef, kepler
from hermite_common import compile_ref as compile_hermite4
from hermite6_common import GAIN, MASS, ORDER_RATIO, REF, Hermite6Ref, compile_ref, kepler_energy_error
from pass_common import same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import SIZES as HOSTILE_SIZES
from specials_common import VARIANTS, hostile_dynamic_system, same_nan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 63, 257, 1025, 2100)   # one body, a pair, a tail below a wave, a block edge, two blocks, three blocks with a tail


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Hermite6Ref(compile_ref(tmp_path_factory.mktemp("hermite6_ref")))


@pytest.fixture(scope="module")
def ref4(tmp_path_factory):
    return HermiteRef(compile_hermite4(tmp_path_factory.mktemp("hermite_ref")))


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_three_steps_and_three_restarts_bit_for_bit(nb, ref, arith):
    """one call of three steps and three calls of one step, each against the statement; the two differ; both fourth values are carried"""
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    flags = REF if mode == nb.ARITH_REFERENCE_STRICT else 0
    dt = 1.0 / 256
    for n in SIZES:
        pos, vel = nb.make_bodies(n, dtype=dtype)
        pos[:, 3] = np.arange(n, dtype=dtype) - 7.5
        vel[:, 3] = 3.25
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            eng.upload(pos, vel)
            eng.step_hermite6(dt, 3)
            carried = eng.download()
            assert same(carried, ref.step(pos, vel, dtype, dt, 3, flags)), n
            eng.upload(pos, vel)
            for _ in range(3):
                eng.step_hermite6(dt, 1)
            restarted = eng.download()
            assert same(restarted, ref.restarted(pos, vel, dtype, dt, 3, flags)), n
            assert n < 257 or not same(carried, restarted)   # (a few bodies' crackle can stay below binary32's last place)
            assert same(carried[0][:, 3], pos[:, 3]) and same(carried[1][:, 3], vel[:, 3])


def state_after(nb, n, pos, vel, ngpus=1, fp64=False):
    with nb.NBody(n, ngpus=ngpus, fp64=fp64) as eng:
        eng.upload(pos, vel)
        eng.step_hermite6(1.0 / 256, 3)
        return eng.download()


def test_bits_do_not_depend_on_devices_or_the_source_split(nb, monkeypatch):
    """one device, three oversubscribed devices with ragged slices, and the snap and jerk passes' splits; timed binary32 and binary64"""
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n = 2100
    for fp64 in (False, True):
        pos, vel = nb.make_bodies(n, dtype=np.float64 if fp64 else np.float32)
        base = state_after(nb, n, pos, vel, fp64=fp64)
        assert not same(base[0], pos)
        assert same(state_after(nb, n, pos, vel, ngpus=3, fp64=fp64), base)
        for env, val in (("NBODY_SNAP_SPLIT", "2"), ("NBODY_SNAP_SPLIT", "7"), ("NBODY_JERK_SPLIT", "3")):
            monkeypatch.setenv(env, val)
            assert same(state_after(nb, n, pos, vel, fp64=fp64), base), (env, val)
            assert same(state_after(nb, n, pos, vel, ngpus=3, fp64=fp64), base), (env, val)
            monkeypatch.delenv(env)


WORKER = """
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step_hermite6(1.0 / 256, 3)
    t, steps = eng.step_hermite6_adaptive(0.01, 0.04, 1e-4, 1.0 / 256, max_steps=2)
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, pos=p, vel=v, t=np.array([t, steps]), done=np.array([eng.info(nb._lib.INFO_STEPS_DONE)]))
"""


def test_two_processes_host_transport_equal_one_process(nb, tmp_path):
    """positions, velocities and predicted accelerations all travel between the ranks in every step"""
    n, world = 2100, 2
    out = str(tmp_path / "h6")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    pos, vel = nb.make_bodies(n, seed=33)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        eng.step_hermite6(1.0 / 256, 3)
        t, steps = eng.step_hermite6_adaptive(0.01, 0.04, 1e-4, 1.0 / 256, max_steps=2)
        want = eng.download()
    for r in range(world):
        assert same((got[r]["pos"], got[r]["vel"]), want), r
        assert (float(got[r]["t"][0]), int(got[r]["t"][1]), int(got[r]["done"][0])) == (t, steps, 5), r
    assert steps == 2 and not same(want[0], pos)


def test_adaptive_loop_is_the_statements(nb, ref):
    """strict binary64, Kepler e = 0.9 over one period, eta = 0.04: state, t_reached and steps_taken are hermite6_ref's loop bit for bit;
    strict binary32 on 257 bodies likewise, stopped by max_steps"""
    pos, vel = kepler(0.9)
    args = (PERIOD, 0.04, 1e-6, 1.0)
    with nb.NBody(2, fp64=True) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos, vel)
        t, steps = eng.step_hermite6_adaptive(*args)
        wp, wv, wt, wsteps = ref.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0)
        assert (t, steps) == (wt, wsteps) and t == PERIOD and same(eng.download(), (wp, wv))
        eng.upload(pos, vel)
        t5, s5 = eng.step_hermite6_adaptive(*args, max_steps=5)
        w5 = ref.adaptive(pos, vel, np.float64, 0.04, PERIOD, 1e-6, 1.0, max_steps=5)
        assert (t5, s5) == w5[2:] and s5 == 5 and same(eng.download(), w5[:2])
    n = 257
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos, vel)
        eta, lo = float(np.float32(0.04)), float(np.float32(1e-6))   # the binary32 entry point takes binary32 arguments
        t, steps = eng.step_hermite6_adaptive(1.0, eta, lo, 1.0 / 64, max_steps=4)
        w = ref.adaptive(pos, vel, np.float32, eta, 1.0, lo, 1.0 / 64, max_steps=4)
        assert (t, steps) == w[2:] and steps == 4 and same(eng.download(), w[:2])


def test_kepler_energy_errors_through_the_device(nb, ref, ref4):
    """strict binary64, Kepler e = 0.5 to t = 1: the device's states are the statement's bit for bit, so its bounds apply to them —
    err(64) / err(128) >= 45, err(128) / err(256) >= 45, err6(128) <= err4(128) / 100 with err4 from tests/hermite_ref.c.
    Measured on an MI355X: 1.723e-8, 2.656e-10, 4.115e-12 (ratios 64.9 and 64.5); err4(128) = 1.838e-7, a ratio of 692."""
    with nb.NBody(2, fp64=True) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)

        def device6(pos, vel, dt, n):
            eng.upload(pos, vel)
            eng.step_hermite6(dt, n)
            got = eng.download()
            assert same(got, ref.step(pos, vel, np.float64, dt, n)), n
            return got

        err = [kepler_energy_error(device6, n) for n in (64, 128, 256)]
        err4 = kepler_energy_error(lambda p, v, dt, n: ref4.step(p, v, np.float64, dt, n), 128)
    print("sixth order %s, ratios %.2f %.2f; fourth order at 128 steps %.3e" % (err, err[0] / err[1], err[1] / err[2], err4))
    assert err[0] / err[1] >= ORDER_RATIO and err[1] / err[2] >= ORDER_RATIO
    assert err[1] <= err4 / GAIN


def test_masses(nb, ref):
    """as tests/test_gpu_masses.py asks of the fourth-order scheme.  masses_common's Kepler pair of masses 3/4 and 1/4, e = 0.5, 128
    steps to t = 1: strict binary64 is the statement bit for bit.  N = 257 with masses in [0.25, 4), 4 steps of 1/256, strict binary64:
    the state is the statement's bit for bit, so |P1 - P0| / sum m |v| is the statement's own figure, and it stays below the roundings
    of four steps, 4 x 4 x 2^-53 x sqrt(N) (each step rounds a body's m v a few times, independently from body to body) — a pair
    weighted by m_i in place of m_j loses O(1) in the same run (tests/test_gpu_masses.py).  Every w = 1 gives the unweighted bits.
    Measured on an MI355X: |dE|/|E| 3.3e-11 for the pair; |dP| / sum m |v| 3.8e-15 against the bound's 2.8e-14."""
    from masses_common import kepler as kepler_masses, numpy_totals, random_masses, with_masses
    pos, vel = kepler_masses(0.75, 0.25, 0.5)
    with nb.NBody(2, fp64=True) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.use_masses()
        eng.upload(pos, vel)
        eng.step_hermite6(1.0 / 128, 128)
        got = eng.download()
    assert same(got, ref.step(pos, vel, np.float64, 1.0 / 128, 128, MASS))
    e0 = numpy_totals(pos, vel)[0]
    print("masses 3/4 and 1/4: |dE|/|E| %.3e" % (abs(numpy_totals(*got)[0] - e0) / abs(e0)))
    n = 257
    p0, v0 = nb.make_bodies(n, dtype=np.float64)
    pos = with_masses(p0, random_masses(n, dtype=np.float64))
    with nb.NBody(n, fp64=True) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(p0 * np.array([1, 1, 1, 0]) + np.array([0, 0, 0, 1.0]), v0)
        eng.step_hermite6(1.0 / 256, 4)
        plain = eng.download()
        eng.use_masses()
        eng.upload(p0 * np.array([1, 1, 1, 0]) + np.array([0, 0, 0, 1.0]), v0)
        eng.step_hermite6(1.0 / 256, 4)
        assert same(eng.download(), plain)
        eng.upload(pos, v0)
        eng.step_hermite6(1.0 / 256, 4)
        got = eng.download()
    assert same(got, ref.step(pos, v0, np.float64, 1.0 / 256, 4, MASS)) and not same(got[0][:, :3], plain[0][:, :3])
    _, mom0, scale = numpy_totals(pos, v0)
    mom1 = numpy_totals(*got)[1]
    dp = np.sqrt(((mom1 - mom0) ** 2).sum()) / scale
    print("|dP| / sum m |v| after 4 steps: %.3e" % dp)
    assert dp <= 4 * 4 * 2.0 ** -53 * np.sqrt(n)


def test_steps_done_and_what_a_call_leaves_alone(nb):
    """NBODY_INFO_STEPS_DONE counts sixth-order steps too; a later nbody_step gives what it gives on a fresh context uploaded with
    the corrected state; jerk() sees the corrected state of all bodies"""
    n = 1025
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        before = eng.info(nb._lib.INFO_STEPS_DONE)
        eng.step_hermite6(1.0 / 256, 3)
        eng.step_hermite6(-1.0 / 256, 1)   # a negative dt is legal
        assert eng.info(nb._lib.INFO_STEPS_DONE) == before + 4
        state = eng.download()
        aj = eng.jerk()
        eng.step(0.01, 2)
        after = eng.download()
    with nb.NBody(n) as eng:
        eng.upload(*state)
        assert same(eng.jerk(), aj)
        eng.step(0.01, 2)
        assert same(eng.download(), after)


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    t, steps = C.c_double(7.0), C.c_int(7)
    ad32 = lambda eta=0.04, t_end=1.0, lo=1e-6, hi=1.0, ms=10: lib.nbody_step_hermite6_adaptive(eta, t_end, lo, hi, ms, C.byref(t), C.byref(steps))
    ad64 = lambda eta=0.04, t_end=1.0, lo=1e-6, hi=1.0, ms=10: lib.nbody_step_hermite6_adaptive_d(eta, t_end, lo, hi, ms, C.byref(t), C.byref(steps))
    nan, inf = float("nan"), float("inf")
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [lib.nbody_step_hermite6(0.01, 1), lib.nbody_step_hermite6_d(0.01, 1), ad32(), ad64()] == [E.ERR_STATE] * 4
        finally:
            mb.serve(False)
    n = 100
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        assert [lib.nbody_step_hermite6(0.01, 0), lib.nbody_step_hermite6(0.01, -3)] == [E.ERR_ARG] * 2
        assert [lib.nbody_step_hermite6(x, 1) for x in (nan, inf, -inf)] == [E.ERR_ARG] * 3
        for kw in (dict(eta=0.0), dict(eta=-1.0), dict(eta=nan), dict(t_end=0.0), dict(t_end=inf), dict(lo=0.0), dict(lo=2.0, hi=1.0), dict(hi=nan), dict(ms=0)):
            assert ad32(**kw) == E.ERR_ARG, kw
        assert (t.value, steps.value) == (7.0, 7) and same(eng.download(), (pos, vel))
        assert [lib.nbody_step_hermite6_d(0.01, 1), ad64()] == [E.ERR_STATE] * 2
        assert lib.nbody_step_hermite6_adaptive(0.04, 0.01, 1e-6, 1.0, 10, None, None) == 0
        assert not same(eng.download()[0], pos)
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert [lib.nbody_step_hermite6(0.01, 1), ad32()] == [E.ERR_STATE] * 2
        assert [lib.nbody_step_hermite6_d(0.01, 1), ad64(t_end=0.01)] == [0, 0]


def test_c_host_program_hermite6_lines(nb):
    """./build/nbody 2048 4 --hermite6 runs, names its loop, prints the energies and leaves the state step_hermite6 leaves; with
    --masses it runs too; --host-loop and --hermite-block are refused beside it"""
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters = 2048, 4
    r = subprocess.run([exe, str(n), str(iters), "--hermite6"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device Hermite-6 loop" in r.stdout
    lines = re.findall(r"^energy at step (\d+): E (\S+) T (\S+) U (\S+)", r.stdout, flags=re.M)
    assert [int(l[0]) for l in lines] == [0, iters], r.stdout
    got = [float(v) for v in re.search(r"^checksum \(sum of positions\): (\S+) (\S+) (\S+)$", r.stdout, flags=re.M).groups()]
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        e0 = eng.energy()["total"]
        eng.step_hermite6(0.01, iters)
        p = eng.download()[0]
        e1 = eng.energy()["total"]
    want = [0.0] * 3
    for k in range(n):   # plain ascending fp64 sums, printed with nine digits
        for c in range(3):
            want[c] += float(p[k, c])
    assert [float("%.9g" % w) for w in want] == got, (got, want)
    assert [float(lines[0][1]), float(lines[1][1])] == [e0, e1]
    r = subprocess.run([exe, str(n), str(iters), "--hermite6", "--masses"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "device Hermite-6 loop" in r.stdout and len(re.findall(r"^energy at step", r.stdout, flags=re.M)) == 2, r.stdout + r.stderr
    for extra in (["--host-loop"], ["--hermite-block", "4"]):
        r = subprocess.run([exe, str(n), str(iters), "--hermite6"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and extra[0] in r.stderr, extra


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_hostile_system_strict_steps(nb, ref, arith):
    """specials_common.hostile_dynamic_system in every variant and size: one call of three steps of 1/256 and three calls of one step,
    each the statement's bit for bit (NaN where it is NaN), both fourth values carried.  In "base" and "overflow" every row of the
    downloaded state is finite — with hostile_system's own velocity of 1e18 (1e150) no row is after one step, and the comparison
    would be NaN against NaN (tests/test_specials_dynamic_reference.py asserts the same of the statement)."""
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    flags = REF if mode == nb.ARITH_REFERENCE_STRICT else 0
    dt = 1.0 / 256
    differ = []
    for n in HOSTILE_SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            for variant in VARIANTS:
                pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
                pos[:, 3] = np.arange(n, dtype=dtype) - 7.5
                vel[:, 3] = 3.25
                with np.errstate(all="ignore"):
                    want = {"carried": ref.step(pos, vel, dtype, dt, 3, flags), "restarted": ref.restarted(pos, vel, dtype, dt, 3, flags)}
                for form, calls in (("carried", (3,)), ("restarted", (1, 1, 1))):
                    eng.upload(pos, vel)
                    for k in calls:
                        eng.step_hermite6(dt, k)
                    got = eng.download()
                    if not (same_nan(got[0], want[form][0]) and same_nan(got[1], want[form][1])):
                        differ.append((n, variant, form))
                    if not (same(got[0][:, 3], pos[:, 3]) and same(got[1][:, 3], vel[:, 3])):
                        differ.append((n, variant, form, "fourth values"))
                    if variant in ("base", "overflow") and not (np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))):
                        differ.append((n, variant, form, "a row is not finite"))
                    if variant in ("nan", "inf") and np.any(np.isfinite(got[0][:, :3]).all(1) & np.isfinite(got[1][:, :3]).all(1)):
                        differ.append((n, variant, form, "a row escaped the poison"))
                if variant in ("base", "overflow") and same(want["carried"], want["restarted"]):
                    differ.append((n, variant, "the carried and the restarted form do not differ"))
    assert not differ, differ
