"""NBODY_OPT_MASSES on the device (include/nbody.h): the option itself; the weighted field, tidal tensor, jerk, potential, energy
totals and the Hermite integrators bit for bit against tests/masses_ref.c in the strict modes; the three exact properties — unit masses
are the option switched off, scaling by 2^k, appended bodies of zero mass —; the timed binary32 arithmetic within the bound derived from
the reference's own error; momentum conservation (m_j, not m_i); a Kepler pair of unequal masses; the same bits however the work is laid
out; the refusals of the unit-mass entry points; the C host program's --masses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from field_common import make_points, make_skip
from jerk_common import TIMED_SHAPE
from hermite6_block_common import Block6Ref
from hermite6_block_common import compile_ref as compile_block6
from hermite6_common import MASS as H6_MASS
from hermite6_common import REF as H6_REF
from hermite6_common import Hermite6Ref
from hermite6_common import compile_ref as compile_hermite6
from masses_common import (R_REF, R_REF_HOSTILE, RSQ_SHARE, SIZES, compile_masses_ref, kepler, numpy_field, numpy_jerk, numpy_totals, random_masses,
                           with_masses, worst)
from pass_common import bits, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from snap_common import SnapRef
from specials_common import INF_MASS_ROW, VARIANTS, hostile_dynamic_system, hostile_masses, hostile_point_words, hostile_points, nan_row, near, same_nan
from specials_common import SIZES as HOSTILE_SIZES

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ARITHS = {"strict": (False, "ARITH_STRICT", False), "reference_strict": (False, "ARITH_REFERENCE_STRICT", True), "fp64_strict": (True, "ARITH_STRICT", False)}
# What masses_ref.c's strict binary64 keeps of |P(4 steps) - P(0)| / sum m |v| at N = 257, masses in [0.25, 4), dt = 1/256, measured on
# the CPU: 8.81e-16 (the sums' rounding; with m_i in place of m_j in the pair a plain numpy run of the same steps loses 4.6, not a small
# number at all: make_bodies has close pairs).  The test's bound is 4 times it.
MOMENTUM_REF = 8.9e-16


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return compile_masses_ref(tmp_path_factory.mktemp("masses_ref"))


def system(nb, n, dtype, masses=None, seed=5):
    """make_bodies with masses in the w of the positions (default: random in [0.25, 4)) and canaries in the w of the velocities"""
    pos, vel = nb.make_bodies(n, dtype=dtype)
    pos = with_masses(pos, random_masses(n, seed, dtype) if masses is None else masses)
    vel[:, 3] = (np.arange(n) % 31).astype(dtype) + dtype(0.25)
    return pos, vel


def queries(nb, pos, m=257):
    n = len(pos)
    pts, on = make_points(nb, pos, m)
    pts[:, 3] = 99.0   # queries have no mass: the w of a points word is ignored
    return pts, nb.make_bodies(m, seed=78, dtype=pos.dtype.type)[1], make_skip(n, m, on)


def totals_of(e):
    return np.concatenate([[e["kinetic"], e["potential"]], e["momentum"], e["angular_momentum"]])


def passes(eng, pts, pvel, skip):
    """every weighted pass of the state on the device, as one tuple of arrays"""
    n = eng.n
    return (*eng.field(pts), *eng.field(pts, skip), eng.tidal(pts, skip), *eng.jerk_at(pts, pvel, skip), *eng.jerk(), eng.potential_rows(0, n),
            totals_of(eng.energy()))


def test_the_option_is_accepted_and_read_back(nb):
    lib, E = nb._lib.load(), nb._lib
    with nb.NBody(100) as eng:
        assert eng.info(E.INFO_MASSES) == 0 and eng.config["masses"] == 0
        eng.use_masses()
        assert eng.info(E.INFO_MASSES) == 1 and eng.config["masses"] == 1
        assert [lib.nbody_set_option(E.OPT_MASSES, v) for v in (2, -1)] == [E.ERR_ARG] * 2
        assert eng.info(E.INFO_MASSES) == 1
        eng.use_masses(False)
        assert eng.info(E.INFO_MASSES) == 0
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        assert lib.nbody_set_option(E.OPT_MASSES, 1) == 0
        mb_info = C.c_longlong()
        assert lib.nbody_get_info(E.INFO_MASSES, C.byref(mb_info)) == 0 and mb_info.value == 1
        assert lib.nbody_set_option(E.OPT_MASSES, 0) == 0
        mb.serve(True, clock_khz=300000)
        try:
            assert lib.nbody_set_option(E.OPT_MASSES, 1) == E.ERR_STATE
        finally:
            mb.serve(False)
    with nb.Mailbox(capacity=1024, faithful=False):   # opening a context resets the option
        assert lib.nbody_get_info(E.INFO_MASSES, C.byref(mb_info)) == 0 and mb_info.value == 0


@pytest.mark.parametrize("arith", list(ARITHS))
def test_strict_bit_for_bit(nb, ref, arith):
    """random masses in [0.25, 4): field with and without skip, tidal, jerk at points and at rows, potential_rows, energy(), three Hermite
    steps of 1/256 and one block call with 3 levels, counters included, at one body, tails below a wave and a workgroup, and one, two and
    three blocks; the downloaded w is the uploaded w"""
    fp64, mode, r = ARITHS[arith]
    dtype = np.float64 if fp64 else np.float32
    for n in SIZES:
        pos, vel = system(nb, n, dtype)
        pts, pvel, skip = queries(nb, pos)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            eng.use_masses()
            eng.upload(pos, vel)
            got = passes(eng, pts, pvel, skip)
            want = (*ref.field(pos, pts, dtype, None, r), *ref.field(pos, pts, dtype, skip, r), ref.tidal(pos, pts, dtype, skip, r),
                    *ref.jerk(pos, vel, pts, pvel, dtype, skip, r), *ref.jerk_rows(pos, vel, dtype, r), ref.potential(pos, dtype, r),
                    ref.totals(pos, vel, dtype, ref=r))
            for k, (g, w) in enumerate(zip(got, want)):
                assert same(g, w), (n, k, int((bits(g) != bits(w)).sum()))
            eng.step_hermite(1.0 / 256, 3)
            state = eng.download()
            assert same(state, ref.hermite(pos, vel, dtype, dtype(1.0 / 256), 3, r)), n
            assert same(state[0][:, 3], pos[:, 3]) and same(state[1][:, 3], vel[:, 3])
            eng.upload(pos, vel)
            counters = eng.step_hermite_block(1.0 / 64, nblocks=1, eta=0.02, levels=3)
            state = eng.download()
            wp, wv, wsteps, wevals = ref.hermite_block(pos, vel, dtype, 0.02, 1.0 / 64, 3, 1, r)
            assert same(state, (wp, wv)) and counters == (wsteps, wevals), (n, counters, wsteps, wevals)
            assert same(state[0][:, 3], pos[:, 3])


MODES = (("fp32 timed", False, "ARITH_FMA3"), ("fp32 reference", False, "ARITH_REFERENCE"), ("fp32 strict", False, "ARITH_STRICT"),
         ("fp64 timed", True, "ARITH_FMA3"), ("fp64 strict", True, "ARITH_STRICT"))


@pytest.mark.parametrize("name,fp64,mode", MODES, ids=[m[0].replace(" ", "_") for m in MODES])
def test_unit_masses_are_the_option_switched_off(nb, name, fp64, mode):
    """property (a) on the device, N = 2100: with every w = 1 and the option on, every pass and a 3-step Hermite call have the bits of
    the same engine with the option off — m * x and fma(1, x, s) are exact, whatever 1/sqrt is"""
    n = 2100
    dtype = np.float64 if fp64 else np.float32
    pos, vel = system(nb, n, dtype, masses=1)
    pts, pvel, skip = queries(nb, pos)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
        out = []
        for on in (False, True):
            eng.use_masses(on)
            eng.upload(pos, vel)
            res = passes(eng, pts, pvel, skip)
            eng.step_hermite(1.0 / 256, 3)
            out.append(res + eng.download())
    assert not same(out[0][-2], pos)
    for k, (a, b) in enumerate(zip(*out)):
        assert same(a, b), (name, k)


@pytest.mark.parametrize("name,fp64,mode", MODES[::2], ids=[m[0].replace(" ", "_") for m in MODES[::2]])
def test_scaling_the_masses_by_a_power_of_two_scales_the_outputs(nb, name, fp64, mode):
    """property (b), N = 1025: masses x 8 and x 1/8 against x 1, exactly, for field, jerk and energy (U by the square)"""
    n = 1025
    dtype = np.float64 if fp64 else np.float32
    pos, vel = system(nb, n, dtype)
    pts, pvel, skip = queries(nb, pos)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
        eng.use_masses()
        res = {}
        for s in (1.0, 8.0, 0.125):
            eng.upload(with_masses(pos, pos[:, 3] * dtype(s)), vel)
            res[s] = (*eng.field(pts, skip), *eng.jerk_at(pts, pvel, skip), *eng.jerk(), totals_of(eng.energy()))
    for s in (8.0, 0.125):
        for g, b in zip(res[s][:-1], res[1.0][:-1]):
            assert same(g, b * dtype(s)), (name, s)
        assert same(res[s][-1], res[1.0][-1] * np.array([s, s * s, s, s, s, s, s, s])), (name, s)


@pytest.mark.parametrize("fp64", [False, True])
def test_appended_bodies_of_zero_mass_are_tracers(nb, fp64):
    """property (c), timed arithmetic: 1025 massive bodies plus 300 appended with w = 0.  Rows 0..1024 of jerk() and, after 2 Hermite
    steps, the first 1025 state words are the 1025-body engine's bit for bit; the tracers have moved"""
    n, extra = 1025, 300
    dtype = np.float64 if fp64 else np.float32
    pos, vel = system(nb, n, dtype)
    tp, tv = nb.make_bodies(extra, seed=31, dtype=dtype)
    pos2, vel2 = np.concatenate([pos, with_masses(tp, 0)]), np.concatenate([vel, tv])
    with nb.NBody(n, fp64=fp64) as eng:
        eng.use_masses()
        eng.upload(pos, vel)
        rows = eng.jerk()
        eng.step_hermite(1.0 / 256, 2)
        state = eng.download()
    with nb.NBody(n + extra, fp64=fp64) as eng:
        eng.use_masses()
        eng.upload(pos2, vel2)
        rows2 = eng.jerk()
        eng.step_hermite(1.0 / 256, 2)
        state2 = eng.download()
    assert same(tuple(r[:n] for r in rows2), rows)
    assert same(tuple(s[:n] for s in state2), state)
    assert np.all(np.abs(rows2[0][n:, :3]).sum(1) > 0)
    assert np.all((bits(state2[0][n:, :3]) != bits(pos2[n:, :3])).any(1)) and same(state2[0][:, 3], pos2[:, 3])


def test_timed_fp32_within_the_bound(nb):
    """n = 65536, m = 512 (jerk_common.TIMED_SHAPE), masses in [0.25, 4): |got - want64| / mag against numpy binary64 for the field and
    the jerk, both timed binary32 arithmetics.  Bound 2 r_ref + v_rsq_f32's share: r_ref = masses_common.R_REF = 4.7e-6 is what
    masses_ref.c's strict binary32 keeps against the same numpy values, asserted on the CPU at this shape (tests/test_masses_abi.py); the
    device's rounding path differs from the strict one by no more than that again, and v_rsq_f32's 1 ulp in inv enters inv3 three-fold
    and b two-fold, <= 5 * 2^-23 = 6e-7 of mag (the share tests/test_gpu_jerk.py uses); the weight is an exact factor of every term and of
    mag.  2 r_ref + 6e-7 = 1e-5."""
    n, m = TIMED_SHAPE
    bound = 2 * R_REF + RSQ_SHARE
    pos, vel = system(nb, n, np.float32)
    pts, pvel, skip = queries(nb, pos, m)
    wa, wphi, mag = numpy_field(pos, pts, skip)
    ja, jj, mag_a, mag_j = numpy_jerk(pos, vel, pts, pvel, skip)
    with nb.NBody(n) as eng:
        eng.use_masses()
        eng.upload(pos, vel)
        for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
            eng.set_option(nb.OPT_ARITH, mode)
            a, phi = eng.field(pts, skip)
            a2, j = eng.jerk_at(pts, pvel, skip)
            figs = (worst(a, wa, mag), float(np.max(np.abs(phi.astype(np.float64) - wphi) / np.abs(wphi))), worst(a2, ja, mag_a), worst(j, jj, mag_j))
            print("timed fp32 arith %d: field accel %.3e phi %.3e, jerk's accel %.3e jerk %.3e (bound %.3e)" % ((mode,) + figs + (bound,)))
            assert same(a, a2) and max(figs) <= bound, (mode, figs)


def test_momentum_is_conserved(nb, ref):
    """the test that catches m_i in place of m_j: N = 257, masses in [0.25, 4), 4 Hermite steps of 1/256 in strict binary64.
    |P1 - P0| / sum m |v| from energy()'s momenta is the reference's bit for bit, and below 4 x MOMENTUM_REF, the figure measured on
    the CPU reference (8.81e-16; a pair weighted by m_i loses 4.6 in the same run)"""
    n = 257
    pos, vel = system(nb, n, np.float64)
    scale = numpy_totals(pos, vel)[2]
    with nb.NBody(n, fp64=True) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.use_masses()
        eng.upload(pos, vel)
        p0 = eng.energy()["momentum"]
        eng.step_hermite(1.0 / 256, 4)
        p1 = eng.energy()["momentum"]
    w0 = ref.totals(pos, vel, np.float64)[2:5]
    w1 = ref.totals(*ref.hermite(pos, vel, np.float64, 1.0 / 256, 4), np.float64)[2:5]
    got, want = np.sqrt(((p1 - p0) ** 2).sum()) / scale, np.sqrt(((w1 - w0) ** 2).sum()) / scale
    print("|dP| / sum m |v|: device %.3e, reference %.3e" % (got, want))
    assert same(np.float64(got), np.float64(want)) and got <= 4 * MOMENTUM_REF


def test_kepler_pair_of_unequal_masses(nb, ref):
    """masses 3/4 and 1/4, e = 0.5, 128 steps to t = 1.  Strict binary64 is masses_ref bit for bit; |dE| / |E| of the timed binary32
    run (energies of the downloaded states in numpy binary64) is within twice masses_ref's strict binary32 figure plus v_rsq_f32's share"""
    steps = 128
    pos, vel = kepler(0.75, 0.25, 0.5)
    with nb.NBody(2, fp64=True) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.use_masses()
        eng.upload(pos, vel)
        eng.step_hermite(1.0 / steps, steps)
        assert same(eng.download(), ref.hermite(pos, vel, np.float64, 1.0 / steps, steps))
    p32, v32 = pos.astype(np.float32), vel.astype(np.float32)
    e0 = numpy_totals(p32, v32)[0]
    de_ref = abs(numpy_totals(*ref.hermite(p32, v32, np.float32, np.float32(1.0 / steps), steps))[0] - e0) / abs(e0)
    with nb.NBody(2) as eng:
        eng.use_masses()
        eng.upload(p32, v32)
        eng.step_hermite(1.0 / steps, steps)
        de = abs(numpy_totals(*eng.download())[0] - e0) / abs(e0)
    print("|dE|/|E|: timed fp32 %.3e, masses_ref fp32 %.3e" % (de, de_ref))
    assert de <= 2 * de_ref + RSQ_SHARE


def hermite_state(nb, n, pos, vel, ngpus=1):
    with nb.NBody(n, ngpus=ngpus) as eng:
        eng.use_masses()
        eng.upload(pos, vel)
        eng.step_hermite(1.0 / 256, 2)
        return eng.download(), eng.energy()


WORKER = """
    from masses_common import random_masses, with_masses
    pos, vel = nb.make_bodies(n)
    pos = with_masses(pos, random_masses(n))
    eng.use_masses()
    eng.upload(pos, vel)
    eng.step_hermite(1.0 / 256, 2)
    p, v = eng.download()
    e = eng.energy()
    np.savez({out!r} + "_%d.npz" % rank, pos=p, vel=v, e=np.concatenate([[e["kinetic"], e["potential"]], e["momentum"], e["angular_momentum"]]))
"""


def test_bits_do_not_depend_on_the_layout(nb, tmp_path, monkeypatch):
    """timed fp32, N = 3001, two Hermite steps with masses: three oversubscribed devices, the forced source split, a small scratch
    bound and two processes over the host transport all give one device's bits; energy() is equal on every rank"""
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    for name in ("NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"):
        monkeypatch.delenv(name, raising=False)
    n = 3001
    pos, vel = nb.make_bodies(n)
    pos = with_masses(pos, random_masses(n))
    base, e_base = hermite_state(nb, n, pos, vel)
    assert not same(base[0], pos) and same(base[0][:, 3], pos[:, 3])
    assert same(hermite_state(nb, n, pos, vel, ngpus=3)[0], base)
    monkeypatch.setenv("NBODY_JERK_SPLIT", "3")
    assert same(hermite_state(nb, n, pos, vel)[0], base)
    assert same(hermite_state(nb, n, pos, vel, ngpus=3)[0], base)
    monkeypatch.setenv("NBODY_JERK_SCRATCH_MB", "1")
    assert same(hermite_state(nb, n, pos, vel)[0], base)
    monkeypatch.delenv("NBODY_JERK_SPLIT")
    got, e_got = hermite_state(nb, n, pos, vel)
    assert same(got, base) and same(totals_of(e_got), totals_of(e_base))
    monkeypatch.delenv("NBODY_JERK_SCRATCH_MB")
    out = str(tmp_path / "ma")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), 2, 300, env_of=shared_gpu_env)
    ranks = [np.load(out + "_%d.npz" % r) for r in range(2)]
    for r in range(2):
        assert same((ranks[r]["pos"], ranks[r]["vel"]), base), r
    assert same(ranks[0]["e"], ranks[1]["e"])
    assert np.allclose(ranks[0]["e"], totals_of(e_base), rtol=1e-12, atol=1e-12)


def refused(fn, *args):
    return fn(*args) == 1006   # NBODY_ERR_UNSUPPORTED


@pytest.mark.parametrize("fp64", [False, True])
def test_unit_mass_entry_points_refuse(nb, fp64):
    """with the option on every unit-mass entry point answers ERR_UNSUPPORTED and leaves sentinel-filled outputs and the state on the
    device untouched; after use_masses(False) each works, and eng.step(dt, 4) gives a fresh context's bits — a graph captured before the
    switch included"""
    lib, E = nb._lib.load(), nb._lib
    n = 1500
    dtype, ct = (np.float64, C.c_double) if fp64 else (np.float32, C.c_float)
    suf = "_d" if fp64 else ""
    fn = lambda name: getattr(lib, name + suf)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(ct))
    iptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    pos, vel = system(nb, n, dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        eng.step(0.01, 9)    # one eager step, then a captured graph that the later call can replay
        eng.sync()
        mid = eng.download()
        eng.use_masses()
        steps_done = eng.info(E.INFO_STEPS_DONE)
        hp, hv = mid[0].copy(), mid[1].copy()
        out, e, idx = np.full((n, 4), 7, dtype), np.full(n, 7, dtype), np.full(n, 7, np.int32)
        t, taken, found = C.c_double(7.0), C.c_int(7), C.c_int(7)
        el = np.full((n, 4), 7.0)
        calls = [lambda: fn("bodyForce")(ptr(hp), ptr(hv), 0.01, n),
                 lambda: fn("nbody_step")(0.01, 4),
                 lambda: fn("nbody_forces")(ptr(hp), ptr(out), n),
                 lambda: fn("nbody_forces_rows")(0, n, ptr(out)),
                 lambda: fn("nbody_step_adaptive")(0.04, 0.01, 1e-6, 1.0, 10, C.byref(t), C.byref(taken)),
                 lambda: fn("nbody_pair_energy_rows")(0, n, ptr(e), iptr(idx)),
                 lambda: lib.nbody_binaries(0.0, n, C.byref(found), iptr(idx), iptr(idx), el.ctypes.data_as(C.POINTER(C.c_double)))]
        assert [c() for c in calls] == [E.ERR_UNSUPPORTED] * len(calls)
        assert np.all(out == 7) and np.all(e == 7) and np.all(idx == 7) and np.all(el == 7.0) and (t.value, taken.value, found.value) == (7.0, 7, 7)
        assert same((hp, hv), mid) and same(eng.download(), mid) and eng.info(E.INFO_STEPS_DONE) == steps_done
        with pytest.raises(nb.NBodyError) as err:
            eng.step(0.01, 4)
        assert err.value.code == E.ERR_UNSUPPORTED
        eng.use_masses(False)
        eng.step(0.01, 4)
        eng.sync()
        after = eng.download()
        assert [c() for c in calls[2:]] == [0] * len(calls[2:]) and calls[0]() == 0
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(*mid)
        eng.step(0.01, 4)
        eng.sync()
        assert same(eng.download(), after)


def test_the_mailbox_refuses(nb):
    lib, E = nb._lib.load(), nb._lib
    pos = nb.make_bodies(300)[0]
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        want = mb.forces(pos)
        assert lib.nbody_set_option(E.OPT_MASSES, 1) == 0
        mb.post(pos)
        mb.ram_b[...] = 0
        before = (mb.ram_a.copy(), mb.ram_b.copy())
        for call in (mb.run, lambda: mb.serve(True, clock_khz=300000)):
            with pytest.raises(nb.NBodyError) as err:
                call()
            assert err.value.code == E.ERR_UNSUPPORTED
        info = C.c_longlong(7)
        assert lib.nbody_get_info(E.INFO_MAILBOX_SERVING, C.byref(info)) == 0 and info.value == 0
        assert np.array_equal(mb.ram_a, before[0]) and np.array_equal(mb.ram_b, before[1])
        assert lib.nbody_set_option(E.OPT_MASSES, 0) == 0
        assert same(mb.forces(pos), want)
        mb.serve(True, clock_khz=300000)
        mb.serve(False)


def test_c_host_program_masses(nb):
    """`nbody 1000 3 --hermite --masses` prints the weighted energy before and after — the engine's own figures for the masses 2^-(i mod 4)
    —, with --hermite-block too; --masses alone is a usage error"""
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters = 1000, 3
    energies = {}
    for extra in ((), ("--hermite-block", "3")):
        r = subprocess.run([exe, str(n), str(iters), "--hermite", "--masses"] + list(extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        lines = re.findall(r"^energy at step (\d+): E (\S+) T (\S+) U (\S+)", r.stdout, flags=re.M)
        assert [l[0] for l in lines] == ["0", str(iters)], r.stdout
        assert all(np.isfinite(float(v)) for l in lines for v in l[1:])
        energies[extra] = [float(l[1]) for l in lines]
    pos, vel = nb.make_bodies(n)
    pos[:, 3] = 2.0 ** -(np.arange(n) % 4)
    with nb.NBody(n) as eng:
        eng.use_masses()
        eng.upload(pos, vel)
        e0 = eng.energy()["total"]
        eng.step_hermite(0.01, iters)
        e1 = eng.energy()["total"]
    assert energies[()] == [e0, e1], (energies, e0, e1)
    r = subprocess.run([exe, str(n), str(iters), "--masses"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--masses" in r.stderr


# ---- the hostile system with hostile masses (specials_common.py) ----

@pytest.fixture(scope="module")
def dynamic_refs(tmp_path_factory):
    """(tests/snap_ref.c, tests/hermite6_ref.c, tests/hermite6_block_ref.c): the statements of the weighted passes masses_ref.c leaves out"""
    from field_common import compile_ref
    d = tmp_path_factory.mktemp("masses_dynamic_ref")
    return SnapRef(compile_ref(d, "snap_ref")), Hermite6Ref(compile_hermite6(d)), Block6Ref(compile_block6(d))


def hostile_bodies(nb, n, dtype, variant, mass_variant=None):
    """hostile_dynamic_system with hostile_masses in the w of the positions and canaries in the w of the velocities"""
    pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
    pos = with_masses(pos, hostile_masses(n, dtype, variant if mass_variant is None else mass_variant))
    vel[:, 3] = (np.arange(n) % 31).astype(dtype) + dtype(0.25)
    return pos, vel


def hostile_queries(nb, pos, vel, variant, m=300):
    pts, skip = hostile_points(nb, pos, m, variant)
    pts[:, 3] = 99.0
    pvel, pacc = hostile_point_words(nb, m, pos.dtype.type, vel)
    return pts, pvel, pacc, skip


HOSTILE_RUN = dict(eta=0.04, dt_max=1.0 / 256, levels=8, nblocks=1)


@pytest.mark.parametrize("arith", list(ARITHS))
def test_hostile_masses_strict_bit_for_bit(nb, ref, dynamic_refs, arith):
    """hostile_dynamic_system with hostile_masses in every variant and size, 300 hostile queries: the field with and without skip, the
    tidal tensor, the jerk at points and at rows, potential_rows and energy() against tests/masses_ref.c, the snap at rows against
    tests/snap_ref.c, one fourth-order and one sixth-order step of 1/256 and one block of each order (eta 0.04, dt_max 1/256, 8 levels)
    with its counters against masses_ref.c, hermite6_ref.c and hermite6_block_ref.c — NaN for NaN, bit for bit elsewhere — and after
    every integrator call the downloaded w is the uploaded w bit for bit: -0, the subnormal and the NaN's payload included."""
    fp64, mode, r = ARITHS[arith]
    dtype = np.float64 if fp64 else np.float32
    snap_ref, h6_ref, b6_ref = dynamic_refs
    flags = H6_MASS | (H6_REF if r else 0)
    dt, run = 1.0 / 256, HOSTILE_RUN
    differ = []
    for n in HOSTILE_SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            eng.use_masses()
            for variant in VARIANTS:
                pos, vel = hostile_bodies(nb, n, dtype, variant)
                pts, pvel, pacc, skip = hostile_queries(nb, pos, vel, variant)
                eng.upload(pos, vel)
                got = passes(eng, pts, pvel, skip) + eng.snap()
                with np.errstate(all="ignore"):
                    want = (*ref.field(pos, pts, dtype, None, r), *ref.field(pos, pts, dtype, skip, r), ref.tidal(pos, pts, dtype, skip, r),
                            *ref.jerk(pos, vel, pts, pvel, dtype, skip, r), *ref.jerk_rows(pos, vel, dtype, r), ref.potential(pos, dtype, r),
                            ref.totals(pos, vel, dtype, ref=r), *snap_ref.rows(pos, vel, dtype, ref=r, mass=True))
                    steps = {"hermite": ref.hermite(pos, vel, dtype, dtype(dt), 1, r) + (None,),
                             "hermite6": h6_ref.step(pos, vel, dtype, dt, 1, flags) + (None,),
                             "hermite_block": (lambda o: (o[0], o[1], (o[2], o[3])))(ref.hermite_block(pos, vel, dtype, run["eta"], run["dt_max"], run["levels"], 1, r)),
                             "hermite6_block": (lambda o: (o[0], o[1], (o[2], o[3])))(b6_ref.run(pos, vel, dtype, ref=r, mass=True, trace=False, **run))}
                assert len(got) == len(want)
                for k, (g, w) in enumerate(zip(got, want)):
                    if not same_nan(np.asarray(g), np.asarray(w)):
                        differ.append((n, variant, "pass %d" % k))
                calls = {"hermite": lambda: eng.step_hermite(dt, 1), "hermite6": lambda: eng.step_hermite6(dt, 1),
                         "hermite_block": lambda: eng.step_hermite_block(run["dt_max"], 1, eta=run["eta"], levels=run["levels"]),
                         "hermite6_block": lambda: eng.step_hermite6_block(run["dt_max"], 1, eta=run["eta"], levels=run["levels"])}
                for name, call in calls.items():
                    eng.upload(pos, vel)
                    counters = call()
                    state = eng.download()
                    wp, wv, wcounters = steps[name]
                    if not (same_nan(state[0], wp) and same_nan(state[1], wv)):
                        differ.append((n, variant, name))
                    if wcounters is not None and tuple(counters) != wcounters:
                        differ.append((n, variant, name, tuple(counters), wcounters))
                    if not (same(state[0][:, 3], pos[:, 3]) and same(state[1][:, 3], vel[:, 3])):
                        differ.append((n, variant, name, "the w of a word was not carried"))
                    if variant in ("base", "overflow") and not (np.all(np.isfinite(state[0][:, :3])) and np.all(np.isfinite(state[1][:, :3]))):
                        differ.append((n, variant, name, "a row is not finite"))
    assert not differ, differ


DOMAIN_MODES = {False: ("ARITH_FMA3", "ARITH_REFERENCE", "ARITH_STRICT", "ARITH_REFERENCE_STRICT"), True: ("ARITH_FMA3", "ARITH_STRICT")}


def domain_passes(eng, pts, pvel, pacc, skip):
    """(query passes, rows passes) of the weighted state on the device"""
    return ((*eng.field(pts, skip), eng.tidal(pts, skip), *eng.jerk_at(pts, pvel, skip), *eng.snap_at(pts, pvel, pacc, skip)),
            (*eng.jerk(), *eng.snap(), eng.potential_rows(0, eng.n)))


@pytest.mark.parametrize("fp64", [False, True])
def test_domain_sentences_of_the_masses(nb, fp64):
    """What include/nbody.h says of the w of a position word (NBODY_OPT_MASSES, DOMAIN), directly, in every arithmetic, the timed ones
    included, on the finite "base" bodies of hostile_dynamic_system so that nothing but the mass is special:
      a NaN mass poisons the acceleration, the potential and the jerk of every query that does not skip the body, and no bit of a query
      that does: those get what they get with 1.5 in its place — in the field, the tidal tensor, the jerk and the snap pass's
      acceleration and jerk; the snap itself is NaN on every query, through the a_j of the sources beside the body;
      an infinite mass leaves no finite contribution: every component of the acceleration and the potential of a query that does not
      skip it is +-inf or NaN, and a query that skips it has the bits of the ordinary system;
      moving bodies of mass +0 from one finite position to another — exactly onto a query, for the bodies on the window edge (63, 64)
      and on the block edge (1023, 1024) as for one inside (12) — changes no bit of any query nor of any other row, in the field, the
      tidal tensor, the jerk, the snap and potential_rows."""
    dtype = np.float64 if fp64 else np.float32
    differ = []
    for n in HOSTILE_SIZES:
        pos, vel = hostile_bodies(nb, n, dtype, "base")
        row = nan_row(n)
        pts, pvel, pacc, skip = hostile_queries(nb, pos, vel, "nan")     # its plan skips nan_row(n) on near cloud points
        skip[200:210] = INF_MASS_ROW
        ordinary = pos.copy()
        ordinary[row, 3] = 1.5
        special = {"nan": with_masses(ordinary, hostile_masses(n, dtype, "nan")), "inf": with_masses(ordinary, hostile_masses(n, dtype, "inf"))}
        special["inf"][row, 3] = 1.5
        movers = [b for b in (12, 63, 64, 1023, 1024) if b < n]
        still, moved = ordinary.copy(), ordinary.copy()
        still[movers, 3] = 0.0
        moved[movers, 3] = 0.0
        moved[movers, :3] = pts[[250 + 4 * k for k in range(len(movers))], :3]     # near cloud queries (192 ..), some with a skip
        others = np.setdiff1d(np.arange(n), movers)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.use_masses()
            for mode in DOMAIN_MODES[fp64]:
                eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
                eng.upload(ordinary, vel)
                base_q, base_r = domain_passes(eng, pts, pvel, pacc, skip)
                ok = near(pts)
                assert all(np.all(np.isfinite(o[ok])) for o in base_q), (n, mode)
                for kind, bad_row in (("nan", row), ("inf", INF_MASS_ROW)):
                    eng.upload(special[kind], vel)
                    q, rws = domain_passes(eng, pts, pvel, pacc, skip)
                    sel = skip == bad_row
                    assert sel.sum() >= 2
                    a, phi, tid, ja, jj, sa, sj, ss = q
                    seen = [k for k, (g, b) in enumerate(zip(q[:7], base_q[:7])) if not same(g[sel], b[sel])]
                    if seen:
                        differ.append((n, mode, kind, "a query that skips the body sees it in query passes", seen))
                    # (the snap itself is out of a skip's reach: the body's mass is in the a_j of every source beside it, include/nbody.h "snap")
                    if np.any(np.isfinite(ss[:, :3])):
                        differ.append((n, mode, kind, "a finite snap beside non-finite accelerations of the sources"))
                    if kind == "nan":
                        if not all(np.all(np.isnan(o[~sel][:, :3])) for o in (a, ja, jj, sa, sj, ss)) or not np.all(np.isnan(phi[~sel])) or not np.all(np.isnan(tid[~sel])):
                            differ.append((n, mode, kind, "a query that does not skip the body escaped"))
                        hit = np.arange(n) != bad_row
                        if not all(np.all(np.isnan(o[hit][:, :3])) for o in rws[:2]) or not np.all(np.isnan(rws[5][hit])) or not np.all(np.isnan(rws[4][:, :3])):
                            differ.append((n, mode, kind, "a row escaped"))
                        if not (np.all(np.isfinite(rws[0][bad_row])) and np.isfinite(rws[5][bad_row])):
                            differ.append((n, mode, kind, "the body's own row has no mass of its own to meet"))
                    else:
                        if np.any(np.isfinite(a[~sel][:, :3])) or np.any(np.isfinite(ja[~sel][:, :3])) or np.any(np.isfinite(sa[~sel][:, :3])) or np.any(np.isfinite(phi[~sel])):
                            differ.append((n, mode, kind, "a finite contribution of an infinite mass"))
                        hit = np.arange(n) != bad_row
                        if np.any(np.isfinite(rws[0][hit][:, :3])) or np.any(np.isfinite(rws[5][hit])):
                            differ.append((n, mode, kind, "a row with a finite contribution of an infinite mass"))
                eng.upload(still, vel)
                still_q, still_r = domain_passes(eng, pts, pvel, pacc, skip)
                eng.upload(moved, vel)
                moved_q, moved_r = domain_passes(eng, pts, pvel, pacc, skip)
                for k, (g, b) in enumerate(zip(moved_q, still_q)):
                    if not same(g, b):
                        differ.append((n, mode, "moved massless bodies", "query pass %d" % k, np.flatnonzero((bits(g) != bits(b)).reshape(len(g), -1).any(1))[:8]))
                for k, (g, b) in enumerate(zip(moved_r, still_r)):
                    if not same(g[others], b[others]):
                        differ.append((n, mode, "moved massless bodies", "rows pass %d" % k, others[np.flatnonzero((bits(g[others]) != bits(b[others])).reshape(len(others), -1).any(1))[:8]]))
                    if k < 5 and same(g[movers], b[movers]):     # (their potential is the far body's 2^100 / 1e15: the cloud is below its last place)
                        differ.append((n, mode, "the massless bodies themselves did not notice their move", k))
            eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
    assert not differ, "\n".join(str(d) for d in differ)


def test_hostile_masses_timed_fp32_within_the_bound(nb):
    """hostile_dynamic_system with hostile_masses, "base" and "overflow", every size, 300 hostile queries with and without skip, both
    timed binary32 arithmetics: |got - want64| / mag of the field and the jerk against numpy binary64 on the near queries whose binary64
    magnitude sums are finite, within 2 r + v_rsq_f32's share (test_timed_fp32_within_the_bound's rule) with r =
    masses_common.R_REF_HOSTILE, what masses_ref.c's strict binary32 keeps on this input (tests/test_specials_dynamic_reference.py).
    r is the far body's figure: see masses_common.  The measured figures are printed."""
    bound = 2 * R_REF_HOSTILE + RSQ_SHARE
    worst_of = {}
    for n in HOSTILE_SIZES:
        with nb.NBody(n) as eng:
            eng.use_masses()
            for variant in ("base", "overflow"):
                pos, vel = hostile_bodies(nb, n, np.float32, variant)
                pts, pvel, pacc, hsk = hostile_queries(nb, pos, vel, variant)
                eng.upload(pos, vel)
                for skip in (None, hsk):
                    wa, wphi, mag = numpy_field(pos, pts, skip)
                    ja, jj, mag_a, mag_j = numpy_jerk(pos, vel, pts, pvel, skip)
                    keep = near(pts) & np.all([np.isfinite(o).all(1) for o in (mag, mag_a, mag_j)], axis=0)
                    assert keep.sum() >= 290, (n, variant)
                    for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                        eng.set_option(nb.OPT_ARITH, mode)
                        a, phi = eng.field(pts, skip)
                        a2, j = eng.jerk_at(pts, pvel, skip)
                        assert same(a, a2), (n, variant, mode)
                        figs = [worst(a[keep], wa[keep], mag[keep]), worst(a2[keep], ja[keep], mag_a[keep]), worst(j[keep], jj[keep], mag_j[keep])]
                        worst_of[(n, mode)] = [max(x, y) for x, y in zip(worst_of.get((n, mode), [0.0] * 3), figs)]
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
    for (n, mode), e in sorted(worst_of.items()):
        print("hostile masses timed fp32 n=%d arith %d: field accel %.3e, jerk's accel %.3e jerk %.3e (bound %.3e)" % (n, mode, *e, bound))
    assert all(max(e) <= bound for e in worst_of.values()), worst_of
