"""Energy, momentum and per-body potential of the state on the device (nbody_energy, nbody_potential_rows(_d); include/nbody.h
"energy and potential"): phi_i bit for bit against tests/potential_ref.c in the strict modes, within the north_star tolerance in the
timed arithmetic, the same bits however the context is configured or sharded, totals against an fp64 evaluation of the downloaded
state and bit for bit against the header's summation order, all of it on the hostile system of specials_common.py too, no effect on the step, the physics of a circular orbit, the mailbox guard and the C host program's --energy lines."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pass_common
from field_common import numpy_field
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import SIZES, VARIANTS, hostile_system, near, same_nan, within

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.array([0x3089705F], np.uint32).view(np.float32)[0])


class Ref:
    """tests/potential_ref.c: phi in the documented order, IEEE 1/sqrt"""

    def __init__(self, lib):
        self.lib = lib

    def phi32(self, pos, r0=0, nr=None, ref=False):
        pos = np.ascontiguousarray(pos, np.float32)
        nr = len(pos) - r0 if nr is None else nr
        out = np.empty(nr, np.float32)
        self.lib.potential_f32(pos.ctypes.data_as(C.c_void_p), len(pos), r0, nr, int(ref), out.ctypes.data_as(C.c_void_p))
        return out

    def phi64(self, pos, r0=0, nr=None):
        pos = np.ascontiguousarray(pos, np.float64)
        nr = len(pos) - r0 if nr is None else nr
        out = np.empty(nr, np.float64)
        self.lib.potential_f64(pos.ctypes.data_as(C.c_void_p), len(pos), r0, nr, out.ctypes.data_as(C.c_void_p))
        return out

    def totals(self, pos, vel, slices, ref=False):
        """{T, U, Px, Py, Pz, Lx, Ly, Lz} in the header's order; slices: the ranks' (first, count)"""
        sl = np.ascontiguousarray(slices, np.int32).reshape(-1, 2)
        out = np.empty(8, np.float64)
        if pos.dtype == np.float32:
            pos, vel = np.ascontiguousarray(pos, np.float32), np.ascontiguousarray(vel, np.float32)
            rc = self.lib.energy_totals_f32(pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p), len(pos),
                                            sl.ctypes.data_as(C.c_void_p), len(sl), int(ref), out.ctypes.data_as(C.c_void_p))
        else:
            pos, vel = np.ascontiguousarray(pos, np.float64), np.ascontiguousarray(vel, np.float64)
            rc = self.lib.energy_totals_f64(pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p), len(pos),
                                            sl.ctypes.data_as(C.c_void_p), len(sl), out.ctypes.data_as(C.c_void_p))
        assert rc == 0
        return out


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("potential_ref") / "potential_ref.so")
    src = os.path.join(ROOT, "tests", "potential_ref.c")
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], []):   # every operation is IEEE-exact: vector width and threads change no bit
        r = subprocess.run(["gcc", "-std=c11", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"] + extra + ["-o", so, src, "-lm"],
                           capture_output=True, timeout=180)
        if r.returncode == 0:
            return Ref(C.CDLL(so))
    pytest.fail("cannot compile tests/potential_ref.c: " + r.stderr.decode()[-2000:])


def fp64_totals(ref, pos, vel):
    """T, U, P, L of a downloaded state in fp64, and the scales |P| and |L| are relative to (sums of magnitudes)"""
    p, v = pos[:, :3].astype(np.float64), vel[:, :3].astype(np.float64)
    lv = np.cross(p, v)
    u = 0.5 * ref.phi64(pos.astype(np.float64)).sum()
    return dict(kinetic=0.5 * (v ** 2).sum(), potential=u, momentum=v.sum(0), angular_momentum=lv.sum(0),
                p_scale=np.linalg.norm(v, axis=1).sum(), l_scale=np.linalg.norm(lv, axis=1).sum())


def bits(e):
    """the eight totals of an energy() result as binary64 words"""
    return pass_common.bits(np.array([e["kinetic"], e["potential"], *e["momentum"], *e["angular_momentum"]]))


@pytest.mark.parametrize("arith", ["strict", "reference_strict"])
def test_strict_fp32_rows_bit_for_bit(nb, ref, arith):
    mode = {"strict": nb.ARITH_STRICT, "reference_strict": nb.ARITH_REFERENCE_STRICT}[arith]
    for n in (1, 2, 63, 64, 65, 1000, 1025, 4099, 20000):
        pos, vel = nb.make_bodies(n)
        with nb.NBody(n) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            eng.upload(pos, vel)
            got = eng.potential_rows(0, n)
            want = ref.phi32(pos, ref=(mode == nb.ARITH_REFERENCE_STRICT))
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, int((got != want).sum()))
            if n == 1:
                e = eng.energy()
                assert got.view(np.uint32)[0] == 0 and e["potential"] == 0.0 and np.float64(e["potential"]).view(np.uint64) == 0


def test_fp64_rows(nb, ref):
    for n in (2, 1025, 4099):
        pos, vel = nb.make_bodies(n, dtype=np.float64)
        want = ref.phi64(pos)
        with nb.NBody(n, fp64=True) as eng:
            eng.upload(pos, vel)
            fast = eng.potential_rows(0, n)
            assert np.max(np.abs(fast - want) / np.abs(want)) < 1e-12, n
            eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
            strict = eng.potential_rows(0, n)
            assert np.array_equal(strict.view(np.uint64), want.view(np.uint64)), (n, int((strict != want).sum()))


def test_fast_fp32_rows_within_north_star_tolerance(nb, ref):
    n = 65536
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        got = eng.potential_rows(0, n)
    want = ref.phi64(pos.astype(np.float64))
    assert np.max(np.abs(got - want) / np.abs(want)) < 1e-5
    n = 1 << 20
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        p64 = pos.astype(np.float64)
        for r0, cnt in ((0, 256), (n - 256, 256), (512 * 1024 - 100, 200)):    # first, last, across the block edge at 2^19
            got = eng.potential_rows(r0, cnt)
            want = ref.phi64(p64, r0, cnt)
            assert np.max(np.abs(got - want) / np.abs(want)) < 1e-5, r0


@pytest.mark.parametrize("fp64", [False, True])
def test_totals_against_fp64(nb, ref, fp64):
    n = 3000
    dtype = np.float64 if fp64 else np.float32
    pos, vel = nb.make_bodies(n, dtype=dtype)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        done = 0
        for steps in (0, 10, 100):
            eng.step(0.01, steps - done)
            done = steps
            e = eng.energy()
            assert np.array_equal(bits(e), bits(eng.energy())), "two calls differ"
            p, v = eng.download()
            w = fp64_totals(ref, p, v)
            assert abs(e["kinetic"] - w["kinetic"]) <= 1e-12 * w["kinetic"], steps
            assert abs(e["potential"] - w["potential"]) <= (1e-12 if fp64 else 1e-6) * abs(w["potential"]), steps
            assert e["total"] == e["kinetic"] + e["potential"]
            assert np.all(np.abs(e["momentum"] - w["momentum"]) <= 1e-12 * w["p_scale"]), steps
            assert np.all(np.abs(e["angular_momentum"] - w["angular_momentum"]) <= 1e-12 * w["l_scale"]), steps


def test_phi_bits_do_not_depend_on_the_force_configuration(nb):
    n = 5000
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        base, ebase = eng.potential_rows(0, n), bits(eng.energy())
        for key, val, default in pass_common.FORCE_CONFIGS:
            eng.set_option(key, val)
            got = eng.potential_rows(0, n)
            assert np.array_equal(got.view(np.uint32), base.view(np.uint32)), (key, val)
            assert np.array_equal(bits(eng.energy()), ebase), (key, val)
            eng.set_option(key, default)


def test_phi_bits_do_not_depend_on_the_device_count(nb, monkeypatch):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n = 3001
    pos, vel = nb.make_bodies(n)
    res = {}
    for ngpus in (1, 3, 8):
        with nb.NBody(n, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            # after a drift on the device each local holds only its own slice's new positions: the pass brings the rest first.  (A
            # drift, not a step: r += v dt is per body, a step's force sums follow the slicing.)
            eng.integrate(pos.copy(), vel.copy(), 0.01)
            res[ngpus] = (eng.potential_rows(0, n), eng.potential_rows(900, 300), eng.energy())
    phi1, win1, e1 = res[1]
    assert np.array_equal(win1.view(np.uint32), phi1[900:1200].view(np.uint32))
    for ngpus in (3, 8):
        phi, win, e = res[ngpus]
        assert np.array_equal(phi.view(np.uint32), phi1.view(np.uint32)), ngpus
        assert np.array_equal(win.view(np.uint32), phi1[900:1200].view(np.uint32)), ngpus
        for k in ("kinetic", "potential"):
            assert abs(e[k] - e1[k]) <= 1e-12 * abs(e1[k]), (ngpus, k)
        for k in ("momentum", "angular_momentum"):
            assert np.all(np.abs(e[k] - e1[k]) <= 1e-12 * np.abs(e1[k]).sum()), (ngpus, k)


WORKER = """
    eng.set_option(nb.OPT_JSUB, 2)
    pos, vel = nb.make_bodies(n, seed=33)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    e = eng.energy()
    phi = eng.potential_rows(0, eng.config["n_local"])
    p, v = eng.download()
    w = np.array([e["kinetic"], e["potential"], *e["momentum"], *e["angular_momentum"]])
    np.save({out!r} + "_%d_energy.npy" % rank, w)
    np.save({out!r} + "_%d_phi.npy" % rank, phi)
    if rank == 0:
        np.save({out!r} + "_pos.npy", p)
        open({out!r} + "_wsplit.txt", "w").write(str(eng.config["wsplit"]))
"""


def test_two_processes_host_transport_equal_one_process(nb, tmp_path, monkeypatch):
    n, world = 6007, 2
    out = str(tmp_path / "en")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    pos, vel = nb.make_bodies(n, seed=33)
    with nb.NBody(n, ngpus=world) as one:
        one.set_option(nb.OPT_JSUB, 2)
        one.set_option(nb.OPT_WSPLIT, int(open(out + "_wsplit.txt").read()))
        one.upload(pos, vel)
        one.step(0.01, 3)
        e = one.energy()
        phi = one.potential_rows(0, n)
        wp, _ = one.download()
    assert np.array_equal(np.load(out + "_pos.npy").view(np.uint32), wp.view(np.uint32)), "the two runs' states differ"
    want = np.array([e["kinetic"], e["potential"], *e["momentum"], *e["angular_momentum"]])
    for r in range(world):
        assert np.array_equal(np.load(out + "_%d_energy.npy" % r).view(np.uint64), want.view(np.uint64)), r
    got_phi = np.concatenate([np.load(out + "_%d_phi.npy" % r) for r in range(world)])
    assert np.array_equal(got_phi.view(np.uint32), phi.view(np.uint32))


def test_energy_calls_leave_the_step_untouched(nb):
    n = 1500
    pos, vel = nb.make_bodies(n)
    probe = lambda eng: (eng.energy(), eng.potential_rows(0, n), eng.potential_rows(n // 3, 7))
    for plan, graph, timing in (([1] * 12, 0, False), ([64, 64, 6, 64], 1, False), ([3, 5, 2], 0, True)):
        a = pass_common.run_steps(nb, n, pos, vel, plan, graph, None, timing)
        b = pass_common.run_steps(nb, n, pos, vel, plan, graph, probe, timing)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (plan, graph)
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (plan, graph)
        assert a[2] == b[2], "energy launches were counted by nbody_kernel_time"


def test_circular_two_body_orbit(nb):
    """Separation 1, unit masses: the force is (1 + eps)^(-3/2), v^2 / (1/2) = F, E_0 = v^2 - (1 + eps)^(-1/2); symplectic Euler
    keeps the energy error bounded (no secular drift) and the momentum at zero."""
    f = (1.0 + EPS) ** -1.5
    v = np.sqrt(0.5 * f)
    period = 2 * np.pi * 0.5 / v
    dt, steps = period / 1000, 2000
    pos = np.array([[-0.5, 0, 0, 0], [0.5, 0, 0, 0]], np.float64)
    vel = np.array([[0, -v, 0, 0], [0, v, 0, 0]], np.float64)
    e0_analytic = v * v - (1.0 + EPS) ** -0.5
    with nb.NBody(2, fp64=True) as eng:
        eng.upload(pos, vel)
        e = eng.energy()
        assert abs(e["total"] - e0_analytic) <= 1e-12 * abs(e0_analytic)
        de, pmax = [], 0.0
        for _ in range(steps):
            eng.step(dt, 1)
            e = eng.energy()
            de.append(abs(e["total"] - e0_analytic))
            pmax = max(pmax, float(np.abs(e["momentum"]).max()))
    first, second = max(de[:steps // 2]), max(de[steps // 2:])
    assert 0 < first and second <= 1.5 * first, (first, second)
    assert pmax <= 1e-12


def test_entry_points_refused_while_the_mailbox_is_served(nb):
    lib = nb._lib.load()
    out = np.zeros(8, np.float64)
    phi32, phi64 = np.zeros(4, np.float32), np.zeros(4, np.float64)
    calls = (lambda: lib.nbody_energy(out.ctypes.data_as(C.POINTER(C.c_double))),
             lambda: lib.nbody_potential_rows(0, 4, phi32.ctypes.data_as(C.POINTER(C.c_float))),
             lambda: lib.nbody_potential_rows_d(0, 4, phi64.ctypes.data_as(C.POINTER(C.c_double))))
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [c() for c in calls] == [nb._lib.ERR_STATE] * 3
        finally:
            mb.serve(False)
        assert [c() for c in calls] == [0, 0, nb._lib.ERR_STATE]       # served no more: an fp32 context again


def test_c_host_program_energy_lines(nb):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters = 4096, 3
    r = subprocess.run([exe, str(n), str(iters), "--energy"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = re.findall(r"energy at step (\d+): E (\S+) T (\S+) U (\S+)", r.stdout)
    assert [int(l[0]) for l in lines] == [0, iters], r.stdout
    assert re.search(r"energy at step %d: .* relative drift \S+" % iters, r.stdout)
    plain = subprocess.run([exe, str(n), str(iters)], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and "energy" not in plain.stdout
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        want = [eng.energy()]
        eng.step(0.01, iters)
        want.append(eng.energy())
    for line, w in zip(lines, want):
        e, t, u = (float(x) for x in line[1:])
        for got, ref_ in ((e, w["total"]), (t, w["kinetic"]), (u, w["potential"])):
            assert abs(got - ref_) <= 1e-6 * abs(ref_), (line, w)


# ---- the hostile system (specials_common.py): what a uniform cloud never shows the pass ----

def planted_ranges(n):
    """the whole system and sub-ranges that start and end on the planted rows"""
    r = [(0, n), (10, 2), (11, 12), (22, 2), (40, 2), (41, 23), (63, 2), (64, 1), (n - 1, 1), (n - 7, 7)]
    if n > 1028:
        r += [(1023, 1), (1023, 2), (1024, 5), (1020, 9), (1024, n - 1024), (1028, n - 1028)]
    return r


def strict_phi(ref, pos, r0, nr, reference=False):
    return ref.phi64(pos, r0, nr) if pos.dtype == np.float64 else ref.phi32(pos, r0, nr, ref=reference)


@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_hostile_system_rows_strict_bit_for_bit(nb, ref, arith):
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    for n in SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                want = strict_phi(ref, pos, 0, n, mode == nb.ARITH_REFERENCE_STRICT)
                if variant == "nan":
                    assert np.all(np.isnan(want))
                else:
                    assert np.all(np.isfinite(want))       # an overflowing square and an infinity are +0 in a sum of 1/sqrt
                for r0, nr in planted_ranges(n):
                    got = eng.potential_rows(r0, nr)
                    assert same_nan(got, want[r0:r0 + nr]), (n, variant, r0, nr, r0 + np.flatnonzero(got != want[r0:r0 + nr])[:8])


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system_rows_timed_arithmetic(nb, ref, fp64):
    """The timed arithmetic on the hostile system: (a) phi_i and the eight totals finite exactly where the strict references are, in
    every variant; (c) on the near rows (every |coordinate| <= 2, not a far-away body) |phi - phi64| <= TOL |phi64| against the plain
    numpy binary64 evaluation, TOL = 1e-5 (binary32, the north_star tolerance) or 1e-12 (binary64, test_fp64_rows' bar).  The strict
    references sit at <= 1.6e-6 and <= 2.8e-15 in that measure (tests/test_specials_reference.py, which requires 3e-6 and 1e-13).
    Measured on an MI355X, worst over sizes and variants: binary32 1.5e-6, binary64 2.8e-15."""
    dtype = np.float64 if fp64 else np.float32
    tol = 1e-12 if fp64 else 1e-5
    for n in SIZES:
        rows_skip = np.arange(n, dtype=np.int32)
        with nb.NBody(n, fp64=fp64) as eng:
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                keep = near(pos, far)
                p64 = numpy_field(pos, pos, rows_skip)[1]
                for mode in (nb.ARITH_FMA3,) if fp64 else (nb.ARITH_FMA3, nb.ARITH_REFERENCE):
                    eng.set_option(nb.OPT_ARITH, mode)
                    want = strict_phi(ref, pos, 0, n, mode == nb.ARITH_REFERENCE)
                    got = eng.potential_rows(0, n)
                    assert np.array_equal(np.isfinite(got), np.isfinite(want)), (n, variant, mode, np.flatnonzero(np.isfinite(got) != np.isfinite(want))[:8])
                    with np.errstate(all="ignore"):
                        print("timed %s n=%d %s arith %d: phi %.3e on %d near rows" % (np.dtype(dtype).name, n, variant, mode,
                              np.nanmax(np.abs(got[keep] - p64[keep]) / np.abs(p64[keep]), initial=0.0), keep.sum()))
                    assert within(got[keep], p64[keep], tol * np.abs(p64[keep])), (n, variant, mode)
                    for r0, nr in planted_ranges(n):
                        assert same_nan(eng.potential_rows(r0, nr), got[r0:r0 + nr]), (n, variant, mode, r0, nr)
                    e = bits(eng.energy()).view(np.float64)
                    w = ref.totals(pos, vel, [(0, n)], ref=(mode == nb.ARITH_REFERENCE))
                    assert np.array_equal(np.isfinite(e), np.isfinite(w)), (n, variant, mode, e, w)
                eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)


@pytest.mark.parametrize("ngpus", [1, 3])
@pytest.mark.parametrize("arith", ["strict", "reference_strict", "fp64_strict"])
def test_totals_bit_for_bit_in_the_documented_order(nb, ref, arith, ngpus, monkeypatch):
    """T, U, P, L in the order include/nbody.h fixes — a rank's rows in groups of 256 from its first body, ascending rows, groups
    ascending, T and U halved, ranks in rank order — restated by tests/potential_ref.c energy_totals_*: the eight values bit for bit
    (NaN for NaN in the "nan" variant) on one device and on three, whose slices are mini_nbody_amd/sharding.py's."""
    from mini_nbody_amd.sharding import slice_bounds
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    fp64 = arith == "fp64_strict"
    dtype = np.float64 if fp64 else np.float32
    mode = nb.ARITH_REFERENCE_STRICT if arith == "reference_strict" else nb.ARITH_STRICT
    for n in SIZES + (3000,):
        slices = [(f0, f1 - f0) for f0, f1 in (slice_bounds(q, n, ngpus) for q in range(ngpus))]
        with nb.NBody(n, fp64=fp64, ngpus=ngpus) as eng:
            eng.set_option(nb.OPT_ARITH, mode)
            systems = [("cloud",) + nb.make_bodies(n, dtype=dtype)] if n == 3000 else [(v,) + hostile_system(nb, n, dtype, v)[:2] for v in VARIANTS]
            for variant, pos, vel in systems:
                eng.upload(pos, vel)
                got = bits(eng.energy()).view(np.float64)
                want = ref.totals(pos, vel, slices, ref=(mode == nb.ARITH_REFERENCE_STRICT))
                assert same_nan(got, want), (n, variant, ngpus, got, want)
                assert np.isnan(want).sum() == (6 if variant == "nan" else 0), (n, variant, want)   # all but Px, Py
