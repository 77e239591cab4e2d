"""Sixth-order individual block time steps (nbody_step_hermite6_block(_d); include/nbody.h "sixth-order individual block time steps"):
the strict modes bit for bit against tests/hermite6_block_ref.c with its counters, one level against nbody_step_hermite6 bit for bit in
every arithmetic, the masses and the zero-mass tracers, the same bits and counters however the work is laid out (the source split,
devices with and without an active row, processes), the timed binary32 run's counters and energy error, the restart rule and the
guards.  The inputs are chosen for what they exercise, and that is asserted from the statement's trace (tests/test_hermite6_block_abi.py
holds the figures; hermite6_block_common says which case is for what)."""
import ctypes as C

import numpy as np
import pytest

from hermite_common import energy
from hermite6_block_common import (ENERGY_RUN, ENERGY_STRICT_F32, ENERGY_TIMED_F32_BOUND, GPU_CASE, GPU_LEVELS, GPU_SIZES, Block6Ref, case_bodies,
                                   compile_ref, energy_system, equal_slices)
from pass_common import bits, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import SIZES as HOSTILE_SIZES
from specials_common import VARIANTS, hostile_dynamic_system, same_nan

pytestmark = pytest.mark.gpu
CASE8 = dict(GPU_CASE, levels=8)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return Block6Ref(compile_ref(tmp_path_factory.mktemp("hermite6_block_ref")))


def block(eng, run):
    return eng.step_hermite6_block(run["dt_max"], run["nblocks"], eta=run["eta"], levels=run["levels"])


STRICT = {"strict": (False, "ARITH_STRICT", False), "reference_strict": (False, "ARITH_REFERENCE_STRICT", True), "fp64_strict": (True, "ARITH_STRICT", False)}


@pytest.mark.parametrize("arith", list(STRICT))
def test_strict_bit_for_bit(nb, ref, arith):
    """eta = 0.04, dt_max = 1/64, two blocks on 1, 3 and 8 levels: the state, the sub-steps and the row evaluations are the statement's,
    and NBODY_INFO_STEPS_DONE grows by the sub-steps.  N = 1 (a lone body: level 0), the Kepler pair of e = 0.9, energy_system, 257 (a
    tail of one row behind a tile) and 611; from the trace on 8 levels: an all-rows sub-step in every case, and at 257 and 611 at least
    3 levels occupied, a one-row sub-step, an active list across a 256-row tile edge."""
    fp64, mode, is_ref = STRICT[arith]
    dtype = np.float64 if fp64 else np.float32
    for n in GPU_SIZES:
        pos, vel = case_bodies(nb, n, dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            done = 0
            for levels in GPU_LEVELS:
                run = dict(GPU_CASE, levels=levels)
                wp, wv, wsteps, wevals, trace = ref.run(pos, vel, dtype, ref=is_ref, **run)
                assert any(len(r) == n for r in trace.rows)
                if levels == 8 and n >= 257:
                    assert trace.occupied_levels() >= 3 and trace.crosses_tile_edge() and any(len(r) == 1 for r in trace.rows)
                eng.upload(pos, vel)
                steps, evals = block(eng, run)
                got = eng.download()
                done += wsteps
                assert eng.info(nb._lib.INFO_STEPS_DONE) == done
                assert (steps, evals) == (wsteps, wevals), (n, levels)
                assert same(got, (wp, wv)), (n, levels, int((bits(got[0]) != bits(wp)).any(1).sum()), int((bits(got[1]) != bits(wv)).any(1).sum()))
                assert same(got[0][:, 3], pos[:, 3]) and same(got[1][:, 3], vel[:, 3])


ONE_LEVEL = {"fma3": (False, "ARITH_FMA3"), "reference": (False, "ARITH_REFERENCE"), "strict": (False, "ARITH_STRICT"),
             "reference_strict": (False, "ARITH_REFERENCE_STRICT"), "fp64": (True, "ARITH_FMA3"), "fp64_strict": (True, "ARITH_STRICT")}


@pytest.mark.parametrize("arith", list(ONE_LEVEL))
def test_one_level_is_the_shared_step(nb, arith):
    """step_hermite6_block(dt, 3, levels=1) is step_hermite6(dt, 3) on the same context bit for bit, timed arithmetics included: the
    coefficients formed per row on the device are those the host forms once per step"""
    fp64, mode = ONE_LEVEL[arith]
    dtype = np.float64 if fp64 else np.float32
    for n in (1, 2, 257, 1025):
        pos, vel = case_bodies(nb, n, dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            for dt in (1.0 / 256, 0.01):
                eng.upload(pos, vel)
                eng.step_hermite6(dt, 3)
                want = eng.download()
                eng.upload(pos, vel)
                assert eng.step_hermite6_block(dt, 3, levels=1) == (3, 3 * n)
                got = eng.download()
                assert same(got, want), (n, dt, int((bits(got[0]) != bits(want[0])).any(1).sum()))
                assert same(got[0][:, 3], pos[:, 3]) and same(got[1][:, 3], vel[:, 3])
                if n > 1:
                    assert not same(got[0], pos)


@pytest.mark.parametrize("fp64", [False, True])
def test_masses_and_tracers(nb, ref, fp64):
    """strict arithmetic, NBODY_OPT_MASSES: 257 bodies of masses 1/4 .. 1 and 40 tracers (w = +0) behind them, eight of them in tight
    orbits about massive bodies so that they add sub-steps of their own — the statement's bits and counters, every w carried bit for
    bit, and no bit of the 257 massive rows differs from the run without the tracers.  w = 1 everywhere gives the unweighted bits."""
    dtype = np.float64 if fp64 else np.float32
    n, extra = 257, 40
    pos, vel = nb.make_bodies(n + extra, dtype=dtype)
    pos[:n, 3] = (1 + np.arange(n) % 4) * 0.25
    pos[n:, 3] = 0
    pos[n:n + 8, :3] = pos[:8, :3] + dtype(0.004)
    ones = pos.copy()
    ones[:, 3] = 1
    want = ref.run(pos, vel, dtype, mass=True, **CASE8)
    with nb.NBody(n + extra, fp64=fp64) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(ones, vel)
        plain_counters = block(eng, CASE8)
        plain = eng.download()
        eng.use_masses()
        eng.upload(ones, vel)
        assert block(eng, CASE8) == plain_counters and same(eng.download(), plain)
        eng.upload(pos, vel)
        counters = block(eng, CASE8)
        both = eng.download()
    assert counters == want[2:4] and same(both, want[:2])
    assert same(both[0][:, 3], pos[:, 3]) and not same(both[0][:, :3], plain[0][:, :3])
    with nb.NBody(n, fp64=fp64) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.use_masses()
        eng.upload(pos[:n], vel[:n])
        alone_counters = block(eng, CASE8)
        alone = eng.download()
    assert same((both[0][:n], both[1][:n]), alone)
    assert counters[0] > alone_counters[0] and counters[1] > alone_counters[1]      # the tracers did add sub-steps


def block_state(nb, n, pos, vel, mode, run, ngpus=1):
    with nb.NBody(n, ngpus=ngpus) as eng:
        eng.set_option(nb.OPT_ARITH, mode)
        eng.upload(pos, vel)
        counters = block(eng, run)
        cfg = eng.config
        return (eng.download(), counters), (cfg["first_body"], cfg["n_local"])


def test_bits_and_counters_do_not_depend_on_the_source_split(nb, ref, monkeypatch):
    """N = 2100 (three source blocks, so that 2 and 3 chunks differ and 7 is clamped), one block on 6 levels, strict binary32 (the
    statement's bits and counters) and timed binary32: NBODY_SNAP_SPLIT = 1, 2, 3, 7, the automatic choice and a 1 MB scratch bound
    give the same bits and counters"""
    for name in ("NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB", "NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"):
        monkeypatch.delenv(name, raising=False)
    n, run = 2100, dict(GPU_CASE, levels=6, nblocks=1)
    pos, vel = case_bodies(nb, n, np.float32)
    wp, wv, wsteps, wevals, trace = ref.run(pos, vel, np.float32, **run)
    assert trace.occupied_levels() >= 3 and wevals < wsteps * n / 2
    for mode in (nb.ARITH_STRICT, nb.ARITH_FMA3):
        monkeypatch.setenv("NBODY_SNAP_SPLIT", "1")
        base = block_state(nb, n, pos, vel, mode, run)[0]
        if mode == nb.ARITH_STRICT:
            assert same(base[0], (wp, wv)) and base[1] == (wsteps, wevals)
        assert not same(base[0][0], pos)
        for split in ("2", "3", "7", None):
            if split is None:
                monkeypatch.delenv("NBODY_SNAP_SPLIT")
            else:
                monkeypatch.setenv("NBODY_SNAP_SPLIT", split)
            got = block_state(nb, n, pos, vel, mode, run)[0]
            assert same(got[0], base[0]) and got[1] == base[1], (mode, split)
        monkeypatch.setenv("NBODY_SNAP_SCRATCH_MB", "1")
        for split in (None, "3"):
            if split:
                monkeypatch.setenv("NBODY_SNAP_SPLIT", split)
            got = block_state(nb, n, pos, vel, mode, run)[0]
            assert same(got[0], base[0]) and got[1] == base[1], (mode, split, "1 MB")
        monkeypatch.delenv("NBODY_SNAP_SPLIT")
        monkeypatch.delenv("NBODY_SNAP_SCRATCH_MB")


def test_bits_and_counters_do_not_depend_on_the_devices(nb, ref, monkeypatch):
    """make_bodies(257) and energy_system, strict binary32 (the statement's bits, so its trace is the run's own) and timed binary32:
    three oversubscribed devices give one device's bits and counters.  By the trace 14 of 235 and 98 of 100 sub-steps leave one of the
    three devices without an active row, the slices being the library's (the first device's are read back from the context)."""
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    for name in ("NBODY_SNAP_SPLIT", "NBODY_SNAP_SCRATCH_MB"):
        monkeypatch.delenv(name, raising=False)
    for n, idle in ((257, 14), (8, 98)):
        pos, vel = case_bodies(nb, n, np.float32)
        wp, wv, wsteps, wevals, trace = ref.run(pos, vel, np.float32, **CASE8)
        assert len(trace.idle_substeps(equal_slices(n, 3))) == idle
        for mode in (nb.ARITH_STRICT, nb.ARITH_FMA3):
            base, own = block_state(nb, n, pos, vel, mode, CASE8)
            assert own == (0, n)
            if mode == nb.ARITH_STRICT:
                assert same(base[0], (wp, wv)) and base[1] == (wsteps, wevals)
            got, own = block_state(nb, n, pos, vel, mode, CASE8, ngpus=3)
            assert own == equal_slices(n, 3)[0]
            assert same(got[0], base[0]) and got[1] == base[1], (n, mode)


WORKER = """
    from hermite6_block_common import case_bodies
    pos, vel = case_bodies(nb, n, np.float32)
    eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
    eng.upload(pos, vel)
    steps, evals = eng.step_hermite6_block(1.0 / 64, 2, eta=0.04, levels=8)
    p, v = eng.download()
    cfg = eng.config
    np.savez({out!r} + "_%d.npz" % rank, pos=p, vel=v, counters=np.array([steps, evals]), own=np.array([cfg["first_body"], cfg["n_local"]]))
"""


def test_two_processes_host_transport_equal_one_process(nb, ref, tmp_path):
    """N = 257, strict binary32, two ranks over the host transport: the statement's bits and counters on both.  Positions, velocities
    and predicted accelerations travel in every sub-step (the accelerations first: full_scratch holds the velocities afterwards), and
    by the trace 14 sub-steps leave a rank without an active row — where a collective could go wrong"""
    n, world = 257, 2
    pos, vel = case_bodies(nb, n, np.float32)
    wp, wv, wsteps, wevals, trace = ref.run(pos, vel, np.float32, **CASE8)
    out = str(tmp_path / "h6b")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    slices = [tuple(int(x) for x in got[r]["own"]) for r in range(world)]      # the ranks' own slices
    assert slices == equal_slices(n, world) and len(trace.idle_substeps(slices)) == 14
    for r in range(world):
        assert same((got[r]["pos"], got[r]["vel"]), (wp, wv)), r
        assert tuple(int(c) for c in got[r]["counters"]) == (wsteps, wevals), r


def test_timed_binary32_on_the_energy_system(nb):
    """energy_system under ENERGY_RUN on a timed binary32 context.  The call returns 0 — its loop refuses a tau beyond the end, so
    every row has reached the end tick, the invariant's end state —; at least one sub-step per block, every row evaluated at every
    block's end and at least one row in every sub-step, never more than all rows; and |dE/E|, measured in binary64 numpy on the
    downloaded state as the CPU figure is, at most 4 x the statement's strict-binary32 3.532e-06 (tests/test_hermite6_block_abi.py
    asserts that figure; hermite6_block_common says why 4)."""
    pos, vel = energy_system(np.float32)
    n, nblocks = len(pos), ENERGY_RUN["nblocks"]
    e0 = energy(pos, vel)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        steps, evals = block(eng, ENERGY_RUN)
        got = eng.download()
    de = abs(energy(*got) - e0) / abs(e0)
    print("timed binary32: %d sub-steps, %d row evaluations, |dE/E| %.3e (strict binary32 on the CPU: %.3e)" % (steps, evals, de, ENERGY_STRICT_F32))
    assert steps >= nblocks and nblocks * n + (steps - nblocks) <= evals <= steps * n
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert de <= ENERGY_TIMED_F32_BOUND


def test_restarts_and_repeated_calls(nb, ref):
    """N = 257, strict binary32, 8 levels: two calls of one block are the statement restarted (each call evaluates afresh, zeroes the
    crackle and assigns the levels anew) and differ from one call of two blocks, which is the statement's too; the same call on the
    same state twice gives the same bits and counters"""
    n = 257
    pos, vel = case_bodies(nb, n, np.float32)
    one = dict(CASE8, nblocks=1)
    first = ref.run(pos, vel, np.float32, **one)
    second = ref.run(first[0], first[1], np.float32, **one)
    carried = ref.run(pos, vel, np.float32, **CASE8)
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos, vel)
        assert block(eng, one) == first[2:4]
        assert block(eng, one) == second[2:4]
        restarted = eng.download()
        eng.upload(pos, vel)
        counters = block(eng, CASE8)
        got = eng.download()
        eng.upload(pos, vel)
        assert block(eng, CASE8) == counters and same(eng.download(), got)
    assert same(restarted, second[:2]) and same(got, carried[:2]) and counters == carried[2:4]
    assert not same(restarted, got)


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    s, e = C.c_longlong(7), C.c_longlong(7)
    b32 = lambda eta=0.02, dt=1.0 / 16, levels=8, nblocks=1: lib.nbody_step_hermite6_block(eta, dt, levels, nblocks, C.byref(s), C.byref(e))
    b64 = lambda eta=0.02, dt=1.0 / 16, levels=8, nblocks=1: lib.nbody_step_hermite6_block_d(eta, dt, levels, nblocks, C.byref(s), C.byref(e))
    untouched = lambda: (s.value, e.value) == (7, 7)
    lib.nbody_shutdown()
    assert [b32(), b64()] == [E.ERR_NOT_INIT] * 2
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert [b32(), b64()] == [E.ERR_STATE] * 2
        finally:
            mb.serve(False)
    assert untouched()
    n = 100
    pos, vel = nb.make_bodies(n)
    inf, nan = float("inf"), float("nan")
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        for kw in (dict(eta=0.0), dict(eta=-1.0), dict(eta=nan), dict(eta=inf), dict(eta=-inf), dict(dt=0.0), dict(dt=-1.0 / 16), dict(dt=nan),
                   dict(dt=inf), dict(levels=0), dict(levels=-1), dict(levels=25), dict(nblocks=0), dict(nblocks=-3),
                   dict(dt=1e-37, levels=8), dict(dt=2.0 ** -120, levels=8)):       # the tick below the smallest normal binary32
            assert b32(**kw) == E.ERR_ARG, kw
        assert b64() == E.ERR_STATE
        assert untouched() and eng.info(E.INFO_STEPS_DONE) == 0
        assert same(eng.download(), (pos, vel))                      # a refused call has changed nothing in the state
        assert lib.nbody_step_hermite6_block(0.02, 1.0 / 16, 8, 1, None, None) == 0
        assert lib.nbody_step_hermite6_block(0.02, 1.0 / 1024, 24, 1, C.byref(s), None) == 0 and s.value >= 1
        assert not same(eng.download()[0], pos)
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert b32() == E.ERR_STATE
        assert b64(dt=1e-307, levels=8) == E.ERR_ARG                 # below the smallest normal binary64
        assert b64() == 0


@pytest.mark.parametrize("arith", list(STRICT))
def test_hostile_system_one_strict_block(nb, ref, arith):
    """specials_common.hostile_dynamic_system in every variant and size, one block of dt_max = 1/256 on 8 levels with eta = 0.04 (the
    fourth-order hostile test's run): the call returns, state and both counters are the statement's (NaN where it is NaN).  In "base"
    and "overflow" every row stays finite and the block takes more than a hundred sub-steps on at least three levels; a row whose
    (a, j) is NaN sits on level 0, so "nan" and "inf" take one sub-step of all n rows."""
    fp64, mode, is_ref = STRICT[arith]
    dtype = np.float64 if fp64 else np.float32
    run = dict(eta=0.04, dt_max=1.0 / 256, levels=8, nblocks=1)
    differ = []
    for n in HOSTILE_SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            for variant in VARIANTS:
                pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                with np.errstate(all="ignore"):
                    wp, wv, wsteps, wevals, trace = ref.run(pos, vel, dtype, ref=is_ref, **run)
                counters = block(eng, run)
                got = eng.download()
                if not (same_nan(got[0], wp) and same_nan(got[1], wv) and counters == (wsteps, wevals)):
                    differ.append((n, variant, counters, (wsteps, wevals)))
                if variant in ("nan", "inf"):
                    assert (trace.level0 == 0).all() and (wsteps, wevals) == (1, n), (n, variant)
                else:
                    assert wsteps > 100 and trace.occupied_levels() >= 3, (n, variant, wsteps)
                    if not (np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))):
                        differ.append((n, variant, "a row is not finite"))
    assert not differ, differ
