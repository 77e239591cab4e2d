"""Individual block time steps (nbody_step_hermite_block(_d); include/nbody.h "individual block time steps"): one level against
nbody_step_hermite bit for bit in every arithmetic, the strict modes bit for bit against tests/hermite_block_ref.c with its counters,
the same bits and counters however the work is laid out (devices with and without an active row, the source split, the batches,
processes), the energy error against the shared step with as many row evaluations, what a call leaves alone, the guards, the hostile
system and the C host program's --hermite-block line.  The inputs are chosen for what they exercise, and that is asserted from the
reference's trace (hermite_block_common.Trace; tests/test_hermite_block_abi.py holds the figures)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from hermite_block_common import ENERGY_RATIO_BOUND, ENERGY_RUN, BlockRef, compile_ref, energy_system, equal_slices, shared_steps_for
from hermite_common import kepler
from pass_common import bits, same
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import SIZES, VARIANTS, hostile_system, same_nan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE = dict(eta=0.04, dt_max=1.0 / 64, levels=8, nblocks=1)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return BlockRef(compile_ref(tmp_path_factory.mktemp("hermite_block_ref")))


def canaries(nb, n, dtype):
    """make_bodies with canaries in the fourth value of both words (tests/test_gpu_hermite.py's): the call must carry them bit for bit"""
    pos, vel = nb.make_bodies(n, dtype=dtype)
    pos[:, 3] = (np.arange(n) % 977).astype(dtype) - dtype(7.5)
    vel[:, 3] = (np.arange(n) % 31).astype(dtype) + dtype(0.25)
    return pos, vel


def block(eng, run):
    return eng.step_hermite_block(run["dt_max"], run["nblocks"], eta=run["eta"], levels=run["levels"])


ONE_LEVEL = {"fma3": (False, "ARITH_FMA3"), "reference": (False, "ARITH_REFERENCE"), "strict": (False, "ARITH_STRICT"),
             "reference_strict": (False, "ARITH_REFERENCE_STRICT"), "fp64": (True, "ARITH_FMA3"), "fp64_strict": (True, "ARITH_STRICT")}


@pytest.mark.parametrize("arith", list(ONE_LEVEL))
def test_one_level_is_the_shared_step(nb, arith):
    """step_hermite_block(dt, 3, levels=1) is step_hermite(dt, 3) on the same context bit for bit, timed arithmetics included"""
    fp64, mode = ONE_LEVEL[arith]
    dtype = np.float64 if fp64 else np.float32
    for n in (1, 2, 63, 257, 1025):
        pos, vel = canaries(nb, n, dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            for dt in (1.0 / 256, 0.01):
                eng.upload(pos, vel)
                eng.step_hermite(dt, 3)
                want = eng.download()
                eng.upload(pos, vel)
                assert eng.step_hermite_block(dt, 3, levels=1) == (3, 3 * n)
                got = eng.download()
                assert same(got, want), (n, dt, int((bits(got[0]) != bits(want[0])).any(1).sum()))
                assert same(got[0][:, 3], pos[:, 3]) and same(got[1][:, 3], vel[:, 3])
                if n > 1:
                    assert not same(got[0], pos)


STRICT = {"strict": (False, "ARITH_STRICT", False), "reference_strict": (False, "ARITH_REFERENCE_STRICT", True), "fp64_strict": (True, "ARITH_STRICT", False)}


@pytest.mark.parametrize("arith", list(STRICT))
def test_strict_bit_for_bit(nb, ref, arith):
    """eta = 0.04, dt_max = 1/64, 8 levels, one block: the state, the sub-steps and the row evaluations are the reference's.  The inputs:
    N = 1 (a lone body: level 0), the Kepler pair of e = 0.9, tails below a wave and a workgroup, and one, two and three source blocks;
    from the trace: at least 3 levels occupied at N >= 63, an all-active sub-step in every case, a one-row sub-step in some, an active
    list across a 256-row workgroup edge at N >= 1025."""
    fp64, mode, is_ref = STRICT[arith]
    dtype = np.float64 if fp64 else np.float32
    one_row = False
    for n in (1, 2, 63, 257, 1025, 2100):
        pos, vel = kepler(0.9, dtype) if n == 2 else canaries(nb, n, dtype)
        wp, wv, wsteps, wevals, trace = ref.run(pos, vel, dtype, ref=is_ref, **CASE)
        assert any(len(r) == n for r in trace.rows)
        assert n < 63 or trace.occupied_levels() >= 3
        assert n < 1025 or trace.crosses_tile_edge()
        one_row = one_row or any(len(r) == 1 for r in trace.rows if n > 1)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, getattr(nb, mode))
            eng.upload(pos, vel)
            steps, evals = block(eng, CASE)
            got = eng.download()
            assert eng.info(nb._lib.INFO_STEPS_DONE) == wsteps
        assert (steps, evals) == (wsteps, wevals), n
        assert same(got, (wp, wv)), (n, int((bits(got[0]) != bits(wp)).any(1).sum()), int((bits(got[1]) != bits(wv)).any(1).sum()))
        assert same(got[0][:, 3], pos[:, 3]) and same(got[1][:, 3], vel[:, 3])
    assert one_row


def block_state(nb, n, pos, vel, mode, ngpus=1):
    with nb.NBody(n, ngpus=ngpus) as eng:
        eng.set_option(nb.OPT_ARITH, mode)
        eng.upload(pos, vel)
        counters = block(eng, CASE)
        cfg = eng.config
        return (eng.download(), counters), (cfg["first_body"], cfg["n_local"])


def test_bits_and_counters_do_not_depend_on_the_layout(nb, ref, monkeypatch):
    """make_bodies(257) and N = 63, strict fp32 (the reference's bits, so its trace is the run's own) and timed fp32: three
    oversubscribed devices, the forced source split and the batches give one device's bits and counters.  By the trace 14 of 107 and
    84 of 104 sub-steps leave one of the three devices without an active row, the slices being the library's (the first device's are
    read back from the context)."""
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    for name in ("NBODY_JERK_SPLIT", "NBODY_JERK_SCRATCH_MB"):
        monkeypatch.delenv(name, raising=False)
    for n, idle in ((257, 14), (63, 84)):
        pos, vel = canaries(nb, n, np.float32)
        wp, wv, wsteps, wevals, trace = ref.run(pos, vel, np.float32, **CASE)
        assert len(trace.idle_substeps(equal_slices(n, 3))) == idle
        for mode in (nb.ARITH_STRICT, nb.ARITH_FMA3):
            base, own = block_state(nb, n, pos, vel, mode)
            assert own == (0, n)
            if mode == nb.ARITH_STRICT:
                assert same(base[0], (wp, wv)) and base[1] == (wsteps, wevals)
            assert not same(base[0][0], pos) and same(base[0][0][:, 3], pos[:, 3])
            got, own = block_state(nb, n, pos, vel, mode, ngpus=3)
            assert own == equal_slices(n, 3)[0]
            assert same(got[0], base[0]) and got[1] == base[1], (n, mode)
            for split in ("1", "3"):
                monkeypatch.setenv("NBODY_JERK_SPLIT", split)
                for ngpus in (1, 3):
                    got = block_state(nb, n, pos, vel, mode, ngpus=ngpus)[0]
                    assert same(got[0], base[0]) and got[1] == base[1], (n, mode, split, ngpus)
            monkeypatch.setenv("NBODY_JERK_SCRATCH_MB", "1")
            got = block_state(nb, n, pos, vel, mode)[0]
            assert same(got[0], base[0]) and got[1] == base[1]
            monkeypatch.delenv("NBODY_JERK_SPLIT")
            got = block_state(nb, n, pos, vel, mode, ngpus=3)[0]
            assert same(got[0], base[0]) and got[1] == base[1]
            monkeypatch.delenv("NBODY_JERK_SCRATCH_MB")


WORKER = """
    pos, vel = nb.make_bodies(n)
    eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
    eng.upload(pos, vel)
    steps, evals = eng.step_hermite_block(1.0 / 64, 1, eta=0.04, levels=8)
    p, v = eng.download()
    cfg = eng.config
    np.savez({out!r} + "_%d.npz" % rank, pos=p, vel=v, counters=np.array([steps, evals]), own=np.array([cfg["first_body"], cfg["n_local"]]))
"""


def test_two_processes_host_transport_equal_one_process(nb, ref, tmp_path):
    """N = 257, strict fp32, two ranks over the host transport: the reference's bits and counters on both; by its trace some sub-steps
    leave a rank without an active row — where a collective could go wrong"""
    n, world = 257, 2
    pos, vel = nb.make_bodies(n)
    wp, wv, wsteps, wevals, trace = ref.run(pos, vel, np.float32, **CASE)
    out = str(tmp_path / "hb")
    run_ranks(tmp_path, worker_source(WORKER, n=n, out=out), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    slices = [tuple(int(x) for x in got[r]["own"]) for r in range(world)]      # the ranks' own slices
    assert slices == equal_slices(n, world) and len(trace.idle_substeps(slices)) == 14
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
        eng.upload(pos, vel)
        counters = block(eng, CASE)
        one = eng.download()
    assert same(one, (wp, wv)) and counters == (wsteps, wevals)
    for r in range(world):
        assert same((got[r]["pos"], got[r]["vel"]), one), r
        assert tuple(int(c) for c in got[r]["counters"]) == counters, r


def test_energy_against_the_shared_step(nb):
    """The system of the energy test (hermite_block_common.energy_system) on a timed fp64 context, eta = 0.02, dt_max = 1/16, 8 levels,
    16 blocks to t = 1: fewer than half of sub-steps x N row evaluations, and |dE/E| at most 1e-2 of nbody_step_hermite's with
    ceil(row_evals / N / 16) * 16 steps to t = 1.  In binary64 on the CPU (tests/hermite_block_ref.c, asserted in
    tests/test_hermite_block_abi.py): 1839 sub-steps, 3876 row evaluations, 1.58e-6 against 2.90e-3 with 496 steps, a ratio of 5.45e-4 —
    a factor 18 inside the bound."""
    pos, vel = energy_system()
    n = len(pos)
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos, vel)
        e0 = eng.energy()["total"]
        steps, evals = block(eng, ENERGY_RUN)
        de_block = abs(eng.energy()["total"] - e0) / abs(e0)
        k = shared_steps_for(evals, n)
        eng.upload(pos, vel)
        eng.step_hermite(1.0 / k, k)
        de_shared = abs(eng.energy()["total"] - e0) / abs(e0)
    print("%d sub-steps, %d row evaluations (%.3f of sub-steps x N); |dE/E| block %.3e, shared dt with %d steps %.3e, ratio %.3e"
          % (steps, evals, evals / (steps * n), de_block, k, de_shared, de_block / de_shared))
    assert evals < steps * n / 2
    assert de_block <= ENERGY_RATIO_BOUND * de_shared


def test_later_calls_are_a_fresh_contexts(nb):
    """after a block call, eng.step(dt, 4) and eng.jerk() give what they give on a fresh context uploaded with the downloaded state, and
    nbody_kernel_time has not counted"""
    n = 1500
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_TIMING, 1)
        eng.upload(pos, vel)
        eng.step(0.01, 9)
        eng.sync()
        counted = eng.kernel_time()[1]
        block(eng, CASE)
        assert eng.kernel_time()[1] == counted
        mid = eng.download()
        jerk = eng.jerk()
        eng.step(0.01, 4)
        eng.sync()
        after = eng.download()
    with nb.NBody(n) as eng:
        eng.upload(*mid)
        assert same(eng.jerk(), jerk)
        eng.step(0.01, 4)
        eng.sync()
        assert same(eng.download(), after)


def test_guards(nb):
    lib, E = nb._lib.load(), nb._lib
    s, e = C.c_longlong(7), C.c_longlong(7)
    b32 = lambda eta=0.02, dt=1.0 / 16, levels=8, nblocks=1: lib.nbody_step_hermite_block(eta, dt, levels, nblocks, C.byref(s), C.byref(e))
    b64 = lambda eta=0.02, dt=1.0 / 16, levels=8, nblocks=1: lib.nbody_step_hermite_block_d(eta, dt, levels, nblocks, C.byref(s), C.byref(e))
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
        assert b32(dt=2.0 ** -120, levels=7) == 0                    # 2^-126 is the smallest normal: a legal tick
        assert lib.nbody_step_hermite_block(0.02, 1.0 / 16, 8, 1, None, None) == 0
        assert lib.nbody_step_hermite_block(0.02, 1.0 / 1024, 24, 1, C.byref(s), None) == 0 and s.value >= 1
        assert not same(eng.download()[0], pos)
    with nb.NBody(n, fp64=True) as eng:
        eng.upload(pos.astype(np.float64), vel.astype(np.float64))
        assert b32() == E.ERR_STATE
        assert b64(dt=1e-307, levels=8) == E.ERR_ARG                 # below the smallest normal binary64
        assert b64(dt=1e-37, levels=8) == 0                          # ... which a binary32 tick's refusal is not about
        assert b64() == 0


@pytest.mark.parametrize("fp64", [False, True])
def test_hostile_system_one_strict_block(nb, ref, fp64):
    """every variant and size, one block of dt_max = 1/256 on 8 levels: the call returns, state and counters are the reference's (NaN
    where it is NaN); a row whose (a, j) is NaN sits on level 0, so the poisoned variants take one sub-step of all rows"""
    dtype = np.float64 if fp64 else np.float32
    run = dict(eta=0.04, dt_max=1.0 / 256, levels=8, nblocks=1)
    differ = []
    for n in SIZES:
        with nb.NBody(n, fp64=fp64) as eng:
            eng.set_option(nb.OPT_ARITH, nb.ARITH_STRICT)
            for variant in VARIANTS:
                pos, vel, far = hostile_system(nb, n, dtype, variant)
                eng.upload(pos, vel)
                with np.errstate(all="ignore"):
                    wp, wv, wsteps, wevals, trace = ref.run(pos, vel, dtype, **run)
                counters = block(eng, run)
                got = eng.download()
                if not (same_nan(got[0], wp) and same_nan(got[1], wv) and counters == (wsteps, wevals)):
                    differ.append((n, variant, counters, (wsteps, wevals)))
                if variant in ("nan", "inf"):     # one NaN or infinite source poisons every row's (a, j): all on level 0, one sub-step
                    assert (trace.level0 == 0).all() and (wsteps, wevals) == (1, n), (n, variant)
    assert not differ, differ


def test_c_host_program_hermite_block_line(nb):
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters, levels = 1000, 2, 6
    r = subprocess.run([exe, str(n), str(iters), "--hermite-block", str(levels)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "device Hermite block loop" in r.stdout
    m = re.search(r"^hermite block: (\d+) levels, (\d+) sub-steps, (\d+) row evaluations \((\S+) of sub-steps x N\)$", r.stdout, flags=re.M)
    got = [float(v) for v in re.search(r"^checksum \(sum of positions\): (\S+) (\S+) (\S+)$", r.stdout, flags=re.M).groups()]
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.upload(pos, vel)
        steps, evals = eng.step_hermite_block(np.float32(0.01), iters, eta=np.float32(0.02), levels=levels)
        p = eng.download()[0]
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (levels, steps, evals)
    assert float(m.group(4)) == float("%.4f" % (evals / (steps * n)))
    want = [0.0] * 3
    for k in range(n):   # plain ascending fp64 sums, printed with nine digits
        for c in range(3):
            want[c] += float(p[k, c])
    assert [float("%.9g" % w) for w in want] == got, (got, want)
    r = subprocess.run([exe, str(n), str(iters), "--hermite-block", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--hermite-block" in r.stderr
    r = subprocess.run([exe, str(n), str(iters), "--hermite-block", "4", "--host-loop"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--host-loop" in r.stderr
