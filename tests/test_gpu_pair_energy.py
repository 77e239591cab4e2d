"""Pair binding energies and the binary finder on the device (nbody_pair_energy_rows(_d), nbody_binaries; include/nbody.h "pair binding
energies and binaries"): every case bit for bit against tests/pair_energy_ref.c — idx equal, e the same bits — in both precisions, on
the hostile system, however the work is laid out (source split, batches, windows of rows, force configuration, arithmetic option, device
and process count); the binaries of systems whose answer is known by construction, their elements against the Python restatement and
the analytic orbit; no effect on the step; the guards; the C host program's --binaries lines."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from pair_energy_common import ANALYTIC, binary_fixture, make_ref, place, python_elements, same, softened_orbit
from pass_common import FORCE_CONFIGS, PLANS, check_step_untouched
from ranks_common import run_ranks, shared_gpu_env, worker_source
from specials_common import SIZES, VARIANTS, hostile_system, same_nan

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ("NBODY_PAIR_ENERGY_SPLIT", "NBODY_PAIR_ENERGY_SCRATCH_MB")
BOTH = pytest.mark.parametrize("fp64", [False, True])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("pair_energy_ref"))


@pytest.fixture(autouse=True)
def clean_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def dtype_of(fp64):
    return np.float64 if fp64 else np.float32


def windows(n):
    """(first_row, n_rows): everything, the last row alone, and windows that start and end inside a wave — across a 64 boundary, inside
    one wave, across a 256 boundary — so that a wave's CMP windows differ from its neighbours'"""
    w = [(0, n), (n - 1, 1)]
    if n > 70:
        w += [(50, 20), (3, 40)]
    if n > 300:
        w.append((200, 100))
    if n > 1100:
        w.append((1000, 77))
    return w


@BOTH
def test_rows_bit_for_bit(nb, ref, fp64):
    dtype = dtype_of(fp64)
    for n in (1, 2, 63, 64, 65, 257, 1025, 3100):   # the window boundary, a tail, one, two and four source blocks, the lone body
        pos, vel = nb.make_bodies(n, dtype=dtype)
        want = ref.rows(pos, vel)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            for first, cnt in windows(n):
                assert same(eng.pair_energy(first, cnt), tuple(w[first:first + cnt] for w in want)), (n, first, cnt)
            assert same(eng.pair_energy(), want), n
            assert same(eng.pair_energy(), want), "two calls return identical values"
        if n > 1:
            assert np.all(want[1] >= 0) and np.all(np.isfinite(want[0])), n


@BOTH
def test_values_do_not_depend_on_the_source_split_or_the_batches(nb, ref, monkeypatch, fp64):
    n, m = 3100, 700   # four blocks
    dtype = dtype_of(fp64)
    pos, vel = nb.make_bodies(n, dtype=dtype)
    want = ref.rows(pos, vel)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)

        def check(tag):
            assert same(eng.pair_energy(), want), tag
            assert same(eng.pair_energy(100, m), tuple(w[100:100 + m] for w in want)), tag

        for split in (None, "1", "2", "3", "4"):
            if split:
                monkeypatch.setenv("NBODY_PAIR_ENERGY_SPLIT", split)
            check(split)
        # 4 chunks x 8 B (fp64: 12 B) = 32 (48) B per row against 0.015 MB = 15728 B: 491 (327) rows fit, batches of 256 rows
        monkeypatch.setenv("NBODY_PAIR_ENERGY_SCRATCH_MB", "0.015")
        for split in ("4", None):
            if split:
                monkeypatch.setenv("NBODY_PAIR_ENERGY_SPLIT", split)
            else:
                monkeypatch.delenv("NBODY_PAIR_ENERGY_SPLIT")
            check(("batches", split))
        monkeypatch.setenv("NBODY_PAIR_ENERGY_SPLIT", "4")
        monkeypatch.setenv("NBODY_PAIR_ENERGY_SCRATCH_MB", "0")   # not even one workgroup's rows fit: no split
        check("no scratch")


@BOTH
def test_values_do_not_depend_on_the_rows_beside_a_row_the_arithmetic_or_the_force_configuration(nb, ref, fp64):
    n = 3100
    pos, vel = nb.make_bodies(n, dtype=dtype_of(fp64))
    want = ref.rows(pos, vel)
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        for first, cnt in ((0, 1), (100, 257), (3099, 1), (63, 66), (1000, 2000)):
            assert same(eng.pair_energy(first, cnt), tuple(w[first:first + cnt] for w in want)), (first, cnt)
        for mode in (nb.ARITH_FMA3, nb.ARITH_REFERENCE, nb.ARITH_STRICT, nb.ARITH_REFERENCE_STRICT):
            eng.set_option(nb.OPT_ARITH, mode)
            assert same(eng.pair_energy(), want), mode
        eng.set_option(nb.OPT_ARITH, nb.ARITH_FMA3)
        for key, val, default in FORCE_CONFIGS:
            eng.set_option(key, val)
            assert same(eng.pair_energy(), want), (key, val)
            eng.set_option(key, default)


@BOTH
def test_hostile_system(nb, ref, monkeypatch, fp64):
    """NaN and inf positions, a NaN velocity, a 1e18 (1e150) velocity whose square is finite, squares of differences that overflow,
    coincident groups across the 1023 | 1024 edge, signed zeros: the floats with the same NaN mask and the same bits elsewhere, idx
    equal, for every split"""
    dtype = dtype_of(fp64)
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_system(nb, n, dtype, variant)
            want = ref.rows(pos, vel)
            assert not np.any(np.isnan(want[0]))   # a NaN is never chosen
            with nb.NBody(n, fp64=fp64) as eng:
                eng.upload(pos, vel)
                for split in (None, "1", "2", "3"):
                    if split:
                        monkeypatch.setenv("NBODY_PAIR_ENERGY_SPLIT", split)
                    e, idx = eng.pair_energy()
                    assert same_nan(e, want[0]) and np.array_equal(idx, want[1]), (n, variant, split)
                monkeypatch.delenv("NBODY_PAIR_ENERGY_SPLIT")
            if n > 1024:   # the coincident group at rest relative to nobody: the finite v2 / 2 - 2 / sqrt(eps)
                assert np.all(np.isfinite(want[0][[1023, 1025]])) and np.all(want[0][[1023, 1025]] < -50000), (n, variant)


@BOTH
def test_hand_made_specials(nb, ref, fp64):
    """the systems of tests/test_pair_energy_abi.py whose answers are known by construction, on the device"""
    dtype = dtype_of(fp64)
    big = 1e30 if dtype is np.float32 else 1e200
    cases = (([[1, 2, 3]], [[1, 0, 0]]),                                                            # N = 1: nobody else
             ([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 4]]),                                      # coincident, different velocities: finite
             ([[0, 0, 0], [np.nan, 0, 0], [0, 3, 0]], [[0, 0, 0], [0, 0, 0], [0, 1, 0]]),           # a NaN body poisons its own pairs only
             ([[0, 0, 0], [big, 0, 0]], [[0, 0, 0], [0, 2, 0]]),                                    # d2 overflows: inv = +0, e = v2 / 2
             ([[0, 0, 0], [1, 0, 0]], [[0, 0, 0], [big, 0, 0]]),                                    # v2 overflows: +inf, never chosen
             ([[0, 0, 0], [2, 1, 0], [-2, -1, 0]], [[0, 0, 0], [0, 0.5, 0], [0, -0.5, 0]]))         # an exact tie in row 0: the lowest j
    for p, v in cases:
        pos, vel = np.zeros((len(p), 4), dtype), np.zeros((len(p), 4), dtype)
        pos[:, :3], vel[:, :3] = p, v
        want = ref.rows(pos, vel)
        with nb.NBody(len(p), fp64=fp64) as eng:
            eng.upload(pos, vel)
            assert same(eng.pair_energy(), want), (p, v)
            found, wi, wj, wel = ref.binaries(pos, vel)
            i, j, el = eng.binaries()
            assert eng.binaries_found == found and np.array_equal(i, wi) and np.array_equal(j, wj), (p, v)
    assert want[1][0] == 1   # (the last case: both mirrored bodies give row 0 the same bits, the lower index is kept)


@BOTH
def test_binaries_of_the_fixture(nb, ref, fp64):
    """exactly the pair (0, 1); elements against the Python restatement on the downloaded state at 1e-12 relative (ecc: 1e-7 absolute,
    a cancellation of order 1e-16 in ecc^2 under a square root), and in a binary32 context against the analytic values at 1e-5 (eight
    inputs rounded at 6e-8, amplified by less than 4)"""
    dtype = dtype_of(fp64)
    pos, vel = binary_fixture(dtype)
    with nb.NBody(len(pos), fp64=fp64) as eng:
        eng.upload(pos, vel)
        now, vnow = eng.download()
        assert same(eng.pair_energy(), ref.rows(now, vnow))
        i, j, el = eng.binaries()
        assert (list(i), list(j), eng.binaries_found) == ([0], [1], 1) and el.shape == (1, 4) and el.dtype == np.float64
        want = python_elements(now, vnow, 0, 1)
        print("elements", el[0], "restatement", want)
        assert np.all(np.abs(el[0][[0, 1, 3]] - want[[0, 1, 3]]) <= 1e-12 * np.abs(want[[0, 1, 3]])) and abs(el[0][2] - want[2]) <= 1e-7
        assert same(el[0], ref.binaries(now, vnow)[3][0])   # (the C statement of the same operations: the same bits)
        rel = np.abs(el[0] - np.array(ANALYTIC)) / np.abs(np.array(ANALYTIC))
        print("relative differences from the analytic {E, a, ecc, period}:", rel)
        assert np.all(rel <= (1e-12 if fp64 else 1e-5)), rel
        # a = 1 means E = -1: nothing is below -2, nothing below -inf; max_pairs = 0 counts
        assert len(eng.binaries(e_max=-2.0)[0]) == 0 and eng.binaries_found == 0
        assert len(eng.binaries(e_max=-math.inf)[0]) == 0 and eng.binaries_found == 0
        assert len(eng.binaries(max_pairs=0)[0]) == 0 and eng.binaries_found == 1
        found = C.c_int(-5)
        assert eng.lib.nbody_binaries(0.0, 0, C.byref(found), None, None, None) == 0 and found.value == 1


@BOTH
def test_binaries_of_three_pairs_and_of_a_triple(nb, ref, fp64):
    dtype = dtype_of(fp64)
    pair = softened_orbit()
    lone = (np.array([[0.0, 0, 0, 0]]), np.array([[0.0, 0, 0, 0]]))
    # a lone body first, then three binaries a hundred lengths apart: the pairs are (1, 2), (3, 4), (5, 6)
    pos, vel = place(((lone[0], lone[1], (0, 50, 0)), (pair[0], pair[1], (0, 0, 0)), (pair[0], pair[1], (100, 0, 0)), (pair[0], pair[1], (0, 0, -100))), dtype)
    with nb.NBody(len(pos), fp64=fp64) as eng:
        eng.upload(pos, vel)
        i, j, el = eng.binaries()
        assert (list(i), list(j)) == ([1, 3, 5], [2, 4, 6]) and eng.binaries_found == 3
        found, wi, wj, wel = ref.binaries(pos, vel)
        assert found == 3 and same(el, wel)
        i, j, el1 = eng.binaries(max_pairs=1)   # the lowest i, and the number found all the same
        assert (list(i), list(j), eng.binaries_found) == ([1], [2], 3) and same(el1, wel[:1])
    # a triple: a tight pair (separation 0.1, at relative rest: e = -20) and a third body one length away, bound to a member of the
    # pair (e = -2) that prefers its mate: only the mutual pair is listed
    pos, vel = np.zeros((3, 4), dtype), np.zeros((3, 4), dtype)
    pos[:, 0] = [1.0, -0.05, 0.05]   # the third body first: the pair is (1, 2)
    with nb.NBody(3, fp64=fp64) as eng:
        eng.upload(pos, vel)
        e, idx = eng.pair_energy()
        assert list(idx) == [2, 2, 1] and e[0] < -1.5   # body 0 is bound, to body 2, which prefers body 1
        i, j, el = eng.binaries()
        assert (list(i), list(j), eng.binaries_found) == ([1], [2], 1)
        assert same(el, ref.binaries(pos, vel)[3])


@BOTH
def test_values_do_not_depend_on_the_device_count(nb, ref, monkeypatch, fp64):
    monkeypatch.setenv("NBODY_OVERSUBSCRIBE", "1")
    n = 1500   # 1500 = 500 x 3: slices that end inside a 64-source window and inside a workgroup's rows
    pos, vel = nb.make_bodies(n, dtype=dtype_of(fp64))
    res = {}
    for ngpus in (1, 3):
        with nb.NBody(n, fp64=fp64, ngpus=ngpus) as eng:
            eng.upload(pos, vel)
            eng.step(0.01, 2)   # each local then holds only its own slice's new positions and velocities: the pass brings the rest
            res[ngpus] = (eng.pair_energy(), eng.pair_energy(450, 600), eng.binaries(), eng.download())
    for g_ in (1, 3):
        now, vnow = res[g_][3]   # (the timed arithmetic's sums follow the device count: each state against its own reference)
        assert not same((vnow,), (vel,)), "the velocities did not change"
        want = ref.rows(now, vnow)
        assert same(res[g_][0], want), g_
        assert same(res[g_][1], tuple(w[450:1050] for w in want)), g_   # a window across both device boundaries: global indices
        found, wi, wj, wel = ref.binaries(now, vnow)
        assert found > 0 and np.any(wi // 500 != wj // 500)   # binaries whose members lie in different devices' slices among them
        assert same(res[g_][2], (wi, wj, wel)), g_


WORKER = """
    pos, vel = nb.make_bodies(n, seed=33, dtype=np.float64 if {fp64} else np.float32)
    eng.upload(pos, vel)
    eng.step(0.01, 3)
    e, idx = eng.pair_energy()                                  # this rank's own rows
    i, j, el = eng.binaries()                                   # the whole system, on every rank
    p, v = eng.download()
    np.savez({out!r} + "_%d.npz" % rank, e=e, idx=idx, i=i, j=j, el=el, first=np.array([eng.config["first_body"], eng.config["n_local"]]), pos=p, vel=v)
"""


@BOTH
def test_two_processes_host_transport_equal_the_reference(nb, ref, tmp_path, fp64):
    """after three steps the velocities differ from the upload, and each rank holds only its own: they must really be gathered (binary64:
    32-byte words through the transport, into full_scratch and back from it for the elements)"""
    n, world = 4007, 2
    out = str(tmp_path / "pe")
    run_ranks(tmp_path, worker_source(WORKER, engine='transport="host", fp64={fp64}', n=n, out=out, fp64=fp64), world, 300, env_of=shared_gpu_env)
    got = [np.load(out + "_%d.npz" % r) for r in range(world)]
    now, vnow = got[0]["pos"], got[0]["vel"]
    assert now.dtype == dtype_of(fp64) and same((now, vnow), (got[1]["pos"], got[1]["vel"]))
    assert not same((vnow,), (nb.make_bodies(n, seed=33, dtype=dtype_of(fp64))[1],)), "the velocities did not change"
    want = ref.rows(now, vnow)
    found, wi, wj, wel = ref.binaries(now, vnow)
    split = int(got[1]["first"][0])
    assert found > 0 and np.any((wi < split) & (wj >= split))   # binaries whose members lie in different ranks' slices among them
    covered = 0
    for r in range(world):
        g_ = got[r]
        first, cnt = (int(v) for v in g_["first"])
        assert same((g_["e"], g_["idx"]), tuple(w[first:first + cnt] for w in want)), r   # global indices
        covered += cnt
        assert same((g_["i"], g_["j"], g_["el"]), (wi, wj, wel)), r   # the same list on both ranks
    assert covered == n


def test_pair_energy_calls_leave_the_step_untouched(nb, monkeypatch):
    n = 1500   # two blocks: a forced split takes the scratch and combine path between the steps too
    probe = lambda eng: (eng.pair_energy(), eng.binaries())
    check_step_untouched(nb, monkeypatch, n, probe, "NBODY_PAIR_ENERGY_SPLIT")


def run_steps_fp64(nb, n, pos, vel, plan, graph, probe, timing):
    """pass_common.run_steps in a binary64 context (that helper opens binary32 contexts only): the steps of `plan` with probe(eng) after
    every call (None: nothing) -> positions, velocities, force launches counted"""
    with nb.NBody(n, fp64=True) as eng:
        eng.set_option(nb.OPT_GRAPH, graph)
        if timing:
            eng.set_option(nb.OPT_TIMING, 1)
        eng.upload(pos, vel)
        for k in plan:
            eng.step(0.01, k)
            if probe:
                probe(eng)
        p, v = eng.download()
        return p, v, eng.kernel_time()[1] if timing else None


def test_pair_energy_calls_leave_the_step_untouched_fp64(nb, monkeypatch):
    """what check_step_untouched asserts, in a binary64 context: the calls between the steps change neither the state nor the count of
    force launches — eager steps, graph replays and the timed form, the split automatic and forced to 2"""
    n = 1500
    pos, vel = nb.make_bodies(n, dtype=np.float64)
    probe = lambda eng: (eng.pair_energy(), eng.binaries())
    for plan, graph, timing in PLANS:
        monkeypatch.delenv("NBODY_PAIR_ENERGY_SPLIT", raising=False)
        a = run_steps_fp64(nb, n, pos, vel, plan, graph, None, timing)
        assert not same(a[:2], (pos, vel))
        for split in (None, "2"):
            if split:
                monkeypatch.setenv("NBODY_PAIR_ENERGY_SPLIT", split)
            b = run_steps_fp64(nb, n, pos, vel, plan, graph, probe, timing)
            assert same(a[:2], b[:2]), (plan, graph, split)
            assert a[2] == b[2], "the pass's launches were counted by nbody_kernel_time (split %s)" % split


@BOTH
def test_guards(nb, fp64):
    """every refusal leaves every output unwritten; `own` is the context's precision, `other` the other one's rows entry point"""
    lib, E = nb._lib.load(), nb._lib
    f32, f64, ip = C.POINTER(C.c_float), C.POINTER(C.c_double), lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    idx, jdx = np.full(4, 7, np.int32), np.full(4, 7, np.int32)
    e32, e64, el = np.full(4, 7, np.float32), np.full(4, 7, np.float64), np.full(16, 7, np.float64)
    found = C.c_int(7)
    e_, d_, i_, j_, el_ = e32.ctypes.data_as(f32), e64.ctypes.data_as(f64), ip(idx), ip(jdx), el.ctypes.data_as(f64)
    untouched = lambda: (np.all(idx == 7) and np.all(jdx == 7) and np.all(e32 == 7) and np.all(e64 == 7) and np.all(el == 7) and found.value == 7)
    own, own_out, mine = (lib.nbody_pair_energy_rows_d, d_, e64) if fp64 else (lib.nbody_pair_energy_rows, e_, e32)
    other, other_out = (lib.nbody_pair_energy_rows, e_) if fp64 else (lib.nbody_pair_energy_rows_d, d_)
    with nb.Mailbox(capacity=1024, faithful=False) as mb:
        mb.serve(True, clock_khz=300000)
        try:
            assert own(0, 4, own_out, i_) == E.ERR_STATE and other(0, 4, other_out, i_) == E.ERR_STATE
            assert lib.nbody_binaries(0.0, 4, C.byref(found), i_, j_, el_) == E.ERR_STATE
        finally:
            mb.serve(False)
        assert untouched()
    n = 100
    pos, vel = nb.make_bodies(n, dtype=dtype_of(fp64))
    with nb.NBody(n, fp64=fp64) as eng:
        eng.upload(pos, vel)
        assert other(0, 4, other_out, i_) == E.ERR_STATE and untouched()
        assert own(0, 4, None, None) == E.ERR_ARG
        for first, rows in ((-1, 4), (0, 0), (0, -2), (97, 4), (100, 1), (0, 101), (1 << 30, 1 << 30)):
            assert own(first, rows, own_out, i_) == E.ERR_ARG, (first, rows)
        for e_max in (math.nan, 1e-30, 0.5, math.inf):
            assert lib.nbody_binaries(e_max, 4, C.byref(found), i_, j_, el_) == E.ERR_ARG, e_max
        assert lib.nbody_binaries(0.0, -1, C.byref(found), i_, j_, el_) == E.ERR_ARG
        assert lib.nbody_binaries(0.0, 4, None, i_, j_, el_) == E.ERR_ARG and lib.nbody_binaries(0.0, 0, None, None, None, None) == E.ERR_ARG
        for args in ((None, j_, el_), (i_, None, el_), (i_, j_, None)):
            assert lib.nbody_binaries(0.0, 4, C.byref(found), *args) == E.ERR_ARG
        assert untouched()
        assert same(eng.download(), (pos, vel))
        assert own(96, 4, None, i_) == 0 and not np.any(idx == 7) and np.all(mine == 7)
        assert own(96, 4, own_out, None) == 0 and not np.any(mine == 7)
        assert lib.nbody_binaries(-math.inf, 4, C.byref(found), i_, j_, el_) == 0 and found.value == 0 and np.all(jdx == 7) and np.all(el == 7)
        assert lib.nbody_binaries(0.0, 0, C.byref(found), None, None, None) == 0 and found.value >= 0   # one entry point for both precisions


def test_c_host_program_binaries_lines(nb, ref):
    """`nbody N iters --binaries`: the count and the five binaries of the smallest a of the program's final state, against the reference
    on the same state (the engine takes the program's steps from the program's initial conditions).
    A DEVIATION from the issue, which asks for this check on the fixture: the program generates its own bodies and cannot load a state,
    so the state is the library's seeded N = 4096 system after 3 steps.  That this state holds at least five binaries (it holds over a
    thousand) is a property of the seed, asserted below so that a change of the generator shows here and not as an empty comparison."""
    exe = os.path.join(ROOT, "build", "nbody")
    n, iters = 4096, 3
    for flags, fp64 in (([], False), (["--fp64"], True)):
        r = subprocess.run([exe, str(n), str(iters), "--binaries"] + flags, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        count = re.findall(r"^binaries: (\d+)$", r.stdout, flags=re.M)
        lines = re.findall(r"^binary: (\d+) (\d+) (\S+) (\S+) (\S+)$", r.stdout, flags=re.M)
        assert len(count) == 1, r.stdout
        plain = subprocess.run([exe, str(n), str(iters)] + flags, capture_output=True, text=True, timeout=300)
        assert plain.returncode == 0 and "binar" not in plain.stdout
        strip = lambda text: [ln for ln in text.splitlines() if "Billion Interactions" not in ln and not ln.startswith("binar")]
        assert strip(r.stdout) == strip(plain.stdout)   # nothing else changes (the rate line carries a time)
        dtype = dtype_of(fp64)
        pos, vel = nb.make_bodies(n, dtype=dtype)
        with nb.NBody(n, fp64=fp64) as eng:
            eng.upload(pos, vel)
            eng.step(float(np.float32(0.01)), iters)   # the program's dt is the binary32 0.01 in fp64 contexts too
            now, vnow = eng.download()
        found, wi, wj, wel = ref.binaries(now, vnow)
        assert int(count[0]) == found and found >= 5
        order = sorted((k for k in range(found) if not math.isnan(wel[k][1])), key=lambda k: (wel[k][1], wi[k]))[:5]
        assert len(lines) == len(order)
        for (i, j, a, ecc, period), k in zip(lines, order):
            assert (int(i), int(j)) == (int(wi[k]), int(wj[k]))
            assert same(np.array([float(a), float(ecc), float(period)]), wel[k][1:]), (i, j)
