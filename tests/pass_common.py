"""What the tests of the diagnostic passes (energy, field, neighbours, knn, friends-of-friends) and the parity tests share: the bit
comparison, the force configurations no pass may depend on, and the check that a pass between the steps leaves the step alone."""
import numpy as np

import mini_nbody_amd as nb


def bits(a):
    """the words of a binary32 / binary64 array or scalar (anything else as it is)"""
    a = np.asarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same(got, want):
    """An array against an array, or a tuple of arrays against a tuple of as many: the same shapes, the same dtypes, integers equal,
    floats the same bits; an entry may be None only where the other one is."""
    if isinstance(got, (tuple, list)) != isinstance(want, (tuple, list)):
        return False
    if not isinstance(got, (tuple, list)):
        got, want = (got,), (want,)
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if g is None or w is None:
            if not (g is None and w is None):
                return False
            continue
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype or not np.array_equal(bits(g), bits(w)):
            return False
    return True


# (option, value, the default to put back): every way to lay the FORCE pass out; no diagnostic pass may follow any of them
FORCE_CONFIGS = ((nb.OPT_VARIANT, nb.VARIANT_SMEM, nb.VARIANT_AUTO), (nb.OPT_VARIANT, nb.VARIANT_LDS, nb.VARIANT_AUTO),
                 (nb.OPT_VARIANT, nb.VARIANT_READLANE, nb.VARIANT_AUTO), (nb.OPT_JSUB, 3, 0), (nb.OPT_JSLICES, 3, 0),
                 (nb.OPT_WSPLIT, 1, -1), (nb.OPT_WSPLIT, 16, -1), (nb.OPT_SUM_ORDER, nb.SUM_SEQ, nb.SUM_BLOCKED),
                 (nb.OPT_SUM_ORDER, nb.SUM_FPGA16, nb.SUM_BLOCKED))

PLANS = (([1] * 12, 0, False), ([64, 64, 6, 64], 1, False), ([3, 5, 2], 0, True))   # (steps per call, NBODY_OPT_GRAPH, count launches)


def run_steps(nb, n, pos, vel, plan, graph, probe, timing=False):
    """the steps of `plan` with probe(eng) after every call (None: nothing) -> positions, velocities, force launches counted"""
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_GRAPH, graph)
        if timing:
            eng.set_option(nb.OPT_TIMING, 1)
        eng.upload(pos, vel)
        for k in plan:
            eng.step(0.01, k)
            if probe:
                probe(eng)
        p, v = eng.download()
        launches = eng.kernel_time()[1] if timing else None
    return p, v, launches


def check_step_untouched(nb, monkeypatch, n, probe, split_env, plans=PLANS):
    """A pass's calls between the steps change neither the state nor the count of force launches: eager steps, graph replays and the
    timed form, with the pass's source split left to the library and forced to 2 (scratch and combine between the steps too)."""
    pos, vel = nb.make_bodies(n)
    for plan, graph, timing in plans:
        monkeypatch.delenv(split_env, raising=False)
        a = run_steps(nb, n, pos, vel, plan, graph, None, timing)
        for split in (None, "2"):
            if split:
                monkeypatch.setenv(split_env, split)
            b = run_steps(nb, n, pos, vel, plan, graph, probe, timing)
            assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), (plan, graph, split)
            assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), (plan, graph, split)
            assert a[2] == b[2], "the pass's launches were counted by nbody_kernel_time (%s=%s)" % (split_env, split)
