"""What the sixth-order block time step tests (test_hermite6_block_abi.py, test_gpu_hermite6_block.py) share: tests/hermite6_block_ref.c
compiled together with tests/snap_ref.c as hermite_block_common.compile_ref compiles its own (-ffp-contract=off), the trace it returns
(hermite_block_common.Trace, with its invariant), a plain numpy binary64 sixth-order block scheme with no stated order, and the figures
the energy bounds are taken from.  The system of the energy test, its run, equal_slices and shared_steps_for are hermite_block_common's."""
import ctypes as C
import os
import subprocess

import numpy as np

from field_common import ROOT
from hermite_block_common import ENERGY_RUN, Trace, energy_system, equal_slices, numpy_want, shared_steps_for   # noqa: F401 (re-exported)
from hermite_common import EPS

REF, MASS = 1, 2   # hermite6_block_ref.c's flags (hermite6_ref.c's)

# What the energy tests assert, and where their bounds come from: energy_system() under ENERGY_RUN (eta = 0.02, dt_max = 1/16, 8 levels,
# 16 blocks to t = 1), all figures from the CPU statements in binary64, printed and asserted by tests/test_hermite6_block_abi.py:
#   sixth-order block scheme (hermite6_block_ref.c; the plain numpy scheme below gives the same):  1839 sub-steps, 3876 row evaluations,
#                                                                                                  |dE/E| = 5.926e-07
#   fourth-order block scheme (hermite_block_ref.c), the same run and the same schedule:           |dE/E| = 1.583e-06   ratio 0.374
#   sixth-order shared dt (hermite6_ref.c) with as many row evaluations (496 steps):               |dE/E| = 1.093e-04   ratio 5.42e-3
# Against the fourth-order block run the condition is that the sixth-order one loses less: ratio < 1.  The measured 0.374 leaves a factor
# 2.7, not the 4 a bound with a margin would want (0.374 x 4 = 1.5 would let it lose MORE), so the condition itself is asserted: the
# statements are IEEE-exact in binary64, the figure does not move.  Why the gain is no larger on this run: the six distant bodies sit on
# level 0 (dt = 1/16, half a period of the inner pair) by the fourth-order ratio |a| / |j|, which does not see the pair's quadrupole;
# their error is not in the asymptotic regime of either order.  With dt_max = 1/64 on 6 levels (the same finest step, 4058 row
# evaluations instead of 3876) the sixth-order run loses 3.13e-8 against 1.53e-6, a ratio of 0.020; with eta = 0.04 on the run above the
# two lose 3.57e-6 and 3.09e-6, a ratio of 1.16: the level rule, not the order, limits it.
ENERGY_RATIO_BOUND_BLOCK4 = 1.0
# ... and against the shared sixth-order step the bound keeps a factor 9 on the measured ratio
ENERGY_RATIO_BOUND_SHARED6 = 5e-2
# Strict binary32 (hermite6_block_ref.c, float) on the same run: 1840 sub-steps, 3877 row evaluations, |dE/E| = 3.532e-06 (the
# reference's d2 form: 4.267e-06) — binary32 roundings of the state, not the scheme, set it.  The timed binary32 arithmetic on the device
# differs from the strict one by v_rsq_f32 (1 ulp), which can move a level choice: another schedule, the same order of error; the GPU
# test allows 4 x the figure.
ENERGY_STRICT_F32 = 3.532e-6
ENERGY_TIMED_F32_BOUND = 4 * ENERGY_STRICT_F32


def compile_ref(tmp_dir):
    """tests/hermite6_block_ref.c + tests/snap_ref.c as one shared library"""
    so = os.path.join(str(tmp_dir), "hermite6_block_ref.so")
    srcs = [os.path.join(ROOT, "tests", f) for f in ("hermite6_block_ref.c", "snap_ref.c")]
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], []):   # every operation is IEEE-exact: vector width and threads change no bit
        r = subprocess.run(["gcc", "-std=c11", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"] + extra + ["-o", so] + srcs + ["-lm"],
                           capture_output=True, timeout=180)
        if r.returncode == 0:
            return C.CDLL(so)
    raise RuntimeError("cannot compile tests/hermite6_block_ref.c: %s" % r.stderr.decode()[-2000:])


class Block6Ref:
    """tests/hermite6_block_ref.c: run() returns (pos, vel, substeps, row_evals, Trace)"""

    def __init__(self, lib):
        self.lib = lib

    def run(self, pos, vel, dtype, eta, dt_max, levels, nblocks, ref=False, mass=False, trace=True):
        p, v = np.array(pos, dtype, order="C"), np.array(vel, dtype, order="C")
        assert p.shape == v.shape and p.shape[1] == 4
        n = len(p)
        fp64 = np.dtype(dtype) == np.float64
        fn = getattr(self.lib, "hermite6_block_f64" if fp64 else "hermite6_block_f32")
        ct = C.c_double if fp64 else C.c_float
        ll, vp = C.c_longlong, C.c_void_p
        fn.argtypes = [vp, vp, C.c_int, C.c_int, ct, ct, C.c_int, C.c_int, C.POINTER(ll), C.POINTER(ll), vp, vp, vp, vp, vp, ll, ll]
        fn.restype = C.c_int
        cap_steps = nblocks << (levels - 1)
        cap_rows = cap_steps * n if trace else 0
        tau, count = np.zeros(cap_steps if trace else 0, np.int64), np.zeros(cap_steps if trace else 0, np.int32)
        rows, lev, level0 = np.zeros(cap_rows, np.int32), np.zeros(cap_rows, np.int32), np.zeros(n, np.int32)
        steps, evals = ll(), ll()
        tr = [a.ctypes.data if trace else None for a in (tau, count, rows, lev, level0)]
        flags = (REF if ref else 0) | (MASS if mass else 0)
        rc = fn(p.ctypes.data, v.ctypes.data, n, flags, float(dtype(eta)), float(dtype(dt_max)), levels, nblocks, C.byref(steps), C.byref(evals),
                *tr, cap_steps, cap_rows)
        assert rc == 0, "hermite6_block_ref: %d (the invariant or a capacity)" % rc
        s, e = steps.value, evals.value
        return p, v, s, e, (Trace(level0, tau[:s], count[:s], rows[:e], lev[:e]) if trace else None)


def numpy_ajs(r, v, acc=None, chunk=256):
    """(a, j, s), (n, 3) binary64 each: acceleration, jerk and snap over all other bodies in plain numpy, no stated order, beside
    hermite_common.numpy_aj.  acc: the bodies' accelerations that the snap takes (a predicted state's); None: those of (r, v) themselves,
    computed first — the two passes of nbody_snap_rows"""
    n = len(r)
    if acc is None:
        acc = numpy_ajs(r, v, np.zeros((n, 3)), chunk)[0]
    a, j, s = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 3))
    for i0 in range(0, n, chunk):
        i1 = min(i0 + chunk, n)
        d = r[None, :, :] - r[i0:i1, None, :]
        w = v[None, :, :] - v[i0:i1, None, :]
        g = acc[None, :, :] - acc[i0:i1, None, :]
        inv = 1.0 / np.sqrt((d * d).sum(2) + EPS)
        inv[np.arange(i1 - i0), np.arange(i0, i1)] = 0.0
        inv2 = inv * inv
        inv3 = (inv * inv2)[:, :, None]
        alpha = ((d * w).sum(2) * inv2)[:, :, None]
        beta = (((w * w).sum(2) + (d * g).sum(2)) * inv2)[:, :, None] + alpha * alpha
        t = w - 3.0 * alpha * d
        a[i0:i1] = (d * inv3).sum(1)
        j[i0:i1] = (t * inv3).sum(1)
        s[i0:i1] = ((g - 6.0 * alpha * t - 3.0 * beta * d) * inv3).sum(1)
    return a, j, s


def numpy_block6(pos, vel, eta, dt_max, levels, nblocks):
    """(pos, vel, substeps, row_evals): the sixth-order block scheme in plain numpy binary64, no stated order of the sums (numpy_ajs over
    all rows, the active ones kept), real-valued h from the integer ticks, the level rule of hermite_block_common.numpy_want"""
    p, u = np.array(pos, np.float64), np.array(vel, np.float64)
    n = len(p)
    x0, v0 = p[:, :3].copy(), u[:, :3].copy()
    a0, j0, s0 = numpy_ajs(x0, v0)
    c0 = np.zeros((n, 3))
    unit = dt_max / (1 << (levels - 1))
    t0, lev = np.zeros(n, np.int64), numpy_want(a0, j0, eta, dt_max, levels)
    end, tau, steps, evals = nblocks << (levels - 1), 0, 0, 0
    while tau < end:
        step = np.int64(1) << (levels - 1 - lev)
        assert (t0 % step == 0).all()
        tau = int((t0 + step).min())
        act = np.flatnonzero(t0 + step == tau)
        h = ((tau - t0) * unit)[:, None]
        xp = x0 + v0 * h + a0 * (h ** 2 / 2) + j0 * (h ** 3 / 6) + s0 * (h ** 4 / 24) + c0 * (h ** 5 / 120)
        vp = v0 + a0 * h + j0 * (h ** 2 / 2) + s0 * (h ** 3 / 6) + c0 * (h ** 4 / 24)
        ap = a0 + j0 * h + s0 * (h ** 2 / 2) + c0 * (h ** 3 / 6)
        a1, j1, s1 = numpy_ajs(xp, vp, ap)
        h, a1, j1, s1 = h[act], a1[act], j1[act], s1[act]
        b0, d0, e0 = a0[act], j0[act], s0[act]
        v1 = v0[act] + (b0 + a1) * (h / 2) + (d0 - j1) * (h ** 2 / 10) + (e0 + s1) * (h ** 3 / 120)
        x1 = x0[act] + (v0[act] + v1) * (h / 2) + (b0 - a1) * (h ** 2 / 10) + (d0 + j1) * (h ** 3 / 120)
        c1 = (60 * (a1 - b0) / h ** 3 - (36 * j1 + 24 * d0) / h ** 2 + (9 * s1 - 3 * e0) / h)
        x0[act], v0[act], a0[act], j0[act], s0[act], c0[act], t0[act] = x1, v1, a1, j1, s1, c1, tau
        w, k = numpy_want(a1, j1, eta, dt_max, levels), lev[act]
        down = (w < k) & (tau % (np.int64(1) << (levels - np.maximum(k, 1))) == 0)
        lev[act] = np.where(w > k, w, np.where(down, k - 1, k))
        steps += 1
        evals += len(act)
    assert (t0 == end).all()
    p[:, :3], u[:, :3] = x0, v0
    return p, u, steps, evals


# The bit-for-bit cases of the GPU tests: eta = 0.04, dt_max = 1/64, two blocks, on 1, 3 and 8 levels, at N = 1 (a lone body: level 0),
# 2 (the Kepler pair of e = 0.9), 8 (energy_system), 257 (a tail of one row behind a 256-row tile) and 611.  What they exercise is
# asserted from the statement's trace on 8 levels in tests/test_hermite6_block_abi.py: at N = 611 all 8 levels occupied, a sub-step
# of one row, sub-steps of all rows, an active list across a 256-row tile edge and, for equal_slices(611, 3), sub-steps in which a slice
# has no active row; N = 257 has those too (and idles a slice in more sub-steps), so the layout tests run at the smaller size.
GPU_CASE = dict(eta=0.04, dt_max=1.0 / 64, nblocks=2)
GPU_LEVELS = (1, 3, 8)
GPU_SIZES = (1, 2, 8, 257, 611)


def case_bodies(nb, n, dtype):
    """the bodies of a bit-for-bit case, with canaries in the fourth value of both words where the system is make_bodies': a call
    must carry them bit for bit"""
    from hermite_common import kepler
    if n == 2:
        return kepler(0.9, dtype)
    if n == 8:
        return energy_system(dtype)
    pos, vel = nb.make_bodies(n, dtype=dtype)
    pos[:, 3] = (np.arange(n) % 977).astype(dtype) - dtype(7.5)
    vel[:, 3] = (np.arange(n) % 31).astype(dtype) + dtype(0.25)
    return pos, vel


def row_traces(trace, n):
    """per row below n the list of (tau, level it goes on with) of the sub-steps in which it is active, and its first level"""
    out = [[] for _ in range(n)]
    for tau, rows, levels in zip(trace.tau, trace.rows, trace.levels):
        for r, l in zip(rows.tolist(), levels.tolist()):
            if r < n:
                out[r].append((int(tau), l))
    return trace.level0[:n].tolist(), out
