"""What the block time step tests (test_hermite_block_abi.py, test_gpu_hermite_block.py) share: tests/hermite_block_ref.c compiled
together with tests/jerk_ref.c as hermite_common.compile_ref compiles its own (-ffp-contract=off), the trace it returns, a plain numpy
binary64 block scheme with no stated order, the system of the energy test, and what the GPU tests assert of their inputs from a trace:
occupied levels, one-row and all-row sub-steps, an active list across a workgroup edge, a slice without an active row."""
import ctypes as C
import os
import subprocess

import numpy as np

from field_common import ROOT
from hermite_common import numpy_aj

ENERGY_RUN = dict(eta=0.02, dt_max=1.0 / 16, levels=8, nblocks=16)   # the run of the energy test: to t = 1
# What the energy test asserts, and where its bound comes from.  Plain numpy binary64 (numpy_block below): 1839 sub-steps, 3876 row
# evaluations (0.263 of sub-steps x N), |dE/E| = 1.58e-6; a shared dt with as many row evaluations rounded up to a multiple of 16 steps
# (496 steps) loses 2.90e-3, the ratio is 5.45e-4 (480 steps: 3.42e-3 and 4.6e-4).  hermite_block_ref.c in binary64 gives the same counters and figures (asserted in
# test_hermite_block_abi.py, which prints them); the bound 1e-2 keeps a factor 18.
ENERGY_RATIO_BOUND = 1e-2


def compile_ref(tmp_dir):
    """tests/hermite_block_ref.c + tests/jerk_ref.c as one shared library"""
    so = os.path.join(str(tmp_dir), "hermite_block_ref.so")
    srcs = [os.path.join(ROOT, "tests", f) for f in ("hermite_block_ref.c", "jerk_ref.c")]
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], []):   # every operation is IEEE-exact: vector width and threads change no bit
        r = subprocess.run(["gcc", "-std=c11", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"] + extra + ["-o", so] + srcs + ["-lm"],
                           capture_output=True, timeout=180)
        if r.returncode == 0:
            return C.CDLL(so)
    raise RuntimeError("cannot compile tests/hermite_block_ref.c: %s" % r.stderr.decode()[-2000:])


class Trace:
    """level0: the first levels; tau, count: per sub-step; rows, levels: per sub-step the active rows (ascending) and the level each
    goes on with"""

    def __init__(self, level0, tau, count, rows, levels):
        self.level0, self.tau, self.count = level0, tau, count
        at = np.concatenate(([0], np.cumsum(count)))
        self.rows = [rows[at[s]:at[s + 1]] for s in range(len(count))]
        self.levels = [levels[at[s]:at[s + 1]] for s in range(len(count))]

    def check_invariant(self, n, n_levels, nblocks):
        """every t0_i a multiple of s_i at every sub-step, tau strictly ascending, every row active at every multiple of 2^(levels - 1),
        nothing steps over one, and the end is nblocks of them"""
        t0, lev = np.zeros(n, np.int64), self.level0.copy()
        top, last = 1 << (n_levels - 1), 0
        for s, tau in enumerate(self.tau):
            step = np.int64(1) << (n_levels - 1 - lev)
            assert (t0 % step == 0).all() and tau > last and tau == (t0 + step).min()
            assert np.array_equal(self.rows[s], np.flatnonzero(t0 + step == tau))
            assert (t0 + step <= (t0 // top + 1) * top).all()
            if tau % top == 0:
                assert len(self.rows[s]) == n
            t0[self.rows[s]] = tau
            lev[self.rows[s]] = self.levels[s]
            assert ((lev >= 0) & (lev < n_levels)).all()
            last = tau
        assert last == nblocks * top and (t0 == last).all()

    def occupied_levels(self):
        seen = set(self.level0.tolist())
        for l in self.levels:
            seen |= set(l.tolist())
        return len(seen)

    def idle_substeps(self, slices):
        """the sub-steps in which at least one of the slices [(first, count), ...] has no active row"""
        return [s for s, rows in enumerate(self.rows) if any(not ((rows >= f) & (rows < f + c)).any() for f, c in slices if c > 0)]

    def crosses_tile_edge(self, tile=256):
        """some sub-step short of all rows whose active list has rows on both sides of a multiple of `tile`"""
        n = len(self.level0)
        return any(len(r) < n and len(set((r // tile).tolist())) > 1 for r in self.rows)


def equal_slices(n, parts):
    """contiguous equal slices as the engine lays N rows over `parts` devices or ranks (the first N mod parts get one row more; a
    context reports its own as first_body and n_local): [(first, count), ...]"""
    base, rem = divmod(n, parts)
    edges = [p * base + min(p, rem) for p in range(parts + 1)]
    return [(edges[p], edges[p + 1] - edges[p]) for p in range(parts)]


class BlockRef:
    """tests/hermite_block_ref.c: run() returns (pos, vel, substeps, row_evals, Trace)"""

    def __init__(self, lib):
        self.lib = lib

    def run(self, pos, vel, dtype, eta, dt_max, levels, nblocks, ref=False, trace=True):
        p, v = np.array(pos, dtype, order="C"), np.array(vel, dtype, order="C")
        assert p.shape == v.shape and p.shape[1] == 4
        n = len(p)
        fp64 = np.dtype(dtype) == np.float64
        fn = getattr(self.lib, "hermite_block_f64" if fp64 else "hermite_block_f32")
        ct = C.c_double if fp64 else C.c_float
        ll, vp = C.c_longlong, C.c_void_p
        fn.argtypes = [vp, vp, C.c_int, C.c_int, ct, ct, C.c_int, C.c_int, C.POINTER(ll), C.POINTER(ll), vp, vp, vp, vp, vp, ll, ll]
        fn.restype = C.c_int
        cap_steps = nblocks << (levels - 1)
        cap_rows = cap_steps * n
        tau, count = np.zeros(cap_steps, np.int64), np.zeros(cap_steps, np.int32)
        rows, lev, level0 = np.zeros(cap_rows, np.int32), np.zeros(cap_rows, np.int32), np.zeros(n, np.int32)
        steps, evals = ll(), ll()
        tr = [a.ctypes.data if trace else None for a in (tau, count, rows, lev, level0)]
        rc = fn(p.ctypes.data, v.ctypes.data, n, int(ref), float(dtype(eta)), float(dtype(dt_max)), levels, nblocks, C.byref(steps), C.byref(evals),
                *tr, cap_steps, cap_rows)
        assert rc == 0, "hermite_block_ref: %d (the invariant or a capacity)" % rc
        s, e = steps.value, evals.value
        return p, v, s, e, (Trace(level0, tau[:s], count[:s], rows[:e], lev[:e]) if trace else None)


def numpy_want(a, j, eta, dt_max, levels):
    """the wanted levels from (a, j), (n, 3) each: the smallest k with dt_max 2^-k <= eta |a| / |j|, in the squared form"""
    with np.errstate(all="ignore"):
        q = (a * a).sum(1) / (j * j).sum(1)
    lim = (dt_max * 0.5 ** np.arange(levels)) ** 2
    e = eta * eta * q
    want = np.full(len(a), levels - 1)
    for k in range(levels - 1, -1, -1):
        want[lim[k] <= e] = k
    want[~(q < np.inf)] = 0
    return want


def numpy_block(pos, vel, eta, dt_max, levels, nblocks):
    """(pos, vel, substeps, row_evals): the block scheme in plain numpy binary64, no stated order of the sums (numpy_aj over all rows,
    the active ones kept), real-valued h from the integer ticks"""
    p, u = np.array(pos, np.float64), np.array(vel, np.float64)
    n = len(p)
    x0, v0 = p[:, :3].copy(), u[:, :3].copy()
    a0, j0 = numpy_aj(x0, v0)
    unit = dt_max / (1 << (levels - 1))
    t0, lev = np.zeros(n, np.int64), numpy_want(a0, j0, eta, dt_max, levels)
    end, tau, steps, evals = nblocks << (levels - 1), 0, 0, 0
    while tau < end:
        step = np.int64(1) << (levels - 1 - lev)
        assert (t0 % step == 0).all()
        tau = int((t0 + step).min())
        act = np.flatnonzero(t0 + step == tau)
        h = ((tau - t0) * unit)[:, None]
        xp = x0 + v0 * h + a0 * (h * h / 2) + j0 * (h ** 3 / 6)
        vp = v0 + a0 * h + j0 * (h * h / 2)
        a1, j1 = numpy_aj(xp, vp)
        h, a1, j1 = h[act], a1[act], j1[act]
        v1 = v0[act] + (a0[act] + a1) * (h / 2) + (j0[act] - j1) * (h * h / 12)
        x1 = x0[act] + (v0[act] + v1) * (h / 2) + (a0[act] - a1) * (h * h / 12)
        x0[act], v0[act], a0[act], j0[act], t0[act] = x1, v1, a1, j1, tau
        w, k = numpy_want(a1, j1, eta, dt_max, levels), lev[act]
        down = (w < k) & (tau % (np.int64(1) << (levels - np.maximum(k, 1))) == 0)
        lev[act] = np.where(w > k, w, np.where(down, k - 1, k))
        steps += 1
        evals += len(act)
    assert (t0 == end).all()
    p[:, :3], u[:, :3] = x0, v0
    return p, u, steps, evals


def energy_system(dtype=np.float64):
    """(pos, vel) words, N = 8 unit masses: a binary of a = 0.1, e = 0.5 at pericentre and six distant bodies on near-circular orbits,
    the mean velocity taken out"""
    pos, vel = np.zeros((8, 4)), np.zeros((8, 4))
    pos[0, 0], pos[1, 0] = -0.025, 0.025
    vel[0, 1], vel[1, 1] = -np.sqrt(60.0) / 2, np.sqrt(60.0) / 2
    for k in range(6):
        r, th = 2 + 0.1 * k, 2 * np.pi * k / 6
        pos[2 + k, :3] = (r * np.cos(th), r * np.sin(th), 0.05 * k)
        vel[2 + k, :3] = np.sqrt(3.5 / r) * np.array([-np.sin(th), np.cos(th), 0.0])
    vel[:, :3] -= vel[:, :3].mean(0)
    return pos.astype(dtype), vel.astype(dtype)


def shared_steps_for(row_evals, n):
    """the shared-dt run the block call is held against: as many row evaluations, rounded up to a multiple of 16 steps to t = 1"""
    return -(-row_evals // (n * 16)) * 16
