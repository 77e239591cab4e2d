"""The mutual pairing of the fp32 force pass on the device (include/nbody.h NBODY_OPT_PAIRING): every unordered pair is
evaluated once, and the pass returns THE BITS of the ordered pass of the same engine and options.

The bar is equality of the uint32 views, never a tolerance: forces, and positions and velocities after three steps, NBODY_PAIRING_MUTUAL
against NBODY_PAIRING_ORDERED.  The one exception is the contract's own: the mirrored side negates a coordinate difference with the operand
modifier (it does not subtract a second time), so where an output is a NaN its sign and payload may differ — for the systems that hold a NaN
or an infinity (every output word of theirs is non-finite) the bar is that the SET of non-finite output words is the same, and that every
finite word has the same bits.

Shapes are N = 1024 nb with the segmentation forced (NBODY_OPT_JSUB, NBODY_OPT_WSPLIT) so that every piece is a whole number of blocks:
  nb = 1   the diagonal unit alone                      nb = 2   only the half offset d = nb / 2
  nb = 3   an odd count: d = 1 for every row block       nb = 4   four pieces of one block each (wave split 4)
  nb = 8   two segments of four blocks (level 2 and the segment join)
  nb = 16  two segments, four pieces each, two blocks per piece (levels 2, 3 and 4)
  nb = 20  more partner blocks (10) than a unit's run (8): a row block spans two units, and the blocks wrap past nb
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT, STEPS = 0.01, 3

#        nb  jsub wsplit
SHAPES = [(1, 1, 1), (2, 2, 1), (3, 3, 1), (4, 1, 4), (8, 2, 1), (16, 2, 4), (20, 1, 4)]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def systems(nb, n):
    """name -> (pos, vel, exact): exact = every output must have the ordered pass's bits; else the NaN limit of the contract"""
    out = {}
    pos, vel = nb.make_bodies(n)
    out["cloud"] = (pos, vel, True)
    # coincident bodies (d2 = eps, the +-0 terms) inside a lane's 16 rows, across lanes, across blocks where there are several, and a
    # cluster at 1e-4 spacing
    p, v = pos.copy(), vel.copy()
    for a, b in ((3, 4), (15, 16), (100, 900), (0, n - 1), (1023, n // 2), (5, 5 + 1024 * (n // 2048))):
        p[b, :3] = p[a, :3]
    k = np.arange(40)
    p[200:240, 0] = p[200, 0] + 1e-4 * k
    p[200:240, 1] = p[200, 1] - 1e-4 * (k % 7)
    p[200:240, 2] = p[200, 2]
    out["coincident"] = (p, v, True)
    p, v = pos.copy(), vel.copy()
    p[n // 3, 1] = np.inf
    out["inf"] = (p, v, False)
    p, v = pos.copy(), vel.copy()
    p[(2 * n) // 3, 2] = np.nan
    out["nan"] = (p, v, False)
    return out


def same(a, b, exact, what):
    ua, ub = u32(a), u32(b)
    if exact:
        assert np.array_equal(ua, ub), "%s: %d words differ" % (what, int((ua != ub).sum()))
        return
    fa, fb = np.isfinite(a), np.isfinite(b)
    assert np.array_equal(fa, fb), "%s: the sets of non-finite words differ" % what
    assert np.array_equal(ua[fa], ub[fb]), "%s: finite words differ" % what


def run(nb, eng, pairing, pos, vel):
    eng.set_option(nb.OPT_PAIRING, pairing)
    f = eng.forces(pos)
    eng.upload(pos, vel)
    eng.step(DT, STEPS)
    p, v = eng.download()
    return f, p, v


@pytest.mark.parametrize("blocks,jsub,wsplit", SHAPES)
def test_mutual_pairing_returns_the_ordered_bits(nb, blocks, jsub, wsplit):
    n = 1024 * blocks
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_JSUB, jsub)
        eng.set_option(nb.OPT_WSPLIT, wsplit)
        cfg = eng.config
        assert cfg["nseg"] == jsub and cfg["wsplit"] == wsplit and cfg["sum_block"] == 1024 and cfg["pairing"] == "ordered", cfg
        ordered_launches = cfg["launches_per_step"]   # (two where the ordered pass of a small launch adds its segments in a combine kernel)
        for name, (pos, vel, exact) in systems(nb, n).items():
            want = run(nb, eng, nb.PAIRING_ORDERED, pos, vel)
            got = run(nb, eng, nb.PAIRING_MUTUAL, pos, vel)
            cfg = eng.config
            assert cfg["pairing"] == "mutual" and cfg["launches_per_step"] == 1 and cfg["variant"] == "isa", cfg   # the rows are finished inside the one launch
            for w, g, what in zip(want, got, ("forces", "positions", "velocities")):
                same(g, w, exact, "nb = %d, %s, %s" % (blocks, name, what))
            if exact:
                assert np.isfinite(got[0]).all()
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_AUTO)      # below 2^20 rows: ordered
        cfg = eng.config
        assert cfg["pairing"] == "ordered" and cfg["launches_per_step"] == ordered_launches, cfg


def test_graph_replay_equals_eager_launches(nb):
    n = 4096
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_JSUB, 2)
        eng.set_option(nb.OPT_WSPLIT, 1)
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_MUTUAL)
        out = {}
        for graph in (0, 1):
            eng.set_option(nb.OPT_GRAPH, graph)
            eng.upload(pos, vel)
            eng.step(DT, 9)          # graph = 1: one eager step, then captured pairs of steps
            out[graph] = eng.download()
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_ORDERED)
        eng.upload(pos, vel)
        eng.step(DT, 9)
        ordered = eng.download()
        for k, what in enumerate(("positions", "velocities")):
            assert np.array_equal(u32(out[0][k]), u32(out[1][k])), what
            assert np.array_equal(u32(out[1][k]), u32(ordered[k])), what
        # one launch, one timed span per step
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_MUTUAL)
        eng.set_option(nb.OPT_TIMING, 1)
        eng.kernel_time(reset=True)
        eng.step(DT, 3)
        ms, spans = eng.kernel_time(reset=True)
        assert spans == 3 and ms > 0.0


def unsupported(nb, fn):
    with pytest.raises(nb.NBodyError) as e:
        fn()
    assert e.value.code == nb._lib.ERR_UNSUPPORTED
    return True


def test_forced_on_an_ineligible_pass_is_refused(nb):
    n = 2048
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_JSUB, 1)
        eng.set_option(nb.OPT_WSPLIT, 1)
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_MUTUAL)
        eng.upload(pos, vel)
        before = eng.download()
        full = eng.forces_rows(0, n)                                   # all rows: a full pass
        assert np.array_equal(u32(full), u32(eng.forces(pos)))
        assert unsupported(nb, lambda: eng.forces_rows(1, n - 1))      # a window of rows
        # pieces that are not whole blocks; another block length; the strict and the reference arithmetic; the FPGA order
        for key, bad, good in ((nb.OPT_JSUB, 3, 1), (nb.OPT_WSPLIT, 16, 1), (nb.OPT_SUM_BLOCK, 512, 1024), (nb.OPT_ARITH, nb.ARITH_STRICT, nb.ARITH_FMA3),
                               (nb.OPT_ARITH, nb.ARITH_REFERENCE, nb.ARITH_FMA3), (nb.OPT_SUM_ORDER, nb.SUM_SEQ, nb.SUM_BLOCKED),
                               (nb.OPT_JSLICES, 3, 1)):
            eng.set_option(key, bad)
            assert eng.config["pairing"] == "ordered"
            assert unsupported(nb, lambda: eng.step(DT, 1)) and unsupported(nb, lambda: eng.forces(pos))
            eng.set_option(key, good)
            assert eng.config["pairing"] == "mutual"
        eng.use_masses(True)                                            # the force path is unit-mass
        assert unsupported(nb, lambda: eng.step(DT, 1))
        eng.use_masses(False)
        after = eng.download()
        for b, a in zip(before, after):                                 # nothing was launched
            assert np.array_equal(u32(b), u32(a))
        eng.step(DT, 1)
    with nb.NBody(n + 100) as eng:                                      # N is not a multiple of 1024
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_MUTUAL)
        assert eng.config["pairing"] == "ordered" and unsupported(nb, lambda: eng.step(DT, 1))
    with nb.NBody(n, fp64=True) as eng:                                 # fp64
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_MUTUAL)
        assert eng.config["pairing"] == "ordered" and unsupported(nb, lambda: eng.step(DT, 1))
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_AUTO)
        eng.step(DT, 1)
