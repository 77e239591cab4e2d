"""The generated unit loop of the mutual pairing on the device (tools/gen_mutual_loop.py): what the seven shapes of
test_gpu_mutual.py do not reach.  The bar and the helpers are that file's: uint32 equality of forces, and of positions and velocities after
three steps, NBODY_PAIRING_MUTUAL against NBODY_PAIRING_ORDERED; the NaN limit only for the systems that hold a NaN or an infinity.

  nb = 17   mutual_max_d = 8: every row block has one unit of exactly kRun partners, and the stream wraps past nb for most A
  nb = 18   9 partners: a full run plus a run of one block; the half offset d = 9 only for A < 9, so the second run has count 1 or 0
  nb = 4    a system with coincident pairs and 1e-4 clusters on the rows either side of every DPP row boundary of the array (255/256, 511/512,
            767/768), on rows 0 and 1023 of every block (lane 0's injection, lane 63's exit) and on the first and last source of a block:
            where a wrong wait state, shift or mask would show
  nb = 17   nine steps replayed from a captured graph: equal to eager launches and to the ordered pass
"""
import numpy as np
import pytest

from test_gpu_mutual import DT, STEPS, run, same, systems, u32

pytestmark = pytest.mark.gpu


def compare(nb, eng, named):
    for name, (pos, vel, exact) in named.items():
        want = run(nb, eng, nb.PAIRING_ORDERED, pos, vel)
        got = run(nb, eng, nb.PAIRING_MUTUAL, pos, vel)
        cfg = eng.config
        assert cfg["pairing"] == "mutual" and cfg["launches_per_step"] == 1 and cfg["variant"] == "isa", cfg
        for w, g, what in zip(want, got, ("forces", "positions", "velocities")):
            same(g, w, exact, "%s, %s" % (name, what))
        if exact:
            assert np.isfinite(got[0]).all()


@pytest.mark.parametrize("blocks", [17, 18])
def test_full_and_short_runs_return_the_ordered_bits(nb, blocks):
    n = 1024 * blocks
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_JSUB, 1)
        eng.set_option(nb.OPT_WSPLIT, 1)
        cfg = eng.config
        assert cfg["nseg"] == 1 and cfg["wsplit"] == 1 and cfg["sum_block"] == 1024, cfg
        compare(nb, eng, systems(nb, n))


def boundary_system(nb, n):
    pos, vel = nb.make_bodies(n)
    p = pos.copy()
    blocks = n // 1024
    k = np.arange(8, dtype=np.float32)
    for b in range(blocks):
        base, nxt = 1024 * b, 1024 * ((b + 1) % blocks)
        # 1e-4 clusters of eight rows around each boundary (the lanes either side of it), and at both ends of the block
        for c in (252, 508, 764, 0, 1016):
            p[base + c:base + c + 8, 0] = p[base + c, 0] + 1e-4 * k
            p[base + c:base + c + 8, 1] = p[base + c, 1] - 1e-4 * (k % 3)
            p[base + c:base + c + 8, 2] = p[base + c, 2]
        # coincident pairs across each boundary inside the block, across the block's ends, and with the next block: its first and last source
        for a, c in ((base + 255, base + 256), (base + 511, base + 512), (base + 767, base + 768), (base, base + 1023),
                     (base + 1, nxt + 1022), (base + 1023, nxt), (base + 256, nxt + 272), (base + 768, nxt + 752)):
            p[c, :3] = p[a, :3]
    return {"boundaries": (p, vel, True)}


def test_lane_and_block_boundaries_return_the_ordered_bits(nb):
    n = 4096
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_JSUB, 1)
        eng.set_option(nb.OPT_WSPLIT, 4)
        cfg = eng.config
        assert cfg["nseg"] == 1 and cfg["wsplit"] == 4 and cfg["sum_block"] == 1024, cfg
        named = boundary_system(nb, n)
        p = named["boundaries"][0]
        assert np.array_equal(p[255, :3], p[256, :3]) and np.array_equal(p[1023, :3], p[1024, :3]) and np.array_equal(p[1024, :3], p[2047, :3])
        compare(nb, eng, named)


def test_graph_replay_at_a_full_run(nb):
    n = 1024 * 17
    pos, vel = nb.make_bodies(n)
    with nb.NBody(n) as eng:
        eng.set_option(nb.OPT_JSUB, 1)
        eng.set_option(nb.OPT_WSPLIT, 1)
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_MUTUAL)
        out = {}
        for graph in (0, 1):
            eng.set_option(nb.OPT_GRAPH, graph)
            eng.upload(pos, vel)
            eng.step(DT, 9)          # graph = 1: one eager step, then captured pairs of steps
            assert eng.config["pairing"] == "mutual"
            out[graph] = eng.download()
        eng.set_option(nb.OPT_PAIRING, nb.PAIRING_ORDERED)
        eng.upload(pos, vel)
        eng.step(DT, 9)
        ordered = eng.download()
        for k, what in enumerate(("positions", "velocities")):
            assert np.array_equal(u32(out[0][k]), u32(out[1][k])), what
            assert np.array_equal(u32(out[1][k]), u32(ordered[k])), what
