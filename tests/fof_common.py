"""What the friends-of-friends tests (test_fof_abi.py, test_gpu_fof.py) share: tests/fof_ref.c compiled as the field tests compile
field_ref.c, a plain numpy fp64 brute force, the linking lengths in units of the mean spacing, and the chain systems whose groups are
known by construction.  planted comes from neighbors_common."""
import ctypes as C
import math

import numpy as np

from field_common import compile_ref
from neighbors_common import planted  # noqa: F401

RATIOS = (0.3, 0.7, 0.9, 1.5)   # linking lengths in mean spacings: mostly singles, around the percolation threshold, one big group


class FofRef:
    """tests/fof_ref.c: (group, n_groups) from every pair once and a union-find whose root is the lowest index"""

    def __init__(self, lib):
        self.lib = lib

    def groups(self, pos, b2):
        dtype = pos.dtype.type
        pos = np.ascontiguousarray(pos)
        fn = self.lib.fof_f64 if dtype == np.float64 else self.lib.fof_f32
        fn.argtypes = [C.c_void_p, C.c_int, C.c_double if dtype == np.float64 else C.c_float, C.c_void_p]
        fn.restype = C.c_int
        group = np.empty(len(pos), np.int32)
        n_groups = fn(pos.ctypes.data_as(C.c_void_p), len(pos), float(dtype(b2)), group.ctypes.data_as(C.c_void_p))
        return group, n_groups


def make_ref(tmp_dir):
    return FofRef(compile_ref(tmp_dir, "fof_ref"))


def b2_for(n, ratio, dtype=np.float32):
    """the square, in dtype, of `ratio` mean spacings of n bodies uniform in [-1, 1)^3 (mean spacing 2 / n^(1/3))"""
    return dtype((ratio * 2.0 / n ** (1.0 / 3.0)) ** 2)


def round_bound(n):
    """the most link passes a call may take: ceil(log2 n) + 1"""
    return (math.ceil(math.log2(n)) if n > 1 else 0) + 1


def lowest_index_labels(n, pairs):
    """group[i] = the lowest index of i's connected component under the given (i, j) links: a plain union-find"""
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i

    for i, j in pairs:
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], np.int32)


def numpy_fof(pos, b2, u):
    """plain numpy fp64: (group, number of unclear pairs, smallest relative gap) — the groups of d2 <= b2 with d2 the fp64 squared
    distance of the positions as given; a pair is unclear when |d2 - b2| <= 10 u (d2 + b2)"""
    p = pos[:, :3].astype(np.float64)
    n = len(p)
    b2 = float(b2)
    d2 = ((p[:, None, :] - p[None, :, :]) ** 2).sum(2)
    iu = np.triu_indices(n, 1)
    v = d2[iu]
    rel = np.abs(v - b2) / (v + b2)
    unclear = int((rel <= 10 * u).sum())
    linked = v <= b2
    return lowest_index_labels(n, zip(iu[0][linked], iu[1][linked])), unclear, float(rel.min())


CHAIN_N = 2100
CHAIN_H = 2.0 ** -6   # spacing: k * h and h * h are exact in either precision for every k < 2^12


def chain(dtype=np.float32, cut=False, seed=11):
    """(pos, b2, group): CHAIN_N bodies on a line along x at spacing h, body perm[k] at k * h for a fixed permutation, so that a
    component's links cross every window, block and chunk; b2 = h * h, which links exactly the neighbours on the line (the next but one
    is at 4 h * h).  One group with label 0.  cut: every 300th link is cut by moving one body away — the bodies at places 300, 600,
    ..., 1800 of the line all go to the one point (0, 64, 0), where they coincide and so form a group of their own at any b2 >= 0 —
    which leaves the seven pieces [0, 300), (300, 600), ..., (1800, 2100) of the line and the far group: eight groups, each labelled
    with its lowest body index."""
    perm = np.random.default_rng(seed).permutation(CHAIN_N)
    pos = np.zeros((CHAIN_N, 4), dtype)
    pos[perm, 0] = np.arange(CHAIN_N) * CHAIN_H
    pos[:, 3] = 1.0
    group = np.zeros(CHAIN_N, np.int32)
    if cut:
        moved = np.arange(300, CHAIN_N, 300)
        pos[perm[moved], :3] = (0.0, 64.0, 0.0)
        group[perm[moved]] = perm[moved].min()
        for a in range(0, CHAIN_N, 300):
            piece = perm[a + (1 if a else 0):a + 300]
            group[piece] = piece.min()
    return pos, dtype(CHAIN_H * CHAIN_H), group
