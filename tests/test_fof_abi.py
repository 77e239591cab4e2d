"""The friends-of-friends entry points (nbody_fof and its _d form; include/nbody.h "friends-of-friends groups") as far as no GPU is
needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement tests/fof_ref.c itself — against a
plain numpy fp64 brute force wherever no pair stands at the linking length within the rounding of d2, and on planted systems whose
groups are known by construction (exact ties at the linking length across a window and a block edge, coincident bodies, a NaN body,
b2 = 0 and b2 = +inf)."""
import ctypes as C

import numpy as np
import pytest

from fof_common import CHAIN_N, RATIOS, b2_for, chain, make_ref, numpy_fof, planted, round_bound

SYMBOLS = {"nbody_fof": 4, "nbody_fof_d": 4}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("fof_ref"))


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs, name
    assert callable(nb.NBody.fof)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    for name in SYMBOLS:
        group, out = np.full(4, 7, np.int32), np.full(2, 7, np.int32)
        fn = getattr(lib, name)
        assert fn(0.25, ip(group), ip(out[:1]), ip(out[1:])) == nb._lib.ERR_NOT_INIT
        assert fn(float("nan"), None, None, None) == nb._lib.ERR_NOT_INIT
        assert np.all(group == 7) and np.all(out == 7)


@pytest.mark.parametrize("n", [300, 1025, 2100])
def test_fof_ref_against_numpy(nb, ref, n):
    """Identical groups wherever no pair's fp64 d2 stands within the rounding of the statement's d2 of the linking length.  The
    statement's d2 carries at most five roundings relative to the exact value (tests/test_neighbors_abi.py derives it:
    |d2 - exact| <= 5 u d2, u = 2^-24 or 2^-53), so d2 <= b2 is decided alike on both sides when |d2 - b2| > 5 u (d2 + b2), twice over
    for the numpy side's own roundings: a pair is unclear when |d2 - b2| <= 10 u (d2 + b2).  With seed 42 no pair is unclear at any of
    the sizes, ratios and precisions here, which is asserted; in fp32 the smallest relative gap |d2 - b2| / (d2 + b2) over the twelve
    cases is 1.3e-5 against the threshold 10 u = 6e-7."""
    pos32 = nb.make_bodies(n, seed=42)[0]
    for dtype, u in ((np.float32, 2.0 ** -24), (np.float64, 2.0 ** -53)):
        pos = pos32.astype(dtype)
        for ratio in RATIOS:
            b2 = b2_for(n, ratio, dtype)
            want, unclear, gap = numpy_fof(pos, b2, u)
            print("%s n=%d ratio %.1f: %d unclear pairs, smallest relative gap %.3g, %d groups"
                  % (np.dtype(dtype).name, n, ratio, unclear, gap, len(np.unique(want))))
            assert unclear == 0, (dtype, ratio, gap)
            group, n_groups = ref.groups(pos, b2)
            assert group.dtype == np.int32 and np.array_equal(group, want), (dtype, ratio)
            assert n_groups == len(np.unique(want)) == int((group == np.arange(n)).sum())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_cases(nb, ref, dtype):
    n = 1100
    pos = planted(nb, n, dtype)
    h2 = dtype(2.0 ** -24)
    group, n_groups = ref.groups(pos, h2)
    # 64, 65, 500 and 1024 are all exactly h away from 63 (d2 == b2: linked), across a window edge and a block edge
    assert all(group[i] == 63 for i in (63, 64, 65, 500, 1024)) and int((group == 63).sum()) == 5
    assert all(group[i] == 3 for i in (3, 70, 900)) and int((group == 3).sum()) == 3
    assert group[200] == 200 and int((group == 200).sum()) == 1           # the NaN body is alone
    assert n_groups == int((group == np.arange(n)).sum())
    for b2 in (dtype(0), dtype(2.0 ** -40), dtype(1e-6)):                 # coincident bodies are linked at any b2 >= 0, b2 = 0 included
        group, _ = ref.groups(pos, b2)
        assert all(group[i] == 3 for i in (3, 70, 900)) and group[200] == 200
    group, n_groups = ref.groups(pos, dtype(0))
    assert n_groups == n - 2 and group[63] == 63 and group[64] == 64      # b2 = 0 links the coincident bodies and nothing else
    group, n_groups = ref.groups(pos, dtype(2.0 ** -25))                  # just below the ties: 63's friends are not linked
    assert all(group[i] == i for i in (63, 64, 65, 500, 1024))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_b2_inf_is_one_group_of_the_non_nan_bodies(nb, ref, dtype):
    n = 1100
    pos = planted(nb, n, dtype)
    group, n_groups = ref.groups(pos, dtype(np.inf))
    others = np.delete(np.arange(n), 200)
    assert np.all(group[others] == 0) and group[200] == 200 and n_groups == 2
    group, n_groups = ref.groups(nb.make_bodies(257, dtype=dtype)[0], dtype(np.inf))
    assert np.all(group == 0) and n_groups == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chains(ref, dtype):
    """the chain systems the GPU tests use are what fof_common says they are: the statement arrives at the groups of the construction"""
    pos, b2, want = chain(dtype)
    group, n_groups = ref.groups(pos, b2)
    assert np.array_equal(group, want) and n_groups == 1 and np.all(group == 0)
    pos, b2, want = chain(dtype, cut=True)
    group, n_groups = ref.groups(pos, b2)
    assert np.array_equal(group, want) and n_groups == 8 and len(np.unique(want)) == 8
    assert np.all(want <= np.arange(CHAIN_N)) and round_bound(CHAIN_N) == 13 and round_bound(1) == 1 and round_bound(2) == 2
