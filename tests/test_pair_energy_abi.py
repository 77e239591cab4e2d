"""The pair binding-energy entry points (nbody_pair_energy_rows(_d), nbody_binaries; include/nbody.h "pair binding energies and
binaries") as far as no GPU is needed: the symbols and their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement
tests/pair_energy_ref.c itself — against a plain Python restatement with an exact fma, the symmetry e_ij == e_ji, hand-made systems
whose answers are known by construction, and the elements of the fixture's binary against the analytic a = 1, ecc = 0.5."""
import ctypes as C
import math

import numpy as np
import pytest

from field_common import EPS
from pair_energy_common import (ANALYTIC, binary_fixture, bits, make_ref, python_elements, python_pair_energy, same, softened_orbit)
from timescale_common import two_body_orbit

SYMBOLS = {"nbody_pair_energy_rows": 4, "nbody_pair_energy_rows_d": 4, "nbody_binaries": 6}


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return make_ref(tmp_path_factory.mktemp("pair_energy_ref"))


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name, nargs in SYMBOLS.items():
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == nargs, name
    assert callable(nb.NBody.pair_energy) and callable(nb.NBody.binaries) and nb._lib.BINARY_WORDS == 4


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    idx, found, el = np.full(4, 7, np.int32), C.c_int(7), np.full(8, 7.0)
    for sfx, dt, ct in (("", np.float32, C.c_float), ("_d", np.float64, C.c_double)):
        e = np.full(4, 7, dt)
        assert getattr(lib, "nbody_pair_energy_rows" + sfx)(0, 4, e.ctypes.data_as(C.POINTER(ct)), ip(idx)) == nb._lib.ERR_NOT_INIT
        assert np.all(e == 7)
    assert lib.nbody_binaries(0.0, 2, C.byref(found), ip(idx), ip(idx[2:]), el.ctypes.data_as(C.POINTER(C.c_double))) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_binaries(0.0, 0, C.byref(found), None, None, None) == nb._lib.ERR_NOT_INIT
    assert np.all(idx == 7) and found.value == 7 and np.all(el == 7)


def test_pair_energy_ref_against_the_python_restatement(nb, ref):
    """binary64, the same IEEE operations in the same order (the fma computed exactly and rounded once, sqrt and divide correctly
    rounded in both): idx equal, e the same bits"""
    systems = [nb.make_bodies(n, seed=40 + n, dtype=np.float64) for n in (2, 3, 17)] + [binary_fixture()]
    for pos, vel in systems:
        got, want = ref.rows(pos, vel), python_pair_energy(pos, vel)
        assert np.array_equal(got[1], want[1]) and same(got[0], want[0]), len(pos)
        if len(pos) > 4:
            assert same(ref.rows(pos, vel, 3, 2), tuple(g[3:5] for g in got))
        found, i, j, el = ref.binaries(pos, vel)
        mutual = [(a, int(b)) for a, b in enumerate(want[1]) if b > a and want[1][b] == a and want[0][a] < 0.0]
        assert found == len(mutual) and list(zip(i.tolist(), j.tolist())) == mutual
        for k, (a, b) in enumerate(mutual):
            assert same(el[k], python_elements(pos, vel, a, b)), (a, b)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pair_energy_is_symmetric_bit_for_bit(nb, ref, dtype):
    """the differences change sign, their squares do not: e_ij and e_ji are the same bits — what makes 'mutual' a well-defined test"""
    for pos, vel in (nb.make_bodies(17, seed=57, dtype=dtype), binary_fixture(dtype)):
        n = len(pos)
        e, idx = ref.rows(pos, vel)
        for i in range(n):
            for j in range(i + 1, n):
                assert bits(ref.pair(pos, vel, i, j)) == bits(ref.pair(pos, vel, j, i)), (i, j)
            assert bits(e[i]) == bits(ref.pair(pos, vel, i, int(idx[i]))), i   # the row's e is its partner's pair value


def test_fixture_elements_against_the_analytic_orbit(ref):
    """The fixture's binary (pair_energy_common.softened_orbit: two_body_orbit(0.5) with r and v corrected for the softening, so that
    the softened pair the header defines has E = -1, a = 1, ecc = 0.5 in real arithmetic) against the analytic a = 1, ecc = 0.5 and
    period pi sqrt(2) within 1e-12 relative: a few dozen binary64 roundings, no cancellation at ecc = 0.5 (ecc^2 = 1 - 3 / 4)."""
    pos, vel = binary_fixture()
    found, i, j, el = ref.binaries(pos, vel)
    assert found == 1 and (int(i[0]), int(j[0])) == (0, 1)
    e, idx = ref.rows(pos, vel)
    assert list(idx[:2]) == [1, 0] and np.all(e[2:] > 0) and abs(e[0] + 1.0) < 1e-14
    for got in (el[0], python_elements(pos, vel, 0, 1)):
        rel = np.abs(got - np.array(ANALYTIC)) / np.abs(np.array(ANALYTIC))
        print("fixture elements: relative differences from the analytic {E, a, ecc, period}:", rel)
        assert np.all(rel <= 1e-12), rel
    # e_max: a = 1 means E = -1; nothing is below -2, nothing below -inf
    assert ref.binaries(pos, vel, e_max=-2.0)[0] == 0 and ref.binaries(pos, vel, e_max=-math.inf)[0] == 0
    assert ref.binaries(pos, vel, max_pairs=0)[0] == 1


def test_the_softening_moves_the_plain_orbit_by_eps_over_r_cubed(ref):
    """why the fixture is corrected: plain two_body_orbit(0.5) (r = 3 / 2) has the SOFTENED energy -1 + eps / r^3 to first order,
    3.0e-10 away from the -1 of the unsoftened orbit — the elements the header defines are those of the softened pair"""
    pos, vel, _ = two_body_orbit(0.5)
    shift = python_elements(pos, vel, 0, 1)[0] + 1.0
    assert abs(shift - EPS / 1.5 ** 3) <= 1e-6 * EPS and 2.9e-10 < shift < 3.0e-10
    p2, v2 = softened_orbit()
    assert abs(python_elements(p2, v2, 0, 1)[0] + 1.0) < 1e-15


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_hand_made_systems(ref, dtype):
    def system(p, v):
        pos, vel = np.zeros((len(p), 4), dtype), np.zeros((len(p), 4), dtype)
        pos[:, :3], vel[:, :3] = p, v
        return pos, vel

    inf, eps = dtype(np.inf), dtype(EPS)
    inv0 = dtype(1.0 / math.sqrt(float(eps)))   # 1 / sqrt(0 + eps): one rounding of the binary64 quotient in binary32, the quotient itself in binary64
    # one body: nobody else
    e, idx = ref.rows(*system([[1, 2, 3]], [[1, 0, 0]]))
    assert idx[0] == -1 and e[0] == inf
    assert ref.binaries(*system([[1, 2, 3]], [[1, 0, 0]]))[0] == 0
    # coincident distinct bodies with different velocities: the finite v2 / 2 - 2 / sqrt(eps)
    e, idx = ref.rows(*system([[1, 1, 1], [1, 1, 1]], [[0, 0, 0], [0, 0, 4]]))
    want = dtype(8.0 - 2.0 * float(inv0))   # (binary32: the binary64 difference is exact, so this is one rounding too)
    assert list(idx) == [1, 0] and np.all(np.isfinite(e)) and np.all(e == want) and e[0] < -60000
    # a NaN body poisons only its own pairs
    e, idx = ref.rows(*system([[0, 0, 0], [np.nan, 0, 0], [0, 3, 0]], [[0, 0, 0], [0, 0, 0], [0, 1, 0]]))
    assert list(idx) == [2, -1, 0] and e[1] == inf and bits(e[0]) == bits(e[2]) and np.isfinite(e[0])
    # a coordinate difference whose square overflows: inv = +0, e = v2 / 2, a legitimate non-negative candidate
    big = 1e30 if dtype is np.float32 else 1e200
    e, idx = ref.rows(*system([[0, 0, 0], [big, 0, 0]], [[0, 0, 0], [0, 2, 0]]))
    assert list(idx) == [1, 0] and list(e) == [2, 2]
    # a velocity difference whose square overflows: e = +inf, never chosen
    e, idx = ref.rows(*system([[0, 0, 0], [1, 0, 0]], [[0, 0, 0], [big, 0, 0]]))
    assert list(idx) == [-1, -1] and np.all(e == inf)
    # an exact tie: a body at rest at the origin, two bodies mirrored in position and velocity: the lowest j wins in row 0
    e, idx = ref.rows(*system([[0, 0, 0], [2, 1, 0], [-2, -1, 0]], [[0, 0, 0], [0, 0.5, 0], [0, -0.5, 0]]))
    assert idx[0] == 1 and list(idx[1:]) == [0, 0]
    assert bits(ref.pair(*system([[0, 0, 0], [2, 1, 0], [-2, -1, 0]], [[0, 0, 0], [0, 0.5, 0], [0, -0.5, 0]]), 0, 1)) == bits(e[0])
    assert bits(ref.pair(*system([[0, 0, 0], [2, 1, 0], [-2, -1, 0]], [[0, 0, 0], [0, 0.5, 0], [0, -0.5, 0]]), 0, 2)) == bits(e[0])
