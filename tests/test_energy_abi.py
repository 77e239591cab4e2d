"""The energy diagnostics' C-ABI without a GPU: nbody_energy and nbody_potential_rows(_d) are exported and bound, answer
ERR_NOT_INIT when no context is open, and the Python engine has the methods; tests/potential_ref.c (the CPU statement of the
potential that tests/test_gpu_energy.py compares the device with) agrees with a plain numpy restatement."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nbody_energy", "nbody_potential_rows", "nbody_potential_rows_d")


def test_energy_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in nb._lib.SYMBOLS, name
    assert nb._lib.ENERGY_WORDS == 8 and nb._lib.ENERGY_POTENTIAL == 1 and nb._lib.ENERGY_LZ == 7


def test_energy_entry_points_need_a_context(nb):
    lib = nb._lib.load()
    out = np.zeros(8, np.float64)
    phi32, phi64 = np.zeros(4, np.float32), np.zeros(4, np.float64)
    assert lib.nbody_energy(out.ctypes.data_as(C.POINTER(C.c_double))) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_potential_rows(0, 4, phi32.ctypes.data_as(C.POINTER(C.c_float))) == nb._lib.ERR_NOT_INIT
    assert lib.nbody_potential_rows_d(0, 4, phi64.ctypes.data_as(C.POINTER(C.c_double))) == nb._lib.ERR_NOT_INIT
    assert not out.any() and not phi32.any() and not phi64.any()


def test_engine_has_the_energy_methods(nb):
    assert callable(getattr(nb.NBody, "energy", None)) and callable(getattr(nb.NBody, "potential_rows", None))


def test_potential_ref_matches_numpy(nb, tmp_path):
    so = str(tmp_path / "potential_ref.so")
    subprocess.run(["gcc", "-std=c11", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-o", so,
                    os.path.join(ROOT, "tests", "potential_ref.c"), "-lm"], check=True, capture_output=True, timeout=120)
    ref = C.CDLL(so)
    n = 2100                                   # three level-1 blocks, the last one short
    pos, _ = nb.make_bodies(n)
    pos[7, :3] = pos[3, :3]                    # two coincident distinct bodies: each sees 1/sqrt(eps) from the other
    eps = float(np.array([0x3089705F], np.uint32).view(np.float32)[0])
    p64 = pos.astype(np.float64)
    d = p64[None, :, :3] - p64[:, None, :3]
    inv = 1.0 / np.sqrt((d ** 2).sum(-1) + eps)
    np.fill_diagonal(inv, 0.0)
    want = -inv.sum(1)
    got32 = np.empty(n, np.float32)
    got64 = np.empty(n, np.float64)
    for r in (0, 1):
        ref.potential_f32(pos.ctypes.data_as(C.c_void_p), n, 0, n, r, got32.ctypes.data_as(C.c_void_p))
        assert np.max(np.abs(got32 - want) / np.abs(want)) < 1e-5
    ref.potential_f64(p64.ctypes.data_as(C.c_void_p), n, 0, n, got64.ctypes.data_as(C.c_void_p))
    assert np.max(np.abs(got64 - want) / np.abs(want)) < 1e-12
    assert abs(got64[3] - want[3]) < 1e-12 * abs(want[3]) and -got64[3] > 1.0 / np.sqrt(eps)
    one = np.empty(1, np.float32)
    ref.potential_f32(pos.ctypes.data_as(C.c_void_p), 1, 0, 1, 0, one.ctypes.data_as(C.c_void_p))
    assert one.view(np.uint32)[0] == 0                          # N = 1: +0 exactly
