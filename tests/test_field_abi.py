"""The field entry points (nbody_field(_d); include/nbody.h "field at arbitrary points") as far as no GPU is needed: the symbols and
their binding, NBODY_ERR_NOT_INIT without a context, and the CPU statement tests/field_ref.c itself — against a plain numpy fp64
evaluation of the definition, and bit for bit against tests/potential_ref.c where the two must agree."""
import ctypes as C

import numpy as np
import pytest

from field_common import EPS, FieldRef, compile_ref, make_points, make_skip, numpy_field, row_rel

TOL = 1e-5   # the project's north_star tolerance (TOL in tests/test_gpu_parity.py)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return FieldRef(compile_ref(tmp_path_factory.mktemp("field_ref"), "field_ref"))


@pytest.fixture(scope="module")
def potential(tmp_path_factory):
    return compile_ref(tmp_path_factory.mktemp("potential_ref"), "potential_ref")


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name in ("nbody_field", "nbody_field_d"):
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == 5
    assert callable(nb.NBody.field)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    for fn, dt, ct in ((lib.nbody_field, np.float32, C.c_float), (lib.nbody_field_d, np.float64, C.c_double)):
        pts = np.zeros((4, 4), dt)
        acc, phi = np.full((4, 4), 7, dt), np.full(4, 7, dt)
        p = lambda a: a.ctypes.data_as(C.POINTER(ct))
        assert fn(p(pts), 4, None, p(acc), p(phi)) == nb._lib.ERR_NOT_INIT
        assert np.all(acc == 7) and np.all(phi == 7)


def test_field_ref_against_numpy(nb, ref):
    n, m = 2100, 300   # three blocks, the last one short
    pos = nb.make_bodies(n)[0]
    pts, on = make_points(nb, pos, m)
    assert on == [0, 5, n - 1] and np.abs(pts[:, :3]).max() > 1.0
    for skip in (None, make_skip(n, m, on)):
        wa, wp = numpy_field(pos, pts, skip)
        for r in (False, True):
            a, p = ref.f32(pos, pts, skip, ref=r)
            ea, ep = row_rel(a, wa), float(np.max(np.abs(p - wp) / np.abs(wp)))
            print("fp32 ref=%d skip=%s: accel %.3e phi %.3e" % (r, skip is not None, ea, ep))
            assert ea < TOL and ep < TOL
            assert np.all(a[:, 3].view(np.uint32) == 0)
        pos64, pts64 = pos.astype(np.float64), pts.astype(np.float64)
        a, p = ref.f64(pos64, pts64, skip)
        ea, ep = row_rel(a, wa), float(np.max(np.abs(p - wp) / np.abs(wp)))
        print("fp64 skip=%s: accel %.3e phi %.3e" % (skip is not None, ea, ep))
        assert ea < 1e-12 and ep < 1e-12


@pytest.mark.parametrize("n", [1, 65, 2100])
def test_field_ref_with_self_skipped_is_potential_ref(nb, ref, potential, n):
    pos = nb.make_bodies(n)[0]
    sk = np.arange(n, dtype=np.int32)
    for r in (False, True):
        want = np.empty(n, np.float32)
        potential.potential_f32(pos.ctypes.data_as(C.c_void_p), n, 0, n, int(r), want.ctypes.data_as(C.c_void_p))
        got = ref.f32(pos, pos, sk, ref=r)[1]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (n, r)
    pos64 = np.ascontiguousarray(pos, np.float64)
    want = np.empty(n, np.float64)
    potential.potential_f64(pos64.ctypes.data_as(C.c_void_p), n, 0, n, want.ctypes.data_as(C.c_void_p))
    got = ref.f64(pos64, pos64, sk)[1]
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), n


def test_a_point_on_a_body_without_skip(nb, ref):
    """the coincident body adds 1/sqrt(eps) to -phi and +0 to a: a is what skipping that body gives, bit for bit"""
    n = 2100
    pos = nb.make_bodies(n)[0]
    pts, on = make_points(nb, pos, 3)
    a, p = ref.f32(pos, pts)
    a_sk, p_sk = ref.f32(pos, pts, np.array(on, np.int32))
    assert np.all(-p.astype(np.float64) > 1.0 / np.sqrt(EPS))
    assert np.all(-p_sk.astype(np.float64) < 0.1 / np.sqrt(EPS))
    assert np.array_equal(a.view(np.uint32), a_sk.view(np.uint32))
    a, p = ref.f64(pos.astype(np.float64), pts.astype(np.float64))
    a_sk, _ = ref.f64(pos.astype(np.float64), pts.astype(np.float64), np.array(on, np.int32))
    assert np.all(-p > 1.0 / np.sqrt(EPS)) and np.array_equal(a.view(np.uint64), a_sk.view(np.uint64))
