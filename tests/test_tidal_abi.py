"""The tidal entry points (nbody_tidal(_d); include/nbody.h "tidal tensor at arbitrary points") as far as no GPU is needed: the symbols
and their binding, NBODY_ERR_NOT_INIT without a context, tidal_matrix, and the CPU statement tests/tidal_ref.c itself — against a plain
numpy fp64 evaluation of the definition in the measure the GPU tests use, its symmetry, the on-body point, and T as the gradient of
tests/field_ref.c's acceleration."""
import ctypes as C

import numpy as np
import pytest

from field_common import EPS, FieldRef, compile_ref, make_points, make_skip
from tidal_common import GRADIENT_H, TidalRef, gradient_error, gradient_points, numpy_tidal, worst

REF_F32 = 5e-6    # what tidal_ref.c's binary32 must keep against binary64 in the mag measure: the GPU test's bound rests on it
REF_F64 = 1e-13


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return TidalRef(compile_ref(tmp_path_factory.mktemp("tidal_ref"), "tidal_ref"))


@pytest.fixture(scope="module")
def field_ref(tmp_path_factory):
    return FieldRef(compile_ref(tmp_path_factory.mktemp("field_ref"), "field_ref"))


def test_symbols_are_exported_and_bound(nb):
    lib = C.CDLL(nb._lib.LIB_PATH)
    for name in ("nbody_tidal", "nbody_tidal_d"):
        assert name in nb._lib.SYMBOLS and hasattr(lib, name), name
        assert len(getattr(nb._lib.load(), name).argtypes) == 4
    assert callable(nb.NBody.tidal) and callable(nb.tidal_matrix)


def test_not_init_without_a_context(nb):
    lib = nb._lib.load()
    lib.nbody_shutdown()
    for fn, dt, ct in ((lib.nbody_tidal, np.float32, C.c_float), (lib.nbody_tidal_d, np.float64, C.c_double)):
        pts = np.zeros((4, 4), dt)
        t = np.full((4, 6), 7, dt)
        p = lambda a: a.ctypes.data_as(C.POINTER(ct))
        assert fn(p(pts), 4, None, p(t)) == nb._lib.ERR_NOT_INIT
        assert np.all(t == 7)


def test_tidal_matrix(nb):
    t6 = np.arange(1, 13, dtype=np.float32).reshape(2, 6)
    full = nb.tidal_matrix(t6)
    assert full.shape == (2, 3, 3) and full.dtype == np.float32
    assert np.array_equal(full[0], [[1, 4, 5], [4, 2, 6], [5, 6, 3]]) and np.array_equal(full[1], full[1].T)
    assert nb.tidal_matrix(t6[1]).shape == (3, 3) and np.array_equal(nb.tidal_matrix(t6[1]), full[1])
    assert np.allclose(np.linalg.eigvalsh(full).sum(1), t6[:, :3].sum(1))
    with pytest.raises(ValueError):
        nb.tidal_matrix(np.zeros((2, 5)))


def test_tidal_ref_against_numpy(nb, ref):
    """n = 2100, m = 300: three blocks, the last one short.  n = 65536, m = 512: the shape of the GPU test of the timed arithmetic,
    whose bound (TOL = 1e-5) is derived from the binary32 figure asserted here.  Measured: 1.3e-6 and 3.7e-6 (binary32)."""
    for n, m in ((2100, 300), (65536, 512)):
        pos = nb.make_bodies(n)[0]
        pts, on = make_points(nb, pos, m)
        assert on == [0, 5, n - 1] and np.abs(pts[:, :3]).max() > 1.0
        for skip in (None, make_skip(n, m, on)):
            want, mag = numpy_tidal(pos, pts, skip)
            for r in (False, True):
                e = worst(ref.f32(pos, pts, skip, ref=r), want, mag)
                print("n=%d fp32 ref=%d skip=%s: %.3e" % (n, r, skip is not None, e))
                assert e <= REF_F32, (n, r)
            if n == 2100:
                e = worst(ref.f64(pos.astype(np.float64), pts.astype(np.float64), skip), want, mag)
                print("n=%d fp64 skip=%s: %.3e" % (n, skip is not None, e))
                assert e <= REF_F64


def test_trace_is_poissons_equation(nb, ref):
    """trace T = -3 eps sum_j inv^5: eleven orders below |T|'s terms, so it shows in binary64 only (to the sums' rounding)"""
    n = 2100
    pos = nb.make_bodies(n)[0].astype(np.float64)
    pts, on = make_points(nb, pos, 40)
    t = ref.f64(pos, pts)[3:]
    want, mag = numpy_tidal(pos, pts[3:])
    d = pos[None, :, :3] - pts[3:, None, :3]
    trace = -3.0 * EPS * (((d * d).sum(2) + EPS) ** -2.5).sum(1)
    assert np.all(trace < 0)
    assert np.all(np.abs(t[:, :3].sum(1) - trace) <= 1e-13 * mag[:, :3].sum(1))


def test_two_bodies_are_symmetric(nb, ref):
    """T at r_0 from body 1 alone is T at r_1 from body 0 alone (d -> -d leaves every product as it is), bit for bit"""
    pos = nb.make_bodies(2)[0]
    sk = np.array([0, 1], np.int32)
    for r in (False, True):
        t = ref.f32(pos, pos, sk, ref=r)
        assert np.array_equal(t[0].view(np.uint32), t[1].view(np.uint32)) and np.all(t != 0)
    t = ref.f64(pos.astype(np.float64), pos.astype(np.float64), sk)
    assert np.array_equal(t[0].view(np.uint64), t[1].view(np.uint64))


def test_a_point_on_a_body_without_skip(nb, ref):
    """the coincident body adds +0 off the diagonal — what skipping it gives, bit for bit — and -eps^(-3/2) on it"""
    n = 2100
    pos = nb.make_bodies(n)[0]
    pts, on = make_points(nb, pos, 3)
    for f, p, x, u in ((ref.f32, pos, pts, np.uint32), (ref.f64, pos.astype(np.float64), pts.astype(np.float64), np.uint64)):
        t, t_sk = f(p, x), f(p, x, np.array(on, np.int32))
        assert np.array_equal(t[:, 3:].view(u), t_sk[:, 3:].view(u))
        gap = t_sk[:, :3].astype(np.float64) - t[:, :3].astype(np.float64)
        assert np.all(np.abs(gap - EPS ** -1.5) <= 1e-6 * EPS ** -1.5), gap


def test_tidal_ref_is_the_gradient_of_field_ref(nb, ref, field_ref):
    """the references alone, as tests/test_gpu_tidal.py asks of the device: the bound is the central difference's truncation error,
    estimated from T itself at +-h, times 4, per point in the Frobenius norm"""
    n, h = 4099, GRADIENT_H
    pos = nb.make_bodies(n, dtype=np.float64)[0]
    x = gradient_points(nb, pos)
    err, trunc, scale = gradient_error(lambda p: ref.f64(pos, p), lambda p: field_ref.f64(pos, p)[0], x, h)
    e, tr = np.sqrt((err ** 2).sum((1, 2))), np.sqrt((trunc ** 2).sum((1, 2)))
    print("tidal_f64 / field_f64: worst error / |T| %.3e, worst error / bound %.3f" % ((e / scale).max(), (e / (4 * tr)).max()))
    assert np.all(e <= 4 * tr)

