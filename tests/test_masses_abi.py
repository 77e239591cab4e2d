"""NBODY_OPT_MASSES (include/nbody.h) as far as no GPU is needed: the constants and their binding, and the CPU statement
tests/masses_ref.c itself — with every w = 1 against tests/field_ref.c, tidal_ref.c, jerk_ref.c and potential_ref.c bit for bit
(property (a)), the exact scaling by 2^k (b), appended bodies of zero mass (c), against plain numpy binary64 in the measure the GPU tests
use, and the weighted acceleration as minus the gradient of the weighted potential (and the weighted tidal tensor as its gradient)."""
import ctypes as C

import numpy as np
import pytest

from field_common import FieldRef, compile_ref, make_points, make_skip
from jerk_common import TIMED_SHAPE, JerkRef
from masses_common import (R_REF, bits, compile_masses_ref, numpy_field, numpy_jerk, numpy_tidal, random_masses, with_masses, worst)
from tidal_common import GRADIENT_H, TidalRef, gradient_error, gradient_points

REF_F64 = 1e-13
N, M = 2100, 300   # three blocks, the last one short


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return compile_masses_ref(tmp_path_factory.mktemp("masses_ref"))


@pytest.fixture(scope="module")
def unweighted(tmp_path_factory):
    d = tmp_path_factory.mktemp("unweighted_refs")
    return (FieldRef(compile_ref(d, "field_ref")), TidalRef(compile_ref(d, "tidal_ref")), JerkRef(compile_ref(d, "jerk_ref")),
            compile_ref(d, "potential_ref"))


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def test_constants_are_bound(nb):
    L = nb._lib
    assert L.OPT_MASSES == 18 and nb.OPT_MASSES == 18
    assert L.INFO_MASSES == L.INFO_MAILBOX_SERVING + 1 and nb.INFO_MASSES == L.INFO_MASSES
    assert callable(nb.NBody.use_masses)
    header = open(L.HERE + "/../include/nbody.h").read()
    assert "NBODY_OPT_MASSES = 18" in header
    keys = header[header.index("enum { NBODY_INFO_N = 1"):]
    keys = keys[:keys.index("};")]
    assert keys.rstrip().endswith("NBODY_INFO_MASSES /* NBODY_OPT_MASSES: 0 or 1 */")   # appended as the last info key


def test_unit_masses_are_the_unweighted_references_bit_for_bit(nb, ref, unweighted):
    """property (a) on the CPU: m * x and fma(1, x, s) are exact"""
    field_ref, tidal_ref, jerk_ref, pot = unweighted
    pos, vel = nb.make_bodies(N)
    pts, on = make_points(nb, pos, M)
    pvel = nb.make_bodies(M, seed=78)[1]
    for dtype in (np.float32, np.float64):
        p1, v, x, u = with_masses(pos.astype(dtype), 1), vel.astype(dtype), pts.astype(dtype), pvel.astype(dtype)
        p0 = with_masses(p1, 7.5)   # the unweighted references never read w
        for skip in (None, make_skip(N, M, on)):
            for r in ((False, True) if dtype == np.float32 else (False,)):
                kw = dict(ref=r) if dtype == np.float32 else {}
                f = field_ref.f32 if dtype == np.float32 else field_ref.f64
                t = tidal_ref.f32 if dtype == np.float32 else tidal_ref.f64
                j = jerk_ref.f32 if dtype == np.float32 else jerk_ref.f64
                wa, wphi = f(p0, x, skip, **kw)
                a, phi = ref.field(p1, x, dtype, skip, r)
                assert same(a, wa) and same(phi, wphi), (dtype, r)
                assert same(ref.tidal(p1, x, dtype, skip, r), t(p0, x, skip, **kw)), (dtype, r)
                wa, wj = j(p0, v, x, u, skip, **kw)
                a, jk = ref.jerk(p1, v, x, u, dtype, skip, r)
                assert same(a, wa) and same(jk, wj), (dtype, r)
        want = np.empty(N, dtype)
        for r in ((False, True) if dtype == np.float32 else (False,)):
            if dtype == np.float32:
                pot.potential_f32(p0.ctypes.data_as(C.c_void_p), N, 0, N, int(r), want.ctypes.data_as(C.c_void_p))
            else:
                pot.potential_f64(p0.ctypes.data_as(C.c_void_p), N, 0, N, want.ctypes.data_as(C.c_void_p))
            assert same(ref.potential(p1, dtype, r), want), (dtype, r)


def everything(ref, pos, vel, pts, pvel, skip, dtype, r):
    """every output of the weighted reference at the queries and rows, as a list of arrays"""
    return [*ref.field(pos, pts, dtype, skip, r), ref.tidal(pos, pts, dtype, skip, r), *ref.jerk(pos, vel, pts, pvel, dtype, skip, r),
            *ref.jerk_rows(pos, vel, dtype, r), ref.potential(pos, dtype, r), ref.totals(pos, vel, dtype, ref=r)]


def test_scaling_every_mass_by_a_power_of_two_scales_every_output(nb, ref):
    """property (b): k = +-3.  The totals scale too: a row's term is mi times a value that does not depend on the masses (T, P, L: by
    2^k) or is linear in them (U's mi * phi_i: by 2^2k), all exact"""
    pos, vel = nb.make_bodies(N)
    pts, on = make_points(nb, pos, M)
    pvel, skip = nb.make_bodies(M, seed=78)[1], make_skip(N, M, on)
    for dtype in (np.float32, np.float64):
        m = random_masses(N, dtype=dtype)
        p, v, x, u = pos.astype(dtype), vel.astype(dtype), pts.astype(dtype), pvel.astype(dtype)
        for r in ((False, True) if dtype == np.float32 else (False,)):
            base = everything(ref, with_masses(p, m), v, x, u, skip, dtype, r)
            for k in (3, -3):
                s = dtype(2.0 ** k)
                got = everything(ref, with_masses(p, m * s), v, x, u, skip, dtype, r)
                for g, b in zip(got[:-1], base[:-1]):
                    assert same(g, b * s), (dtype, r, k)
                scale = np.array([s, s * s, s, s, s, s, s, s], np.float64)
                assert same(got[-1], base[-1] * scale), (dtype, r, k)


def test_appended_bodies_of_zero_mass_change_no_bit(nb, ref):
    """property (c): 100 bodies with w = +0 behind the N massive ones: the first N rows' and every query's results keep their bits, and
    the tracers themselves are accelerated"""
    pos, vel = nb.make_bodies(N)
    tp, tv = nb.make_bodies(100, seed=31)
    pts, on = make_points(nb, pos, M)
    pvel, skip = nb.make_bodies(M, seed=78)[1], make_skip(N, M, on)
    for dtype in (np.float32, np.float64):
        p = with_masses(pos.astype(dtype), random_masses(N, dtype=dtype))
        v, x, u = vel.astype(dtype), pts.astype(dtype), pvel.astype(dtype)
        p2, v2 = np.concatenate([p, with_masses(tp.astype(dtype), 0)]), np.concatenate([v, tv.astype(dtype)])
        for r in ((False, True) if dtype == np.float32 else (False,)):
            base, got = everything(ref, p, v, x, u, skip, dtype, r), everything(ref, p2, v2, x, u, skip, dtype, r)
            for i, (g, b) in enumerate(zip(got, base)):
                assert same(g[:len(b)] if i in (5, 6, 7) else g, b), (dtype, r, i)   # 5, 6, 7: the rows' accel, jerk and phi
            assert np.all(np.abs(got[5][N:, :3]).sum(1) > 0)
            p3, v3 = ref.hermite(p2, v2, dtype, 1.0 / 256, 2, r)
            q3, w3 = ref.hermite(p, v, dtype, 1.0 / 256, 2, r)
            assert same(p3[:N], q3) and same(v3[:N], w3) and same(p3[:, 3], p2[:, 3])
            assert np.all(bits(v3[N:, :3]) != bits(v2[N:, :3]))


def test_masses_ref_against_numpy(nb, ref):
    """Masses in [0.25, 4), n = 2100, m = 300 and n = 65536, m = 512 (jerk_common.TIMED_SHAPE): the shape of the GPU test of the timed
    arithmetic, whose bound 2 R_REF + RSQ_SHARE rests on the binary32 figure asserted here, R_REF = 4.7e-6 in the mag measure.
    Measured at (65536, 512), binary32: acceleration 3.08e-7, jerk 8.61e-7 (FMA3 form; 7.08e-7 in the reference's), potential 1.79e-7,
    tidal 3.51e-6 (the worst of all); at (2100, 300): acceleration 9.47e-7, jerk 6.62e-7, potential 8.60e-7, tidal 2.18e-6; binary64 at
    (2100, 300): 4.4e-15.  The weight's one more rounding per pair stays inside the unweighted references' budget."""
    assert TIMED_SHAPE == (65536, 512)
    for n, m in ((N, M), TIMED_SHAPE):
        pos, vel = nb.make_bodies(n)
        pos = with_masses(pos, random_masses(n))
        pts, on = make_points(nb, pos, m)
        pvel = nb.make_bodies(m, seed=78)[1]
        for skip in ((None, make_skip(n, m, on)) if n == N else (make_skip(n, m, on),)):
            wa, wphi, mag = numpy_field(pos, pts, skip)
            wt, mag_t = numpy_tidal(pos, pts, skip)
            ja, jj, mag_a, mag_j = numpy_jerk(pos, vel, pts, pvel, skip)
            assert np.allclose(ja, wa, rtol=1e-12, atol=0)
            for dtype, bound in ((np.float32, R_REF), (np.float64, REF_F64)):
                if dtype == np.float64 and n != N:
                    continue
                for r in ((False, True) if dtype == np.float32 else (False,)):
                    a, phi = ref.field(pos, pts, dtype, skip, r)
                    t = ref.tidal(pos, pts, dtype, skip, r)
                    a2, j = ref.jerk(pos, vel, pts, pvel, dtype, skip, r)
                    figs = (worst(a, wa, mag), float(np.max(np.abs(phi.astype(np.float64) - wphi) / np.abs(wphi))), worst(t, wt, mag_t),
                            worst(a2, ja, mag_a), worst(j, jj, mag_j))
                    print("n=%d %s ref=%d skip=%s: accel %.3e phi %.3e tidal %.3e jerk's accel %.3e jerk %.3e"
                          % ((n, np.dtype(dtype).name, r, skip is not None) + figs))
                    assert max(figs) <= bound, (n, dtype, r, figs)


def test_weighted_acceleration_is_minus_the_gradient_of_the_weighted_potential(nb, ref):
    """binary64, tidal_common's central-difference check: a_b against -(phi(x + h e_b) - phi(x - h e_b)) / 2h, the bound the
    difference's truncation error h^2 |d^2 a_b / dx_b^2| / 6 estimated from a itself at +-h, times 4, per point in the Euclidean norm;
    and the weighted tensor as the gradient of the weighted acceleration by gradient_error itself"""
    n, h = 4099, GRADIENT_H
    pos = nb.make_bodies(n, dtype=np.float64)[0]
    x = gradient_points(nb, pos)
    pos = with_masses(pos, random_masses(n, dtype=np.float64))
    words = lambda p3: np.concatenate([p3, np.zeros((len(p3), 1))], axis=1)
    a0 = ref.field(pos, words(x), np.float64)[0][:, :3]
    err, trunc = np.zeros((len(x), 3)), np.zeros((len(x), 3))
    for b in range(3):
        e = h * np.eye(3)[b]
        ap, phip = ref.field(pos, words(x + e), np.float64)
        am, phim = ref.field(pos, words(x - e), np.float64)
        err[:, b] = np.abs(-(phip - phim) / (2 * h) - a0[:, b])
        trunc[:, b] = np.abs(ap[:, b] - 2 * a0[:, b] + am[:, b]) / 6
    e, tr = np.sqrt((err ** 2).sum(1)), np.sqrt((trunc ** 2).sum(1))
    print("a = -grad phi: worst error / |a| %.3e, worst error / bound %.3f" % ((e / np.sqrt((a0 ** 2).sum(1))).max(), (e / (4 * tr)).max()))
    assert np.all(e <= 4 * tr)
    err, trunc, scale = gradient_error(lambda p: ref.tidal(pos, p, np.float64), lambda p: ref.field(pos, p, np.float64)[0], x, h)
    e, tr = np.sqrt((err ** 2).sum((1, 2))), np.sqrt((trunc ** 2).sum((1, 2)))
    print("T = grad a: worst error / |T| %.3e, worst error / bound %.3f" % ((e / scale).max(), (e / (4 * tr)).max()))
    assert np.all(e <= 4 * tr)
