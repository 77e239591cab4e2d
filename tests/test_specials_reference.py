"""The hostile system of specials_common.py on the CPU alone: the planted rows do what their labels say, and the strict references
(tests/field_ref.c, tests/potential_ref.c) sit inside the tolerance the GPU tests hold the timed arithmetic to, with headroom — so a
tolerance test on the device cannot pass or fail because of the reference.  Needs no GPU."""
import ctypes as C

import numpy as np
import pytest

from field_common import EPS, FieldRef, compile_ref, numpy_field
from specials_common import SIZES, VARIANTS, hostile_points, hostile_system, nan_row, near, same_nan, special_row, within

# the reference's own worst error on the near rows must stay this far inside the device tests' tolerances (1e-5 and 1e-12)
HEADROOM = {np.float32: 3e-6, np.float64: 1e-13}


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    d = tmp_path_factory.mktemp("specials_ref")
    return FieldRef(compile_ref(d, "field_ref")), compile_ref(d, "potential_ref")


def strict_field(field, pos, pts, skip):
    return field.f32(pos, pts, skip) if pos.dtype == np.float32 else field.f64(pos, pts, skip)


def strict_phi(lib, pos):
    out = np.empty(len(pos), pos.dtype)
    if pos.dtype == np.float32:
        lib.potential_f32(pos.ctypes.data_as(C.c_void_p), len(pos), 0, len(pos), 0, out.ctypes.data_as(C.c_void_p))
    else:
        lib.potential_f64(pos.ctypes.data_as(C.c_void_p), len(pos), 0, len(pos), out.ctypes.data_as(C.c_void_p))
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_planted_rows_do_what_their_labels_say(nb, dtype):
    f32 = dtype == np.float32
    eps = dtype(EPS)
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_system(nb, n, dtype, variant)
            assert pos.dtype == dtype and vel.dtype == dtype and pos.shape == (n, 4)
            with np.errstate(all="ignore"):
                def d2(i, j):
                    d = pos[j, :3] - pos[i, :3]
                    return dtype(d[0] * d[0] + (d[1] * d[1] + (d[2] * d[2] + eps)))
                assert d2(10, 11) == eps and np.any(pos[10, :3] != pos[11, :3])
                assert np.signbit(pos[22, :3]).tolist() == [True, False, True] and np.signbit(pos[23, :3]).tolist() == [False, True, False]
                assert np.all(pos[22, :3] == 0) and np.all(pos[23, :3] == 0)
                if n > 1028:
                    for i in (1023, 1025, 1026, 1027, 1028):
                        assert same_nan(pos[i, :3], pos[1024, :3]) or variant == "nan"
                tiny = np.finfo(dtype).tiny
                if n > 64:
                    assert 0 < pos[64, 0] < 10 * tiny and pos[64, 1] == -pos[64, 0]
                for i in (41, n - 1):      # d2 finite, the cube subnormal or zero
                    inv = dtype(1) / np.sqrt(d2(0, i))
                    inv3 = dtype(inv * dtype(inv * inv))
                    assert np.isfinite(d2(0, i)) and inv > 0 and inv3 < tiny, (n, i, inv3)
                inv40 = dtype(1) / np.sqrt(d2(0, 40))
                assert dtype(inv40 * dtype(inv40 * inv40)) >= tiny
                if variant == "overflow":
                    assert np.isinf(d2(0, 63)) and np.all(np.isfinite(pos[63]))
                if variant == "inf":
                    assert np.isinf(pos[63, 0]) and np.all(np.isfinite(pos[63, 1:]))
                assert np.isnan(pos).sum() == (variant == "nan") and (variant != "nan" or np.isnan(pos[nan_row(n), 1]))
                assert np.isnan(vel).sum() == (variant == "nan")
            want_far = {40, 41, n - 1} | ({63} if variant in ("overflow", "inf") else set())
            assert set(far.tolist()) == want_far
            assert special_row(n, variant) == {"base": None, "overflow": 63, "inf": 63, "nan": nan_row(n)}[variant]
            big = 1e18 if f32 else 1e150
            assert vel[6, 0] == dtype(big) and vel[7, 1] == dtype(1 / big) and np.signbit(vel[5, :3]).tolist() == [True, False, True]


def test_planted_points_land_on_the_loop_edges(nb):
    for n in SIZES:
        pos, vel, far = hostile_system(nb, n, np.float32, "nan")
        for m in (1, 65, 300):
            pts, skip = hostile_points(nb, pos, m, "nan")
            assert pts.shape == (m, 4) and skip.shape == (m,) and skip.dtype == np.int32 and pts.dtype == pos.dtype
            assert np.all((skip >= -1) & (skip < n)) and skip[m - 1] == n - 1 and m % 64 != 0
        pts, skip = hostile_points(nb, pos, 300, "nan")
        on = sorted({b for b in (0, 63, 64, 1023, 1024, n - 1) if b < n})
        for k, b in enumerate(on):
            assert same_nan(pts[2 * k], pos[b]) and same_nan(pts[2 * k + 1], pos[b]) and skip[2 * k] == b and skip[2 * k + 1] == -1
        k = 2 * len(on)
        assert same_nan(pts[k], pos[nan_row(n)]) and skip[k] == -1
        assert skip[k + 1] == skip[k + 2] == nan_row(n) and np.all(np.abs(pts[k + 1:k + 3, :3]) <= 1.5)
        assert np.all(skip[64:128] == min(1023, n - 1))
        assert skip[128 + 37] == min(1024, n - 1) and np.all(np.delete(skip[128:192], 37) == -1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strict_references_sit_inside_the_tolerances_with_headroom(nb, refs, dtype):
    """field_ref.c and potential_ref.c in the context precision against the plain numpy binary64 evaluation of the definition, on the
    near rows and points (every |coordinate| <= 2, not a far-away body): |a - a64| / sum_j |term_j| per component and |phi - phi64| /
    |phi64|.  Measured, worst over the four variants:
      binary32  n = 70: accel 4.6e-7, phi 3.5e-7;    n = 1100: accel 1.6e-6, phi 1.6e-6;    n = 2085: accel 1.1e-6, phi 1.6e-6
      binary64  n = 70: accel 5.1e-16, phi 6.5e-16;  n = 1100: accel 1.6e-15, phi 2.8e-15;  n = 2085: accel 4.7e-15, phi 2.3e-15
    against the device tests' 1e-5 and 1e-12 (this test requires 3e-6 and 1e-13).  Everywhere, the far-away rows included, the two are
    finite in the same places."""
    field, potential = refs
    bound = HEADROOM[dtype]
    for n in SIZES:
        worst_a = worst_p = 0.0
        for variant in VARIANTS:
            pos, vel, far = hostile_system(nb, n, dtype, variant)
            rows_skip = np.arange(n, dtype=np.int32)
            pts, skip = hostile_points(nb, pos, 300, variant)
            for x, sk, keep in ((pos, rows_skip, near(pos, far)), (pts, skip, near(pts)), (pts, None, near(pts))):
                a, phi = strict_field(field, pos, x, sk)
                a64, phi64, mag = numpy_field(pos, x, sk, mags=True)
                assert np.array_equal(np.isfinite(a[:, :3]), np.isfinite(a64[:, :3])) and np.array_equal(np.isfinite(phi), np.isfinite(phi64))
                assert keep.sum() >= (0.9 * len(x) if len(x) > 100 else 1)
                assert within(a[keep, :3], a64[keep, :3], bound * mag[keep]), (n, variant)
                assert within(phi[keep], phi64[keep], bound * np.abs(phi64[keep])), (n, variant)
                with np.errstate(all="ignore"):
                    worst_a = max(worst_a, float(np.nanmax(np.abs(a[keep, :3] - a64[keep, :3]) / mag[keep], initial=0.0)))
                    worst_p = max(worst_p, float(np.nanmax(np.abs(phi[keep] - phi64[keep]) / np.abs(phi64[keep]), initial=0.0)))
            # the potential's own reference states the same sums
            assert same_nan(strict_phi(potential, pos), strict_field(field, pos, pos, rows_skip)[1])
        print("%s n=%d: reference against numpy binary64 on the near rows: accel %.2e phi %.2e (bound %.0e)"
              % (np.dtype(dtype).name, n, worst_a, worst_p, bound))
