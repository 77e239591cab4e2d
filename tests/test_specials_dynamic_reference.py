"""The hostile inputs of the dynamic passes on the CPU alone (specials_common.hostile_dynamic_system, hostile_point_words,
hostile_masses): the conditions that give the device tests of the snap, the sixth-order Hermite integrator, its block scheme and
NBODY_OPT_MASSES their power, asserted on the statements themselves (tests/snap_ref.c, hermite6_ref.c, hermite6_block_ref.c,
hermite_block_ref.c, masses_ref.c) — the finite variants stay finite on EVERY row through the steps and spread over the block levels,
the poisoned ones are poisoned everywhere and take one sub-step — and the strict binary32 statements' own error against plain numpy
binary64 on these inputs, which the device tests' tolerances are made of.  Needs no GPU."""
import numpy as np
import pytest

import masses_common
import snap_common
from field_common import compile_ref
from hermite6_block_common import Block6Ref
from hermite6_block_common import compile_ref as compile_block6
from hermite6_common import MASS, REF, Hermite6Ref
from hermite6_common import compile_ref as compile_hermite6
from hermite_block_common import BlockRef
from hermite_block_common import compile_ref as compile_block4
from masses_common import compile_masses_ref, with_masses
from snap_common import SnapRef, numpy_snap
from specials_common import (DYNAMIC_FAST, INF_MASS_ROW, NAN_PAYLOAD, SIZES, VARIANTS, bits, far_mass, hostile_dynamic_system, hostile_masses,
                             hostile_point_words, hostile_points, hostile_system, nan_row, near, same_nan)

RUN = dict(eta=0.04, dt_max=1.0 / 256, levels=8, nblocks=1)
DT = 1.0 / 256
FINITE = ("base", "overflow")
POISONED = ("nan", "inf")


class Refs:
    def __init__(self, d):
        self.snap = SnapRef(compile_ref(d, "snap_ref"))
        self.h6 = Hermite6Ref(compile_hermite6(d))
        self.b6 = Block6Ref(compile_block6(d))
        self.b4 = BlockRef(compile_block4(d))
        self.masses = compile_masses_ref(d)


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return Refs(tmp_path_factory.mktemp("specials_dynamic_ref"))


def forms(dtype):
    """the d2 forms a precision has: the FMA3 form, and in binary32 the reference's roundings too"""
    return (False, True) if dtype == np.float32 else (False,)


def finite3(*arrays):
    return all(bool(np.all(np.isfinite(a[:, :3]))) for a in arrays)


def bodies(nb, n, dtype, variant, masses):
    pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
    if masses:
        pos = with_masses(pos, hostile_masses(n, dtype, variant))
    return pos, vel, far


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_the_dynamic_system_and_the_masses_are_what_they_say(nb, dtype):
    fi = np.finfo(dtype)
    for n in SIZES:
        for variant in VARIANTS:
            pos, vel, far = hostile_system(nb, n, dtype, variant)
            dpos, dvel, dfar = hostile_dynamic_system(nb, n, dtype, variant)
            changed = np.zeros(vel.shape, bool)
            changed[6, 0] = changed[7, 1] = True
            assert same_nan(pos, dpos) and np.array_equal(far, dfar) and same_nan(vel[~changed], dvel[~changed])
            assert dvel[6, 0] == dtype(DYNAMIC_FAST) and dvel[7, 1] == dtype(1.0 / DYNAMIC_FAST) and dvel.dtype == dtype
            w = hostile_masses(n, dtype, variant)
            assert w.shape == (n,) and w.dtype == dtype
            assert [bits(w[i:i + 1])[0] == bits(np.array([v], dtype))[0] for i, v in ((12, 0.0), (13, -0.0), (22, 0.0))] == [True] * 3
            assert w[14] == fi.smallest_subnormal and w[15] == fi.tiny and w[16] == 2.0 ** 20 and w[17] == 2.0 ** -20 and w[30] < 0
            assert w[41] == far_mass(dtype) and 41 in far and (n <= 1024 or variant == "nan" or bits(w[1024:1025])[0] == 0)
            assert np.isnan(w).sum() == (variant == "nan") and np.isinf(w).sum() == (variant == "inf")
            if variant == "nan":
                assert int(bits(w[nan_row(n):nan_row(n) + 1])[0]) & 0xffff == NAN_PAYLOAD
            if variant == "inf":
                assert w[INF_MASS_ROW] == np.inf and np.all(np.isfinite(dpos[INF_MASS_ROW])) and near(dpos)[INF_MASS_ROW]
            if variant == "overflow":
                assert bits(w[63:64])[0] == 0
        pvel, pacc = hostile_point_words(nb, 300, dtype)
        assert np.signbit(pvel[0, :3]).tolist() == [True, False, True] and np.signbit(pacc[299, :3]).tolist() == [False, True, False]
        assert not pvel[[0, 1, 299], :3].any() and not pacc[[0, 1, 299], :3].any()
        own_v, own_a = hostile_point_words(nb, 300, dtype, dvel, dpos)
        assert same_nan(own_v[:2, :3], dvel[[0, 0], :3]) and same_nan(own_a[:2, :3], dpos[[0, 0], :3]) and same_nan(own_v[2:], pvel[2:])


@pytest.mark.parametrize("masses", [False, True], ids=["unit", "masses"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_finite_variants_stay_finite_on_every_row(nb, refs, dtype, masses):
    """ "base" and "overflow", both d2 forms: a, j and s finite on every row; every row finite after three shared sixth-order steps of
    1/256, after one sixth-order block (eta 0.04, dt_max 1/256, 8 levels) and after the same fourth-order block; the sixth-order block
    occupies at least three levels and takes more than one sub-step.  With the masses also the potential, the totals and three
    fourth-order steps.  No row is excused."""
    for n in SIZES:
        for variant in FINITE:
            pos, vel, far = bodies(nb, n, dtype, variant, masses)
            for r in forms(dtype):
                what = (n, variant, r)
                flags = (REF if r else 0) | (MASS if masses else 0)
                with np.errstate(all="ignore"):
                    assert finite3(*refs.snap.rows(pos, vel, dtype, ref=r, mass=masses)), what
                    assert finite3(*refs.h6.step(pos, vel, dtype, DT, 3, flags)), what
                    assert finite3(*refs.h6.restarted(pos, vel, dtype, DT, 3, flags)), what
                    p, v, steps, evals, trace = refs.b6.run(pos, vel, dtype, ref=r, mass=masses, **RUN)
                    assert finite3(p, v) and steps > 1 and trace.occupied_levels() >= 3, what + (steps, trace.occupied_levels())
                    trace.check_invariant(n, RUN["levels"], RUN["nblocks"])
                    if masses:
                        p4, v4, steps4, evals4 = refs.masses.hermite_block(pos, vel, dtype, RUN["eta"], RUN["dt_max"], RUN["levels"], 1, r)
                        assert np.isfinite(refs.masses.potential(pos, dtype, r)).all() and np.isfinite(refs.masses.totals(pos, vel, dtype, ref=r)).all(), what
                        assert finite3(*refs.masses.hermite(pos, vel, dtype, dtype(DT), 3, r)), what
                    else:
                        p4, v4, steps4, evals4, trace4 = refs.b4.run(pos, vel, dtype, ref=r, **RUN)
                        assert trace4.occupied_levels() >= 3
                    assert finite3(p4, v4) and steps4 > 1, what
            levels = np.bincount(np.concatenate([trace.level0] + trace.levels), minlength=8)
            print("%s n=%d %s masses=%d: sixth-order block %d sub-steps, %d row evaluations, first levels %s"
                  % (np.dtype(dtype).name, n, variant, masses, steps, evals, np.bincount(trace.level0, minlength=8).tolist()))
            assert (levels > 0).sum() >= 3


@pytest.mark.parametrize("masses", [False, True], ids=["unit", "masses"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_poisoned_variants_are_poisoned_on_every_row(nb, refs, dtype, masses):
    """ "nan" and "inf": the NaN (infinite) body makes a (in "inf": its x), j and s NaN on every row — the others through the pair, the
    body itself through its own position — and both blocks take exactly one sub-step of n rows, every row on level 0"""
    for n in SIZES:
        for variant in POISONED:
            pos, vel, far = bodies(nb, n, dtype, variant, masses)
            for r in forms(dtype):
                what = (n, variant, r)
                with np.errstate(all="ignore"):
                    a, j, s = refs.snap.rows(pos, vel, dtype, ref=r, mass=masses)
                    # ("inf": dx = inf meets inv = 0 in x alone, so the acceleration's y and z stay finite; rv carries it to all of j and s)
                    assert np.all(np.isnan(a[:, :3 if variant == "nan" else 1])) and np.all(np.isnan(j[:, :3])) and np.all(np.isnan(s[:, :3])), what
                    p, v, steps, evals, trace = refs.b6.run(pos, vel, dtype, ref=r, mass=masses, **RUN)
                    assert (steps, evals) == (1, n) and (trace.level0 == 0).all(), what
                    if masses:
                        assert refs.masses.hermite_block(pos, vel, dtype, RUN["eta"], RUN["dt_max"], RUN["levels"], 1, r)[2:] == (1, n), what
                    else:
                        assert refs.b4.run(pos, vel, dtype, ref=r, **RUN)[2:4] == (1, n), what


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_special_mass_alone(nb, refs, dtype):
    """the "nan" and "inf" masses on the otherwise finite "base" bodies, where nothing but the mass is special: a NaN mass makes the
    acceleration and the jerk of every row but its own NaN (a row skips itself) and, through the a_j, the snap of every row; an infinite
    mass leaves no finite non-zero acceleration behind (+-inf or NaN) on any other row"""
    for n in SIZES:
        pos, vel, far = hostile_dynamic_system(nb, n, dtype, "base")
        for r in forms(dtype):
            with np.errstate(all="ignore"):
                row = nan_row(n)
                a, j, s = refs.snap.rows(with_masses(pos, hostile_masses(n, dtype, "nan")), vel, dtype, ref=r, mass=True)
                others = np.arange(n) != row
                assert np.all(np.isnan(a[others, :3])) and np.all(np.isnan(j[others, :3])) and np.all(np.isnan(s[:, :3])), (n, r)
                assert finite3(a[row:row + 1], j[row:row + 1]), (n, r)
                a, j, s = refs.snap.rows(with_masses(pos, hostile_masses(n, dtype, "inf")), vel, dtype, ref=r, mass=True)
                others = np.arange(n) != INF_MASS_ROW
                assert not np.any(np.isfinite(a[others, :3]) & (a[others, :3] != 0)), (n, r)
                assert finite3(a[INF_MASS_ROW:INF_MASS_ROW + 1]), (n, r)


def snap_queries(nb, pos, vel, acc, variant, m=300):
    pts, skip = hostile_points(nb, pos, m, variant)
    pvel, pacc = hostile_point_words(nb, m, pos.dtype.type, vel, acc)
    return pts, pvel, pacc, skip


def test_strict_snap_statement_sits_inside_r_ref_hostile(nb, refs):
    """snap_ref.c in strict binary32, both d2 forms, against snap_common.numpy_snap in binary64 on hostile_dynamic_system ("base" and
    "overflow") at hostile_points(…, 300, variant) with hostile_point_words, with and without skip, the sources' accelerations being the
    statement's own first pass: |got - want64| / mag on the queries that are near (specials_common.near) and finite in binary64 — at
    least 290 of 300, none of them left out.  The worst figure is snap_common.R_REF_HOSTILE's; the device test of the timed arithmetic
    is made of it."""
    dtype = np.float32
    overall = [0.0, 0.0, 0.0]
    for n in SIZES:
        fig = [0.0, 0.0, 0.0]
        for variant in FINITE:
            pos, vel, far = hostile_dynamic_system(nb, n, dtype, variant)
            for r in forms(dtype):
                with np.errstate(all="ignore"):
                    acc = refs.snap.rows(pos, vel, dtype, ref=r)[0]
                assert finite3(acc)
                pts, pvel, pacc, hsk = snap_queries(nb, pos, vel, acc, variant)
                for skip in (None, hsk):
                    full = numpy_snap(pos, vel, acc, pts, pvel, pacc, skip)
                    with np.errstate(all="ignore"):
                        got = refs.snap.f32(pos, vel, acc, pts, pvel, pacc, skip, ref=r)
                    keep = near(pts) & np.all([np.isfinite(o).all(1) for o in full], axis=0)
                    assert keep.sum() >= 290, (n, variant, int(keep.sum()))
                    for k in range(3):
                        assert np.all(np.isfinite(got[k][keep, :3])) and np.all(full[3 + k][keep] > 0), (n, variant, r, k)
                        fig[k] = max(fig[k], snap_common.worst(got[k][keep], full[k][keep], full[3 + k][keep]))
        print("binary32 n=%d: snap_ref.c against numpy binary64 on the near queries: accel %.3e jerk %.3e snap %.3e (R_REF_HOSTILE %.3e)"
              % (n, fig[0], fig[1], fig[2], snap_common.R_REF_HOSTILE))
        overall = [max(o, f) for o, f in zip(overall, fig)]
    assert max(overall) <= snap_common.R_REF_HOSTILE, overall
    assert max(overall) > snap_common.R_REF_HOSTILE / 1.1, "R_REF_HOSTILE is the measured figure rounded up by no more than a tenth"


def mass_keep(pts, *mags):
    """(keep, removed): the near queries whose binary64 magnitude sums are finite, and how many near queries that leaves out"""
    ok = near(pts)
    fin = np.all([np.isfinite(m).all(1) for m in mags], axis=0)
    return ok & fin, int((ok & ~fin).sum())


def test_weighted_field_and_jerk_statements_sit_inside_r_ref_hostile(nb, refs):
    """masses_ref.c's weighted field and jerk in strict binary32, both d2 forms, against masses_common.numpy_field and numpy_jerk in
    binary64 on hostile_dynamic_system with hostile_masses ("base", "overflow"), on the near queries whose binary64 magnitude sums are
    finite (the exclusion removes at most 10 of 300; printed).  The figure is large beside the cloud's masses_common.R_REF, and it is
    the far body's: 2^100 times an inv^3 that binary32 holds as one subnormal bit is a term of order one with an error of order one,
    on every query alike.  It is recorded as masses_common.R_REF_HOSTILE."""
    dtype = np.float32
    overall, removed_most = 0.0, 0
    for n in SIZES:
        fig = [0.0, 0.0, 0.0]
        for variant in FINITE:
            pos, vel, far = bodies(nb, n, dtype, variant, True)
            pts, skip = hostile_points(nb, pos, 300, variant)
            pvel = hostile_point_words(nb, 300, dtype, vel)[0]
            for sk in (None, skip):
                wa, wphi, mag = masses_common.numpy_field(pos, pts, sk)
                ja, jj, mag_a, mag_j = masses_common.numpy_jerk(pos, vel, pts, pvel, sk)
                keep, removed = mass_keep(pts, mag, mag_a, mag_j)
                removed_most = max(removed_most, removed)
                assert removed <= 10 and keep.sum() >= 290, (n, variant, removed)
                for r in forms(dtype):
                    with np.errstate(all="ignore"):
                        a, phi = refs.masses.field(pos, pts, dtype, sk, r)
                        a2, j = refs.masses.jerk(pos, vel, pts, pvel, dtype, sk, r)
                    assert same_nan(a, a2) and finite3(a[keep], j[keep])
                    fig[0] = max(fig[0], masses_common.worst(a[keep], wa[keep], mag[keep]))
                    fig[1] = max(fig[1], masses_common.worst(a2[keep], ja[keep], mag_a[keep]))
                    fig[2] = max(fig[2], masses_common.worst(j[keep], jj[keep], mag_j[keep]))
        print("binary32 n=%d: masses_ref.c against numpy binary64 on the near queries: field accel %.3e, jerk's accel %.3e jerk %.3e "
              "(R_REF_HOSTILE %.3e; finite-magnitude exclusion removed at most %d of 300)" % (n, fig[0], fig[1], fig[2], masses_common.R_REF_HOSTILE, removed_most))
        overall = max(overall, max(fig))
    assert overall <= masses_common.R_REF_HOSTILE, overall
    assert overall > masses_common.R_REF_HOSTILE / 1.1, "R_REF_HOSTILE is the measured figure rounded up by no more than a tenth"
