"""The hostile system for plain distances (specials_common.hostile_distance_system) on the CPU alone: the four references of the exact
distance passes — tests/neighbors_ref.c, knn_ref.c, fof_ref.c, hist_ref.c — against an independent statement in plain numpy IN THE
CONTEXT'S PRECISION (differences, three products and two additions in dtype, so that overflow and underflow happen where they do on
the device; a stable argsort by (d2, index); a Python union-find; searchsorted binning), the planted rows' labels, and four subtly wrong
statements that the inputs must tell from the right one.  So a bit comparison on the device cannot pass or fail because of the
reference, and a kernel that flushed a subnormal, tied the wrong way, started its scan from the wrong value or counted +inf below a
+inf edge could not pass it.  Needs no GPU."""
import numpy as np
import pytest

import fof_common
import hist_common
import knn_common
import neighbors_common
from specials_common import (DISTANCE_ROWS, HOSTILE_BINS, SIZES, VARIANTS, bits, distance_h, hostile_b2, hostile_distance_system, hostile_edges,
                             hostile_points, hostile_radii, hostile_system, nan_row, planted_rows, same_nan, subnormal_between)

WRONG = ("flush", "le", "finite_start", "inf_edge")
# the variants of the system in which a wrong statement must show: a subnormal d2 and ties at +0 are everywhere; a query without a
# candidate needs the NaN body or the two infinite ones; a d2 of +inf needs an overflow or an infinity
SHOWS_IN = {"flush": VARIANTS, "le": VARIANTS, "finite_start": ("nan", "inf"), "inf_edge": ("overflow", "inf")}
POINTS = 300


class Refs:
    def __init__(self, d):
        self.nbr, self.knn, self.fof, self.hist = (neighbors_common.make_ref(d), knn_common.make_ref(d), fof_common.make_ref(d),
                                                   hist_common.make_ref(d))


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return Refs(tmp_path_factory.mktemp("distance_ref"))


def ulp(x):
    """the unit in the last place of |x| (numpy.spacing, which looks upwards, has none for the largest finite value)"""
    ax = np.abs(np.asarray(x))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(ax == np.finfo(ax.dtype).max, ax - np.nextafter(ax, ax.dtype.type(0)), np.spacing(ax))


def bound(x):
    """what the fused d2 (three roundings) and the unfused one (five) may differ by at a finite non-zero value x: every term is
    non-negative, so each rounding is at most half a unit in the last place of a partial sum that does not exceed the result — 8 halves,
    4 units — or one smallest subnormal if that is larger"""
    return np.maximum(4 * ulp(x), np.finfo(np.asarray(x).dtype).smallest_subnormal)


def margin(x):
    """how far a d2 must be from a threshold or from the next d2 for the decision to be the same in both statements: four times the
    bound — twice for the two values that meet, twice again for a neighbour in the next binade, whose unit is twice as large"""
    return 4 * bound(x)


def groups_of(linked):
    """group[i] = the lowest index of i's connected component under the symmetric boolean matrix `linked`: a quick-find union-find"""
    n = len(linked)
    label = np.arange(n)
    for i in range(n):
        js = np.flatnonzero(linked[i, i + 1:])
        if len(js) == 0:
            continue
        labs = np.unique(np.append(label[js + i + 1], label[i]))
        if len(labs) > 1:
            label[np.isin(label, labs[1:])] = labs[0]
    return label.astype(np.int32)


class Statement:
    """The four passes on (pos, queries, skip) in plain numpy, in the dtype of pos.  queries None: the rows form.  wrong: None, or one
    of WRONG —
      "flush"         a subnormal d2 is +0;
      "le"            the scan replaces on <= (the last of equal values wins, and a +inf is chosen) and an edge holds d2 <= e;
      "finite_start"  the scan starts from the largest finite value instead of +inf;
      "inf_edge"      a d2 of +inf is below an edge of +inf."""

    def __init__(self, pos, queries=None, skip=None, wrong=None):
        assert wrong is None or wrong in WRONG
        self.dtype = pos.dtype.type
        self.fi = np.finfo(self.dtype)
        self.wrong = wrong
        self.rows = queries is None
        q = pos if self.rows else queries
        self.m, self.n = len(q), len(pos)
        with np.errstate(all="ignore"):
            dx, dy, dz = (pos[None, :, c] - q[:, None, c] for c in range(3))
            d2 = dx * dx + (dy * dy + dz * dz)
        assert d2.dtype == self.dtype and d2.shape == (self.m, self.n)
        if self.rows:
            skip = np.arange(self.n)
        if skip is not None:
            k = np.flatnonzero(np.asarray(skip) >= 0)
            d2[k, np.asarray(skip)[k]] = np.nan   # the excluded body is below nothing
        if wrong == "flush":
            d2[d2 < self.fi.tiny] = 0
        self.d2 = d2
        self.order = np.argsort(d2, axis=1, kind="stable")   # ascending (d2, index); NaN last
        self.sorted = np.take_along_axis(d2, self.order, 1)
        self.tri = tuple(np.take_along_axis(np.abs(c), self.order, 1) for c in (dx, dy, dz))
        with np.errstate(all="ignore"):   # at most one square is not zero: both statements return exactly that square
            self.single = np.take_along_axis(sum((c * c != 0).astype(np.int8) for c in (dx, dy, dz)) <= 1, self.order, 1)

    # ---- the passes
    def nearest(self):
        """(idx, d2) of the ascending scan"""
        start = self.dtype(self.fi.max if self.wrong == "finite_start" else np.inf)
        s0 = self.sorted[:, 0]
        with np.errstate(invalid="ignore"):
            if self.wrong == "le":
                ok = s0 <= start
                idx = self.n - 1 - np.argmax((self.d2 == s0[:, None])[:, ::-1], axis=1)
            else:
                ok = s0 < start
                idx = self.order[:, 0]
        return np.where(ok, idx, -1).astype(np.int32), np.where(ok, s0, start)

    def cum(self, t, side):
        """(m, len(t)): per query the number of d2 below ("left") or not above ("right") each t; a NaN d2 is neither"""
        t = np.atleast_1d(np.asarray(t, self.dtype))
        return np.stack([np.searchsorted(r, t, side) for r in self.sorted]).astype(np.int32)

    def count(self, r2):
        return self.cum(r2, "right")[:, 0]

    def knn(self, k):
        idx, d2 = np.full((self.m, k), -1, np.int32), np.full((self.m, k), np.inf, self.dtype)
        w = min(k, self.n)
        ok = self.sorted[:, :w] < np.inf
        idx[:, :w] = np.where(ok, self.order[:, :w], -1)
        d2[:, :w] = np.where(ok, self.sorted[:, :w], np.inf)
        return idx, d2

    def hist(self, edges):
        edges = np.asarray(edges, self.dtype)
        c = self.cum(edges, "right" if self.wrong == "le" else "left")
        if self.wrong == "inf_edge":
            c[:, np.isposinf(edges)] = self.cum(np.inf, "right")
        return np.diff(c, axis=1)

    def closest_pair(self):
        u = np.where(np.triu(np.ones((self.n, self.n), bool), 1) & (self.d2 < np.inf), self.d2, np.inf)
        f = int(np.argmin(u))   # the first of equal values: the lowest i, then the lowest j
        i, j = divmod(f, self.n)
        return (i, j, u[i, j]) if u[i, j] < np.inf else (-1, -1, self.dtype(np.inf))

    def fof(self, b2, unclear=0):
        """the groups at b2; unclear = -1 / +1: with every pair whose d2 is within the margin of b2 cut / linked"""
        b2 = self.dtype(b2)
        with np.errstate(invalid="ignore"):
            linked = self.d2 <= b2
            if unclear:
                linked = np.where(self.near_pairs(b2), unclear > 0, linked)
        return groups_of(linked)

    # ---- where a decision is safe from the five roundings against three
    def zone(self, t):
        """[lo, hi]: the finite non-zero d2 a threshold t cannot place safely — within the margin of t (t = 0: of the smallest subnormal);
        nothing for an infinite t, which only the class of a d2 decides"""
        t = self.dtype(t)
        if not np.isfinite(t):
            return None
        z = margin(t if t > 0 else self.fi.smallest_subnormal)
        with np.errstate(over="ignore"):
            return max(self.dtype(t - z), self.fi.smallest_subnormal), min(self.dtype(t + z), self.fi.max)

    def near_pairs(self, t):
        """(m, n): the d2 in the zone of the threshold t"""
        z = self.zone(t)
        with np.errstate(invalid="ignore"):
            return np.zeros(self.d2.shape, bool) if z is None else (self.d2 >= z[0]) & (self.d2 <= z[1])

    def clear_at(self, thresholds):
        """(m,): no d2 of the query is in the zone of any of the thresholds"""
        zones = [z for z in (self.zone(t) for t in np.atleast_1d(thresholds)) if z is not None]
        if not zones:
            return np.ones(self.m, bool)
        return (self.cum([z[1] for z in zones], "right") == self.cum([z[0] for z in zones], "left")).all(1)

    def clear_order(self, k):
        """(m,): entries 0 .. k of the ascending list (the k listed ones and the first one left out) are in an order the roundings
        cannot change — each next one either further away than the margin, or equal for a reason that holds in every arithmetic: both
        +0 (the classes agree), both no candidate, the same three |differences|, or both with a single square that is not zero"""
        w = min(k + 1, self.n)
        a, b = self.sorted[:, :w - 1], self.sorted[:, 1:w]
        with np.errstate(invalid="ignore", over="ignore"):
            apart = (b - a > margin(b)) | np.isnan(b) | (np.isposinf(b) & (a < np.inf))
            same_tri = np.ones(a.shape, bool)
            for c in self.tri:
                same_tri &= c[:, :w - 1] == c[:, 1:w]
            single = self.single[:, :w - 1] & self.single[:, 1:w]
            tied = (a == b) & ((b == 0) | np.isposinf(b) | same_tri | single) | (np.isnan(a) & np.isnan(b))
        return (apart | tied).all(1)


def all_pairs_of_the_reference(nbr, pos, queries):
    """(m, n): every d2 as tests/neighbors_ref.c computes it, one source at a time — a one-body system's nearest is that body unless its
    d2 is NaN or +inf, and its count at r2 = +inf tells those two apart (NaN: 0, +inf: 1)"""
    out = np.empty((len(queries), len(pos)), pos.dtype)
    for j in range(len(pos)):
        idx, d2, cnt = nbr.points(pos[j:j + 1], queries, r2=np.inf)
        assert np.all((idx == 0) | np.isposinf(d2)) and np.all(cnt[idx == 0] == 1)
        out[:, j] = np.where(cnt == 0, np.nan, d2)
    return out


def classes(d2):
    """0: NaN, 1: +inf, 2: +0, 3: any other value"""
    return np.where(np.isnan(d2), 0, np.where(np.isposinf(d2), 1, np.where(bits(d2) == 0, 2, 3)))


def compare_values(got, want, worst):
    """the same class everywhere; the finite non-zero values within the bound; worst[0] = the largest difference in units of the last
    place seen, worst[1] in smallest subnormals among the subnormal values"""
    assert np.array_equal(classes(got), classes(want))
    k = classes(want) == 3
    g, w = got[k].astype(np.float64), want[k].astype(np.float64)
    diff = np.abs(g - w)
    assert np.all(diff <= bound(want[k]).astype(np.float64))
    if diff.size:
        worst[0] = max(worst[0], float((diff / ulp(want[k]).astype(np.float64)).max()))
        sub = np.abs(want[k]) < np.finfo(want.dtype).tiny
        if sub.any():
            worst[1] = max(worst[1], float((diff[sub] / float(np.finfo(want.dtype).smallest_subnormal)).max()))


def share(clear, planted=None):
    """at least 95 % of the queries are held to exact agreement, every planted one among them"""
    assert clear.mean() >= 0.95, clear.mean()
    if planted is not None:
        assert np.all(clear[planted]), planted[~clear[planted]]
    return clear


def check_queries(refs, st, pos, pts, skip, radii, planted, worst, tag):
    """neighbours, k nearest neighbours and radial counts of one set of queries (pts None: the rows) against the statement"""
    nbr = (lambda r2: refs.nbr.rows(pos, r2=r2)) if pts is None else (lambda r2: refs.nbr.points(pos, pts, skip, r2=r2))
    clear1 = share(st.clear_order(1), planted)
    widx, wd2 = st.nearest()
    for r2 in radii:
        idx, d2, cnt = nbr(r2)
        compare_values(d2, wd2, worst)
        assert np.array_equal(idx == -1, widx == -1) and np.array_equal(idx[clear1], widx[clear1]), (tag, r2)
        ok = share(st.clear_at(r2), planted)
        assert np.array_equal(cnt[ok], st.count(r2)[ok]), (tag, r2)
    lists = {}
    for k in (32, 5, 4, 1):
        lists[k] = refs.knn.rows(pos, k) if pts is None else refs.knn.points(pos, pts, k, skip)
        assert np.array_equal(lists[k][0], lists[32][0][:, :k]) and same_nan(lists[k][1], lists[32][1][:, :k]), (tag, k)   # prefixes
        ok = share(st.clear_order(k), planted)
        widx_k, wd2_k = st.knn(k)
        compare_values(lists[k][1][ok], wd2_k[ok], worst)
        assert np.array_equal(lists[k][0] == -1, widx_k == -1) and np.array_equal(lists[k][0][ok], widx_k[ok]), (tag, k)   # the padding everywhere
    assert np.array_equal(lists[1][0][:, 0], nbr(None)[0]) and same_nan(lists[1][1][:, 0], nbr(None)[1]), tag   # column 0 is the neighbour pass
    for n_bins in HOSTILE_BINS:
        e = hostile_edges(pos, n_bins)
        got = refs.hist.rows(pos, e) if pts is None else refs.hist.points(pos, pts, e, skip)
        ok = share(st.clear_at(e), planted)
        want = st.hist(e)
        assert np.array_equal(got[ok], want[ok]), (tag, n_bins)
        assert np.array_equal(got.sum(1), want.sum(1)) and np.all(got[:, e[:-1] == e[1:]] == 0), (tag, n_bins)   # every finite d2 once; the empty bin
    return lists[32]


def check_labels(refs, st, pos, n, variant, knn32, radii):
    """the planted rows do what their labels say, in the references' own output"""
    dtype = pos.dtype.type
    fi = np.finfo(dtype)
    h = float(distance_h(dtype))
    idx, d2, cnt = refs.nbr.rows(pos, r2=np.inf)
    assert (idx[62], idx[65]) == (65, 62) and d2[62] == d2[65] == dtype(4 * h * h) and 0 < d2[62] < fi.tiny
    assert knn32[0][62, 0] == 65 and knn32[0][65, 0] == 62 and d2[62] < knn32[1][62, 1] <= dtype(9 * h * h) and d2[65] < knn32[1][65, 1] < fi.tiny
    assert st.d2[62, 22] == st.d2[62, 64] == dtype(9 * h * h)   # the bodies at zero
    # the exact zeros: partners at +0 in ascending index (each other; 10, 11 and 64 by underflow), then two distinct subnormal values
    for i, other in ((22, 23), (23, 22)):
        assert list(knn32[0][i, :6]) == sorted((10, 11, 64, other)) + [62, 65] and np.all(bits(knn32[1][i, :4]) == 0)
        assert list(knn32[1][i, 4:6]) == [dtype(9 * h * h), dtype(25 * h * h)] and knn32[1][i, 5] < fi.tiny
        assert np.any(pos[i, :3] != pos[10, :3]) and np.any(pos[i, :3] != pos[64, :3])
    e32 = hostile_edges(pos, 32)
    rows32 = refs.hist.rows(pos, e32)
    if variant == "overflow":
        assert (idx[63], idx[66]) == (66, 63) and np.isfinite(d2[63]) and d2[63] == d2[66] > 1
        assert np.all(knn32[0][[63, 66], 1:] == -1) and np.all(np.isposinf(knn32[1][[63, 66], 1:]))
        assert list(rows32[63]) == [0] * 30 + [1, 0] and list(rows32[66]) == [0] * 30 + [1, 0]   # the one finite d2, below the largest finite edge
    if variant == "inf":
        assert idx[63] == idx[66] == -1 and np.all(np.isposinf(d2[[63, 66]]))
        assert np.all(knn32[0][[63, 66]] == -1) and np.all(np.isposinf(knn32[1][[63, 66]])) and not np.any(rows32[[63, 66]])
        assert cnt[63] == cnt[66] == n - 2   # +inf <= +inf for every body but the other infinite one (inf - inf = NaN)
    if variant in ("overflow", "inf"):
        for n_bins in HOSTILE_BINS:
            assert refs.hist.rows(pos, hostile_edges(pos, n_bins), 0, 1).sum() < n - 1   # a +inf d2 is below no edge, +inf included ...
        assert cnt[0] == n - 1                                                            # ... and is counted at r2 = +inf
    nans = int(np.isnan(pos[:, :3]).any(1).sum())
    assert nans == (variant == "nan")
    group, n_groups = refs.fof.groups(pos, dtype(np.inf))
    assert n_groups == 1 + nans and (variant != "nan" or group[nan_row(n)] == nan_row(n))
    if variant == "inf":
        assert group[63] == group[66] == 0   # through any finite body: inf <= inf
    group, n_groups = refs.fof.groups(pos, dtype(0))
    assert all(group[i] == 10 for i in (10, 11, 22, 23, 64)) and int((group == 10).sum()) == 5 and group[62] == 62 and group[65] == 65
    if n > 1028:
        members = [i for i in range(1023, 1029) if not (variant == "nan" and i == 1024)]
        assert all(group[i] == 1023 for i in members) and int((group == 1023).sum()) == len(members)
    if variant == "overflow":
        between = radii[4]   # the largest finite: between d2(63, 66) and +inf
        group, _ = refs.fof.groups(pos, between)
        assert group[63] == group[66] == 63 and int((group == 63).sum()) == 2


def check_discrimination(pos, n, variant, radii):
    """each wrong statement changes what is expected of at least one pass, on the planted rows alone"""
    rows = planted_rows(n, variant)
    q, sk = pos[rows], rows.astype(np.int32)
    right = Statement(pos, q, sk)
    edges = [hostile_edges(pos, b) for b in HOSTILE_BINS]

    def outputs(st):
        idx, d2 = st.nearest()
        return {"neighbours": (idx, bits(d2)) + tuple(st.count(r2) for r2 in radii),
                "knn": st.knn(32)[:1], "hist": tuple(st.hist(e) for e in edges)}

    want = outputs(right)
    shown = {}
    for wrong in WRONG:
        got = outputs(Statement(pos, q, sk, wrong))
        shown[wrong] = [p for p in want if not all(np.array_equal(a, b) for a, b in zip(got[p], want[p]))]
        if variant in SHOWS_IN[wrong]:
            assert shown[wrong], (n, variant, wrong)
    assert "neighbours" in shown["flush"] and "knn" in shown["flush"] and "hist" in shown["flush"]
    return shown


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_references_against_the_numpy_statement(nb, refs, dtype, n):
    """Every variant at one size and precision.  Every d2 of neighbors_ref.c (one source at a time) has the numpy statement's class —
    NaN, +inf, +0, other — and, where finite and non-zero, its value to 4 units in the last place or one smallest subnormal, the derived
    bound (bound() above).  Measured, worst over the variants, rows and 300 points, in units of the last place:
      binary32  n = 70: 2.0   n = 1100: 2.0   n = 2085: 2.0        binary64  n = 70: 1.0   n = 1100: 1.0   n = 2085: 1.0
    and 0 smallest subnormals among the subnormal values (the planted ones are exact in both statements).
    idx, list order, counts, bins and groups agree exactly wherever the statement's decision is further than the margin from a
    threshold or a tie — at every planted row and at >= 95 % of the queries of every case, both asserted (measured: every query at
    n = 70 and in binary64, 98.6 % at n = 1100 and 98.0 % at n = 2085 in binary32, the lowest of any list or edge set)."""
    worst = [0.0, 0.0]
    clear_share = 1.0
    for variant in VARIANTS:
        pos = hostile_distance_system(nb, n, dtype, variant)[0]
        planted = planted_rows(n, variant)
        radii = hostile_radii(pos)
        st = Statement(pos)
        own = np.eye(n, dtype=bool)   # the statement leaves a row's own body out, the one-source reference does not
        compare_values(np.where(own, np.nan, all_pairs_of_the_reference(refs.nbr, pos, pos)), st.d2, worst)
        knn32 = check_queries(refs, st, pos, None, None, radii, planted, worst, (n, variant, "rows"))
        clear_share = min(clear_share, st.clear_order(32).mean(), st.clear_at(hostile_edges(pos, 32)).mean())
        # the closest pair, and the pair histogram as half the rows' sums
        i, j, d2 = refs.nbr.closest_pair(pos)
        wi, wj, wd2 = st.closest_pair()
        assert (i, j) == (wi, wj) == (10, 11) and bits(d2) == bits(wd2) == 0, (n, variant)
        for n_bins in HOSTILE_BINS:
            e = hostile_edges(pos, n_bins)
            rows = refs.hist.rows(pos, e).astype(np.int64).sum(0)
            assert np.all(rows % 2 == 0) and np.array_equal(refs.hist.pairs(pos, e), rows // 2), (n, variant, n_bins)
        # the groups: exact wherever cutting or linking every pair within the margin of b2 gives the same groups
        for b2 in hostile_b2(pos):
            want = st.fof(b2)
            if st.near_pairs(b2).any():
                assert np.array_equal(st.fof(b2, -1), want) and np.array_equal(st.fof(b2, +1), want), (n, variant, b2)
            group, n_groups = refs.fof.groups(pos, b2)
            assert np.array_equal(group, want) and n_groups == int((want == np.arange(n)).sum()), (n, variant, b2)
            # a body is alone iff nobody is within b2 — iff its nearest d2 is not <= b2, where it has a nearest (the +inf of a body
            # without a candidate is no distance: the NaN body is alone at b2 = +inf)
            idx, d2, cnt = refs.nbr.rows(pos, r2=b2)
            alone = np.bincount(group, minlength=n)[group] == 1
            assert np.array_equal(alone, cnt == 0) and np.array_equal(alone[idx >= 0], ~(d2 <= b2)[idx >= 0]), (n, variant, b2)
        check_labels(refs, st, pos, n, variant, knn32, radii)
        # the points form, with and without skip
        pts, skip = hostile_points(nb, pos, POINTS, variant)
        plain = Statement(pos, pts)
        compare_values(all_pairs_of_the_reference(refs.nbr, pos, pts), plain.d2, worst)
        for sk in (skip, None):
            sp = plain if sk is None else Statement(pos, pts, sk)
            check_queries(refs, sp, pos, pts, sk, radii, None, worst, (n, variant, "points", sk is not None))
        shown = check_discrimination(pos, n, variant, radii)
        print("%s n=%d %s: wrong statements show in %s" % (np.dtype(dtype).name, n, variant, shown))
    print("%s n=%d: reference against the numpy statement in the same precision: worst %.2f units in the last place (bound 4), "
          "%.2f smallest subnormals among the subnormal d2 (bound 4); exact agreement held at >= %.4f of the queries"
          % (np.dtype(dtype).name, n, worst[0], worst[1], clear_share))


def test_hostile_system_is_untouched_below_the_new_rows(nb):
    """hostile_system's output is what it was, and the new helper changes the rows it names and nothing else"""
    for dtype in (np.float32, np.float64):
        for variant in VARIANTS:
            n = 1100
            pos, vel, far = hostile_system(nb, n, dtype, variant)
            dpos, dvel, dfar = hostile_distance_system(nb, n, dtype, variant)
            keep = np.setdiff1d(np.arange(n), DISTANCE_ROWS)
            assert same_nan(dpos[keep], pos[keep]) and same_nan(dvel, vel) and np.array_equal(dfar, far)
            again = hostile_system(nb, n, dtype, variant)[0]
            assert same_nan(again, pos) and not same_nan(dpos[[62, 65]], pos[[62, 65]])   # a copy was changed, not the system
            assert same_nan(dpos[66], pos[66]) == (variant in ("base", "nan"))
    # the rows other tests' recorded numbers rest on, by value: one size and variant
    pos = hostile_system(nb, 1100, np.float32, "overflow")[0]
    cloud = nb.make_bodies(1100, seed=1234, dtype=np.float32)[0]
    named = [10, 11, 22, 23, 40, 41, 63, 64, 1023, 1025, 1026, 1027, 1028, 1099]
    assert same_nan(np.delete(pos, named, 0), np.delete(cloud, named, 0))
    assert pos[63, :3].tolist() == [np.float32(3e19), np.float32(-2e19), np.float32(1e19)] and pos[64, :3].tolist() == [np.float32(1e-38), np.float32(-1e-38), 0.0]
    assert np.all(bits(pos[22, :3]) == [0x80000000, 0, 0x80000000]) and same_nan(pos[1023, :3], pos[1024, :3])


def test_radii_edges_and_linking_lengths(nb):
    for dtype in (np.float32, np.float64):
        fi = np.finfo(dtype)
        h = float(distance_h(dtype))
        pos = hostile_distance_system(nb, 1100, dtype, "overflow")[0]
        radii = hostile_radii(pos)
        assert [type(r) for r in radii] == [dtype] * 6 and radii == hostile_b2(pos)
        sub = subnormal_between(dtype)
        assert radii[0] == 0 and radii[1] == sub and 4 * h * h < sub < 9 * h * h < fi.tiny and radii[2] == fi.tiny
        assert 0.1 < radii[3] < 12.5 and radii[4] == fi.max and np.isposinf(radii[5])
        for n_bins in HOSTILE_BINS:
            e = hostile_edges(pos, n_bins)
            assert e.dtype == dtype and len(e) == n_bins + 1 and not np.any(np.isnan(e)) and not np.any(e[1:] < e[:-1])
            assert (np.isneginf(e[0]) or e[0] == 0) and int((e == 0).sum()) == 2 and sub in e and np.isposinf(e[-1])
            if n_bins > 3:
                assert fi.tiny in e and fi.max in e and dtype(12.5) in e and dtype(1e-3) in e
