"""One hostile system for the smooth passes (energy, potential, field) and the force path, stated once: the inputs a uniform cloud never
produces — coincident bodies across a 64-source window edge and a 1024-source block edge, a separation whose square underflows, signed
zeros, a near-subnormal body, bodies so far away that inv^2 or inv^3 is subnormal or zero while d2 is finite, squares that overflow, an
infinity, a NaN — and the points and skip indices that land on the edges of the field pass's loops; and, for the four passes that take
the plain squared distance without a softening (neighbours, k nearest neighbours, friends-of-friends, radial counts), the same system
with a subnormal d2, a d2 that overflows for all partners but one and an inf - inf planted on top (hostile_distance_system), its radii,
edges and linking lengths, and hand-made two- and three-body systems.  A plain helper module like field_common.py (no fixtures, no
hooks)."""
import numpy as np

VARIANTS = ("base", "overflow", "nan", "inf")
SIZES = (70, 1100, 2085)     # one block with a ragged tail; two blocks, a tail of 12; three blocks with a ragged tail
POINT_COUNTS = (1, 65, 300)


def nan_row(n):
    """the body the "nan" variant poisons: the first row of the second block where there is one"""
    return 1024 if n > 1024 else n // 2


def special_row(n, variant):
    """the body a variant adds (None for "base"): what a skip index must be able to remove without a trace"""
    return {"base": None, "overflow": 63, "inf": 63, "nan": nan_row(n)}[variant]


def hostile_system(nb, n, dtype, variant):
    """(pos, vel, far): make_bodies(n, seed=1234) with the rows below overwritten (a row that does not exist at this n is left out), and
    the indices of the far-away bodies — the rows whose own results are dominated by one- or two-bit subnormals and are therefore held
    to finiteness and to bit comparisons, never to a tolerance."""
    assert variant in VARIANTS
    dtype = np.dtype(dtype).type
    f32 = dtype is np.float32
    pos, vel = nb.make_bodies(n, seed=1234, dtype=dtype)
    far = []

    def put(a, i, xyz):
        if 0 <= i < n:
            a[i, :3] = xyz
            return True
        return False

    # coincident groups across the window edge 1023 | 1024, which is the block edge too
    for i in (1023, 1025, 1026, 1027, 1028):
        if 1024 < n:
            put(pos, i, pos[1024, :3])
    small = dtype(1e-30 if f32 else 1e-170)
    put(pos, 11, [2 * small, -3 * small, small])                         # small enough for the difference below to survive the addition
    pos[10, :3] = pos[11, :3] + small                                    # a difference whose square underflows: d2 == eps exactly
    put(pos, 22, [-0.0, 0.0, -0.0])
    put(pos, 23, [0.0, -0.0, 0.0])
    tiny = 1e-38 if f32 else 1e-307
    put(pos, 64, [tiny, -tiny, 0.0])                                     # next to the subnormal range
    if put(pos, 40, [1e10, 1e10, 1e10]):                                 # large, inv^3 still normal
        far.append(40)
    # d2 finite, inv^2 or inv^3 subnormal or zero
    if put(pos, 41, [2e14, -1e15, 3e13] if f32 else [2e104, -1e105, 3e103]):
        far.append(41)
    if put(pos, n - 1, [-4e12, 1e13, 2e12] if f32 else [-4e102, 1e103, 2e102]):
        far.append(n - 1)
    if variant == "overflow":
        put(pos, 63, [3e19, -2e19, 1e19] if f32 else [3e160, -2e160, 1e160])   # d2 = inf, inv = 0
        far.append(63)
    elif variant == "inf":
        pos[63, 0] = np.inf                                              # dx = inf, inf * 0 = NaN in every arithmetic
        far.append(63)
    elif variant == "nan":
        pos[nan_row(n), 1] = np.nan
    # the energy totals' velocities
    put(vel, 5, [-0.0, 0.0, -0.0])
    big = 1e18 if f32 else 1e150
    vel[6, 0] = big
    vel[7, 1] = 1.0 / big
    if variant == "nan":
        vel[8, 2] = np.nan
    return pos, vel, np.array(sorted(set(far)), np.int64)


def hostile_points(nb, pos, m, variant):
    """(points, skip) for the field pass on hostile_system(...)'s pos: 1.5 x cloud points (field_common.make_points' family) with,
    as far as m reaches,
      points 0 ..        on bodies 0, 63, 64, 1023, 1024 and n - 1 (those there are), each with skip = that body and with skip = -1;
      then               one point on nan_row(n) with skip = -1 and two cloud points whose skip is the variant's special body (body 63
                         in "base");
      points 64 .. 127   a wave whose 64 points share one skip index, the last row of the first block (clipped to n - 1);
      points 128 .. 191  a wave in which only lane 37 has a skip, the first row of the second block (clipped to n - 1): the NaN body
                         where there is one;
      points 192 ..      cloud points, every third with an arbitrary skip;
      the last point     skip = n - 1 (m is no multiple of 64: the lanes beyond m are clamped to this point)."""
    n = len(pos)
    pts = (1.5 * nb.make_bodies(m, seed=77)[0].astype(np.float64)).astype(pos.dtype)
    skip = np.full(m, -1, np.int32)
    plan = []
    for b in sorted({b for b in (0, 63, 64, 1023, 1024, n - 1) if b < n}):
        plan += [(b, b), (b, -1)]
    plan.append((nan_row(n), -1))
    special = special_row(n, variant)
    special = 63 if special is None else special
    plan += [(None, special), (None, special)]
    for k, (body, sk) in enumerate(plan[:m]):
        if body is not None:
            pts[k] = pos[body]
        skip[k] = sk
    if m >= 128:
        skip[64:128] = min(1023, n - 1)
    if m >= 192:
        skip[128 + 37] = min(1024, n - 1)
    for p in range(192, m):
        if p % 3 == 1:
            skip[p] = (p * 7919) % n
    skip[m - 1] = n - 1
    return pts, skip


# ---- the dynamic passes (snap, sixth-order Hermite, block steps) and the masses ----

DYNAMIC_FAST = 1e6   # the one fast velocity of hostile_dynamic_system, both precisions


def hostile_dynamic_system(nb, n, dtype, variant):
    """(pos, vel, far) of hostile_system(...) with the one velocity tamed: vel[6, 0] = 1e6 in both precisions, vel[7, 1] = 1e-6.
    hostile_system's 1e18 (1e150) was put there for the energy totals.  In the snap w . w times inv^2 overflows with it (binary32: rows 6
    and 37 at n = 70, 13 rows at n = 1100, the acceleration and the jerk stay finite), and the sixth-order predictor carries a row's
    a0 + h j0 + c2 s0 + c3 c0 to every other row through g, so that one non-finite row leaves no finite row after one step: a test on
    that input compares NaN with NaN and passes for almost any kernel.  With 1e6 every row of "base" and "overflow" stays finite through
    three shared steps of 1/256 and through one block of eta 0.04, dt_max 1/256 on 8 levels, whose rows still spread over the levels
    (1e9 or 1e50 stay finite too but leave levels 0 and 7 only; 1e12 or 1e75 do not stay finite).  tests/test_specials_reference.py
    asserts all of it."""
    pos, vel, far = hostile_system(nb, n, dtype, variant)
    vel = vel.copy()
    vel[6, 0] = DYNAMIC_FAST
    vel[7, 1] = 1.0 / DYNAMIC_FAST
    return pos, vel, far


def hostile_point_words(nb, m, dtype, vel=None, acc=None):
    """(pvel, pacc) for hostile_points(...) on hostile_dynamic_system(...)'s bodies: the cloud words of test_gpu_snap.point_words with
      points 0 and 1   (both sit on body 0; point 0 skips it, point 1 does not) the body's own velocity vel[0] and acceleration acc[0],
                       acc being the accelerations the pass gives the sources: w = g = +0 exactly on the coincident pair, which then adds
                       +0 to all nine sums, so the two points get the same bits.  Without vel or acc: signed zeros in their place;
      the last point   signed zeros, -0 +0 -0 in the velocity and +0 -0 +0 in the acceleration (at m = 1 it is point 0: the body's own
                       words where they are given)."""
    dtype = np.dtype(dtype).type
    pvel, pacc = nb.make_bodies(m, seed=78, dtype=dtype)[1], nb.make_bodies(m, seed=79, dtype=dtype)[1]
    for k in sorted({m - 1, min(1, m - 1), 0}, reverse=True):
        pvel[k, :3] = [-0.0, 0.0, -0.0]
        pacc[k, :3] = [0.0, -0.0, 0.0]
        if k <= 1 and vel is not None:
            pvel[k, :3] = vel[0, :3]
        if k <= 1 and acc is not None:
            pacc[k, :3] = acc[0, :3]
    return pvel, pacc


MASS_ROWS = {12: "+0", 13: "-0", 14: "smallest subnormal", 15: "smallest normal", 16: "2^20", 17: "2^-20", 22: "+0", 1024: "+0",
             30: "negative", 41: "far and heavy"}
INF_MASS_ROW = 33     # a finite cloud row
NAN_PAYLOAD = 0x1234  # the "nan" variant's mass is a quiet NaN with this payload: a download must bring it back bit for bit


def far_mass(dtype):
    """the mass of the far body 41: 2^100 (binary32) or 2^300 (binary64) — its inv^3 is subnormal or zero while m * inv^3 would be
    normal; small enough for m_i m_j of the energy totals to stay finite (2^700 in binary64 does not)"""
    return np.dtype(dtype).type(2.0 ** 100 if np.dtype(dtype) == np.float32 else 2.0 ** 300)


def hostile_masses(n, dtype, variant):
    """n masses for the w of hostile_dynamic_system(...)'s positions: masses_common.random_masses (log-uniform in [0.25, 4)) with
      rows 12 .. 17   +0, -0, the smallest subnormal, the smallest normal, 2^20, 2^-20
      rows 22, 1024   +0 (a massless body at signed zeros, and one on the coincident group at the block edge)
      row 30          -1.5: nothing is promised about negative masses, but the strict bits are the statement's
      row 41          far_mass(dtype) on the far body
    and per variant  "nan": a NaN with a payload on special_row(n, "nan");  "inf": +inf on row 33, a finite cloud body;
    "overflow": +0 on body 63, whose d2 overflows.  A row that does not exist at this n is left out."""
    from masses_common import random_masses
    assert variant in VARIANTS
    dtype = np.dtype(dtype).type
    fi = np.finfo(dtype)
    w = random_masses(n, 5, dtype)
    planted = {12: 0.0, 13: -0.0, 14: fi.smallest_subnormal, 15: fi.tiny, 16: 2.0 ** 20, 17: 2.0 ** -20, 22: 0.0, 1024: 0.0, 30: -1.5,
               41: far_mass(dtype)}
    assert set(planted) == set(MASS_ROWS)
    for i, v in planted.items():
        if i < n:
            w[i] = v
    if variant == "nan":
        u = {4: np.uint32, 8: np.uint64}[w.itemsize]
        quiet = np.array([np.nan], dtype).view(u)
        w[nan_row(n)] = (quiet | u(NAN_PAYLOAD)).view(dtype)[0]
    elif variant == "inf":
        w[INF_MASS_ROW] = np.inf
    elif variant == "overflow":
        w[63] = 0.0
    return w


def distance_h(dtype):
    """h of hostile_distance_system: 2^-70 (binary32) or 2^-520 (binary64) — h * h is far below the smallest subnormal's neighbours'
    reach (4 h^2 = 2^11 or 2^36 smallest subnormals), and h is far above the ±tiny, ±1e-30 (1e-170) bodies around the origin"""
    dtype = np.dtype(dtype).type
    return dtype(2.0 ** -70 if dtype is np.float32 else 2.0 ** -520)


def subnormal_between(dtype):
    """6 h^2: a subnormal strictly between the planted pair's d2 = 4 h^2 and its d2 = 9 h^2 to the bodies at zero"""
    h = float(distance_h(dtype))
    return np.dtype(dtype).type(6.0 * h * h)


def hostile_distance_system(nb, n, dtype, variant):
    """(pos, vel, far) of hostile_system(...) with further rows overwritten on a copy, for the four passes that take the plain squared
    distance without a softening (neighbours, k nearest neighbours, friends-of-friends, radial counts), where d2 itself can be
    subnormal, underflow to +0 between distinct bodies, overflow, or be inf - inf:
      rows 62, 65   (3h, 0, 0) and (5h, 0, 0), h = distance_h(dtype), either side of the 63 | 64 window edge: d2(62, 65) = 4 h^2 and
                    d2 = 9 h^2 (25 h^2) to the bodies at zero (22, 23; 10, 11 and 64 are at zero as far as h can tell) are exact, non-zero
                    and subnormal, so the two are each other's nearest — unless a subnormal is flushed, which ties them at 0 with rows
                    10, 11, 22, 23 and 64.  Rows 22 and 23 get partners at exactly +0 (each other; 10, 11, 64 by underflow) followed by
                    two distinct subnormal values.
      row 66        "overflow": row 63's position with x four units in the last place up — d2(63, 66) is large and finite while both
                    are at +inf from everybody else.  "inf": x = +inf as row 63's — inf - inf = NaN between the two, +inf to the rest.
                    "base", "nan": the cloud body it was."""
    pos, vel, far = hostile_system(nb, n, dtype, variant)
    pos = pos.copy()
    dtype = pos.dtype.type
    assert n > 66
    h = distance_h(dtype)
    pos[62, :3] = [3 * h, 0, 0]
    pos[65, :3] = [5 * h, 0, 0]
    if variant == "overflow":
        pos[66, :3] = pos[63, :3]
        for _ in range(4):
            pos[66, 0] = np.nextafter(pos[66, 0], dtype(np.inf))
    elif variant == "inf":
        pos[66, 0] = np.inf
    return pos, vel, far


DISTANCE_ROWS = (62, 65, 66)   # the rows hostile_distance_system overwrites


def planted_rows(n, variant):
    """every row of hostile_distance_system(...) whose distances were put where they are on purpose (those that exist at this n; row
    40's 1e10 is an ordinary large position to a plain distance)"""
    rows = {10, 11, 22, 23, 41, 62, 63, 64, 65, 66, n - 1, nan_row(n)} | ({1023, 1024, 1025, 1026, 1027, 1028} if n > 1028 else set())
    return np.array(sorted(r for r in rows if 0 <= r < n), np.int64)


def _r2_030(pos):
    """the radius (squared) that holds about 30 % of the bodies around body 0 (neighbors_common.r2_for at 0.3, without its overflow
    warnings), moved up by 2^-10 of itself: off body 0's own d2 it was read from, into the gap above it"""
    with np.errstate(all="ignore"):
        d = ((pos[:, :3].astype(np.float64) - pos[0, :3].astype(np.float64)) ** 2).sum(1)
    return pos.dtype.type(np.sort(d)[min(len(d) - 1, int(0.3 * len(d)))] * (1.0 + 2.0 ** -10))


def hostile_radii(pos):
    """r2 for the neighbour count, in the dtype of pos: 0, the subnormal between the planted pair's two distances, the smallest normal,
    a radius that holds about 30 % of the bodies around body 0, the largest finite, +inf"""
    dtype = pos.dtype.type
    fi = np.finfo(dtype)
    return [dtype(0), subnormal_between(dtype), dtype(fi.tiny), _r2_030(pos), dtype(fi.max), dtype(np.inf)]


def hostile_b2(pos):
    """the linking lengths (squared) for friends-of-friends: the same six values"""
    return hostile_radii(pos)


HOSTILE_BINS = (3, 9, 17, 32)   # capacities 4, 16, 32 and the full 32: binary32 edges in SGPRs (up to 16) and in VGPRs (32)


def hostile_edges(pos, n_bins):
    """n_bins + 1 squared radii, non-decreasing, in the dtype of pos.  n_bins = 9, 17, 32:
        -inf (9, 32) or nothing (17), 0, 0 (an empty bin), the subnormal between the planted pair's two distances, the smallest normal,
        geometric steps from 1e-3 up to 12.5, the largest finite, +inf;
    n_bins = 3 has room for four edges only: 0, 0, that subnormal, +inf."""
    dtype = pos.dtype.type
    fi = np.finfo(dtype)
    assert n_bins in HOSTILE_BINS
    if n_bins == 3:
        return np.array([0, 0, subnormal_between(dtype), np.inf], dtype)
    head = ([] if n_bins == 17 else [-np.inf]) + [0, 0, subnormal_between(dtype), fi.tiny]
    steps = n_bins + 1 - len(head) - 2
    e = np.array(head + list(np.geomspace(1e-3, 12.5, steps)) + [fi.max, np.inf], dtype)
    assert len(e) == n_bins + 1 and not np.any(e[1:] < e[:-1])
    return e


def hand_made_distances(dtype):
    """(systems, v): two- and three-body systems whose plain distances are known by construction, {name: (n, 4) positions}, and the
    values their answers are made of — v.h2 = (2h)^2, an exact non-zero subnormal; v.u, a separation whose square underflows to +0;
    v.big, a coordinate whose square overflows; v.max, the largest finite; v.sub, the smallest subnormal."""
    dtype = np.dtype(dtype).type
    f32 = dtype is np.float32
    fi = np.finfo(dtype)
    h = float(distance_h(dtype))
    u, big = (1e-30, 1e30) if f32 else (1e-170, 1e200)

    class v:
        pass
    v.h2, v.u, v.big, v.max, v.sub, v.inf = dtype(4 * h * h), dtype(u), dtype(big), dtype(fi.max), dtype(fi.smallest_subnormal), dtype(np.inf)
    assert 0 < v.h2 < fi.tiny and v.u * v.u == 0 and v.u > 0
    rows = {"alone": [[1, 2, 3]],
            "coincident": [[1, 1, 1], [1, 1, 1]],
            "underflow": [[0, 0, 0], [u, 0, 0]],                         # distinct, d2 = +0
            "subnormal": [[0, 0, 0], [2 * h, 0, 0]],                     # d2 = v.h2
            "overflow": [[0, 0, 0], [big, 0, 0], [0, 3, 0]],             # d2 = +inf to body 1, 9 between the other two
            "nan": [[0, 0, 0], [np.nan, 0, 0], [0, 3, 0]],               # d2 = NaN to body 1
            "inf": [[0, 0, 0], [np.inf, 0, 0], [0, 3, 0]],               # d2 = +inf to body 1
            "two_inf": [[np.inf, 0, 0], [np.inf, 1, 0], [0, 0, 0]],      # inf - inf = NaN between 0 and 1, +inf to body 2
            "tied": [[1, 1, 0], [1, 0, 1], [0, 1, 1]]}                   # every pair at d2 = 2
    systems = {}
    for name, xyz in rows.items():
        pos = np.ones((len(xyz), 4), dtype)
        pos[:, :3] = xyz
        systems[name] = pos
    return systems, v


def near(x, far=()):
    """rows or points with every |coordinate| <= 2 that are not in `far`: where the tolerances of the timed arithmetic apply"""
    with np.errstate(invalid="ignore"):
        ok = np.all(np.abs(x[:, :3].astype(np.float64)) <= 2.0, axis=1)
    ok[np.asarray(far, np.int64)] = False
    return ok


def bits(a):
    return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_nan(a, b):
    """the same NaN mask and identical bits everywhere else (as test_extreme_values_strict_bit_exact compares); None equals None"""
    if a is None or b is None:
        return a is None and b is None
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb_ = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb_) and np.array_equal(bits(a)[~na], bits(b)[~nb_]))


def within(got, want, bound):
    """|got - want| <= bound where want is finite, and NaN exactly where want is NaN (no element is left out)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    with np.errstate(invalid="ignore"):
        return bool(np.array_equal(np.isnan(got), nan) and np.all(np.abs(got - want)[~nan] <= np.broadcast_to(bound, want.shape)[~nan]))
