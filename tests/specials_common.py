"""One hostile system for the smooth passes (energy, potential, field) and the force path, stated once: the inputs a uniform cloud never
produces — coincident bodies across a 64-source window edge and a 1024-source block edge, a separation whose square underflows, signed
zeros, a near-subnormal body, bodies so far away that inv^2 or inv^3 is subnormal or zero while d2 is finite, squares that overflow, an
infinity, a NaN — and the points and skip indices that land on the edges of the field pass's loops.  A plain helper module like
field_common.py (no fixtures, no hooks)."""
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
