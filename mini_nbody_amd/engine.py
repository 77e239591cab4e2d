"""Host-side mirror of the path's interface: bodyForce()/integrate() on a
{pos, vel} structure of arrays, the device-resident step loop and the
force-only (mailbox) entry point — thin Python over the C-ABI of
include/nbody.h.  All compute happens in libnbody_hip.so (HIP, gfx950).
"""
import ctypes as C

import numpy as np

from . import _lib as L


def _as(a, dtype):
    a = np.ascontiguousarray(a, dtype)
    if a.ndim != 2 or a.shape[1] != 4:
        raise ValueError("expected an (n, 4) array of %s words" % np.dtype(dtype).name)
    return a


class NBody:
    """One context per process (the reference handles one request at a time, S/top_level.vhd:180-186)."""

    def __init__(self, n, fp64=False, tile=0, ngpus=1, rank=None, nranks=None, uid=None):
        self.lib = L.load()
        self.n, self.fp64 = int(n), bool(fp64)
        self.dtype = np.float64 if fp64 else np.float32
        if rank is None:
            L.check(self.lib.nbody_init(self.n, int(ngpus), int(self.fp64), int(tile)))
        else:
            buf = C.create_string_buffer(bytes(uid), 128) if uid is not None else None
            L.check(self.lib.nbody_init_rank(self.n, int(self.fp64), int(tile), int(rank), int(nranks), buf))
        self._by_rank = rank is not None   # rows are those of this rank's slice (nbody_init_rank)
        self._open = True
        self.fof_rounds = None             # link passes of the last fof() call
        self.binaries_found = None         # pairs the last binaries() call found (it may have returned fewer: max_pairs)

    # ---- options / info ----
    def set_option(self, key, value):
        """(A strict binary32 arithmetic is granted by the library only after every device of the context has proved its 1/sqrt —
        nbody_strict_proof in include/nbody.h — and refused with ERR_UNSUPPORTED otherwise.)"""
        L.check(self.lib.nbody_set_option(int(key), int(value)))

    def info(self, key):
        v = C.c_longlong()
        L.check(self.lib.nbody_get_info(int(key), C.byref(v)))
        return v.value

    @property
    def config(self):
        names = {L.VARIANT_SMEM: "smem", L.VARIANT_LDS: "lds", L.VARIANT_READLANE: "readlane", L.VARIANT_ISA: "isa"}
        sums = {L.SUM_SEQ: "seq", L.SUM_FPGA16: "fpga16", L.SUM_BLOCKED: "blocked"}
        return dict(variant=names.get(self.info(L.INFO_VARIANT), "?"), iblock=self.info(L.INFO_IBLOCK),
                    jsub=self.info(L.INFO_JSUB), nseg=self.info(L.INFO_NSEG), tile=self.info(L.INFO_TILE),
                    sum_order=sums.get(self.info(L.INFO_SUM_ORDER), "?"), sum_block=self.info(L.INFO_SUM_BLOCK),
                    launches_per_step=self.info(L.INFO_LAUNCHES_PER_STEP), wsplit=self.info(L.INFO_WSPLIT),
                    isa_phase=self.info(L.INFO_ISA_PHASE), long_buffers=self.info(L.INFO_LONG_BUFFERS),
                    xcd_map=self.info(L.INFO_XCD_MAP), fuse=self.info(L.INFO_FUSE_COMBINE),
                    n_local=self.info(L.INFO_N_LOCAL), first_body=self.info(L.INFO_FIRST_BODY),
                    rank=self.info(L.INFO_RANK), nranks=self.info(L.INFO_NRANKS), masses=self.info(L.INFO_MASSES),
                    pairing={1: "ordered", 2: "mutual", 3: "ordered (no memory for the mutual table)"}.get(self.info(L.INFO_PAIRING), "?"))

    def use_masses(self, on=True):
        """NBODY_OPT_MASSES: with on, body j has the mass pos[j, 3] — the w of its position word as it lies on the device, uploaded and
        downloaded with the positions and carried by every integrator — in energy(), potential_rows(), field(), tidal(), jerk() and the
        Hermite integrators; the unit-mass entry points (step, forces, bodyForce, step_adaptive, pair energies, binaries, the mailbox)
        raise ERR_UNSUPPORTED until it is switched off again.  Launches nothing and invalidates nothing."""
        self.set_option(L.OPT_MASSES, 1 if on else 0)

    # ---- state ----
    def _bs(self, pos, vel):
        if self.fp64:
            return L.BodySystemD(pos.ctypes.data_as(C.POINTER(C.c_double)), vel.ctypes.data_as(C.POINTER(C.c_double)))
        return L.BodySystem(pos.ctypes.data_as(C.POINTER(C.c_float)), vel.ctypes.data_as(C.POINTER(C.c_float)))

    def upload(self, pos, vel):
        pos, vel = _as(pos, self.dtype), _as(vel, self.dtype)
        if len(pos) != self.n or len(vel) != self.n:
            raise ValueError("upload expects the full %d bodies" % self.n)
        bs = self._bs(pos, vel)
        L.check((self.lib.nbody_upload_d if self.fp64 else self.lib.nbody_upload)(C.byref(bs)))

    def download(self):
        pos = np.empty((self.n, 4), self.dtype)
        vel = np.empty((self.n, 4), self.dtype)
        bs = self._bs(pos, vel)
        L.check((self.lib.nbody_download_d if self.fp64 else self.lib.nbody_download)(C.byref(bs)))
        return pos, vel

    def download_slice(self):
        """This rank's own bodies only (n_local words each), no collective."""
        cnt = self.info(L.INFO_N_LOCAL)
        pos = np.empty((cnt, 4), self.dtype)
        vel = np.empty((cnt, 4), self.dtype)
        L.check(self.lib.nbody_download_slice(pos.ctypes.data_as(C.c_void_p), vel.ctypes.data_as(C.c_void_p)))
        return pos, vel

    # ---- the path: same names and argument meaning as the C entry points ----
    def bodyForce(self, pos, vel, dt):
        """v += dt * F(pos), in place on vel; pos is read-only."""
        p, v = _as(pos, self.dtype), _as(vel, self.dtype)
        ct = C.c_double if self.fp64 else C.c_float
        fn = self.lib.bodyForce_d if self.fp64 else self.lib.bodyForce
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), v.ctypes.data_as(C.POINTER(ct)), dt, len(p)))
        if v is not vel:
            vel[...] = v
        return vel

    def integrate(self, pos, vel, dt):
        """r += v * dt, in place on pos."""
        p, v = _as(pos, self.dtype), _as(vel, self.dtype)
        ct = C.c_double if self.fp64 else C.c_float
        fn = self.lib.integrate_d if self.fp64 else self.lib.integrate
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), v.ctypes.data_as(C.POINTER(ct)), dt, len(p)))
        if p is not pos:
            pos[...] = p
        return pos

    def step(self, dt, nsteps=1):
        """nsteps x {bodyForce; integrate} on the uploaded state; asynchronous."""
        L.check((self.lib.nbody_step_d if self.fp64 else self.lib.nbody_step)(dt, int(nsteps)))

    def sync(self):
        L.check(self.lib.nbody_sync())

    def forces(self, pos):
        """{Fx, Fy, Fz, 0} per body from {x, y, z, .} words (the reference's RAM images)."""
        p = _as(pos, self.dtype)
        out = np.empty_like(p)
        ct = C.c_double if self.fp64 else C.c_float
        fn = self.lib.nbody_forces_d if self.fp64 else self.lib.nbody_forces
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), out.ctypes.data_as(C.POINTER(ct)), len(p)))
        return out

    def forces_rows(self, first_row, n_rows):
        """Forces on a row sample (rows of this rank's slice) from the state on the device."""
        out = np.empty((n_rows, 4), self.dtype)
        if self.fp64:
            L.check(self.lib.nbody_forces_rows_d(int(first_row), int(n_rows), out.ctypes.data_as(C.POINTER(C.c_double))))
        else:
            L.check(self.lib.nbody_forces_rows(int(first_row), int(n_rows), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def energy(self):
        """Energy and momenta of the state on the device (nbody_energy; unit masses, or after use_masses() the masses in pos[:, 3]; G = 1, the
        force's softening): dict(kinetic,
        potential, total, momentum=(3,), angular_momentum=(3,)), fp64.  Collective in a multi-rank job; every rank gets the same bits."""
        out = np.zeros(L.ENERGY_WORDS, np.float64)
        L.check(self.lib.nbody_energy(out.ctypes.data_as(C.POINTER(C.c_double))))
        t, u = float(out[L.ENERGY_KINETIC]), float(out[L.ENERGY_POTENTIAL])
        return dict(kinetic=t, potential=u, total=t + u, momentum=out[L.ENERGY_PX:L.ENERGY_PZ + 1].copy(),
                    angular_momentum=out[L.ENERGY_LX:L.ENERGY_LZ + 1].copy())

    def potential_rows(self, first_row, n_rows):
        """phi_i = -sum_{j != i} (|r_j - r_i|^2 + eps)^(-1/2) of n_rows bodies from first_row (rows as in forces_rows), in the
        context precision, from the state on the device (nbody_potential_rows)."""
        out = np.empty(int(n_rows), self.dtype)
        if self.fp64:
            L.check(self.lib.nbody_potential_rows_d(int(first_row), int(n_rows), out.ctypes.data_as(C.POINTER(C.c_double))))
        else:
            L.check(self.lib.nbody_potential_rows(int(first_row), int(n_rows), out.ctypes.data_as(C.POINTER(C.c_float))))
        return out

    def field(self, points, skip=None, accel=True, potential=True):
        """(accel, phi) of the bodies on the device at arbitrary points (nbody_field): a(x) = sum_j (r_j - x) (|r_j - x|^2 + eps)^(-3/2),
        phi(x) = -sum_j (|r_j - x|^2 + eps)^(-1/2) over ALL j.  points: (m, 4) words or (m, 3) in the context dtype; skip: None or m
        ints, each -1 or the global index of a body to leave out of that point's sums.  accel: (m, 4) {ax, ay, az, 0} or None when not
        asked for; phi: (m,) or None.  Collective in a multi-rank job (every rank brings its own points)."""
        p, m, sk = self._queries(points, skip)
        ct = C.c_double if self.fp64 else C.c_float
        if not (accel or potential):
            raise ValueError("ask for accel, potential or both")
        a = np.empty((m, 4), self.dtype) if accel else None
        phi = np.empty(m, self.dtype) if potential else None
        fn = self.lib.nbody_field_d if self.fp64 else self.lib.nbody_field
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), m, sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                   a.ctypes.data_as(C.POINTER(ct)) if accel else None, phi.ctypes.data_as(C.POINTER(ct)) if potential else None))
        return a, phi

    def _queries(self, points, skip):
        """points ((m, 4) words or (m, 3)) and skip (None or m ints) of a query pass as (words, m, skip array or None): contiguous, in
        the context dtype, (m, 3) points padded to words"""
        p = np.asarray(points, self.dtype)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise ValueError("expected an (m, 4) or (m, 3) array of %s" % np.dtype(self.dtype).name)
        if p.shape[1] == 3:
            p = np.concatenate([p, np.zeros((len(p), 1), self.dtype)], axis=1)
        p = np.ascontiguousarray(p)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (len(p),):
                raise ValueError("skip must hold one index per point")
        return p, len(p), sk

    def tidal(self, points, skip=None):
        """The tidal tensor T = grad a = -grad grad phi of the bodies on the device at arbitrary points (nbody_tidal):
        T_ab(x) = sum_j (3 d_a d_b inv^5 - delta_ab inv^3), d = r_j - x, inv = (|d|^2 + eps)^(-1/2), over ALL j.  points and skip as in
        field().  Returns (m, 6) values {xx, yy, zz, xy, xz, yz} in the context dtype; tidal_matrix() spreads them into (m, 3, 3).
        Collective in a multi-rank job (every rank brings its own points)."""
        p, m, sk = self._queries(points, skip)
        ct = C.c_double if self.fp64 else C.c_float
        t = np.empty((m, 6), self.dtype)
        fn = self.lib.nbody_tidal_d if self.fp64 else self.lib.nbody_tidal
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), m, sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None,
                   t.ctypes.data_as(C.POINTER(ct))))
        return t

    def jerk_at(self, points, velocities, skip=None):
        """(accel, jerk), each (m, 4) in the context dtype, of the bodies on the device at m phase-space points (nbody_jerk): accel the
        a(x) of field(), bit for bit, jerk its time derivative for a point that moves with velocity u,
        j(x, u) = sum_j (w inv^3 - 3 (d . w) d inv^5), d = r_j - x, w = v_j - u, over ALL j.  points, velocities: (m, 4) words or (m, 3),
        padded as tidal() pads them; skip as in field().  Collective in a multi-rank job (every rank brings its own queries)."""
        p, m, sk = self._queries(points, skip)
        u, mu, _ = self._queries(velocities, None)
        if mu != m:
            raise ValueError("expected one velocity per point")
        ct = C.c_double if self.fp64 else C.c_float
        a, j = np.empty((m, 4), self.dtype), np.empty((m, 4), self.dtype)
        fn = self.lib.nbody_jerk_d if self.fp64 else self.lib.nbody_jerk
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), u.ctypes.data_as(C.POINTER(ct)), m,
                   sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None, a.ctypes.data_as(C.POINTER(ct)), j.ctypes.data_as(C.POINTER(ct))))
        return a, j

    def jerk(self, first_row=0, n_rows=None):
        """(accel, jerk), each (n_rows, 4) in the context dtype, of n_rows bodies from first_row (rows as in timescales(); default: all of
        them) from the state on the device (nbody_jerk_rows): row i is jerk_at(r_i, v_i, skip=i) bit for bit, read where it lies on the
        device.  Collective in a multi-rank job."""
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        m = int(n_rows)
        ct = C.c_double if self.fp64 else C.c_float
        a, j = np.empty((max(m, 0), 4), self.dtype), np.empty((max(m, 0), 4), self.dtype)
        fn = self.lib.nbody_jerk_rows_d if self.fp64 else self.lib.nbody_jerk_rows
        L.check(fn(int(first_row), m, a.ctypes.data_as(C.POINTER(ct)), j.ctypes.data_as(C.POINTER(ct))))
        return a, j

    def snap_at(self, points, velocities, accelerations, skip=None):
        """(accel, jerk, snap), each (m, 4) in the context dtype, of the bodies on the device at m phase-space points (nbody_snap): accel
        and jerk those of jerk_at(), bit for bit, snap the second time derivative of accel for a point that moves with velocity u and
        acceleration a_x, s = sum_j (g inv^3 - 6 alpha J_j - 3 beta A_j) with g = a_j - a_x.  The bodies' own accelerations a_j come
        from a jerk rows pass the call runs first.  points, velocities, accelerations: (m, 4) words or (m, 3); skip as in field().
        Collective in a multi-rank job (every rank brings its own queries)."""
        p, m, sk = self._queries(points, skip)
        u, mu, _ = self._queries(velocities, None)
        g, mg, _ = self._queries(accelerations, None)
        if mu != m or mg != m:
            raise ValueError("expected one velocity and one acceleration per point")
        ct = C.c_double if self.fp64 else C.c_float
        a, j, s = (np.empty((m, 4), self.dtype) for _ in range(3))
        fn = self.lib.nbody_snap_d if self.fp64 else self.lib.nbody_snap
        ptr = lambda x: x.ctypes.data_as(C.POINTER(ct))
        L.check(fn(ptr(p), ptr(u), ptr(g), m, sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None, ptr(a), ptr(j), ptr(s)))
        return a, j, s

    def snap(self, first_row=0, n_rows=None):
        """(accel, jerk, snap), each (n_rows, 4) in the context dtype, of n_rows bodies from first_row (rows as in jerk(); default: all of
        them) from the state on the device (nbody_snap_rows): row i is snap_at(r_i, v_i, a_i, skip=i) bit for bit, a_i being jerk()'s
        acceleration of row i; accel and jerk are jerk()'s.  Two all-pairs passes.  Collective in a multi-rank job."""
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        m = int(n_rows)
        ct = C.c_double if self.fp64 else C.c_float
        a, j, s = (np.empty((max(m, 0), 4), self.dtype) for _ in range(3))
        fn = self.lib.nbody_snap_rows_d if self.fp64 else self.lib.nbody_snap_rows
        L.check(fn(int(first_row), m, a.ctypes.data_as(C.POINTER(ct)), j.ctypes.data_as(C.POINTER(ct)), s.ctypes.data_as(C.POINTER(ct))))
        return a, j, s

    def _near_out(self, m, r2):
        ct = C.c_double if self.fp64 else C.c_float
        idx, d2 = np.empty(m, np.int32), np.empty(m, self.dtype)
        cnt = np.empty(m, np.int32) if r2 is not None else None
        ip = C.POINTER(C.c_int)
        return idx, d2, cnt, (idx.ctypes.data_as(ip), d2.ctypes.data_as(C.POINTER(ct)), float(self.dtype(0 if r2 is None else r2)),
                              cnt.ctypes.data_as(ip) if cnt is not None else None)

    def neighbors(self, first_row=0, n_rows=None, r2=None):
        """(idx, d2, count) of n_rows bodies from first_row (rows as in forces_rows; default: all of them) from the state on the
        device (nbody_neighbors_rows): idx the GLOBAL index of the nearest other body (-1: none), d2 its plain squared distance in the
        context precision (no softening; +inf: none), count the number of other bodies with d2 <= r2 (r2 already squared), or None
        when r2 is None.  Ties go to the lowest index.  Collective in a multi-rank job."""
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        idx, d2, cnt, out = self._near_out(int(n_rows), r2)
        fn = self.lib.nbody_neighbors_rows_d if self.fp64 else self.lib.nbody_neighbors_rows
        L.check(fn(int(first_row), int(n_rows), *out))
        return idx, d2, cnt

    def nearest(self, points, skip=None, r2=None):
        """(idx, d2, count) as neighbors(), of the bodies on the device at arbitrary points (nbody_nearest).  points: (m, 4) words or
        (m, 3) in the context dtype; skip: None or m ints, each -1 or the global index of a body to leave out for that point.  A
        point on a body without a skip finds that body at d2 = 0."""
        p = np.asarray(points, self.dtype)
        if p.ndim != 2 or p.shape[1] not in (3, 4):
            raise ValueError("expected an (m, 4) or (m, 3) array of %s" % np.dtype(self.dtype).name)
        if p.shape[1] == 3:
            p = np.concatenate([p, np.zeros((len(p), 1), self.dtype)], axis=1)
        p = np.ascontiguousarray(p)
        m = len(p)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (m,):
                raise ValueError("skip must hold one index per point")
        idx, d2, cnt, out = self._near_out(m, r2)
        ct = C.c_double if self.fp64 else C.c_float
        fn = self.lib.nbody_nearest_d if self.fp64 else self.lib.nbody_nearest
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), m, sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None, *out))
        return idx, d2, cnt

    def closest_pair(self):
        """(i, j, d2) of the pair i < j with the smallest plain squared distance over the whole system (nbody_closest_pair), ties to
        the lowest i, then the lowest j; (-1, -1, inf) when N = 1.  Collective in a multi-rank job; every rank gets the same values."""
        i, j = C.c_int(), C.c_int()
        d2 = C.c_double() if self.fp64 else C.c_float()
        L.check((self.lib.nbody_closest_pair_d if self.fp64 else self.lib.nbody_closest_pair)(C.byref(i), C.byref(j), C.byref(d2)))
        return i.value, j.value, self.dtype(d2.value)

    def _knn_out(self, m, k):
        k = int(k)
        if not 1 <= k <= L.KNN_MAX:
            raise ValueError("k must be in 1..%d" % L.KNN_MAX)
        ct = C.c_double if self.fp64 else C.c_float
        idx, d2 = np.empty((m, k), np.int32), np.empty((m, k), self.dtype)
        return idx, d2, (k, idx.ctypes.data_as(C.POINTER(C.c_int)), d2.ctypes.data_as(C.POINTER(ct)))

    def knn(self, k, first_row=0, n_rows=None):
        """(idx, d2), each (n_rows, k), of n_rows bodies from first_row (rows as in forces_rows; default: all of them) from the state on
        the device (nbody_knn_rows): per body the k nearest other bodies in ascending (d2, index) order — idx their GLOBAL indices
        (int32; -1 where there are fewer than k), d2 their plain squared distances in the context precision (no softening; +inf there).
        1 <= k <= 32.  Column 0 is neighbors().  Collective in a multi-rank job."""
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        if int(n_rows) < 1:
            raise ValueError("expected at least one row")
        idx, d2, out = self._knn_out(int(n_rows), k)
        fn = self.lib.nbody_knn_rows_d if self.fp64 else self.lib.nbody_knn_rows
        L.check(fn(int(first_row), int(n_rows), *out))
        return idx, d2

    def knn_at(self, points, k, skip=None):
        """(idx, d2), each (m, k), as knn(), of the bodies on the device at arbitrary points (nbody_knn).  points: (m, 4) words or
        (m, 3) in the context dtype; skip: None or m ints, each -1 or the global index of a body to leave out for that point.  A
        point on a body without a skip lists that body first at d2 = 0.  Column 0 is nearest()."""
        p = np.asarray(points, self.dtype)
        if p.ndim != 2 or p.shape[1] not in (3, 4) or len(p) < 1:
            raise ValueError("expected an (m, 4) or (m, 3) array of %s, m >= 1" % np.dtype(self.dtype).name)
        if p.shape[1] == 3:
            p = np.concatenate([p, np.zeros((len(p), 1), self.dtype)], axis=1)
        p = np.ascontiguousarray(p)
        m = len(p)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (m,):
                raise ValueError("skip must hold one index per point")
        idx, d2, out = self._knn_out(m, k)
        ct = C.c_double if self.fp64 else C.c_float
        fn = self.lib.nbody_knn_d if self.fp64 else self.lib.nbody_knn
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), m, sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None, *out))
        return idx, d2

    def fof(self, b2):
        """(group, n_groups): the friends-of-friends groups of the state on the device at the linking length whose SQUARE is b2, in
        the context precision (nbody_fof).  Bodies with plain squared distance d2 <= b2 are linked, a group is a connected component;
        group: (N,) int32, the lowest GLOBAL body index of every body's group over all N bodies, n_groups the number of groups
        (numpy.bincount(group) gives their sizes).  b2 = inf is legal.  The number of link passes the call ran is left in
        self.fof_rounds.  Collective in a multi-rank job; every rank gets the same values."""
        b2 = float(self.dtype(b2))
        if not b2 >= 0:
            raise ValueError("b2 must be a squared length: not NaN, not negative")
        group = np.empty(self.n, np.int32)
        n_groups, rounds = C.c_int(), C.c_int()
        fn = self.lib.nbody_fof_d if self.fp64 else self.lib.nbody_fof
        L.check(fn(b2, group.ctypes.data_as(C.POINTER(C.c_int)), C.byref(n_groups), C.byref(rounds)))
        self.fof_rounds = rounds.value
        return group, n_groups.value

    def _hist_edges(self, edges2):
        e = np.ascontiguousarray(np.asarray(edges2, self.dtype).reshape(-1))
        if not 2 <= len(e) <= L.HIST_MAX_BINS + 1:
            raise ValueError("expected 2..%d edges (1..%d bins)" % (L.HIST_MAX_BINS + 1, L.HIST_MAX_BINS))
        if np.isnan(e).any() or (e[1:] < e[:-1]).any():
            raise ValueError("edges2 must hold no NaN and must not descend")
        return e, len(e) - 1, e.ctypes.data_as(C.POINTER(C.c_double if self.fp64 else C.c_float))

    def radial_counts(self, edges2, first_row=0, n_rows=None):
        """counts, (n_rows, n_bins) int32, of n_rows bodies from first_row (rows as in forces_rows; default: all of them) from the state
        on the device (nbody_radial_counts_rows): per body the number of other bodies j with edges2[b] <= d2_j < edges2[b + 1], d2 the
        plain squared distance in the context precision (no softening).  edges2: 2..33 squared radii, cast to the context dtype, no
        NaN, non-decreasing; the last may be inf.  Collective in a multi-rank job."""
        e, nb, ep = self._hist_edges(edges2)
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        if int(n_rows) < 1:
            raise ValueError("expected at least one row")
        counts = np.empty((int(n_rows), nb), np.int32)
        fn = self.lib.nbody_radial_counts_rows_d if self.fp64 else self.lib.nbody_radial_counts_rows
        L.check(fn(int(first_row), int(n_rows), ep, nb, counts.ctypes.data_as(C.POINTER(C.c_int))))
        return counts

    def radial_counts_at(self, points, edges2, skip=None):
        """counts, (m, n_bins) int32, as radial_counts(), of the bodies on the device around arbitrary points (nbody_radial_counts).
        points: (m, 4) words or (m, 3) in the context dtype; skip: None or m ints, each -1 or the global index of a body to leave out
        for that point.  A point on a body without a skip counts that body in the bin that holds 0."""
        e, nb, ep = self._hist_edges(edges2)
        p = np.asarray(points, self.dtype)
        if p.ndim != 2 or p.shape[1] not in (3, 4) or len(p) < 1:
            raise ValueError("expected an (m, 4) or (m, 3) array of %s, m >= 1" % np.dtype(self.dtype).name)
        if p.shape[1] == 3:
            p = np.concatenate([p, np.zeros((len(p), 1), self.dtype)], axis=1)
        p = np.ascontiguousarray(p)
        m = len(p)
        sk = None
        if skip is not None:
            sk = np.ascontiguousarray(skip, np.int32)
            if sk.shape != (m,):
                raise ValueError("skip must hold one index per point")
        counts = np.empty((m, nb), np.int32)
        ct = C.c_double if self.fp64 else C.c_float
        fn = self.lib.nbody_radial_counts_d if self.fp64 else self.lib.nbody_radial_counts
        L.check(fn(p.ctypes.data_as(C.POINTER(ct)), m, sk.ctypes.data_as(C.POINTER(C.c_int)) if sk is not None else None, ep, nb,
                   counts.ctypes.data_as(C.POINTER(C.c_int))))
        return counts

    def pair_histogram(self, edges2):
        """pairs, (n_bins,) int64: the number of unordered pairs i < j of the whole system with edges2[b] <= d2_ij < edges2[b + 1]
        (nbody_pair_histogram) — DD(r), the numerator of the radial distribution function.  edges2 as in radial_counts().  The rows'
        counts are added on the device; collective in a multi-rank job, every rank gets the same values."""
        e, nb, ep = self._hist_edges(edges2)
        pairs = np.empty(nb, np.int64)
        fn = self.lib.nbody_pair_histogram_d if self.fp64 else self.lib.nbody_pair_histogram
        L.check(fn(ep, nb, pairs.ctypes.data_as(C.POINTER(C.c_longlong))))
        return pairs

    def timescales(self, first_row=0, n_rows=None):
        """(tau2, idx, d2min) of n_rows bodies from first_row (rows as in forces_rows; default: all of them) from the state on the
        device (nbody_timescale_rows): tau2 the smallest pair crossing time squared |r_ij|^2 / |v_ij|^2 over the other bodies in the
        context precision (+inf: none), idx the GLOBAL index of the body that gives it (-1: none; ties to the lowest index), d2min the
        smallest plain squared distance, bit for bit neighbors()'s d2.  Collective in a multi-rank job."""
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        m = int(n_rows)
        ct = C.c_double if self.fp64 else C.c_float
        tau2, idx, d2min = np.empty(m, self.dtype), np.empty(m, np.int32), np.empty(m, self.dtype)
        fn = self.lib.nbody_timescale_rows_d if self.fp64 else self.lib.nbody_timescale_rows
        L.check(fn(int(first_row), m, tau2.ctypes.data_as(C.POINTER(ct)), idx.ctypes.data_as(C.POINTER(C.c_int)),
                   d2min.ctypes.data_as(C.POINTER(ct))))
        return tau2, idx, d2min

    def min_timescale(self):
        """(tau2, i, j, d2min) of the whole system (nbody_min_timescale): the smallest pair crossing time squared, the lowest row i
        that reaches it and its partner j, and the smallest plain squared distance (closest_pair()'s d2); (inf, -1, -1, inf) when
        there is none.  Collective in a multi-rank job; every rank gets the same values."""
        i, j = C.c_int(), C.c_int()
        tau2, d2min = (C.c_double(), C.c_double()) if self.fp64 else (C.c_float(), C.c_float())
        fn = self.lib.nbody_min_timescale_d if self.fp64 else self.lib.nbody_min_timescale
        L.check(fn(C.byref(tau2), C.byref(i), C.byref(j), C.byref(d2min)))
        return self.dtype(tau2.value), i.value, j.value, self.dtype(d2min.value)

    def step_adaptive(self, t_end, eta, dt_min, dt_max, max_steps=1000000):
        """(t_reached, steps): steps of a shared adaptive dt = eta * sqrt(min(tau2, tff2)) clamped to [dt_min, dt_max] from t = 0
        until t_end or max_steps (nbody_step_adaptive), tau2 and d2min of min_timescale() before every step and tff2 the unit-mass
        pair free-fall time squared at d2min.  Collective in a multi-rank job."""
        t, steps = C.c_double(0.0), C.c_int(0)
        fn = self.lib.nbody_step_adaptive_d if self.fp64 else self.lib.nbody_step_adaptive
        L.check(fn(eta, t_end, dt_min, dt_max, int(max_steps), C.byref(t), C.byref(steps)))
        return t.value, steps.value

    def pair_energy(self, first_row=0, n_rows=None):
        """(e, idx) of n_rows bodies from first_row (rows as in timescales(); default: all of them) from the state on the device
        (nbody_pair_energy_rows): e the lowest specific two-body energy v2 / 2 - 2 / sqrt(d2 + eps) over the other bodies in the
        context precision (+inf: none), idx the GLOBAL index of the body that gives it (-1: none; ties to the lowest index): every
        body's most bound partner.  Collective in a multi-rank job."""
        if n_rows is None:
            n_rows = self.info(L.INFO_N_LOCAL if self._by_rank else L.INFO_N) - int(first_row)
        m = int(n_rows)
        ct = C.c_double if self.fp64 else C.c_float
        e, idx = np.empty(m, self.dtype), np.empty(m, np.int32)
        fn = self.lib.nbody_pair_energy_rows_d if self.fp64 else self.lib.nbody_pair_energy_rows
        L.check(fn(int(first_row), m, e.ctypes.data_as(C.POINTER(ct)), idx.ctypes.data_as(C.POINTER(C.c_int))))
        return e, idx

    def binaries(self, e_max=0.0, max_pairs=None):
        """(i, j, elements) of the binaries of the whole system (nbody_binaries): the pairs i < j that are each other's most bound
        partner with a pair energy below e_max (<= 0), in ascending i; elements, (n, 4) float64, holds {E, a, ecc, period} per pair.
        max_pairs=None counts first and then fetches all; otherwise at most max_pairs are returned and self.binaries_found holds the
        number found.  A body whose best partner prefers someone else is not listed.  Collective in a multi-rank job; every rank
        gets the same list."""
        ip = C.POINTER(C.c_int)
        found = C.c_int()
        if max_pairs is None:
            L.check(self.lib.nbody_binaries(float(e_max), 0, C.byref(found), None, None, None))
            max_pairs = found.value
        k = int(max_pairs)
        i, j, el = np.empty(k, np.int32), np.empty(k, np.int32), np.empty((k, L.BINARY_WORDS), np.float64)
        L.check(self.lib.nbody_binaries(float(e_max), k, C.byref(found), i.ctypes.data_as(ip), j.ctypes.data_as(ip),
                                        el.ctypes.data_as(C.POINTER(C.c_double))))
        self.binaries_found = found.value
        n = min(found.value, k)
        return i[:n], j[:n], el[:n]

    def step_hermite(self, dt, nsteps=1):
        """nsteps fourth-order Hermite steps of a shared dt on the state on the device (nbody_step_hermite): predict, one jerk rows
        pass over the predicted state, correct.  A call evaluates (a, j) afresh at its start — k + 1 passes for k steps — so k calls
        of one step are k restarts and in general give other bits than one call of k steps.  Same bits on any number of devices or
        ranks.  Synchronous; collective in a multi-rank job."""
        L.check((self.lib.nbody_step_hermite_d if self.fp64 else self.lib.nbody_step_hermite)(float(dt), int(nsteps)))

    def min_aarseth(self):
        """(q, row) of the whole system (nbody_min_aarseth): the smallest |a|^2 / |j|^2 over the rows of jerk(), in binary64, and
        the lowest global row that reaches it; (inf, -1) when no row has a finite one.  eta * sqrt(q) is the shared Aarseth step.
        Collective in a multi-rank job; every rank gets the same values."""
        q, row = C.c_double(), C.c_int()
        L.check(self.lib.nbody_min_aarseth(C.byref(q), C.byref(row)))
        return q.value, row.value

    def step_hermite_adaptive(self, t_end, eta, dt_min, dt_max, max_steps=1000000):
        """(t_reached, steps): Hermite steps of a shared dt = eta * sqrt(min_i |a_i|^2 / |j_i|^2) clamped to [dt_min, dt_max] from
        t = 0 until t_end or max_steps (nbody_step_hermite_adaptive); the minimum comes from the (a, j) the integrator carries, no
        extra pass.  Collective in a multi-rank job."""
        t, steps = C.c_double(0.0), C.c_int(0)
        fn = self.lib.nbody_step_hermite_adaptive_d if self.fp64 else self.lib.nbody_step_hermite_adaptive
        L.check(fn(eta, t_end, dt_min, dt_max, int(max_steps), C.byref(t), C.byref(steps)))
        return t.value, steps.value

    def step_hermite6(self, dt, nsteps=1):
        """nsteps sixth-order Hermite steps (Nitadori & Makino 2008) of a shared dt on the state on the device (nbody_step_hermite6):
        predict positions, velocities and accelerations with (a, j, s) and the crackle carried from the step before, one snap rows pass
        over the predicted state, correct.  A call evaluates (a, j, s) afresh at its start as snap() does — k + 2 passes for k steps —
        and starts from a crackle of zero, so k calls of one step are k restarts and give other bits than one call of k steps.  Same
        bits on any number of devices or ranks.  Synchronous; collective in a multi-rank job."""
        L.check((self.lib.nbody_step_hermite6_d if self.fp64 else self.lib.nbody_step_hermite6)(float(dt), int(nsteps)))

    def step_hermite6_adaptive(self, t_end, eta, dt_min, dt_max, max_steps=1000000):
        """(t_reached, steps): step_hermite_adaptive()'s loop — the shared Aarseth step from the carried (a, j) — over sixth-order
        Hermite steps (nbody_step_hermite6_adaptive).  Collective in a multi-rank job."""
        t, steps = C.c_double(0.0), C.c_int(0)
        fn = self.lib.nbody_step_hermite6_adaptive_d if self.fp64 else self.lib.nbody_step_hermite6_adaptive
        L.check(fn(eta, t_end, dt_min, dt_max, int(max_steps), C.byref(t), C.byref(steps)))
        return t.value, steps.value

    def step_hermite_block(self, dt_max, nblocks=1, eta=0.02, levels=8):
        """(substeps, row_evals): the state advanced by nblocks * dt_max with individual block time steps (nbody_step_hermite_block):
        level k has the step dt_max * 2^-k, k < levels; a sub-step predicts every body to the system's next time and evaluates and
        corrects only the bodies that are due, which then take the level eta^2 |a|^2 / |j|^2 asks for.  substeps: the distinct times
        visited; row_evals: the sum of the active counts.  levels = 1 is step_hermite(dt_max, nblocks) bit for bit.  Stateless,
        synchronous; same bits on any number of devices or ranks; collective in a multi-rank job."""
        steps, evals = C.c_longlong(0), C.c_longlong(0)
        fn = self.lib.nbody_step_hermite_block_d if self.fp64 else self.lib.nbody_step_hermite_block
        L.check(fn(float(eta), float(dt_max), int(levels), int(nblocks), C.byref(steps), C.byref(evals)))
        return steps.value, evals.value

    def step_hermite6_block(self, dt_max, nblocks=1, eta=0.02, levels=8):
        """(substeps, row_evals): step_hermite_block() over the sixth-order scheme (nbody_step_hermite6_block): the call opens as
        step_hermite6() does, a sub-step predicts every body's position, velocity and acceleration to the system's next time, and the
        bodies that are due are evaluated by the snap pass and corrected with their own step, crackle included.  The levels follow
        eta^2 |a|^2 / |j|^2 as in step_hermite_block().  levels = 1 is step_hermite6(dt_max, nblocks) bit for bit.  Stateless,
        synchronous; same bits on any number of devices or ranks; collective in a multi-rank job."""
        steps, evals = C.c_longlong(0), C.c_longlong(0)
        fn = self.lib.nbody_step_hermite6_block_d if self.fp64 else self.lib.nbody_step_hermite6_block
        L.check(fn(float(eta), float(dt_max), int(levels), int(nblocks), C.byref(steps), C.byref(evals)))
        return steps.value, evals.value

    def comm_selftest(self):
        """Push a patterned array through the RCCL calls of the multi-GPU path (all-gather + one ring step); returns
        the bytes this rank received.  Needs the communicator of NBody(..., rank=, nranks=, uid=)."""
        moved = C.c_longlong()
        L.check(self.lib.nbody_comm_selftest(C.byref(moved)))
        return moved.value

    def comm_selftest_virtual(self, vranks, form):
        """The transfer plans of `vranks` virtual ranks run through real ncclSend/ncclRecv on a one-rank communicator."""
        moved = C.c_longlong()
        L.check(self.lib.nbody_comm_selftest_virtual(int(vranks), int(form), C.byref(moved)))
        return moved.value

    def comm_probe(self, nbytes, when):
        """(ms of one RCCL ring step of nbytes from enqueue to done, ms of the force pass beside it); when = 0 alone,
        1 enqueued just before a full force pass, 2 just after it."""
        c, f = C.c_double(), C.c_double()
        L.check(self.lib.nbody_comm_probe(int(nbytes), int(when), C.byref(c), C.byref(f)))
        return c.value, f.value

    def comm_time(self, reset=False):
        """(ms the compute stream waited for arriving slices, number of waits) since the last reset (OPT_TIMING = 1)."""
        ms, cnt = C.c_double(), C.c_longlong()
        L.check(self.lib.nbody_comm_time(C.byref(ms), C.byref(cnt), int(reset)))
        return ms.value, cnt.value

    @property
    def order(self):
        """The summation order of the current configuration as keyword arguments of the oracle's order()
        (tests mirror the engine's order with it)."""
        cfg = self.config
        nsl = cfg["nseg"] // cfg["jsub"]
        return dict(nslices=nsl, sub=cfg["jsub"], block=cfg["sum_block"] or 1024,
                    summ={"seq": 0, "fpga16": 1, "blocked": 2}[cfg["sum_order"]], wsplit=cfg["wsplit"])

    def kernel_time(self, reset=False):
        ms, cnt = C.c_double(), C.c_longlong()
        L.check(self.lib.nbody_kernel_time(C.byref(ms), C.byref(cnt), int(reset)))
        return ms.value, cnt.value

    def device_ptr(self, which):
        p, b = C.c_void_p(), C.c_size_t()
        L.check(self.lib.nbody_device_ptr(int(which), C.byref(p), C.byref(b)))
        return p.value, b.value

    def set_host_gather(self, fn):
        """Multi-process transport through host memory: fn(host_ptr, n_total, word_bytes, rank, nranks) -> 0 must
        all-gather the array in place (see nbody_set_host_gather in include/nbody.h)."""
        def tramp(user, host_ptr, n_total, word_bytes, rank, nranks):
            try:
                return int(fn(host_ptr, n_total, word_bytes, rank, nranks) or 0)
            except Exception:   # an exception must not unwind through the C frame
                import traceback
                traceback.print_exc()
                return 1
        self._gather_cb = L.HOST_GATHER_FN(tramp)      # keep the thunk alive as long as the engine
        L.check(self.lib.nbody_set_host_gather(self._gather_cb, None))

    def close(self):
        if self._open:
            self.lib.nbody_shutdown()
            self._open = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def tidal_matrix(t6):
    """(m, 6) values {xx, yy, zz, xy, xz, yz} of NBody.tidal() (or one point's six) as symmetric (m, 3, 3) matrices (or one (3, 3)),
    in the same dtype: np.linalg.eigvalsh applies directly."""
    t6 = np.asarray(t6)
    if t6.shape[-1:] != (6,):
        raise ValueError("expected six values {xx, yy, zz, xy, xz, yz} per point")
    return t6[..., [[0, 3, 4], [3, 1, 5], [4, 5, 2]]]


def aarseth_dt(accel, jerk, eta):
    """eta |a| / |j| per row in fp64, the Aarseth time step from NBody.jerk() or jerk_at(): accel, jerk (m, 4) or (m, 3) (the first three
    components count), +inf where |j| = 0."""
    a, j = np.asarray(accel, np.float64), np.asarray(jerk, np.float64)
    if a.ndim != 2 or a.shape != j.shape or a.shape[1] not in (3, 4):
        raise ValueError("expected accel and jerk of one shape, (m, 4) or (m, 3)")
    na, nj = np.sqrt((a[:, :3] ** 2).sum(1)), np.sqrt((j[:, :3] ** 2).sum(1))
    dt = np.full(len(a), np.inf)
    np.divide(float(eta) * na, nj, out=dt, where=nj != 0)
    return dt


def comm_plan(form, rank, nranks, n):
    """The transfer plan of one rank as a list of dicts (pure host arithmetic in the library: no GPU needed)."""
    lib = L.load()
    cnt = C.c_int()
    L.check(lib.nbody_comm_plan(int(form), int(rank), int(nranks), int(n), None, 0, C.byref(cnt)))
    buf = (C.c_longlong * (7 * max(1, cnt.value)))()
    L.check(lib.nbody_comm_plan(int(form), int(rank), int(nranks), int(n), buf, cnt.value, C.byref(cnt)))
    keys = ("group", "send_peer", "send_first", "send_count", "recv_peer", "recv_first", "recv_count")
    return [dict(zip(keys, buf[7 * k:7 * k + 7])) for k in range(cnt.value)]


def strict_proof():
    """The library's gate for the strict binary32 arithmetic (nbody_strict_proof): every positive normal binary32 through the
    eight-operation 1/sqrt and through its IEEE definition on every device of the open context (else on the device a one-GPU context
    would take), cached per device.  Returns (mismatches, first mismatching pattern) — (0, 0) when proved."""
    bad, first = C.c_ulonglong(), C.c_uint()
    rc = L.load().nbody_strict_proof(C.byref(bad), C.byref(first))
    if rc not in (0, L.ERR_UNSUPPORTED):
        L.check(rc)
    return bad.value, first.value


def rsqrt_selftest(first_bits=0, count=1 << 32):
    """The strict 1/sqrt against its definition for `count` binary32 bit patterns from first_bits (default: every float), on the
    device: (mismatches — must be 0, patterns evaluated by the IEEE form, smallest mismatching pattern)."""
    bad, slow, first = C.c_ulonglong(), C.c_ulonglong(), C.c_uint()
    L.check(L.load().nbody_rsqrt_selftest(int(first_bits), int(count), C.byref(bad), C.byref(slow), C.byref(first)))
    return bad.value, slow.value, first.value


def rsqrt_strict(x, ieee_only=False):
    """y = the strict 1/sqrt of the float32 array x, as the force kernels evaluate it (or by the IEEE expression alone)."""
    import numpy as np
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.empty_like(x)
    fp = C.POINTER(C.c_float)
    L.check(L.load().nbody_rsqrt_strict(x.ctypes.data_as(fp), y.ctypes.data_as(fp), int(x.size), 1 if ieee_only else 0))
    return y


def unique_id():
    buf = C.create_string_buffer(128)
    L.check(L.load().nbody_unique_id(buf))
    return bytes(buf.raw)
