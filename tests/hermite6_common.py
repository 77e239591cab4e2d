"""What the sixth-order Hermite tests (test_hermite6_abi.py, test_gpu_hermite6.py) share: tests/hermite6_ref.c compiled together with
tests/snap_ref.c as hermite_common compiles its own (-ffp-contract=off), and the relative energy error of the Kepler pair.  The Kepler
pair, the energy of a state and the fourth-order statement are hermite_common's."""
import ctypes as C
import os
import subprocess

import numpy as np

from field_common import ROOT
from hermite_common import energy, kepler

REF, MASS, NO_CRACKLE = 1, 2, 4   # hermite6_ref.c's flags; NO_CRACKLE is the wrong, fifth-order scheme the order test must tell apart

# The bounds of the Kepler tests (e = 0.5 from pericentre to t = 1, binary64, relative energy error err(n) after n steps).  With the
# crackle term the scheme is of sixth order, err(n) / err(2n) -> 64; without it of fifth, -> 32: the bound between them is their
# geometric mean.  Measured with tests/hermite6_ref.c: 65.0 and 64.5; without the crackle 32.8 and 32.6.
ORDER_RATIO = 45.0
# err6(128) <= err4(128) / GAIN, err4 from tests/hermite_ref.c.  Measured: err6 = 2.7e-10, err4 = 1.84e-7, a ratio of 690.
GAIN = 100.0


def compile_ref(tmp_dir):
    """tests/hermite6_ref.c + tests/snap_ref.c as one shared library"""
    so = os.path.join(str(tmp_dir), "hermite6_ref.so")
    srcs = [os.path.join(ROOT, "tests", f) for f in ("hermite6_ref.c", "snap_ref.c")]
    for extra in (["-march=native", "-fopenmp"], ["-fopenmp"], []):   # every operation is IEEE-exact: vector width and threads change no bit
        r = subprocess.run(["gcc", "-std=c11", "-O3", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math"] + extra + ["-o", so] + srcs + ["-lm"],
                           capture_output=True, timeout=180)
        if r.returncode == 0:
            return C.CDLL(so)
    raise RuntimeError("cannot compile tests/hermite6_ref.c: %s" % r.stderr.decode()[-2000:])


class Hermite6Ref:
    """tests/hermite6_ref.c.  dtype float32 or float64 picks the statement; every method returns new (pos, vel) words, (n, 4) each"""

    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def _words(pos, vel, dtype):
        p, v = np.array(pos, dtype, order="C"), np.array(vel, dtype, order="C")
        assert p.shape == v.shape and p.shape[1] == 4
        return p, v

    @staticmethod
    def _suf(dtype):
        return "f64" if np.dtype(dtype) == np.float64 else "f32"

    def _stepper(self, name, pos, vel, dtype, dt, count, flags):
        p, v = self._words(pos, vel, dtype)
        fn = getattr(self.lib, name + "_" + self._suf(dtype))
        ct = C.c_double if np.dtype(dtype) == np.float64 else C.c_float
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, ct, C.c_int, C.c_int]
        fn.restype = None
        fn(p.ctypes.data, v.ctypes.data, len(p), float(dt), int(count), int(flags))
        return p, v

    def step(self, pos, vel, dtype, dt, nsteps, flags=0):
        """one call of nsteps steps (the carried form)"""
        return self._stepper("hermite6", pos, vel, dtype, dt, nsteps, flags)

    def restarted(self, pos, vel, dtype, dt, ncalls, flags=0):
        """ncalls calls of one step each"""
        return self._stepper("hermite6_restarted", pos, vel, dtype, dt, ncalls, flags)

    def adaptive(self, pos, vel, dtype, eta, t_end, dt_min, dt_max, max_steps=1000000, flags=0):
        """(pos, vel, t_reached, steps)"""
        p, v = self._words(pos, vel, dtype)
        fn = getattr(self.lib, "hermite6_adaptive_" + self._suf(dtype))
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int,
                       C.POINTER(C.c_double), C.POINTER(C.c_int)]
        fn.restype = None
        t, steps = C.c_double(), C.c_int()
        fn(p.ctypes.data, v.ctypes.data, len(p), int(flags), eta, t_end, dt_min, dt_max, int(max_steps), C.byref(t), C.byref(steps))
        return p, v, t.value, steps.value


def kepler_energy_error(stepper, n, e=0.5):
    """|E(1) - E(0)| / |E(0)| of the Kepler pair of eccentricity e after n steps of 1 / n; stepper(pos, vel, dt, nsteps) -> (pos, vel)"""
    pos, vel = kepler(e)
    e0 = energy(pos, vel)
    p, v = stepper(pos, vel, 1.0 / n, n)
    return abs(energy(p, v) - e0) / abs(e0)
