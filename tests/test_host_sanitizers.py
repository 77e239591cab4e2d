"""The library's HOST code — everything in libnbody_hip.so that is not device code — under AddressSanitizer + UBSan and under
ThreadSanitizer, on the CPU (sanitizers run on the CPU build only; the GPU pool has none).  Every case is a stand-alone program with
its own main, linked from the host files under test, the stubs and one driver; nothing is loaded into Python under a sanitizer.
tests/host_stub/hip_stub.cpp stands in for the HIP runtime ("device" memory is malloc'd, so ASan sees every offset the host computed;
streams run synchronously, a capture records closures) and for kernels.hip (a simple stand-in force pushed through the REAL data flow
of a launch: ForceArgs, segment bounds, partial sums, arrival counters, ascending combine, apply, the mailbox's ingest and
device-written completion) and energy.hip (predictable values written through the real EnergyArgs); <pass>_stub.cpp stands in for
<pass>.hip the same way (predictable values pushed through the real PointSumsArgs / NeighborsArgs / KnnArgs / FofArgs / HistArgs /
TimescaleArgs: chunk bounds, the blocks' or chunks' scratch layout, the combine) and refuses what the real launch functions refuse, by
the same predicates (diag_pass.hpp and the passes' *_args.hpp).  stub_rule.hpp is the contract between the distance passes' stubs and
their drivers — the one candidate a block of sources offers a query — stub_common.hpp the stubs' skeleton, sanity_common.hpp the
drivers' kit.  The drivers, one per row of CASES (point_sums_sanity.cpp serves two, by its argument):
  host_sanity.cpp       contexts of several sizes, 70-step loops (graph capture and replay), every segmentation / combine form / wave
                        split, row windows, the energy entry points, fp64, one process over three stub devices with ragged slices, the
                        mailbox in every form with the RTL's address map checked against a sentinel, a request whose completion wait
                        fails, and the SERVED mailbox with a second thread hammering nbody_get_info and the refused entry points (VERDICT
                        r05 item 4: "a TSan build of a host-only stub of the serve loop");
  point_sums_sanity.cpp field: nbody_field(_d): m = 1, 255, 256, 257, 5000, skip present and absent, either output NULL;
                        tidal: nbody_tidal(_d) likewise, the six values per point, nbody_field calls between tidal calls on one
                        context, whose query and output buffers the two passes share;
  neighbors_sanity.cpp  nbody_neighbors_rows, nbody_nearest, nbody_closest_pair: row windows that straddle devices, each output NULL in
                        turn, the closest pair over three devices, nbody_field calls between nbody_nearest calls on one context, whose
                        query buffers the two passes share;
  knn_sanity.cpp        nbody_knn_rows, nbody_knn: k = 1, 5 and 32, the [m][k] outputs, nbody_nearest calls between nbody_knn calls;
  fof_sanity.cpp        nbody_fof(_d) on a one-dimensional system whose groups it finds by sorting: N = 1, 255, 256, 257 and 5000, the
                        active-row list against NBODY_FOF_ALL_ROWS=1;
  hist_sanity.cpp       nbody_radial_counts_rows, nbody_radial_counts, nbody_pair_histogram: n_bins = 1, 5 and 32, the right-aligned
                        edge slots, the [m][n_bins] outputs, the batches of the pair histogram's rows and its 64-bit sums over the
                        devices, nbody_nearest calls between histogram calls;
  timescale_sanity.cpp  nbody_timescale_rows, nbody_min_timescale, nbody_step_adaptive: windows of rows across the devices, the two
                        minima and an index per row, both source streams — the gather of all N velocities on three devices after
                        steps have changed them — and the driver loop against nbody_step.
Every pass driver runs over one and three stub devices with ragged slices, the source split forced and automatic, the batched path
and every NBODY_ERR_ARG case; and every driver runs the failure sweep (the stub fails the k-th creating call of every entry point that
allocates, k = 1, 2, ...: the call reports it, nothing is live after nbody_shutdown, the same call then works).
What this checks is the host's logic — buffer sizes and offsets, a request's force pass over its own N beside a context that keeps its
own, the service thread's hand-over, the guard, lifetimes at shutdown; the kernels' arithmetic is the GPU tests' business."""
import atexit
import os
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-Wall", "-Wno-unused-function"]
ASAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
TSAN = ["-fsanitize=thread"]
HOST = ("context.cpp", "comm.cpp", "mailbox.cpp", "energy.cpp")
NEIGHBORS_ENV = ("NBODY_NEIGHBORS_SPLIT", "NBODY_NEIGHBORS_SCRATCH_MB", "NBODY_NEIGHBORS_LOOP")
# name: (host files from mini_nbody_amd/csrc, stubs and driver from tests/host_stub (the driver last), the driver's arguments, the environment
#        variables it must not inherit, the line it prints when everything held)
CASES = {
    "host": (HOST, ("hip_stub.cpp", "host_sanity.cpp"), ["2000"], (), "host_sanity ok"),
    "field": (HOST + ("point_sums.cpp",), ("hip_stub.cpp", "point_sums_stub.cpp", "point_sums_sanity.cpp"), ["field"],
              ("NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"), "point_sums_sanity field ok"),
    "tidal": (HOST + ("point_sums.cpp",), ("hip_stub.cpp", "point_sums_stub.cpp", "point_sums_sanity.cpp"), ["tidal"],
              ("NBODY_TIDAL_SPLIT", "NBODY_TIDAL_SCRATCH_MB", "NBODY_FIELD_SPLIT", "NBODY_FIELD_SCRATCH_MB"), "point_sums_sanity tidal ok"),
    "neighbors": (HOST + ("neighbors.cpp", "point_sums.cpp"), ("hip_stub.cpp", "neighbors_stub.cpp", "point_sums_stub.cpp", "neighbors_sanity.cpp"), [],
                  NEIGHBORS_ENV, "neighbors_sanity ok"),
    "knn": (HOST + ("neighbors.cpp", "point_sums.cpp", "knn.cpp"),
            ("hip_stub.cpp", "neighbors_stub.cpp", "point_sums_stub.cpp", "knn_stub.cpp", "knn_sanity.cpp"), [],
            ("NBODY_KNN_SPLIT", "NBODY_KNN_SCRATCH_MB") + NEIGHBORS_ENV, "knn_sanity ok"),
    "fof": (HOST + ("neighbors.cpp", "point_sums.cpp", "knn.cpp", "fof.cpp"),
            ("hip_stub.cpp", "neighbors_stub.cpp", "point_sums_stub.cpp", "knn_stub.cpp", "fof_stub.cpp", "fof_sanity.cpp"), [],
            ("NBODY_FOF_SPLIT", "NBODY_FOF_SCRATCH_MB", "NBODY_FOF_ALL_ROWS"), "fof_sanity ok"),
    "hist": (HOST + ("neighbors.cpp", "hist.cpp"), ("hip_stub.cpp", "neighbors_stub.cpp", "hist_stub.cpp", "hist_sanity.cpp"), [],
             ("NBODY_HIST_SPLIT", "NBODY_HIST_SCRATCH_MB", "NBODY_HIST_LOOP") + NEIGHBORS_ENV, "hist_sanity ok"),
    "timescale": (HOST + ("timescale.cpp",), ("hip_stub.cpp", "timescale_stub.cpp", "timescale_sanity.cpp"), [],
                  ("NBODY_TIMESCALE_SPLIT", "NBODY_TIMESCALE_SCRATCH_MB"), "timescale_sanity ok"),
}
_objects = {}      # (source, sanitizer flags) -> object file: every source is compiled once per flag set and session
_dir = []


def clang(args, timeout=300):
    if not os.path.exists(CXX):
        pytest.skip("no clang++ under /opt/rocm")
    r = subprocess.run([CXX] + args, capture_output=True, text=True, timeout=timeout)
    if r.returncode != 0 and "sanitize" in r.stderr and "unsupported" in r.stderr:
        pytest.skip("sanitizer runtime not installed: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-3000:]


def build(name, san):
    """the program of CASES[name] under the sanitizer flags `san`: objects from the session's cache, one link"""
    if not _dir:
        _dir.append(tempfile.mkdtemp(prefix="nbody_host_sanitizers_"))
        atexit.register(shutil.rmtree, _dir[0], ignore_errors=True)
    host, stub = CASES[name][:2]
    objs = []
    for src in [os.path.join(ROOT, "mini_nbody_amd", "csrc", f) for f in host] + [os.path.join(ROOT, "tests", "host_stub", f) for f in stub]:
        key = (src, tuple(san))
        if key not in _objects:
            obj = os.path.join(_dir[0], "%d_%s.o" % (len(_objects), os.path.basename(src)))
            clang(FLAGS + san + ["-c", src, "-o", obj])
            _objects[key] = obj
        objs.append(_objects[key])
    exe = os.path.join(_dir[0], "%s_%d" % (name, len(_objects)))
    clang(san + objs + ["-o", exe, "-ldl", "-lpthread"])
    return exe


def run(name, exe, args, extra_env):
    clear, ok = CASES[name][3:]
    env = dict(os.environ, STUB_DEVICES="3", NBODY_OVERSUBSCRIBE="1", **extra_env)
    for k in clear:
        env.pop(k, None)
    out = subprocess.run([exe] + args, capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert ok in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr and "runtime error" not in out.stderr, out.stderr[-4000:]


@pytest.mark.skipif(shutil.which("make") is None, reason="no toolchain")
@pytest.mark.parametrize("name", list(CASES))
def test_host_code_is_address_and_ub_clean(name):
    run(name, build(name, ASAN), CASES[name][2], {"ASAN_OPTIONS": "detect_leaks=1"})


def test_served_mailbox_is_race_free_under_tsan():
    """the service thread against a second thread that calls nbody_get_info and every refused entry point while 4000 served requests of
    alternating sizes are posted and polled from memory"""
    run("host", build("host", TSAN), ["4000", "mailbox-only"], {"TSAN_OPTIONS": "halt_on_error=1"})
