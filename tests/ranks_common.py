"""The ranks of a multi-process test: started and supervised by the product's own launcher (mini_nbody_amd/launcher.py, covered by
tests/test_bench_launcher.py), and the prologue and epilogue the worker scripts share.  Every rank gets a session of its own, a
parent-death signal and log files instead of pipes; the first non-zero exit (a signal counts) or the deadline ends the wait with a
reason; and whatever happened — a failure, the deadline, Ctrl-C — exactly the process groups that were started are ended before
run_ranks returns, so no rank is left in a barrier with the GPU open.  Covered by tests/test_ranks_common.py."""
import os
import sys
import textwrap

from mini_nbody_amd import launcher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROLOGUE = textwrap.dedent("""
    import json, os, sys, time
    import numpy as np
    sys.path[:0] = [{root!r}, os.path.join({root!r}, "tests"), os.path.join({root!r}, "oracle")]
    import torch, torch.distributed as dist
    import mini_nbody_amd as nb
    import mini_nbody_amd.distributed as D
    rank, world, local = D.init_process_group("gloo")
""")
ENGINE = textwrap.dedent("""
    n = {n}
    eng = D.make_engine(n, %s)
""")
EPILOGUE = textwrap.dedent("""
    dist.barrier(); dist.destroy_process_group()
""")


def worker_source(body, engine='transport="host"', **fmt):
    """The script of one rank: the imports and the gloo rendezvous, `eng = D.make_engine(n, <engine>)` (engine: the arguments after
    n, None for a worker that has no engine), `body`, then eng.close(), the barrier and the group's end.  `body` and `engine` are
    str.format templates over `fmt` (and root)."""
    parts = [PROLOGUE, "" if engine is None else ENGINE % engine, textwrap.dedent(body), "" if engine is None else "eng.close()", EPILOGUE]
    return "".join(parts).format(root=ROOT, **fmt)


def shared_gpu_env(rank):
    """every rank on this box's one GPU"""
    return {"NBODY_DEVICE": "0", "HSA_ENABLE_IPC_MODE_LEGACY": "0"}


def run_ranks(tmp_path, source, world, timeout_s, env_of=None, local_of=None, tag="worker"):
    """Run `source` as `world` ranks (RANK, WORLD_SIZE, LOCAL_RANK = local_of(rank) or 0, MASTER_ADDR, MASTER_PORT set; env_of(rank) on
    top) and return once all have exited with 0.  Raises AssertionError with the reason and the end of every rank's logs otherwise."""
    script = tmp_path / (tag + ".py")
    script.write_text(source)
    logdir = tmp_path / (tag + "_logs")
    logdir.mkdir(exist_ok=True)
    # start_worker drops OMP_NUM_THREADS for bench.py's CPU-baseline leg; a test's ranks keep what the caller (or the machine) set
    keep = {k: os.environ[k] for k in ("OMP_NUM_THREADS",) if k in os.environ}
    port = launcher.free_port()
    procs = []
    try:
        for r in range(world):
            env = dict(keep, **(env_of(r) if env_of else {}))
            procs.append(launcher.start_worker([sys.executable, str(script)], r, local_of(r) if local_of else 0, world, port, None, str(logdir), 0, env))
        reason = launcher.wait_workers(procs, timeout_s)
    finally:
        for p, _, _ in procs:
            launcher.kill_group(p)
    if reason is not None:
        logs = ["rank %d (exit %s)\n  stdout: %s\n  stderr: %s" % (r, p.returncode, launcher.tail(out, 3000), launcher.tail(err, 3000))
                for r, (p, out, err) in enumerate(procs)]
        raise AssertionError("%s: %s\n%s" % (tag, reason, "\n".join(logs)))
