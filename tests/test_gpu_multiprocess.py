"""Process-per-GPU flow on hardware: two (three) OS processes, each with its own HIP context on this box's one GPU,
rendezvous over gloo, nbody_init_rank(), positions exchanged every step through the host-staged transport
(nbody_set_host_gather) — i.e. everything the 8-GPU job does except that the slices travel through host memory
instead of RCCL/xGMI.  Result must equal one process configured with the same segmentation, bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

from mini_nbody_amd.launcher import free_port
from ranks_common import run_ranks, shared_gpu_env, worker_source

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = """
    steps = {steps}
    eng.set_option(nb.OPT_JSUB, {jsub})
    eng.set_option(nb.OPT_OVERLAP, {overlap})
    if {comm} >= 0:
        eng.set_option(nb.OPT_COMM, {comm})
        eng.comm_selftest()
    pos, vel = nb.make_bodies(n, seed=33, dtype=np.float64 if {fp64} else np.float32)
    f = eng.forces(pos)                      # every process gets all N force words (the other ranks' rows are gathered)
    eng.upload(pos, vel)
    eng.step(0.01, steps)
    p, v = eng.download()
    cfg = eng.config
    assert cfg["nranks"] == world and cfg["rank"] == rank
    if rank == 0:
        open({out!r} + "_wsplit.txt", "w").write(str(cfg["wsplit"]))
    if rank == world - 1:
        np.save({out!r} + "_force.npy", f)
    if rank == 0:
        np.save({out!r} + "_pos.npy", p); np.save({out!r} + "_vel.npy", v)
"""


def run_job(tmp_path, tag, world, timeout_s, env_of, local_of=None, **fmt):
    """WORKER as `world` ranks; -> the stem of the files ranks 0 and world - 1 leave"""
    out = str(tmp_path / tag)
    run_ranks(tmp_path, worker_source(WORKER, engine="fp64={fp64}, transport={transport!r}", out=out, **fmt), world, timeout_s, env_of, local_of,
              tag="worker_" + tag)
    return out


def check_against_one_gpu(nb, out, n, world, jsub, steps, fp64=False, what=None):
    """The job's result against ONE process configured with the job's summation order: its slices, its pieces per slice, its waves per
    workgroup (<out>_wsplit.txt: the engine picks them from a rank's body count, which differs between the job and this one-GPU
    restatement) — forces, positions and velocities bit for bit."""
    u = np.uint64 if fp64 else np.uint32
    pos, vel = nb.make_bodies(n, seed=33, dtype=np.float64 if fp64 else np.float32)
    one = nb.NBody(n, fp64=fp64)
    try:
        one.set_option(nb.OPT_JSUB, jsub)
        one.set_option(nb.OPT_JSLICES, world)
        one.set_option(nb.OPT_WSPLIT, int(open(out + "_wsplit.txt").read()))
        wf = one.forces(pos)
        one.upload(pos, vel)
        one.step(0.01, steps)
        wp, wv = one.download()
    finally:
        one.close()
    assert np.array_equal(np.load(out + "_pos.npy").view(u), wp.view(u)), what
    assert np.array_equal(np.load(out + "_vel.npy").view(u), wv.view(u)), what
    assert np.array_equal(np.load(out + "_force.npy").view(u), wf.view(u)), what


@pytest.mark.parametrize("world,overlap", [(2, 1), (3, 0), (3, 2)])
def test_two_processes_one_gpu_host_transport(nb, tmp_path, world, overlap):
    n, steps, jsub = 12000 + 7, 3, 2
    out = run_job(tmp_path, "mp", world, 600, shared_gpu_env, n=n, steps=steps, jsub=jsub, overlap=overlap, transport="host", comm=-1, fp64=False)
    check_against_one_gpu(nb, out, n, world, jsub, steps)


def test_bench_launches_and_supervises_its_own_workers(tmp_path):
    """`python bench.py --gpus 2` with no WORLD_SIZE: the parent starts two fresh worker processes (it never touches the GPU
    itself), both share this box's one GPU, RCCL refuses a second rank on the same device, the supervisor ends that attempt
    and the job runs again on the peer-copy transport (one process, two virtual ranks) — one JSON line with n_gpus 2,
    roofline, cpu_baseline, the transport used, why RCCL was not, and the exposed communication."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["NBODY_OVERSUBSCRIBE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--bodies", "262144", "--steps", "3", "--warmup", "1",
                        "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["value"] > 0 and out["config"]["finite"]
    assert out["roofline"]["frac"] > 0 and out["cpu_baseline"]["value"] > 0
    assert "peer copies" in out["config"]["comm"] and "rccl attempt:" in out["config"]["comm"] and "RCCL error" in out["config"]["comm"]
    assert out["comm_exposed_ms_per_step"] >= 0 and out["config"]["kernel"]["nranks"] == 2
    # machine-readable account of what ran: a scaling driver must not take this for the RCCL point
    assert out["transport_used"] == "peer" and out["fallback_from"] == "rccl" and "RCCL error" in out["fallback_reason"]
    assert [a["transport"] for a in out["attempts"]] == ["rccl", "peer"] and out["attempts"][1]["result"] == "ok"
    assert out["attempts"][0]["import_s"] is not None and out["supervisor_seconds"] > 0
    # the extras pass ran in the same workers after the headline line: one entry for a transport that has no forms
    assert set(out["comm_forms"]) == {"peer"} and out["comm_forms"]["peer"]["ms_per_step"] > 0 and "extras" not in out
    assert "config5" not in out          # BASELINE configs[4] is an 8-GPU configuration: only there (or with --extras all)


def test_bench_no_fallback_exit_code(tmp_path):
    """--no-fallback: RCCL refuses the second rank on the one device -> exit code 3, no line, no retry on peer copies"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["NBODY_OVERSUBSCRIBE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--bodies", "65536", "--steps", "2", "--no-fallback",
                        "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 3, r.stdout[-2000:] + r.stderr[-3000:]
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")] and "attempt 1" not in r.stderr


def test_bench_peer_copy_transport(tmp_path):
    """`--transport peer`, the first fallback when RCCL cannot be used: rank 0 drives all the GPUs from one process with
    peer copies (here: two virtual ranks on the one GPU), the other rank only keeps the barriers."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["NBODY_OVERSUBSCRIBE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--bodies", "262144", "--steps", "3", "--warmup", "1",
                        "--transport", "peer", "--full", "--no-cpu-baseline", "--extras", "all", "--config5-bodies", "65536"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["finite"]
    assert "hipMemcpyPeerAsync" in out["config"]["comm"] and "one process driving all 2 GPUs" in out["config"]["comm"]
    assert out["config"]["kernel"]["nranks"] == 2 and out["config"]["kernel"]["launches_per_step"] == 2
    assert out["roofline"]["kernel_launches"] == 2 * 3 and 0 < out["roofline"]["frac"] < 1
    assert out["transport_used"] == "peer" and out["fallback_from"] is None and len(out["attempts"]) == 1
    # --extras all: the transfer "forms" of this transport (one) and the fp64 configuration (here at 65536 bodies), after the headline
    assert set(out["comm_forms"]) == {"peer"} and "extras" not in out
    c5 = out["config5"]
    assert c5["value"] > 0 and 0 < c5["roofline"]["frac"] < 1 and c5["roofline"]["peak"] == 78.6 and c5["hbm_gb_per_s"] > 0
    assert c5["kernel"]["n_local"] == 32768 and c5["comm_exposed_ms_per_step"] >= 0


def gpu_count():
    """devices on this box, without initialising the GPU in the test process (torch.cuda.device_count() does not, on this image)"""
    import torch
    return torch.cuda.device_count()


def test_real_rccl_job_is_bit_identical_to_one_gpu(nb, tmp_path):
    """the first real multi-rank RCCL run must not be the timed benchmark.  Needs >= 2 GPUs (skipped on the one-GPU
    box): one process per GPU, RCCL over xGMI, every transfer form and overlap mode, ragged N (slices of different lengths, so
    NBODY_COMM_AUTO resolves to DIRECT and ALLGATHER to RING) — forces, positions and velocities after 4 steps bit for bit equal
    to one GPU configured with the job's segmentation (NBODY_OPT_JSLICES = P, the job's pieces per slice and waves per workgroup)."""
    if gpu_count() < 2:
        pytest.skip("needs two GPUs: RCCL refuses two ranks on one device")
    world = min(gpu_count(), 4)
    for comm_name, overlap in (("auto", 1), ("auto", 0), ("ring", 2), ("ring", 1), ("direct", 1), ("direct", 2), ("allgather", 0)):
        _one_rccl_job(nb, tmp_path, world, comm_name, overlap)


def _one_rccl_job(nb, tmp_path, world, comm_name, overlap):
    comm = {"auto": nb.COMM_AUTO, "ring": nb.COMM_RING, "direct": nb.COMM_DIRECT, "allgather": nb.COMM_ALLGATHER}[comm_name]
    n, steps, jsub = 30000 + 7, 4, 2
    out = run_job(tmp_path, "rccl_%s_%d" % (comm_name, overlap), world, 600, lambda r: {"NBODY_DEVICE": str(r), "HSA_ENABLE_IPC_MODE_LEGACY": "0"},
                  local_of=lambda r: r, n=n, steps=steps, jsub=jsub, overlap=overlap, transport="rccl", comm=comm, fp64=False)
    check_against_one_gpu(nb, out, n, world, jsub, steps, what=(comm_name, overlap))


@pytest.mark.parametrize("virtual_hosts", [False, True])
def test_bench_under_torch_distributed_run(tmp_path, virtual_hosts):
    """The driver's own form for N > 1: `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1
    --master-port P bench.py --gpus N --steps K --warmup W`.  Every rank process then supervises its own worker and the supervisors
    agree through their shared directory (port, verdicts, the "headline printed" marker).  On this box both workers land on the one
    GPU: RCCL refuses the second rank, every supervisor ends its attempt, the peer-copy attempt runs (rank 0's worker drives two
    virtual ranks), the extras pass follows the headline — and exactly ONE line comes out, from rank 0's supervisor."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env["NBODY_OVERSUBSCRIBE"] = "1"
    if virtual_hosts:       # every rank poses as its own host: the RCCL attempt itself succeeds (two real ranks over loopback sockets)
        env["NBODY_VIRTUAL_HOSTS"] = "1"
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--bodies", "131072", "--full"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 3 and out["value"] > 0 and out["config"]["finite"]
    # round 5: an N > 1 line carries a MEASURED host-CPU baseline of its own (a 3-second row sample on rank 0 while the other ranks wait)
    cb = out["cpu_baseline"]
    assert out["roofline"]["frac"] > 0 and cb["value"] > 0 and cb["cores"] >= 1 and cb["kind"] == "port" and "extras" not in out
    if virtual_hosts:
        assert out["transport_used"] == "rccl" and out["fallback_from"] is None and [a["transport"] for a in out["attempts"]] == ["rccl"]
        assert set(out["comm_forms"]) == {"allgather", "direct", "ring", "allgather_gather_first"} and "/ rccl /" in out["config"]["comm"]
    else:
        assert out["transport_used"] == "peer" and out["fallback_from"] == "rccl" and [a["transport"] for a in out["attempts"]] == ["rccl", "peer"]
        assert set(out["comm_forms"]) == {"peer"}


def virtual_host_env(rank):
    """several RCCL ranks on ONE device: each poses as a host of its own (RCCL compares host id and bus id before refusing a duplicate GPU)
    and RCCL connects them through its socket transport over loopback"""
    return dict(shared_gpu_env(rank), NCCL_HOSTID="nbody-virtual-host-%d" % rank, NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")


@pytest.mark.parametrize("world", [2, 3])
def test_real_rccl_ranks_on_one_gpu_over_loopback(nb, tmp_path, world):
    """ADVICE r03, answered on the one-GPU box after all: a REAL multi-rank RCCL job — `world` processes, ncclCommInitRank over `world` ranks,
    ncclAllGather / grouped ncclSend + ncclRecv between different ranks, the second stream, the per-slice events, the hand-shake — with the
    ranks sharing this box's one GPU and posing as separate hosts so that RCCL links them by loopback sockets instead of refusing the
    duplicate device.  Every transfer form and overlap mode, ragged N: the self-test checks every received word, and forces, positions and
    velocities after 4 steps equal the one-GPU restatement of the job's summation order bit for bit."""
    forms = (("auto", 1), ("auto", 0), ("ring", 2), ("ring", 1), ("direct", 1), ("direct", 2), ("allgather", 1)) if world == 2 else \
            (("auto", 1), ("ring", 2), ("direct", 1), ("allgather", 0))
    for comm_name, overlap in forms:
        comm = {"auto": nb.COMM_AUTO, "ring": nb.COMM_RING, "direct": nb.COMM_DIRECT, "allgather": nb.COMM_ALLGATHER}[comm_name]
        n, steps, jsub = 30000 + 7, int(os.environ.get("NBODY_TEST_RCCL_STEPS", "4")), 2      # (a soak sets the step count: profiles/r04_rccl_soak.txt)
        out = run_job(tmp_path, "lo_%s_%d" % (comm_name, overlap), world, 240, virtual_host_env, n=n, steps=steps, jsub=jsub, overlap=overlap,
                      transport="rccl", comm=comm, fp64=False)
        check_against_one_gpu(nb, out, n, world, jsub, steps, what=(comm_name, overlap))


def test_bench_rccl_attempt_with_virtual_hosts(tmp_path):
    """`NBODY_VIRTUAL_HOSTS=1 python bench.py --gpus 2`: the supervised RCCL attempt itself succeeds on this box — two worker processes, one
    RCCL communicator of two ranks, the transfer self-test, the timed steps with the all-gather on the second stream — so the line says
    transport_used rccl with no fallback, and the extras pass measures the three transfer forms and the fp64 configuration over RCCL."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env["NBODY_VIRTUAL_HOSTS"] = "1"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--bodies", "262144", "--steps", "3", "--warmup", "1",
                        "--full", "--no-cpu-baseline", "--extras", "all", "--config5-bodies", "65536", "--autotune"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["config"]["finite"]
    assert out["transport_used"] == "rccl" and out["fallback_from"] is None and [a["transport"] for a in out["attempts"]] == ["rccl"]
    assert "/ rccl /" in out["config"]["comm"] and "autotuned in warm-up" in out["config"]["comm"]
    assert set(out["comm_forms"]) == {"allgather", "direct", "ring", "allgather_gather_first"} and all(e["ms_per_step"] > 0 for e in out["comm_forms"].values())
    assert out["comm_forms"]["allgather_gather_first"]["overlap"] == 0 and out["comm_forms"]["allgather_gather_first"]["comm_exposed_ms_per_step"] > 0
    assert out["comm_forms"]["ring"]["form_resolved"] == "ring" and out["comm_forms"]["ring"]["overlap"] == 2
    assert out["config5"]["value"] > 0 and out["config5"]["kernel"]["n_local"] == 32768 and "extras" not in out
    assert out["comm_exposed_ms_per_step"] >= 0 and out["config"]["kernel"]["nranks"] == 2


def test_real_rccl_fp64_job_on_one_gpu_over_loopback(nb, tmp_path):
    """config 5's arithmetic over real RCCL: a two-rank fp64 job (32-byte words through ncclAllGather), ranks sharing the GPU as separate
    virtual hosts — bit-identical to the one-GPU restatement"""
    world, n, steps, jsub = 2, 20000 + 3, 3, 2
    out = run_job(tmp_path, "lo64", world, 240, virtual_host_env, n=n, steps=steps, jsub=jsub, overlap=1, transport="rccl", comm=nb.COMM_AUTO, fp64=True)
    check_against_one_gpu(nb, out, n, world, jsub, steps, fp64=True)
