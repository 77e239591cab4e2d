"""tests/ranks_common.py run_ranks, the launcher of every multi-process test, with plain Python scripts as ranks (no torch, no GPU):
a rank that fails ends the run at once and takes its peers with it, a rank's own children included; ranks that hang are ended at
the deadline; output far beyond a pipe buffer blocks nobody."""
import os
import textwrap
import time

import pytest

from ranks_common import run_ranks

MIB = 1 << 20


def script(body):
    return "import os, subprocess, sys, time\nrank = int(os.environ['RANK'])\n" + textwrap.dedent(body)


def wait_for(path):
    return "while not os.path.exists(%r): time.sleep(0.01)\n" % str(path)


def gone(pid, wait_s=5.0):
    """the process has ended: no entry under /proc, or a zombie that only awaits its (adoptive) parent's wait"""
    t0 = time.time()
    while time.time() - t0 < wait_s:
        try:
            state = open("/proc/%d/stat" % pid).read().rsplit(")", 1)[1].split()[0]
        except OSError:
            return True
        if state == "Z":
            return True
        time.sleep(0.02)
    return False


def test_a_failing_rank_ends_the_run_and_its_peer(tmp_path):
    pidfile = tmp_path / "pid1"
    src = script("""
        if rank == 0:
            %s
            print("rank zero gives up on purpose")
            sys.exit(3)
        sys.stdout.write("x" * %d)
        sys.stdout.flush()
        open(%r + ".tmp", "w").write(str(os.getpid()))
        os.replace(%r + ".tmp", %r)
        time.sleep(600)
    """ % (wait_for(pidfile).strip(), MIB, str(pidfile), str(pidfile), str(pidfile)))
    t0 = time.time()
    with pytest.raises(AssertionError) as e:
        run_ranks(tmp_path, src, 2, 300)
    assert time.time() - t0 < 10          # neither the sleeper nor the deadline was waited for
    assert "code 3" in str(e.value) and "rank zero gives up on purpose" in str(e.value)
    assert gone(int(pidfile.read_text()))


def test_ranks_that_hang_are_ended_at_the_deadline(tmp_path):
    src = script("""
        open(%r + str(rank), "w").write(str(os.getpid()))
        time.sleep(600)
    """ % str(tmp_path / "pid"))
    t0 = time.time()
    with pytest.raises(AssertionError, match="timed out"):
        run_ranks(tmp_path, src, 2, 2)
    assert time.time() - t0 < 12
    for r in range(2):
        assert gone(int((tmp_path / ("pid%d" % r)).read_text())), r


def test_a_ranks_own_child_goes_with_the_group(tmp_path):
    pidfile = tmp_path / "pids"
    src = script("""
        if rank == 0:
            %s
            sys.exit(3)
        child = subprocess.Popen([sys.executable, "-c", "import time; time.sleep(600)"])
        open(%r + ".tmp", "w").write("%%d %%d" %% (os.getpid(), child.pid))
        os.replace(%r + ".tmp", %r)
        time.sleep(600)
    """ % (wait_for(pidfile).strip(), str(pidfile), str(pidfile), str(pidfile)))
    with pytest.raises(AssertionError, match="code 3"):
        run_ranks(tmp_path, src, 2, 300)
    rank1, grandchild = (int(v) for v in pidfile.read_text().split())
    assert gone(rank1) and gone(grandchild)


def test_success_with_output_beyond_any_pipe_buffer(tmp_path):
    src = script("""
        sys.stdout.write("o" * %d + "\\nrank %%d done\\n" %% rank)
        sys.stderr.write("e" * %d)
    """ % (MIB, MIB))
    t0 = time.time()
    run_ranks(tmp_path, src, 2, 60, tag="loud")
    assert time.time() - t0 < 30
    for r in range(2):
        out = (tmp_path / "loud_logs" / ("a0_rank%d.out" % r)).read_text()
        assert len(out) > MIB and out.endswith("rank %d done\n" % r)
        assert os.path.getsize(tmp_path / "loud_logs" / ("a0_rank%d.err" % r)) == MIB


def test_a_rank_ended_by_a_signal_counts_as_failed(tmp_path):
    src = script("""
        if rank == 1:
            os.kill(os.getpid(), 9)
        time.sleep(600)
    """)
    with pytest.raises(AssertionError, match="code -9"):
        run_ranks(tmp_path, src, 2, 300)


def test_environment_of_a_rank(tmp_path, monkeypatch):
    """RANK, WORLD_SIZE, LOCAL_RANK and the rendezvous address are set, env_of(rank) lies on top, and the caller's OMP_NUM_THREADS,
    which the launcher takes away for the benchmark's sake, is handed back"""
    monkeypatch.setenv("OMP_NUM_THREADS", "5")
    src = script("""
        e = os.environ
        assert e["WORLD_SIZE"] == "3" and e["LOCAL_RANK"] == str(10 + rank) and e["MASTER_ADDR"] == "127.0.0.1" and int(e["MASTER_PORT"]) > 0
        assert e["OMP_NUM_THREADS"] == ("1" if rank == 2 else "5") and e["MINE"] == "r%d" % rank
    """)
    run_ranks(tmp_path, src, 3, 60, env_of=lambda r: dict({"MINE": "r%d" % r}, **({"OMP_NUM_THREADS": "1"} if r == 2 else {})), local_of=lambda r: 10 + r)
