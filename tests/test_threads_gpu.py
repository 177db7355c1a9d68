"""The threading contract of include/rho2sdf_hip.h with concurrent host threads (tests/thread_cases.py has the cases, the
method and the child process).  Every other GPU test calls the library from one thread: a work buffer used outside its lock,
a thread_local table that became a plain global or a second user of the shared smoothing buffer that forgot the mutex
would pass them all.

One child interpreter per group, one at a time (the parent and one child have the GPU open); in it 4 threads run their
calls 8 times over and compare every output with the serial pass bit for bit.

  A  one r2s_rbf_field and one r2s_mesh_index read by all 4 threads, each with its own points and stream, host and _dev
     forms; a second field and index used by two of the threads in alternation ("one object may be used from several streams
     and threads at once");
  B  the families that lock a per-device work cache, each in turn and then mixed, with inputs of three sizes so that the
     buffers regrow between neighbouring calls ("concurrent calls are safe and run one after the other"), and the thread's
     last table after every call ("the calling thread's last ...");
  C  a HEX8 and a TET4 plan on two threads and two streams, the host-pointer entry points from the other two ("different
     plans are independent"; the per-device host session), then r2s_rho2sdf beside smoothing, field and tool calls;
  D  two threads whose calls are refused in between valid ones, two that make valid calls only (r2s_last_error belongs to
     the calling thread; a refused call leaves its outputs alone).

r2s_release_cache beside running calls is not tested: the header puts it outside the contract ("must not run concurrently
with any other call of the library"), and the code agrees - release_host_sessions() deletes a session that a caller may
have looked up and not yet locked.
"""
import json
import os
import subprocess
import sys
import time

import pytest

import thread_cases as C

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "thread_cases.py")
CHILD_SECONDS = 180     # the figure of test_large_paths_gpu.py; the child itself gives up (with every stack) after 150 s


def run_child(group, tmp_path):
    out = str(tmp_path / f"threads_{group}.json")
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable, CHILD, group, out], capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"group {group}: the child hung ({CHILD_SECONDS} s)\n{e.stdout}\n{e.stderr}", returncode=3)
    wall = time.perf_counter() - t0
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        # killed by a signal or a GPU fault: start nothing more on this GPU
        pytest.exit(f"group {group}: the child died (status {r.returncode})\n{r.stdout}{r.stderr}", returncode=3)
    if "Timeout (" in r.stderr and "most recent call first" in r.stderr:
        # faulthandler's dump: a deadlock; the stacks are the evidence
        pytest.exit(f"group {group}: the child hung, its threads were at\n{r.stderr}", returncode=3)
    assert r.returncode == 0, f"group {group}:\n{r.stdout}{r.stderr}"
    with open(out) as f:
        res = json.load(f)
    print(f"\n[threads {group}] child wall {wall:.1f} s; serial pass {res['serial_seconds']} s, concurrent pass "
          f"{res['concurrent_seconds']} s; live device bytes {res['live_before']} -> {res['live_after']}")
    for rd in res["rounds"]:
        print(f"  {rd['round']}: {rd['threads']} threads, {rd['compared']} calls compared, {rd['differ_calls']} differ "
              f"({rd['differ_words']} words), {rd['overlaps']} overlapping pairs of calls, {rd['seconds']} s")
    return res


@pytest.mark.parametrize("group", C.GROUPS)
def test_concurrent_threads(pkg, group, tmp_path):
    res = run_child(group, tmp_path)
    for rd in res["rounds"]:
        assert rd["differ_calls"] == 0, (group, rd["round"], rd["differ_calls"], rd["differ_words"], rd["notes"])
        assert rd["compared"] >= rd["threads"] * C.REPEATS, (group, rd)
        # a round in which no two threads were inside the library at once proves nothing
        assert rd["overlaps"] >= 1, (group, rd["round"], "no two calls of different threads overlapped in time")
    assert res["live_after"] == res["live_before"], (group, res["live_before"], res["live_after"])
