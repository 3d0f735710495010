"""Runs a worker file's tests through pytest in a child process and hands back each test's outcome (tests/test_gpu_attn_decode_paged_ring.py,
tests/test_gpu_stream_group_endless.py): the launch counts of vox_debug_attn_launches are per process, and other tests of the suite hold the slots of the ring-table
forms to 0 in theirs."""
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

TESTS = os.path.dirname(os.path.abspath(__file__))


def run_worker(worker, tmp_dir, timeout):
    """-> ({test name: (outcome, detail)}, the child's output).  outcome: "passed", "failed", "skipped"."""
    xml = os.path.join(str(tmp_dir), "worker.xml")
    p = subprocess.run([sys.executable, "-m", "pytest", os.path.join(TESTS, worker), "-q", "-s", "-p", "no:cacheprovider", f"--junitxml={xml}"],
                       capture_output=True, text=True, timeout=timeout, cwd=os.path.dirname(TESTS))
    out = p.stdout + p.stderr
    assert os.path.exists(xml), f"{worker} left no report (exit status {p.returncode}):\n{out[-4000:]}"
    res = {}
    for case in ET.parse(xml).getroot().iter("testcase"):
        bad = [(c.tag, (c.get("message") or "") + "\n" + (c.text or "")) for c in case if c.tag in ("failure", "error", "skipped")]
        res[case.get("name")] = ("passed", "") if not bad else ("skipped" if bad[0][0] == "skipped" else "failed", bad[0][1])
    return res, out


def check(run, name):
    res, out = run
    assert name in res, f"{name} did not run; the worker ran {sorted(res)}:\n{out[-3000:]}"
    outcome, detail = res[name]
    assert outcome == "passed", f"{name} {outcome} in the worker process:\n{detail[-6000:]}"
