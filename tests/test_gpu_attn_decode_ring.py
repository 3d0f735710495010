"""The ring decode attention (attn_decode_kernel<128, false, true>, launch_attn_decode_ring) one launch at a time through vox_debug_attn_decode_ring: cases and
layout in tests/attn_ring_cases.py.  Per run: (a) the output has the bits of the flat launch (vox_debug_attn_decode) on the same keys laid out from row 0 with
pos = n - 1 and the same window; (b) it is within attn_decode_ref.BAR of the float64 reference, row by row; (c) exactly one launch ran, counted in slot [13] of
vox_debug_attn_launches; and once: (d) window + 1 > max_seq is refused, nothing launched.  Every ring row outside the window is NaN, so a key read there shows.

The launches run in ONE child process (tests/attn_ring_worker.py: the launch counts are per process, and the suite's other tests hold slot [13] to 0); this module
asserts on what it wrote.  The head_dim-64 instantiation has no caller (the entry refuses head_dim != 128, as vox_debug_attn_decode does)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import attn_decode_ref as R
import attn_ring_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RING_SLOT, FLAT_SLOT = 13, 3


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("attn_ring") / "out.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "attn_ring_worker.py"), ROOT, out], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, f"the ring worker failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    with np.load(out) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("rid", list(RC.RUNS))
def test_ring_launch(results, rid):
    run = RC.RUNS[rid]
    flat, q, k, v = RC.flat_inputs(run)
    ring, flat_out = results[rid + "/ring"], results[rid + "/flat"]
    # (c) one launch, of the ring form; the flat twin took the per-head flat form
    want = np.zeros(16, np.int64); want[RING_SLOT] = 1
    assert np.array_equal(results[rid + "/ring_counts"], want), results[rid + "/ring_counts"]
    want = np.zeros(16, np.int64); want[FLAT_SLOT] = 1
    assert np.array_equal(results[rid + "/flat_counts"], want), results[rid + "/flat_counts"]
    # (b) the float64 reference, on the flat layout
    ref = R.reference(flat, q, k, v)
    e = R.row_err(ring, ref, flat.H)
    print(f"{rid}: {RC.window_of(run)[1]} keys from ring row {RC.window_of(run)[0] % run.cap}, worst row {e.max():.2e} of its max (bar {R.BAR:.0e})")
    assert np.isfinite(ring).all(), "a NaN ring row (outside the window) was read"
    assert (e <= R.BAR).all(), e
    assert (R.row_err(flat_out, ref, flat.H) <= R.BAR).all()
    # (a) the flat launch's bits
    assert np.array_equal(ring.view(np.uint32), flat_out.view(np.uint32)), f"{int((ring.view(np.uint32) != flat_out.view(np.uint32)).sum())} values differ from the flat launch"


def test_window_past_the_ring_is_refused(results):
    msg = str(results["refusal/message"])
    assert "window" in msg and "ring" in msg, msg
    assert not results["refusal/counts"].any()
