"""Worker of tests/test_gpu_attn_decode_ring.py: every ring decode attention launch of that module, in a process of its own.  The launch counts of
vox_debug_attn_launches are per process and model_fixtures.attn_launches holds slot [13] to 0, so a ring launch in the test process itself would fail every later
test that counts launches.  Usage: attn_ring_worker.py <repository root> <out.npz>.  For each run of ring_cases.RUNS: the ring launch's output, the flat launch's
output on the same keys laid out from row 0, and the launch counts each call added; then the refusal of window + 1 > max_seq."""
import ctypes
import os
import sys

import numpy as np

root, out_path = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from importlib import import_module

from __graft_entry__ import load_package

import attn_ring_cases as RC

pkg = load_package()
gg = import_module(pkg.__name__ + ".gguf")
N_SLOTS = 16


def counts():
    a = (ctypes.c_uint64 * N_SLOTS)()
    assert pkg.lib().vox_debug_attn_launches(a, N_SLOTS) == 0
    return np.array([int(x) for x in a], np.int64)


ctx = pkg.Context(0)
res = {}
for rid, run in RC.RUNS.items():
    flat, q, k, v = RC.flat_inputs(run)
    rk, rv = RC.to_ring(run, k, v)
    c0 = counts()
    out_flat = gg.attn_decode(ctx, q, k, v, flat.pos, flat.H, flat.KV, window=flat.window)
    c1 = counts()
    out_ring = gg.attn_decode_ring(ctx, q, rk, rv, [run.pos], flat.H, flat.KV, flat.window)
    c2 = counts()
    res[rid + "/flat"] = out_flat; res[rid + "/ring"] = out_ring; res[rid + "/flat_counts"] = c1 - c0; res[rid + "/ring_counts"] = c2 - c1

# (d) window + 1 > max_seq is refused, nothing is launched
run = RC.RUNS[next(iter(RC.RUNS))]
flat, q, k, v = RC.flat_inputs(run)
rk, rv = RC.to_ring(run, k, v)
c0 = counts()
try:
    gg.attn_decode_ring(ctx, q, rk, rv, [run.pos], flat.H, flat.KV, run.cap)
    msg = ""
except gg.VoxError as e:
    msg = str(e)
res["refusal/message"] = np.array(msg)
res["refusal/counts"] = counts() - c0
ctx.close()
np.savez(out_path, **res)
