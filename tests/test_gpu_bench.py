"""bench.py on the GPU: a plain run does only what its headline figure needs, and its timed steps compute the golden ids."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 2e-4      # as tests/test_gpu_fullsize.py: a top-2 margin within 10 x TOL of the largest logit is a near-tie
EXTRAS = ("roofline", "batch", "fleurs_like", "fleurs_like_cli", "fleurs_like_sessions", "strong_scaling", "streaming_encoder", "piecewise", "f32", "cpu_baseline")


@pytest.mark.gpu
def test_bench_plain_run_is_lean(tmp_path):
    """`bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR` in a process of its own: exit 0, one result line with the headline fields and none of the
    --full extras, the dumped ids equal to the CPU oracle's golden for this clip and model (up to its first near-tie), and at most 30 s of the run's wall
    time outside the 3 steps (start-up, weight synthesis, load, first-step capture, teardown)."""
    steps, warmup = 2, 1
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=600)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert (out["metric"], out["unit"], out["higher_is_better"], out["dtype"]) == ("decode_tok_per_s", "tok/s", True, "f32")
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == steps and out["warmup"] == warmup
    assert not [k for k in EXTRAS if k in out]
    g = np.load(os.path.join(ROOT, "tests", "golden", "fullsize_16s_oracle.npz"))
    ids = np.load(os.path.join(str(tmp_path), "ids.npy"))
    rids, top1, top2, amax = g["ids"], g["top1"], g["top2"], float(g["logit_absmax"])
    near = (top1 - top2) <= 10 * TOL * max(1.0, amax); first_tie = int(np.argmax(near)) if near.any() else len(rids)
    assert len(ids) == out["config"]["ids_per_clip"] == len(rids) == 108
    assert (ids[:first_tie] == rids[:first_tie]).all()
    outside = wall - (steps + warmup) * out["ms_per_step"] / 1e3
    print(f"plain bench: {wall:.1f} s wall, {outside:.1f} s outside the steps (weights synthesised in {out['weight_synthesis_s']} s, loaded in {out['load_s']} s)")
    assert outside <= 30.0
