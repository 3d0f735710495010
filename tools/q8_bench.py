#!/usr/bin/env python3
"""Times the Q8_0 linear kernels (csrc/vox_q8.hip) at the model's matrix shapes against the Q4_0 kernels the same entry picks for a Q4 handle of the same shape:
    python tools/q8_bench.py [--out profiles/q8_linear.txt] [--rounds 7] [--calls 40] [--shapes "dec w2,enc w2"] [--root OTHER_CHECKOUT]
Every (shape, M) runs `rounds` rounds that alternate a batch of Q8 calls and a batch of Q4 calls on device buffers (vox_linear_forward_ex, VOX_MEM_DEVICE), each batch
between two stream synchronisations under a host clock; the medians are reported.  The calls of a batch walk over `copies` device copies of the matrix so that the
weights come from memory, not from the 256 MB last-level cache, where 16 copies suffice for that (column `mem`; `llc`: the Q4 copies together stay below 320 MB
and may be served from the cache).  The calls are enqueued from Python: a call shorter than the enqueue itself measures the enqueue.
GB/s counts the algorithmic bytes: the weight blocks once, the rows in, the rows out.  For M <= 4 the kernels are bandwidth-bound and the derived expectation for
Q8 / Q4 is the bytes ratio 34 / 18 = 1.89.
A second table times the K-slice operator (csrc/vox_q8_slices.hip) through its own entry, vox_q8_rows_forward, at the decode shapes with K <= 8192, where the linear
entry runs q8_rows_kernel: new operator, rows kernel and Q4 GEMV alternate in every round.  The operator's two launches are timed together (a host clock cannot
separate the finishing launch).  --root: load the package of another checkout (the parent commit, built there) to time both in one visit; a package without the
new entry prints the first table only.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
from __graft_entry__ import load_package  # noqa: E402

SHAPES = [("enc q|k|v", 6144, 1280), ("enc wo", 1280, 2048), ("enc w1|w3", 10240, 1280), ("enc w2", 1280, 5120),
          ("dec q|k|v", 6144, 3072), ("dec w1|w3", 18432, 3072), ("dec w2", 3072, 9216)]
ROWS = (1, 4, 16, 64)
SLICE_SHAPES, SLICE_ROWS = ("dec q|k|v", "dec w1|w3", "enc w2"), (1, 4)          # the second table: K <= 8192, M <= 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None); ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--shapes", default=None); ap.add_argument("--root", default=None)
    a = ap.parse_args()
    shapes = [s for s in SHAPES if a.shapes is None or s[0] in a.shapes.split(",")]
    pkg = load_package(); ctx = pkg.Context(0); L = pkg.lib(); rng = np.random.default_rng(0)
    lines = [f"# tools/q8_bench.py --rounds {a.rounds} --calls {a.calls}: median us per call, GB/s on algorithmic bytes, Q8 / Q4 time (bytes ratio 1.89)",
             f"# {'shape':10s} {'N':>6s} {'K':>5s} {'M':>3s} {'mem':>4s} {'q8 kernel':>9s} {'q8 us':>8s} {'q8 GB/s':>8s} {'q4 us':>8s} {'q4 GB/s':>8s} {'q8/q4':>6s}"]
    slice_lines = [f"# vox_q8_rows_forward (K-slice operator, two launches) next to q8_rows_kernel and the Q4 GEMV: median us per call",
                   f"# {'shape':10s} {'N':>6s} {'K':>5s} {'M':>3s} {'slices us':>9s} {'rows us':>8s} {'q4 us':>8s} {'sl/rows':>7s} {'sl/q4':>6s}"]
    for name, N, K in shapes:
        q4_bytes, q8_bytes = N * K // 32 * 18, N * K // 32 * 34
        copies = min(16, -(-(320 << 20) // q4_bytes))
        raw4 = pkg.synth.synth_q4_blocks(rng, N * K, 0.03)
        raw8 = pkg.quantize_q8_0(pkg.synth.dequantize_q4_0(raw4, N * K))
        t4 = [pkg.Q4Tensor.from_q4_bytes(raw4, [N, K], ctx) for _ in range(copies)]
        t8 = [pkg.q8_tensor_from_bytes(raw8, [N, K], ctx) for _ in range(copies)]
        for M in ROWS:
            dx = ctx.upload(rng.standard_normal((M, K)).astype(np.float32)); dy = ctx.alloc(M * N * 4)

            def batch(ts, n):
                ctx.synchronize(); t0 = time.perf_counter()
                for i in range(n):
                    pkg._lib.check(L.vox_linear_forward_ex(ctx.h, ts[i % copies].h, None, C.c_void_p(dx), 1, M, C.c_void_p(dy), 0, 1))
                ctx.synchronize()
                return (time.perf_counter() - t0) / n * 1e6
            batch(t8, 2 * copies); batch(t4, 2 * copies)          # every copy of every kernel once
            us8, us4 = [], []
            for _ in range(a.rounds):
                us8.append(batch(t8, a.calls)); us4.append(batch(t4, a.calls))
            m8, m4 = statistics.median(us8), statistics.median(us4)
            io = (M * K + M * N) * 4
            lines.append(f"  {name:10s} {N:6d} {K:5d} {M:3d} {'llc' if copies * q4_bytes < (320 << 20) else 'hbm':>4s} {('rows' if K <= 8192 else 'slices' if hasattr(pkg, 'q8_rows_forward') else 'gemm') if M <= 4 else 'gemm':>9s} {m8:8.1f} {(q8_bytes + io) / m8 / 1e3:8.0f} "
                         f"{m4:8.1f} {(q4_bytes + io) / m4 / 1e3:8.0f} {m8 / m4:6.2f}   (spread q8 {min(us8):.1f}..{max(us8):.1f}, q4 {min(us4):.1f}..{max(us4):.1f})")
            print(lines[-1], flush=True)
            if name in SLICE_SHAPES and M in SLICE_ROWS and hasattr(pkg, "q8_rows_forward"):
                def batch_s(n):
                    ctx.synchronize(); t0 = time.perf_counter()
                    for i in range(n):
                        pkg._lib.check(L.vox_q8_rows_forward(ctx.h, t8[i % copies].h, None, None, C.c_float(0.0), C.c_void_p(dx), M, C.c_void_p(dy), 0, 0, None, 1))
                    ctx.synchronize()
                    return (time.perf_counter() - t0) / n * 1e6
                batch_s(2 * copies); uss, usr, usq = [], [], []
                for _ in range(a.rounds):
                    uss.append(batch_s(a.calls)); usr.append(batch(t8, a.calls)); usq.append(batch(t4, a.calls))
                ms, mr, mq = statistics.median(uss), statistics.median(usr), statistics.median(usq)
                slice_lines.append(f"  {name:10s} {N:6d} {K:5d} {M:3d} {ms:9.1f} {mr:8.1f} {mq:8.1f} {ms / mr:7.2f} {ms / mq:6.2f}   (spread slices {min(uss):.1f}..{max(uss):.1f}, rows {min(usr):.1f}..{max(usr):.1f}, q4 {min(usq):.1f}..{max(usq):.1f})")
                print(slice_lines[-1], flush=True)
            ctx.free(dx); ctx.free(dy)
        for t in t4 + t8:
            t.close()
    if len(slice_lines) > 2:
        lines += slice_lines
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
