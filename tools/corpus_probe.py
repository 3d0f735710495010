#!/usr/bin/env python3
"""Stage breakdown of the FLEURS-like corpus call (bench.py `fleurs_like`): one vox_transcribe_batch over 647 clips with VOX_BATCH_VERBOSE=1.
    python tools/corpus_probe.py [n_clips=647] [reps=2] [sessions=1]      (sessions > 1: vox_model_set_sessions)
    python tools/corpus_probe.py [n_clips] [reps] [sessions] --records [K=8]
--records: what the per-id records cost.  The same corpus call unscored, scored (scores alone) and scored with K alternatives, alternating, `reps` times each after one
warm-up round: wall time, tok/s, decode ms per replayed step, graph replays and launch counts per variant, medians at the end.  Then the records kernel alone on
1024 device rows of the model's vocabulary: the fused launch (vox_records_rows, k = K) next to score_rows followed by alternatives_rows, the live sessions' two launches."""
import importlib, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from __graft_entry__ import load_package
import bench
argv = sys.argv[1:]
records = None
if "--records" in argv:
    i = argv.index("--records"); records = 8
    if i + 1 < len(argv) and argv[i + 1].isdigit():
        records = int(argv.pop(i + 1))
    argv.pop(i)
    if not 1 <= records <= 8:
        sys.exit("--records takes K in 1..8")
n = int(argv[0]) if len(argv) > 0 else 647
reps = int(argv[1]) if len(argv) > 1 else 2
sessions = int(argv[2]) if len(argv) > 2 else 1
pkg = load_package(); ctx = pkg.Context(0)
shard = importlib.import_module(pkg.__name__ + ".shard")
path = bench.full_gguf_path(pkg, 42, 0, lambda: None)
m = pkg.Q4ModelLoader.from_file(path).load(ctx); t = pkg.TimeEmbedding(m.config.dec_dim).embed(6.0)
durs = shard.fleurs_like_durations(n, seed=7)
clips = [pkg.synth.synth_audio(durs[i], seed=9000 + i) for i in range(n)]
if sessions > 1:
    m.set_sessions(sessions)


def launches():
    from model_fixtures import attn_launches, gemm_launches
    return sum(gemm_launches(pkg).values()) + sum(attn_launches(pkg).values())


def one(label, call):
    l0 = launches(); ctx.synchronize(); t0 = time.perf_counter(); outs = call(); ctx.synchronize(); dt = time.perf_counter() - t0
    tm = m.timings(); ids = sum(len(o) for o in outs); step = tm["decode_ms"] / max(tm["graph_replays"], 1)
    print(f"{label}: {dt:.3f} s, {ids} ids, {ids / dt:.0f} tok/s; stage ms: pre {tm['preprocess_ms']:.0f} enc {tm['encode_ms']:.0f} dec {tm['decode_ms']:.0f}, replays {tm['graph_replays']}, "
          f"decode ms per replayed step {step:.3f}, linear + attention launches {launches() - l0}", flush=True)
    return dt, ids / dt, step, outs


if records is None:
    os.environ["VOX_BATCH_VERBOSE"] = "1"
    for r in range(reps + 1):
        one(f"rep {r}", lambda: m.transcribe_batch(clips, t))
else:
    if not hasattr(m, "transcribe_batch_scored"):      # (a library from before the records: the unscored call alone, for its spread)
        variants = {"unscored": lambda: m.transcribe_batch(clips, t)}
    else:
        variants = {"unscored": lambda: m.transcribe_batch(clips, t), "scored k=0": lambda: m.transcribe_batch_scored(clips, t, alternatives=0)[0],
                    f"scored k={records}": lambda: m.transcribe_batch_scored(clips, t, alternatives=records)[0]}
    os.environ["VOX_BATCH_NO_CALIB"] = "1"      # one slot plan for every call: the variants run the same steps
    res = {k: [] for k in variants}; ref = None
    for r in range(reps + 1):
        for k, call in variants.items():
            dt, rate, step, outs = one(f"{'warm-up' if r == 0 else f'rep {r}'}, {k}", call)
            if ref is None:
                ref = outs
            same = all((a == b).all() for a, b in zip(ref, outs))
            if not same:
                print(f"  !! {k}: ids differ from the first call's", flush=True)
            if r > 0:
                res[k].append((dt, rate, step))
    for k, v in res.items():
        print(f"median of {len(v)}, {k}: {statistics.median(x[0] for x in v):.3f} s (min {min(x[0] for x in v):.3f}, max {max(x[0] for x in v):.3f}), "
              f"{statistics.median(x[1] for x in v):.0f} tok/s, decode ms per replayed step {statistics.median(x[2] for x in v):.3f}", flush=True)
    if hasattr(pkg, "records_rows"):
        import numpy as np
        V = m.config.vocab; M = 1024
        x = (3.0 * np.random.default_rng(5).standard_normal((M, V))).astype(np.float32); p = ctx.upload(x)

        def timed(call, n_it=5):
            call(); ts = []
            for _ in range(n_it):
                ctx.synchronize(); t0 = time.perf_counter(); call(); ts.append(time.perf_counter() - t0)      # (every call ends in a synchronise)
            return statistics.median(ts) * 1e3
        fused = timed(lambda: pkg.records_rows(ctx, None, records, device_ptr=p, shape=(M, V)))
        fused0 = timed(lambda: pkg.records_rows(ctx, None, 0, device_ptr=p, shape=(M, V)))
        two = timed(lambda: (pkg.score_rows(ctx, None, device_ptr=p, shape=(M, V)), pkg.alternatives_rows(ctx, None, records, device_ptr=p, shape=(M, V))))
        sc_only = timed(lambda: pkg.score_rows(ctx, None, device_ptr=p, shape=(M, V)))
        print(f"records kernel alone, {M} rows x {V} ({M * V * 4 / 1e6:.0f} MB of logits), median of 5 host-timed calls that end in a synchronise: fused k={records} {fused:.3f} ms "
              f"({fused / M * 1e3:.2f} us per row), fused scores alone {fused0:.3f} ms, score_rows + alternatives_rows {two:.3f} ms, score_rows alone {sc_only:.3f} ms; "
              f"two launches / fused = {two / fused:.2f}", flush=True)
        ctx.free(p)
m.close(); ctx.close()
