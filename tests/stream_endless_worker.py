"""Worker of tests/test_gpu_stream_endless.py: an endless session and a bounded one side by side across the endless session's wrap, in a process of its own (past the
wrap the endless session launches the ring decode attention; the launch counts of vox_debug_attn_launches are per process and the suite's other tests hold slot
[13] to 0).  Usage: stream_endless_worker.py <repository root> <out.npz>.

The tiny model, device-resident synthetic audio (a 40 s clip repeated), the logits tap on both sessions.  Both are fed the same samples up to P = ring rows + 300
positions: the bounded session (max_positions 16 384) in calls of 1024 ticks, the endless one the same way up to about 100 ticks before its wrap and from there in
irregular cuts of one sample to three ticks.  Both peek once before any sample (which reserves the peek save area, so that the bytes can be compared later) and
once at the same sample count near position ring rows + 150, and go on.  Both run with scores on and alternatives at k = 3: the endless session's record
lists grow (by doubling) at its wrap."""
import ctypes as C
import os
import sys
import time

import numpy as np

root, out_path = sys.argv[1], sys.argv[2]
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
from __graft_entry__ import load_package

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _t

pkg = load_package()
L = pkg.lib()
TICK = 2560
TAIL = 63


def attn_counts():
    a = (C.c_uint64 * 16)()
    assert L.vox_debug_attn_launches(a, 16) == 0
    return np.array([int(v) for v in a], np.int64)


ctx = pkg.Context(0)
m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
t = _t(pkg, m)
window = m.config.dec_window
RING = (window + 1 + TAIL + 63) // 64 * 64      # the default dec_ring_rows
P = RING + 300
base = pkg.synth.synth_audio(40.0, seed=4242)
n = P * TICK + 1000
x = np.tile(base, n // len(base) + 1)[:n].copy()
gain = _gain(base)
n_peek = (RING + 150) * TICK + 777
res = {"ring_rows": np.int64(RING), "P": np.int64(P)}

# refusal: a ring of dec_window + 1 rows has no room for a tail
try:
    m.create_stream(t, gain=gain, endless=True, dec_ring_rows=window + 1).close()
    res["refusal"] = np.array("")
except pkg.VoxError as e:
    res["refusal"] = np.array(str(e))

dev = C.c_void_p(); pkg._lib.check(L.vox_dev_alloc(ctx.h, n * 4, C.byref(dev)))
pkg._lib.check(L.vox_dev_upload(ctx.h, dev, x.ctypes.data, n * 4))


def feed(st, cuts):
    """push x[a:b] from device memory for every cut; a peek where a cut ends at n_peek -> ids, peeked ids, info after every push"""
    ids, peeked, infos = [], None, []
    for a, b in cuts:
        ids.append(st.push(device_ptr=dev.value + 4 * a, n_samples=b - a))
        if b == n_peek:
            before = st.info(); peeked = st.peek(); after = st.info()
            assert before == after, (before, after)
        infos.append(st.info())
    return np.concatenate(ids), peeked, infos


def cuts_of(edges):
    return list(zip(edges[:-1], edges[1:]))


big = sorted(set(list(range(0, n, 1024 * TICK)) + [n_peek, n]))
rng = np.random.default_rng(99)
start = (RING - 100) * TICK
edges = [e for e in big if e < start] + [start]
while edges[-1] < n:
    step = int(rng.choice([1, 39, 40, 41, 333, TICK - 1, TICK, TICK + 1, 2 * TICK + 17, 3 * TICK]))
    nxt = min(n, edges[-1] + step)
    if edges[-1] < n_peek < nxt:
        nxt = n_peek
    edges.append(nxt)

c0 = attn_counts()
t0 = time.time()
sb = m.create_stream(t, gain=gain, max_positions=16384)
sb.tap_arm(P + 8); sb.set_scores(True); sb.set_alternatives(3); res["b_peek0"] = sb.peek()
ids_b, peek_b, infos_b = feed(sb, cuts_of(big))
rec_b = np.frombuffer(sb.scores()[-400:].tobytes(), np.uint8); alt_b = np.frombuffer(sb.alternatives()[-400:].tobytes(), np.uint8)
lg_b = sb.tap_fetch(); info_b = sb.info(); sb.close()
c1 = attn_counts()
res["seconds_bounded"] = np.float64(time.time() - t0)

t0 = time.time()
se = m.create_stream(t, gain=gain, endless=True)
se.tap_arm(P + 8); se.set_scores(True); se.set_alternatives(3); res["e_peek0"] = se.peek()
info_e0 = se.info()
ids_e, peek_e, infos_e = feed(se, cuts_of(edges))
rec_e = np.frombuffer(se.scores()[-400:].tobytes(), np.uint8); alt_e = np.frombuffer(se.alternatives()[-400:].tobytes(), np.uint8)
lg_e = se.tap_fetch(); info_e = se.info()
c2 = attn_counts()
res["seconds_endless"] = np.float64(time.time() - t0)

# after reset: a 6 s clip against a fresh bounded session
clip = pkg.synth.synth_audio(6.0, seed=77)
se.reset()
res["reset_ids"] = np.concatenate([se.push(clip[:50000]), se.push(clip[50000:]), se.finish()])
res["reset_info_positions"] = np.int64(se.info()["positions"])
se.close()
sf = m.create_stream(t, gain=gain)
res["fresh_ids"] = np.concatenate([sf.push(clip), sf.finish()])
res["fresh_info_positions"] = np.int64(sf.info()["positions"])
sf.close()
pkg._lib.check(L.vox_dev_free(ctx.h, dev))

cfg = m.config
res.update(rec_b=rec_b, rec_e=rec_e, alt_b=alt_b, alt_e=alt_e, ids_b=ids_b, ids_e=ids_e, peek_b=peek_b, peek_e=peek_e, lg_b=lg_b[-400:], lg_e=lg_e[-400:], rows_b=np.int64(len(lg_b)), rows_e=np.int64(len(lg_e)),
           pos_b=np.int64(info_b["positions"]), pos_e=np.int64(info_e["positions"]), bytes_b=np.int64(infos_b[-1]["bytes"]), bytes_e0=np.int64(info_e0["bytes"]),
           e_positions=np.array([i["positions"] for i in infos_e], np.int64), e_bytes=np.array([i["bytes"] for i in infos_e], np.int64),
           e_steps=np.array([info_e["engine_steps"], info_e["operator_steps"]], np.int64), counts_bounded=c1 - c0, counts_endless=c2 - c1,
           dims=np.array([cfg.dec_layers, cfg.dec_kv_heads, 128, cfg.vocab], np.int64))
m.close(); ctx.close()
np.savez(out_path, **res)
