"""Plain functions the live-session GPU tests share (tests/test_gpu_stream*.py): the synthetic full-size model, a session's t_embed and gain, the cuts of a clip, the
ids rule of the group files, and vox_stream_group_advance with hand-made entries.  Fixtures, and helpers that differ from file to file, stay in the files."""
import os

import numpy as np

from model_fixtures import cache_dir, check_greedy_ids


def _full_path(peaked):
    name, seed = ("full_q4_peaked_seed44.gguf", 44) if peaked else ("full_q4_seed42.gguf", 42)
    path = os.path.join(cache_dir(), name)
    if not os.path.exists(path):
        from __graft_entry__ import load_package
        S = load_package().synth
        S.write_synthetic_gguf(path + ".tmp", S.ModelDims(), seed=seed, **({"peaked": True} if peaked else {})); os.replace(path + ".tmp", path)
    return path


def _t(pkg, m, delay=6.0):
    return pkg.TimeEmbedding(m.config.dec_dim).embed(delay)


def _gain(x):
    """peak_normalize(0.95)'s scale (audio/io.rs:59-68): 0.95 / max|x| in f32, 1 for silence; 16-bit samples count as x / 32768."""
    x = x.astype(np.float32) / np.float32(32768) if x.dtype == np.int16 else x
    mx = np.float32(np.abs(x).max()) if x.size else np.float32(0)
    return float(np.float32(0.95) / mx) if mx >= 1e-10 else 1.0


def _pieces(n, size, start=0):
    return [(a, min(n, a + size)) for a in range(start, n, size)]


def _stop(lg, tol):
    """The reference's first near-tie: the first row whose top-2 margin is within 10 tol of the logits' scale."""
    srt = np.sort(lg, axis=1); safe = (srt[:, -1] - srt[:, -2]) > 10 * tol * max(1.0, float(np.abs(lg).max()))
    return len(safe) if safe.all() else int(np.argmin(safe))


def _held(ids, rids, rlg, label, tol):
    """The ids rule of the group files: equal outright before the reference's first near-tie, which lies at or beyond half of the ids; check_greedy_ids behind it."""
    stop = _stop(rlg, tol)
    assert len(ids) == len(rids) and len(ids) >= 8, (label, len(ids), len(rids))
    assert 2 * stop >= len(rids), f"{label}: the reference's first near-tie ({stop}) lies in the first half of {len(rids)} ids: the clip cannot carry the claim"
    assert (ids[:stop] == rids[:stop]).all(), f"{label}: ids differ from the solo stream's at {np.flatnonzero(ids[:stop] != rids[:stop])[:8]} (first near-tie at {stop})"
    check_greedy_ids(ids, rids, rlg, tol)
    return int((ids == rids).sum())


def _raw_advance(pkg, g, entries, s16=False, mem_kind=0):
    """vox_stream_group_advance / _s16 with hand-made entries [(member, finish, samples or None, n, cap)] -> (code, message, ids per entry)."""
    L = pkg.lib(); arr = (pkg._lib.StreamFeed * len(entries))(); bufs = []
    for e, (member, finish, x, n, cap) in zip(arr, entries):
        ids = np.zeros(max(cap, 1), np.int32); bufs.append(ids)
        e.member = member; e.finish = finish; e.samples = None if x is None or not x.size else x.ctypes.data; e.n_samples = n; e.out_ids = ids.ctypes.data; e.cap = cap
    code = (L.vox_stream_group_advance_s16 if s16 else L.vox_stream_group_advance)(g.h, arr, len(entries), mem_kind)
    return code, (L.vox_last_error() or b"").decode(), [b[:e.n_ids].copy() for b, e in zip(bufs, arr)]
