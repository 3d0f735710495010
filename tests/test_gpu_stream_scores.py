"""Scores of the live sessions' ids (vox_token_score; DESIGN.md section 8, "Scores"): the row-scoring kernel through vox_score_rows, then the records a solo stream and
a stream group hand out, against numpy in float64 on the same f32 logits rows (the sessions' rows come from their logits taps).

The reference and what is asked of the kernel:
  id, runner_up   exact (the project's argmax rule: the largest wins, the lowest index wins a tie, a NaN or -inf never wins; runner_up over the columns != id, -1
                  when none can win);
  margin          bit for bit np.float32(L[id]) - np.float32(L[runner_up]) (L[id] - (-inf) without a runner-up);
  logprob         within tol = 2^-23 (|ref| + V / 256 + 32): one rounding of L[id] - m and one of the final subtraction, expf / logf at a few ulp, summation chains of
                  at most about V / 256 adds in front of the tree.  A worst-case bound, so the inputs are chosen such that a dropped or doubled column moves logprob
                  by far more; NaN where the row holds a NaN or its maximum is not finite, -inf where L[id] is."""
import base64
import ctypes as C
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _full_path, _gain, _pieces, _t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------------
def _argmax_rule(row, skip=-1):
    """The project's rule on a host row, column `skip` left out: -1 when nothing can win."""
    ok = ~np.isnan(row) & (row > -np.inf)
    if 0 <= skip < row.size:
        ok[skip] = False
    if not ok.any():
        return -1
    return int(np.flatnonzero(ok & (row == row[ok].max()))[0])


def _ref(row, t=None):
    """(logprob in float64, margin as f32, runner_up, id) of one f32 row; t None: the row's argmax (0 when nothing wins, as vox_argmax_rows)."""
    row = np.asarray(row, dtype=F32)
    if t is None:
        t = max(_argmax_rule(row), 0)
    r = _argmax_rule(row, t)
    with np.errstate(invalid="ignore", over="ignore"):
        margin = F32(row[t]) - (F32(row[r]) if r >= 0 else F32(-np.inf))
        L = row.astype(np.float64); m = L.max() if not np.isnan(L).any() else np.nan
        lp = L[t] - (m + np.log(np.exp(L - m).sum())) if np.isfinite(m) else np.nan
    return lp, margin, r, int(t)


def _tol(ref, V):
    return 2.0 ** -23 * (abs(ref) + V / 256.0 + 32.0)


def _check(rec, rows, ids, label, worst=None):
    """Every record of `rec` against the reference on its row.  ids None: computed."""
    V = rows.shape[1]
    assert len(rec) == len(rows), (label, len(rec), len(rows))
    for k, row in enumerate(rows):
        lp, margin, r, t = _ref(row, None if ids is None else int(ids[k]))
        got = rec[k]; where = f"{label}, row {k} (V {V}, id {t})"
        assert int(got["id"]) == t and int(got["runner_up"]) == r, (where, got, r)
        if np.isnan(margin):
            assert np.isnan(got["margin"]), (where, got)
        else:
            assert got["margin"] == margin and np.signbit(got["margin"]) == np.signbit(margin), (where, got, margin)
        if np.isnan(lp):
            assert np.isnan(got["logprob"]), (where, got)
        elif np.isinf(lp):
            assert got["logprob"] == lp, (where, got, lp)
        else:
            err = abs(float(got["logprob"]) - lp)
            if worst is not None:
                worst[0] = max(worst[0], err / _tol(lp, V))
            assert err <= _tol(lp, V), (where, float(got["logprob"]), lp, err, _tol(lp, V))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    yield m
    m.close()


def _score(pkg, ctx, x, ids, device):
    """vox_score_rows on host rows, or on their copy in device memory."""
    if not device:
        return pkg.score_rows(ctx, x, ids)
    p = ctx.upload(x)
    try:
        return pkg.score_rows(ctx, None, ids, device_ptr=p, shape=x.shape)
    finally:
        ctx.free(p)


# ---- 1. the kernel's edges through vox_score_rows ----------------------------------------------------------------------------------------------------------------------
def _handmade(V, rng):
    """The hand-made rows that exist at this V."""
    rnd = lambda: (3.0 * rng.standard_normal(V)).astype(F32)
    rows = [("all equal", np.full(V, 1.25, F32))]
    if V >= 2:
        a = rnd(); a[[V // 3, V - 1]] = a.max() + F32(1); rows.append(("the maximum at two indices", a))
        a = rnd(); a[1::3] = -np.inf; rows.append(("-inf columns", a))
    a = rnd(); a[V - 1] = a.max() + F32(2); rows.append(("the maximum at V - 1", a))
    a = (1e4 * np.where(rng.random(V) < 0.5, -1.0, 1.0) + rng.standard_normal(V)).astype(F32); a[V // 2] = abs(a[V // 2]); rows.append(("around +-1e4", a))
    a = rnd(); a[V // 2] = np.nan; rows.append(("a NaN column", a))
    rows.append(("all -inf", np.full(V, -np.inf, F32)))
    return rows


@pytest.mark.parametrize("V", [1, 2, 3, 5, 63, 64, 65, 511, 512, 1023, 1024, 1025, 4099])
def test_score_rows_edges(pkg, ctx, V):
    """M in {1, 3, 17} at every V (rows 1 and up of a matrix with V % 4 != 0 are misaligned), host and device logits, ids computed and given -- given ids include ids that
    are not the argmax, a NaN column and a -inf column.  The 17-row matrix carries every hand-made row behind a random one; each hand-made row also goes alone."""
    rng = np.random.default_rng([2026, V]); worst = [0.0]
    hand = _handmade(V, rng)
    rnd = lambda n: (3.0 * rng.standard_normal((n, V))).astype(F32)
    mats = [("M 1", rnd(1)), ("M 3", np.vstack([rnd(1), hand[V % len(hand)][1][None], rnd(1)])),
            ("M 17", np.vstack([rnd(1)] + [r[None] for _, r in hand] + [rnd(16 - len(hand))]))] + [(f"alone: {n}", r[None].copy()) for n, r in hand]
    assert [m.shape[0] for _, m in mats[:3]] == [1, 3, 17]
    for name, x in mats:
        x = np.ascontiguousarray(x)
        top = np.array([max(_argmax_rule(r), 0) for r in x], dtype=np.int32)
        other = np.array([(t + 1 + k) % V for k, t in enumerate(top)], dtype=np.int32)      # not the argmax (V > 1); lands on NaN and -inf columns too
        special = np.array([V // 2 if k % 2 else min(1, V - 1) for k in range(len(x))], dtype=np.int32)      # the NaN column / a -inf column of the hand-made rows
        for device in (False, True):
            for ids in (None, top, other, special):
                rec = _score(pkg, ctx, x, ids, device)
                _check(rec, x, ids, f"{name}, {'device' if device else 'host'} logits, ids {'computed' if ids is None else 'given'}", worst)
        assert _same_bits(_score(pkg, ctx, x, None, True), _score(pkg, ctx, x, top, False))      # computed = given the argmax, host = device: one function of the row
    print(f"V {V}: largest |logprob - ref| / tol = {worst[0]:.3f}")


def test_score_rows_facts_of_the_handmade_rows(pkg, ctx):
    """What the issue states about single rows, spelled out (the reference above agrees by construction: this pins the reference too)."""
    V = 1025
    rec = pkg.score_rows(ctx, np.full((1, V), 1.25, F32))[0]
    assert rec["id"] == 0 and rec["runner_up"] == 1 and rec["margin"] == 0 and abs(float(rec["logprob"]) + np.log(V)) <= _tol(np.log(V), V)
    one = pkg.score_rows(ctx, np.full((1, 1), -3.5, F32))[0]
    assert one["id"] == 0 and one["runner_up"] == -1 and one["margin"] == np.inf and one["logprob"] == 0
    x = np.zeros((1, 8), F32); x[0, 5] = 2
    rec = pkg.score_rows(ctx, x, [2])[0]
    assert rec["id"] == 2 and rec["runner_up"] == 5 and rec["margin"] == -2
    rec = pkg.score_rows(ctx, np.full((1, 8), -np.inf, F32))[0]
    assert rec["id"] == 0 and rec["runner_up"] == -1 and np.isnan(rec["logprob"]) and np.isnan(rec["margin"])
    x = np.zeros((1, 8), F32); x[0, 3] = np.inf
    rec = pkg.score_rows(ctx, x)[0]
    assert rec["id"] == 3 and rec["runner_up"] == 0 and np.isnan(rec["logprob"]) and rec["margin"] == np.inf


# ---- 2. the full vocabulary: boundary spikes ----------------------------------------------------------------------------------------------------------------------------
def test_full_vocabulary_boundary_spikes(pkg, ctx):
    """V = 131072: twelve columns at 0 over a background of N(0, 1) - 30, at the ends of the row, of the float4 groups, of a thread's stride and of the halves -- each
    carries a twelfth of the mass, so a lost or doubled one moves logprob by log(12 / 11) = 0.087 (tol: 7e-5).  The second row is the same row one float further on:
    misaligned, scanned in the same order, so its record has the same bits."""
    V = 131072; spikes = [0, 3, 4, 1023, 1024, 1025, 4095, 4096, 65535, 65536, 131068, 131071]
    rng = np.random.default_rng(131072)
    row = (rng.standard_normal(V) - 30.0).astype(F32); row[spikes] = 0
    assert abs(_ref(row)[0] + np.log(12.0)) < 1e-6 and _tol(np.log(12.0), V) < 1e-4
    two = np.stack([row, row])
    for ids in (None, [131071, 4096], [7, 65537]):
        rec = pkg.score_rows(ctx, two, ids)
        _check(rec, two, ids, f"aligned rows, ids {ids}")
        buf = np.zeros(2 * V + 5, F32); buf[1:V + 1] = row; buf[V + 1:2 * V + 1] = row      # [2][V] from one float past a 16-byte boundary
        p = ctx.upload(buf); assert p % 16 == 0
        try:
            mis = pkg.score_rows(ctx, None, ids, device_ptr=p + 4, shape=(2, V))
        finally:
            ctx.free(p)
        _check(mis, two, ids, f"misaligned rows, ids {ids}")
        if ids is None:
            assert _same_bits(mis[:1], mis[1:])
        assert _same_bits(mis, rec), (mis, rec)      # the scan order does not depend on the alignment
    rec = pkg.score_rows(ctx, two)
    assert list(rec["id"]) == [0, 0] and list(rec["runner_up"]) == [3, 3] and list(rec["margin"]) == [0, 0]


# ---- the sessions ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _loud(seconds, seed, sr=16000):
    rng = np.random.default_rng(seed); n = int(seconds * sr)
    return (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * (0.07 * 16000 / sr))).astype(F32)


def _run(st, x, size):
    out = [st.push(x[a:b]) for a, b in _pieces(len(x), size)] + [st.finish()]
    return np.concatenate(out).astype(np.int32)


def test_solo_tiny_records_equal_the_reference_and_do_not_depend_on_the_cuts(pkg, ctx, tiny):
    """3 s through a tiny solo stream with the tap armed: every record is the reference's on the tapped row of its id.  Then the same clip cut as 1600 / 2560 / 7777
    samples / all at once with no tap (the rows go through the stream's own logits row): bit-identical score arrays."""
    m = tiny; t = _t(pkg, m); x = _loud(3.0, 11); g = _gain(x)
    st = m.create_stream(t, gain=g)
    try:
        st.set_scores(True); st.tap_arm(64)
        ids = _run(st, x, 1600); sc = st.scores(); lg = st.tap_fetch()
    finally:
        st.close()
    assert len(ids) == pkg.stream_schedule(len(x), finished=True)[1] == len(sc) == len(lg) and len(ids) >= 20
    assert np.array_equal(sc["id"], ids)
    _check(sc, lg, ids, "tiny solo stream")
    assert np.isfinite(sc["logprob"]).all() and (sc["margin"] >= 0).all()      # greedy ids on finite rows
    for size in (1600, 2560, 7777, len(x)):
        st = m.create_stream(t, gain=g)
        try:
            st.set_scores(True)
            ids2 = _run(st, x, size); sc2 = st.scores()
            assert _same_bits(st.scores(3, 5), sc2[3:8]) and len(st.scores(len(ids2), 0)) == 0
        finally:
            st.close()
        assert np.array_equal(ids2, ids) and _same_bits(sc2, sc), f"pieces of {size} samples"


def test_solo_tiny_toggling_reset_refusals_and_bytes(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); x = _loud(3.0, 12); g = _gain(x); L = pkg.lib(); V = m.config.vocab
    plain = m.create_stream(t, gain=g); full = m.create_stream(t, gain=g); st = m.create_stream(t, gain=g, max_positions=256)
    try:
        ids = _run(plain, x, 1600)
        assert len(plain.scores()) == len(ids) and np.isnan(plain.scores()["logprob"]).all()      # never scored: the records say so, nothing was allocated
        full.set_scores(True); assert np.array_equal(_run(full, x, 1600), ids); ref = full.scores()
        # off -> on -> off across pushes
        b0 = st.info()["bytes"]
        a, b = 16000, 32000
        got = [st.push(x[:a])]; n_off = len(got[0])
        st.set_scores(True); b1 = st.info()["bytes"]
        got.append(st.push(x[a:b])); n_on = n_off + len(got[1])
        st.set_scores(False)
        got += [st.push(x[b:]), st.finish()]
        got = np.concatenate(got); sc = st.scores()
        assert np.array_equal(got, ids) and np.array_equal(sc["id"], ids) and 0 < n_off < n_on < len(ids)
        off = np.r_[0:n_off, n_on:len(ids)]
        assert np.isnan(sc["logprob"][off]).all() and np.isnan(sc["margin"][off]).all() and (sc["runner_up"][off] == -1).all()
        assert _same_bits(sc[n_off:n_on], ref[n_off:n_on])      # the ids produced while on: the records of a stream that scored everything
        assert b1 - b0 == (256 + 2) * 16 + V * 4      # the records of every position the stream was created for + one logits row, at the first set_scores(True) ...
        st.set_scores(True); st.set_scores(False); st.set_scores(True)
        assert st.info()["bytes"] == b1               # ... only
        # out-of-range requests: refused, nothing written
        n = len(ids); buf = np.full(n + 4, -7, dtype=pkg.SCORE_DTYPE); before = buf.tobytes()
        for first, cnt in ((0, n + 1), (n, 1), (-1, 2), (2, -1), (n + 1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert L.vox_stream_scores(st.h, first, cnt, buf.ctypes.data) == 1 and "handed out" in L.vox_last_error().decode(), (first, cnt)
        assert buf.tobytes() == before
        # reset: the records start over, the flag stays
        st.reset()
        assert len(st.scores()) == 0 and L.vox_stream_scores(st.h, 0, 1, buf.ctypes.data) == 1 and st.info()["bytes"] == b1
        again = _run(st, x, 2560)
        assert np.array_equal(again, ids) and _same_bits(st.scores(), ref)
    finally:
        plain.close(); full.close(); st.close()


def test_solo_full_size_engine_path(pkg, ctx):
    """The full-size peaked model, 3 s: every decode step is an engine launch, its logits row written on request; the ids are the unscored stream's, the records the
    reference's on the tapped rows at V = 131072."""
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    try:
        t = _t(pkg, m); x = _loud(3.0, 13); g = _gain(x)
        a = m.create_stream(t, gain=g); b = m.create_stream(t, gain=g)
        try:
            a.set_scores(True); a.tap_arm(64)
            ids = _run(a, x, 2560); sc = a.scores(); lg = a.tap_fetch(); info = a.info()
            plain = _run(b, x, 2560)
        finally:
            a.close(); b.close()
        assert info["engine_steps"] > 0 and info["engine_steps"] + info["operator_steps"] == len(ids)
        assert lg.shape == (len(ids), 131072) and np.array_equal(plain, ids) and np.array_equal(sc["id"], ids)
        _check(sc, lg, ids, "full-size solo stream")
    finally:
        m.close()


def test_group_tiny_rounds_of_three_widths(pkg, ctx, tiny):
    """Three members fed 1.3 s, 2.1 s and 3 s in ONE call that finishes them all: rounds of width 3, 2 and 1, the member with the most ticks in slot 0.  Scores on for
    members 0 and 2: their records are the reference's on their own tapped rows; member 1 gets the records of an unscored id."""
    m = tiny; t = _t(pkg, m)
    clips = [_loud(1.3, 21), _loud(2.1, 22), _loud(3.0, 23)]
    g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips])
    try:
        b0 = [g.info(k)["bytes"] for k in range(3)]
        g.set_scores(0, True); g.set_scores(2, True)
        b1 = [g.info(k)["bytes"] for k in range(3)]
        assert b1[1] == b0[1] and b1[0] - b0[0] == b1[2] - b0[2] == (g.info(0)["bytes"] - b0[0]) > 0
        for k in range(3):
            g.tap_arm(k, 64)
        out = g.advance({k: x for k, x in enumerate(clips)}, finish=[0, 1, 2])
        n = [len(out[k]) for k in range(3)]
        assert n == [pkg.stream_schedule(len(x), finished=True)[1] for x in clips] and n[0] < n[1] < n[2]
        for k in (0, 2):
            sc = g.scores(k); lg = g.tap_fetch(k)
            assert np.array_equal(sc["id"], out[k]) and len(lg) == n[k]
            _check(sc, lg, out[k], f"group member {k}")
        sc = g.scores(1)
        assert np.array_equal(sc["id"], out[1]) and np.isnan(sc["logprob"]).all() and np.isnan(sc["margin"]).all() and (sc["runner_up"] == -1).all()
        L = pkg.lib(); buf = np.full(4, -7, dtype=pkg.SCORE_DTYPE); before = buf.tobytes()
        assert L.vox_stream_group_scores(g.h, 0, n[0] - 1, 2, buf.ctypes.data) == 1 and L.vox_stream_group_scores(g.h, 3, 0, 1, buf.ctypes.data) == 1 and buf.tobytes() == before
        g.reset(0, _gain(clips[0]))      # the member's next connection: its records start over, its flag stays
        assert len(g.scores(0)) == 0
        again = g.advance({0: clips[0]}, finish=[0])[0]
        assert np.array_equal(again, out[0]) and not np.isnan(g.scores(0)["logprob"]).any()
    finally:
        g.close()


def test_group_member_at_48k_s16_equals_the_member_fed_the_resampled_samples(pkg, ctx, tiny):
    """A scored member fed 48 kHz 16-bit PCM against the same member of a 16 kHz group fed vox_resample's samples in the same calls (the single-pass invariant of the
    capture-rate groups): the same ids, the same records, bit for bit."""
    m = tiny; t = _t(pkg, m); rates = [48000, 16000]
    rng = np.random.default_rng(31)
    pcm = [np.clip(np.round(9000.0 * rng.standard_normal(int(sr * 2.2) + 7) + 7000.0 * np.sin(np.arange(int(sr * 2.2) + 7) * (0.07 * 16000 / sr))), -32768, 32767).astype(np.int16)
           for sr in rates]
    f32 = [v.astype(F32) / F32(32768) for v in pcm]
    x16 = [pkg.resample(ctx, f32[0], 48000), f32[1]]; gains = [_gain(v) for v in x16]
    calls = []      # per call: member -> (lo, hi, finish) in input samples, sr / 5 + 1 per call
    for c in range(64):
        call = {k: (c * (sr // 5 + 1), min(len(pcm[k]), (c + 1) * (sr // 5 + 1))) for k, sr in enumerate(rates) if c * (sr // 5 + 1) < len(pcm[k])}
        if not call:
            break
        calls.append({k: (lo, hi, hi == len(pcm[k])) for k, (lo, hi) in call.items()})
    res = []
    for native in (True, False):
        g = m.create_stream_group(t, 2, gains=gains, sample_rates=rates if native else None)
        try:
            g.set_scores(0, True); ids = []
            for call in calls:
                if native:
                    feeds = {k: pcm[k][lo:hi] for k, (lo, hi, _) in call.items()}
                else:
                    feeds = {k: x16[k][pkg.stream_schedule_rate(lo, rates[k])[2]:pkg.stream_schedule_rate(hi, rates[k], finished=fin)[2]] for k, (lo, hi, fin) in call.items()}
                out = g.advance(feeds, finish=[k for k, v in call.items() if v[2]])
                ids.extend(out.get(0, []))
            res.append((np.array(ids, np.int32), g.scores(0)))
        finally:
            g.close()
    (ia, sa), (ib, sb) = res
    assert len(ia) >= 15 and np.array_equal(ia, ib) and np.array_equal(sa["id"], ia) and not np.isnan(sa["logprob"]).any()
    assert _same_bits(sa, sb)


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def _tekken(n=1200):      # as tests/test_tokenizer_cli.py: every text id decodes to " w<index>"
    vocab = [{"rank": i, "token_bytes": base64.b64encode(f" w{i}".encode()).decode(), "token_str": f" w{i}"} for i in range(n)]
    return {"config": {"pattern": "", "num_vocab_tokens": n, "default_vocab_size": 131072, "default_num_special_tokens": 1000, "version": "v7"}, "vocab": vocab}


def _write_wav(path, x, sr=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _cli_files(pkg, tmp_path):
    S = pkg.synth
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wavs = []
    for k, sec in enumerate((3.0, 2.0)):
        wavs.append(str(tmp_path / f"a{k}.wav")); _write_wav(wavs[-1], S.synth_audio(sec, seed=2 + k))
    return [sys.executable, os.path.join(ROOT, "voxtral-mini-realtime-rs_amd", "cli.py"), "--gguf", gguf, "--tokenizer", tok], wavs


def _word_lines(path):
    return [json.loads(l) for l in open(path, encoding="utf-8").read().splitlines()]


def _check_words(words, line):
    assert "".join(w["text"] for w in words).strip() == line
    assert all(np.isfinite(w["logprob"]) and w["logprob"] <= 0 and w["min_margin"] >= 0 and w["first_id"] <= w["last_id"] for w in words)
    due = [w["due_s"] for w in words]
    assert due == sorted(due) and len(set(due)) == len(due) and all(d == (2560 * w["last_id"] + 40) / 16000.0 for d, w in zip(due, words))


def test_cli_live_words(pkg, tmp_path):
    """--live --live-words: the words' texts joined are the stdout line, which is the line without the flag; finite logprob, due_s ascending."""
    cmd, wavs = _cli_files(pkg, tmp_path); out = str(tmp_path / "words.jsonl")
    r = subprocess.run(cmd + ["--audio", wavs[0], "--live", "--live-words", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n"); assert len(lines) == 2 and lines[1] == "" and lines[0]
    words = _word_lines(out)
    assert len(words) >= 3 and all(w["file"] == wavs[0] for w in words)
    _check_words(words, lines[0])
    r2 = subprocess.run(cmd + ["--audio", wavs[0], "--live"], capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and r2.stdout == r.stdout      # stdout keeps its one final line, unchanged
    r3 = subprocess.run(cmd + ["--audio", wavs[0], "--live-words", out], capture_output=True, text=True, timeout=300)
    assert r3.returncode == 2 and "--live-words applies with --live" in r3.stderr and r3.stdout == ""


def test_cli_live_group_words(pkg, tmp_path):
    """--live-group 2 --live-words: one line per word with its file; each file's words join to that file's stdout line."""
    cmd, wavs = _cli_files(pkg, tmp_path); out = str(tmp_path / "words.jsonl")
    r = subprocess.run(cmd + ["--audio", wavs[0], "--audio", wavs[1], "--live", "--live-group", "2", "--live-words", out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Error" not in r.stderr, r.stderr
    lines = r.stdout.split("\n"); assert len(lines) == 3 and lines[2] == ""
    words = _word_lines(out)
    assert {w["file"] for w in words} == set(wavs)
    for path, line in zip(wavs, lines):
        _check_words([w for w in words if w["file"] == path], line)
