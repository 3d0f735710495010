"""Records of the offline and batch paths (vox_records_rows, vox_transcribe_audio_scored, vox_transcribe_batch_scored; DESIGN.md 3.3, "Records of the batch paths").

The contract, asserted bit for bit throughout: for every id a scored call returns, its score record is vox_score_rows(row, id) and its alternatives record is
vox_alternatives_rows(row, k), `row` being the f32 logits row the id was taken from (the debug taps hand the rows out), and the record's id is the returned id.  The row
kernels themselves are held to numpy in float64 by tests/test_gpu_stream_scores.py and tests/test_gpu_stream_alternatives.py; here they are the reference, so equality
is exact and carries no tolerance.  The one tolerance (the full-size test) is the header's stated bound on logprob, 2^-23 (|logprob| + V / 256 + 32)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from model_fixtures import attn_launches, cache_dir, gemm_launches, parse_batch_verbose, tiny_gguf
from test_gpu_model import _TINY_FORMS, _WIDE_FORMS
from test_gpu_stream_scores import _cli_files, _same_bits, _word_lines

pytestmark = pytest.mark.gpu
F32 = np.float32


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


def _cut(rec8, k):
    """the list for k from the list for 8: its first k entries, n capped, the entropy as it is"""
    out = rec8.copy()
    out["n"] = np.minimum(out["n"], k); out["alt"]["id"][:, k:] = -1; out["alt"]["logprob"][:, k:] = np.nan
    return out


def _rows_check(pkg, ctx, rows, ids, sc, al, k, label):
    """records of a call against the row kernels on the rows its ids were taken from"""
    assert len(rows) == len(ids) == len(sc) and (al is None or len(al) == len(ids)), (label, len(rows), len(ids), len(sc))
    if len(ids) == 0:
        return
    assert np.array_equal(sc["id"], ids), (label, sc["id"], ids)
    assert _same_bits(sc, pkg.score_rows(ctx, rows, ids=ids)), (label, sc, pkg.score_rows(ctx, rows, ids=ids))
    if al is not None:
        assert np.array_equal(al["alt"]["id"][:, 0], ids), label
        assert _same_bits(al, pkg.alternatives_rows(ctx, rows, k)), (label, k)


# ---- a. the kernel alone ----------------------------------------------------------------------------------------------------------------------------------------------
def _handmade(V, rng):
    rnd = lambda: (3.0 * rng.standard_normal(V)).astype(F32)
    rows = [rnd(), np.full(V, -np.inf, F32)]                                     # random; all -inf (nothing wins: id 0)
    a = rnd(); a[V // 2] = np.nan; rows.append(a)                                 # a NaN
    a = rnd(); a[V - 1] = np.inf; rows.append(a)                                  # a +inf
    a = rnd(); a[[V // 3, V - 1]] = a.max() + F32(1); rows.append(a)              # an exact tie at the top (one column when V < 3)
    if V >= 12:                                                                   # exact ties at rank 8 / 9: seven distinct leaders, then three equal columns
        a = rnd(); top = a.max(); order = rng.permutation(V)[:10]
        a[order[:7]] = top + F32(10) - np.arange(7, dtype=F32); a[order[7:]] = top + F32(1); rows.append(a)
    a = np.full(V, -np.inf, F32); a[rng.permutation(V)[:min(V, 5)]] = rnd()[:min(V, 5)]; rows.append(a)      # fewer than k winnable columns
    a = np.full(V, np.nan, F32); a[0] = -np.inf; rows.append(a)                   # NaN and -inf only
    rows.append(np.full(V, 1.25, F32))                                            # all equal
    return rows


@pytest.mark.parametrize("V", [1, 3, 4, 5, 512, 1027])
def test_records_rows_equal_the_row_kernels(pkg, ctx, V):
    """vox_records_rows on hand-built rows, as one 17-row matrix (rows 1 and up are off a 16-byte boundary when V % 4 != 0) and each row alone (M = 1); on a device
    matrix that starts one float past a 16-byte boundary too.  For k = 0 and every k in 1..8: scores == score_rows(row, argmax), alts == alternatives_rows(row, k), bit
    for bit; the list for k is the list for 8 cut short; a row's record is the same alone, in the matrix, shuffled among other neighbours, host or device."""
    rng = np.random.default_rng([2031, V])
    hand = _handmade(V, rng)
    x = np.ascontiguousarray(np.vstack([r[None] for r in hand] + [(3.0 * rng.standard_normal((17 - len(hand), V))).astype(F32)]))
    assert x.shape == (17, V)
    ref_sc = pkg.score_rows(ctx, x); ref8 = pkg.alternatives_rows(ctx, x, 8)
    assert int(ref_sc["id"][1]) == 0 and int(ref8["n"][1]) == 0                   # (the all -inf row: nothing wins)
    sc0, al0 = pkg.records_rows(ctx, x, 0)
    assert al0 is None and _same_bits(sc0, ref_sc), (sc0, ref_sc)
    perm = rng.permutation(17)
    for k in range(1, 9):
        sc, al = pkg.records_rows(ctx, x, k)
        assert _same_bits(sc, ref_sc), (k, sc, ref_sc)
        assert _same_bits(al, pkg.alternatives_rows(ctx, x, k)) and _same_bits(al, _cut(ref8, k)), (k, al)
        scp, alp = pkg.records_rows(ctx, np.ascontiguousarray(x[perm]), k)        # other neighbours, other alignment
        assert _same_bits(scp, sc[perm]) and _same_bits(alp, al[perm]), k
    for r in range(17):                                                           # M = 1 against M = 17
        for k in (0, 1, 2, 8):
            sc1, al1 = pkg.records_rows(ctx, x[r], k)
            assert _same_bits(sc1, ref_sc[r:r + 1]), (r, k, sc1, ref_sc[r])
            assert al1 is None or _same_bits(al1, _cut(ref8[r:r + 1], k)), (r, k)
    # a device matrix one float past a 16-byte boundary, and the alts-only form of the C call
    flat = np.zeros(17 * V + 1, F32); flat[1:] = x.reshape(-1)
    p = ctx.upload(flat)
    try:
        for k in (0, 3, 8):
            scd, ald = pkg.records_rows(ctx, None, k, device_ptr=p + 4, shape=(17, V))
            assert _same_bits(scd, ref_sc) and (ald is None or _same_bits(ald, _cut(ref8, k))), k
        only = np.zeros(17, dtype=pkg.ALTS_DTYPE)
        pkg._lib.check(pkg.lib().vox_records_rows(ctx.h, C.c_void_p(p + 4), 17, V, 8, None, only.ctypes.data, 1))
        assert _same_bits(only, ref8)
    finally:
        ctx.free(p)


# ---- b. every step form -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def form_clips(pkg):
    secs = [0.4 + 0.23 * ((7 * i) % 19) for i in range(90)]
    secs[5] = 0.05; secs[41] = 0.12                                               # the shortest units: a few ids from the pad alone
    return [pkg.synth.synth_audio(s, seed=1900 + i) for i, s in enumerate(secs)]


@pytest.mark.parametrize("form", list(_TINY_FORMS))
def test_batch_records_every_step_form(pkg, ctx, tiny, form, form_clips, capfd, monkeypatch):
    """The form table and the 90 ragged clips of test_batch_logits_every_step_form_vs_teacher_forced.  One call with tap and records together (every unit tapped,
    k = 8): the ids are the unscored call's, every record of every unit is the row kernels' on the tapped row -- row 0 (the prefill row), slot 0, the last slot and a
    unit that started in a vacated slot among them; VOX_BATCH_VERBOSE proves the form ran.  A scores-only call gives the same score records."""
    m = tiny; t = pkg.TimeEmbedding(256).embed(6.0)
    n, env, ran = _TINY_FORMS[form]
    clips = form_clips[:n]
    monkeypatch.setenv("VOX_BATCH_NO_CALIB", "1"); monkeypatch.setenv("VOX_BATCH_VERBOSE", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    plain = m.transcribe_batch(clips, t)
    capfd.readouterr()
    outs, scs, als, taps = m.transcribe_batch_scored(clips, t, alternatives=8, tap_units=list(range(n)))
    v = parse_batch_verbose(capfd.readouterr().err)
    assert m.timings()["graph_replays"] > 0
    outs0, scs0, als0 = m.transcribe_batch_scored(clips, t, alternatives=0)
    for k in env:
        monkeypatch.delenv(k)
    if form in _WIDE_FORMS and v["slots"] and v["forms"]["wide"] + v["forms"]["split"] == 0:
        pytest.skip(f"{form}: the wide step does not cover the tiny geometry")
    assert ran(v), f"{form}: the form did not run: {v}"
    assert als0 is None and len(outs) == len(plain) == len(outs0) == n
    lens = [len(x) for x in outs]
    assert min(lens) < 12 and max(lens) > 30      # (the 0.05 s and 0.12 s clips are the shortest units: the left pad alone gives them a few ids)
    for u in range(n):
        assert np.array_equal(outs[u], plain[u]) and np.array_equal(outs0[u], plain[u]), (form, u)
        _rows_check(pkg, ctx, taps[u], outs[u], scs[u], als[u], 8, f"{form}, unit {u}")
        assert _same_bits(scs0[u], scs[u]), (form, u)
    if v["plan"]:      # what the covered units include
        slot0, last = v["plan"][0][0], next(q[0] for q in reversed(v["plan"]) if q)
        refills = [q[1] for q in v["plan"] if len(q) > 1]
        assert lens[slot0] > 1 and lens[last] > 1 and (n <= len(v["plan"]) or (refills and lens[refills[-1]] > 1))


def test_batch_records_past_n_ids_are_untouched(pkg, ctx, tiny, form_clips):
    """vox_transcribe_batch_scored through ctypes, record arrays pre-filled: the entries from n_ids[i] on keep their bytes."""
    m = tiny; t = np.ascontiguousarray(pkg.TimeEmbedding(256).embed(6.0), dtype=F32).reshape(-1); L = pkg.lib()
    clips = [np.ascontiguousarray(c, dtype=F32) for c in form_clips[:8]]; n = len(clips)
    caps = [c.size // 1280 + 128 for c in clips]
    ids = [np.zeros(cp, np.int32) for cp in caps]
    sc = [np.zeros(cp, dtype=pkg.SCORE_DTYPE) for cp in caps]; al = [np.zeros(cp, dtype=pkg.ALTS_DTYPE) for cp in caps]
    for a in sc + al:
        a.view(np.uint8)[:] = 0xA5
    arr = lambda xs: (C.c_void_p * n)(*[a.ctypes.data for a in xs])
    nids = (C.c_int32 * n)()
    pkg._lib.check(L.vox_transcribe_batch_scored(m.h, n, arr(clips), (C.c_size_t * n)(*[c.size for c in clips]), None, t.ctypes.data, arr(ids), (C.c_int32 * n)(*caps), nids,
                                                 arr(sc), arr(al), 3, 0))
    ref = m.transcribe_batch(clips, pkg.TimeEmbedding(256).embed(6.0))
    assert [int(v) for v in nids] == [len(r) for r in ref] and 0 < min(nids) < min(caps)
    for u in range(n):
        k = nids[u]
        assert np.array_equal(ids[u][:k], ref[u]) and np.array_equal(sc[u]["id"][:k], ref[u]) and np.array_equal(al[u]["alt"]["id"][:k, 0], ref[u])
        assert (al[u]["n"][:k] == 3).all()
        assert (sc[u][k:].view(np.uint8) == 0xA5).all() and (al[u][k:].view(np.uint8) == 0xA5).all(), u


# ---- c. single clip -----------------------------------------------------------------------------------------------------------------------------------------------------
def _tap_of(pkg, ctx, m, x, t):
    mel = pkg.MelSpectrogram.voxtral(ctx).compute_log(pkg.pad_audio(pkg.peak_normalize(x)))
    return m.transcribe_streaming(np.ascontiguousarray(mel.T)[None], t, return_logits=True)


@pytest.mark.parametrize("sec", [0.05, 0.5, 3.0])
def test_single_clip_records(pkg, ctx, tiny, sec):
    """vox_transcribe_audio_scored: the ids are vox_transcribe_audio's, the records the row kernels' on vox_transcribe_streaming's logits tap for the same mel; k = 8,
    k = 1 and scores alone."""
    m = tiny; t = pkg.TimeEmbedding(256).embed(6.0)
    x = pkg.synth.synth_audio(sec, seed=77)
    ref = m.transcribe_audio(x, t)
    tids, lg = _tap_of(pkg, ctx, m, x, t)
    assert np.array_equal(tids, ref) and len(ref) > 0
    for k in (8, 1, 0):
        ids, sc, al = m.transcribe_audio_scored(x, t, alternatives=k)
        assert np.array_equal(ids, ref), k
        assert (al is None) == (k == 0)
        _rows_check(pkg, ctx, lg, ids, sc, al, k, f"single clip {sec} s, k {k}")
    assert np.array_equal(m.transcribe_audio(x, t), ref)      # and the unscored call is as before


# ---- d. sessions --------------------------------------------------------------------------------------------------------------------------------------------------------
def test_batch_records_two_sessions(pkg, ctx, tiny, monkeypatch):
    """256 clips of 0.6 s under vox_model_set_sessions(2): the scored call is served (no VOX_ERR_UNSUPPORTED), every session writes its own units' records.  Every
    record's id is the returned id; wherever a unit's ids agree with a one-session tapped call's, its records are the row kernels' on that call's tapped rows."""
    m = tiny; t = pkg.TimeEmbedding(256).embed(6.0)
    many = [pkg.synth.synth_audio(0.6, seed=650 + i) for i in range(256)]
    monkeypatch.setenv("VOX_BATCH_NO_CALIB", "1")
    one_ids, taps = m.transcribe_batch(many, t, tap_units=list(range(256)))
    m.set_sessions(2)
    try:
        outs, scs, als = m.transcribe_batch_scored(many, t, alternatives=8)
        assert m.timings()["decode_tokens"] == sum(len(o) for o in outs)
    finally:
        m.set_sessions(1)
    agree = 0
    for u in range(256):
        assert len(outs[u]) == len(scs[u]) == len(als[u]) > 0 and np.array_equal(scs[u]["id"], outs[u]) and np.array_equal(als[u]["alt"]["id"][:, 0], outs[u]), u
        same = len(outs[u]) == len(one_ids[u]) and np.array_equal(outs[u], one_ids[u])
        if same:
            agree += 1
            _rows_check(pkg, ctx, taps[u], outs[u], scs[u], als[u], 8, f"two sessions, unit {u}")
    assert agree >= 192, agree      # (ids may part at a near-tie between two plans; most units must be comparable for the check to mean something)


# ---- e. the off path ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_unscored_call_is_untouched_by_scored_calls(pkg, ctx, tiny, form_clips, monkeypatch):
    """A plain call before and after scored calls: the same ids, graph_replays and launch counts (the records launch is not a counted form, so a plain call's counts
    are its own work alone)."""
    m = tiny; t = pkg.TimeEmbedding(256).embed(6.0)
    monkeypatch.setenv("VOX_BATCH_NO_CALIB", "1")

    def plain(clips):
        g0, a0 = gemm_launches(pkg), attn_launches(pkg)
        ids = m.transcribe_batch(clips, t)
        g1, a1 = gemm_launches(pkg), attn_launches(pkg)
        return ids, m.timings()["graph_replays"], {k: g1[k] - g0[k] for k in g1}, {k: a1[k] - a0[k] for k in a1}

    for n in (12, 40):
        clips = form_clips[:n]
        plain(clips)                                  # (first use of a form on this context: warm-up steps)
        before = plain(clips)
        m.transcribe_batch_scored(clips, t, alternatives=8)
        m.transcribe_batch_scored(clips, t, alternatives=0)
        after = plain(clips)
        assert all(np.array_equal(a, b) for a, b in zip(before[0], after[0])) and before[1:] == after[1:], (n, before[1:], after[1:])
        assert before[1] > 0


# ---- f. the CLI ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cli_batch_words(pkg, tmp_path):
    """--batch 4 --words on the two wavs of the CLI fixtures: stdout is the run's without the flags, each file's word texts join to its line, no due_s; with
    --alternatives 3 every line has entropy and weakest.  One by one (no --batch): the same word lines."""
    cmd, wavs = _cli_files(pkg, tmp_path)
    files = ["--audio", wavs[0], "--audio", wavs[1]]
    run = lambda extra: subprocess.run(cmd + files + extra, capture_output=True, text=True, timeout=300)
    w0, w3, w1 = (str(tmp_path / f) for f in ("w0.jsonl", "w3.jsonl", "w1.jsonl"))
    base = run(["--batch", "4"])
    r0 = run(["--batch", "4", "--words", w0]); r3 = run(["--batch", "4", "--words", w3, "--alternatives", "3"]); r1 = run(["--words", w1])
    for r in (base, r0, r3, r1):
        assert r.returncode == 0 and "Error" not in r.stderr and "failed" not in r.stderr, r.stderr
    assert r0.stdout == base.stdout == r3.stdout == r1.stdout and len(base.stdout.split("\n")) == 3 and all(base.stdout.split("\n")[:2])
    words0, words3, words1 = _word_lines(w0), _word_lines(w3), _word_lines(w1)
    for path, line in zip(wavs, base.stdout.split("\n")):
        ws = [w for w in words0 if w["file"] == path]
        assert len(ws) >= 3 and "".join(w["text"] for w in ws).strip() == line
        assert all(set(w) == {"text", "first_id", "last_id", "logprob", "min_margin", "file"} for w in ws)
        assert all(np.isfinite(w["logprob"]) and w["logprob"] <= 0 and w["min_margin"] >= 0 for w in ws)
    assert all("entropy" in w and "weakest" in w and len(w["weakest"]["alternatives"]) == 3 and "due_s" not in w for w in words3) and len(words3) == len(words0)
    assert [{k: v for k, v in w.items() if k not in ("entropy", "weakest")} for w in words3] == words0
    assert [(w["file"], w["text"], w["first_id"], w["last_id"]) for w in words1] == [(w["file"], w["text"], w["first_id"], w["last_id"]) for w in words0]


# ---- full size ----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(pkg):
    import os
    S = pkg.synth
    path = os.path.join(cache_dir(), "full_q4_seed42.gguf")
    if not os.path.exists(path):
        S.write_synthetic_gguf(path + ".tmp", S.ModelDims(), seed=42); os.replace(path + ".tmp", path)
    c = pkg.Context(0)
    m = pkg.Q4ModelLoader.from_file(path).load(c)
    yield m, c
    m.close(); c.close()


def test_full_size_lockstep_records_and_single_clip_engine(pkg, full):
    """V = 131072.  Three clips of 2 - 3 s as one lock-step call with tap and records (k = 8): the records are the row kernels' on the tapped rows bit for bit, and
    logprob lies within the header's bound 2^-23 (|logprob| + V / 256 + 32) of a float64 log-softmax of the tapped row.  Then one of the clips through
    vox_transcribe_audio_scored with the decode engine on and off: the records are the row kernels' on vox_transcribe_streaming's tap in the same engine state."""
    m, ctx = full; t = pkg.TimeEmbedding(m.config.dec_dim).embed(6.0); V = m.config.vocab
    assert V == 131072
    clips = [pkg.synth.synth_audio(s, seed=310 + i) for i, s in enumerate((2.0, 3.0, 2.5))]
    outs, scs, als, taps = m.transcribe_batch_scored(clips, t, alternatives=8, tap_units=[0, 1, 2])
    worst = 0.0
    for u in range(3):
        assert len(outs[u]) > 20 and taps[u].shape == (len(outs[u]), V)
        _rows_check(pkg, ctx, taps[u], outs[u], scs[u], als[u], 8, f"full size, unit {u}")
        L = taps[u].astype(np.float64); mx = L.max(axis=1, keepdims=True)
        lsm = L - mx - np.log(np.exp(L - mx).sum(axis=1, keepdims=True))
        ref = lsm[np.arange(len(outs[u])), outs[u]]
        tol = 2.0 ** -23 * (np.abs(ref) + V / 256.0 + 32.0)
        err = np.abs(scs[u]["logprob"].astype(np.float64) - ref)
        worst = max(worst, float((err / tol).max()))
        assert (err <= tol).all(), (u, float((err / tol).max()))
        assert np.array_equal(als[u]["alt"]["logprob"][:, 0].view(np.uint32), scs[u]["logprob"].view(np.uint32))
    print(f"full-size lock-step records: largest |logprob - float64 log-softmax| / bound = {worst:.3f}")
    x = clips[0]
    was = m.set_decode_engine(True)
    try:
        for on in (True, False):
            m.set_decode_engine(on)
            tids, lg = _tap_of(pkg, ctx, m, x, t)
            ids, sc, al = m.transcribe_audio_scored(x, t, alternatives=8)
            assert np.array_equal(ids, tids), on
            _rows_check(pkg, ctx, lg, ids, sc, al, 8, f"full-size single clip, engine {on}")
    finally:
        m.set_decode_engine(was)
