"""Peek (vox_stream_peek, vox_stream_group_peek; DESIGN.md section 8, "Peek"): the ids finish would return now, and the session goes on as if nobody had asked.

Every comparison is == on ids, on tapped f32 logits rows and on score records: no tolerance anywhere.  The references are twin sessions on the same model:
 * a twin that FINISHES at the sample count of a peek -- the peek's ids, logits rows and records are that finish's;
 * a twin that NEVER peeks, fed the same pieces -- the peeking session's ids per call, logits rows, finish and vox_stream_info words (all but [5], the bytes, which
   grow by the save area of the first peek) are the twin's.
A solo stream's bits do not depend on how its samples were cut into pushes (tests/test_gpu_stream.py), so a twin may be fed in other pieces; a group's round width
selects the GEMM kernels, so a group's twins are fed exactly the same calls."""
import ctypes as C

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _full_path, _gain, _pieces, _t

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def full_model(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    yield m
    m.close()


@pytest.fixture(scope="module", params=["tiny", "full"])
def model(request):
    return request.getfixturevalue("tiny" if request.param == "tiny" else "full_model"), request.param


def _words(info):
    return {k: v for k, v in info.items() if k != "bytes"}


_CLIPS = {}


def _clip(pkg, seconds, seed):
    if (seconds, seed) not in _CLIPS:
        x = pkg.synth.synth_audio(seconds, seed=seed); x.setflags(write=False)
        _CLIPS[(seconds, seed)] = x
    return _CLIPS[(seconds, seed)]


def _walk(m, t, x, cuts, peek_after=(), scores=False, tap=256, finish=True, twice=False, gain=None, **kw):
    """One session: push x[a:b] for every (a, b) of cuts; after push k, for k in peek_after (-1: before the first push), a peek with its records and its logits rows.
    -> per (ids per push), peeks {k: (ids, records, rows)}, fin (finish's ids), lg (the tap: the session's OWN rows), rec (its own records), info (before finish),
    end (after), save (bytes the first peek added).  gain: the session's (default: the peak gain of x; a twin fed a part of a clip takes the clip's)."""
    st = m.create_stream(t, gain=_gain(x) if gain is None else gain, **kw)
    out = dict(per=[], peeks={}, fin=None, save=None)
    try:
        st.tap_arm(tap)
        if scores:
            st.set_scores(True)

        def peek(k):
            before = st.info()
            ids, rec = st.peek(return_scores=True); rows = st.tap_peeked(len(ids))
            after = st.info()
            assert _words(after) == _words(before), (k, before, after)
            if out["save"] is None:
                out["save"] = after["bytes"] - before["bytes"]
                assert out["save"] > 0
            else:
                assert after["bytes"] == before["bytes"]      # the save area is allocated once
            if twice:
                ids2, rec2 = st.peek(return_scores=True)
                assert np.array_equal(ids, ids2) and rec.tobytes() == rec2.tobytes() and np.array_equal(rows, st.tap_peeked(len(ids))), k
            assert len(ids) == len(rows) and np.array_equal(rows.argmax(axis=1), ids), k
            out["peeks"][k] = (ids, rec, rows)

        if -1 in peek_after:
            peek(-1)
        for k, (a, b) in enumerate(cuts):
            out["per"].append(st.push(x[a:b]))
            if k in peek_after:
                peek(k)
        out["info"] = st.info()
        if finish:
            out["fin"] = st.finish()
        out["end"] = st.info(); out["lg"] = st.tap_fetch()
        out["rec"] = st.scores() if scores else None
    finally:
        st.close()
    return out


def _same_session(a, b, label):
    """the peeking session `a` against the twin `b` that never peeked"""
    assert len(a["per"]) == len(b["per"])
    for k, (u, v) in enumerate(zip(a["per"], b["per"])):
        assert np.array_equal(u, v), f"{label}: push {k} returned {u}, the twin's {v}"
    assert (a["fin"] is None and b["fin"] is None) or np.array_equal(a["fin"], b["fin"]), f"{label}: finish differs from the twin's"
    assert a["lg"].shape == b["lg"].shape, (label, a["lg"].shape, b["lg"].shape)
    assert np.array_equal(a["lg"], b["lg"]), f"{label}: logits rows {np.unique(np.nonzero(a['lg'] != b['lg'])[0])[:8]} differ from the twin's"
    assert _words(a["info"]) == _words(b["info"]) and _words(a["end"]) == _words(b["end"]), (label, a["end"], b["end"])
    assert a["end"]["bytes"] - (a["save"] or 0) == b["end"]["bytes"], (label, a["end"]["bytes"], a["save"], b["end"]["bytes"])
    if a["rec"] is not None:
        assert a["rec"].tobytes() == b["rec"].tobytes(), f"{label}: the session's own records differ from the twin's"


def _peek_is_finish(peek, twin, label):
    """a peek's (ids, records, rows) against the twin that finished at that sample count"""
    ids, rec, rows = peek; n = len(twin["fin"])
    assert n >= 8 and np.array_equal(ids, twin["fin"]), f"{label}: peek {ids}, finish {twin['fin']}"
    assert np.array_equal(rows, twin["lg"][len(twin["lg"]) - n:]), f"{label}: the peek's logits rows differ from finish's"
    if twin["rec"] is not None:
        assert rec.tobytes() == twin["rec"][len(twin["rec"]) - n:].tobytes(), f"{label}: the peek's records differ from finish's"
        assert np.array_equal(rec["id"], ids) and np.isfinite(rec["logprob"]).all()
    else:
        assert np.isnan(rec["logprob"]).all() and np.isnan(rec["margin"]).all() and (rec["runner_up"] == -1).all() and np.array_equal(rec["id"], ids)      # the "off" records


# ---- 1. peek equals finish ----------------------------------------------------------------------------------------------------------------------------------------------
def test_peek_equals_finish(pkg, ctx, model):
    """The 16 s clip, peeks with nothing pushed, after 6.3 s and after all of it, each against a twin that finishes there (ids, logits rows, records); a second peek
    gives the first one's answer; the session's own finish behind the peeks is the twin's."""
    m, size = model
    x = _clip(pkg, 16.0, 1234); t = _t(pkg, m)
    cuts = [(0, 100777), (100777, len(x))]
    a = _walk(m, t, x, cuts, peek_after=(-1, 0, 1), scores=True, twice=True)
    assert len(a["peeks"]) == 3
    for k, n in ((-1, 0), (0, 100777), (1, len(x))):
        twin = _walk(m, t, x[:n], _pieces(n, 16000), scores=True, gain=_gain(x))
        assert len(twin["fin"]) == pkg.stream_peek_ids(n, pkg.stream_schedule(n)[1])
        _peek_is_finish(a["peeks"][k], twin, f"{size}: peek after {n} samples")
        if n == len(x):      # peek, then finish: finish's ids, rows and records, and the session's list holds the utterance's records alone
            assert np.array_equal(a["fin"], twin["fin"]) and np.array_equal(a["lg"], twin["lg"]) and a["rec"].tobytes() == twin["rec"].tobytes()
            assert _words(a["end"]) == _words(twin["end"])
    off = _walk(m, t, x[:100777], [(0, 100777)], peek_after=(0,), scores=False, gain=_gain(x))      # scores off: the records say so
    _peek_is_finish(off["peeks"][0], _walk(m, t, x[:100777], [(0, 100777)], gain=_gain(x)), f"{size}: scores off")


# ---- 2. the session goes on untouched -------------------------------------------------------------------------------------------------------------------------------------
def test_the_session_goes_on_untouched(pkg, ctx, model):
    """A peek after every push (tiny: 1600-sample pushes, 160 peeks; full: 16 000-sample pushes) against the twin that never peeks."""
    m, size = model
    x = _clip(pkg, 16.0, 1234); t = _t(pkg, m)
    cuts = _pieces(len(x), 1600 if size == "tiny" else 16000)
    a = _walk(m, t, x, cuts, peek_after=range(len(cuts)), scores=True)
    b = _walk(m, t, x, cuts, scores=True)
    assert len(a["peeks"]) == len(cuts) and sum(len(p) for p in b["per"]) + len(b["fin"]) == 108
    _same_session(a, b, f"{size}: a peek after every push")
    for k, (ids, rec, rows) in a["peeks"].items():      # every peek hands out what the schedule says finish would
        n = cuts[k][1]
        assert len(ids) == pkg.stream_peek_ids(n, pkg.stream_schedule(n)[1]), (k, n)
    assert np.array_equal(a["peeks"][len(cuts) - 1][0], b["fin"])


# ---- 3. ring rows ---------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cap", [755, 768])
def test_ring_rows_are_restored(pkg, ctx, tiny, cap):
    """33 s: 972 encoder rows through a ring of `cap` (755 is the smallest a 750-row window allows).  Peeks from before the ring's first wrap (24 s) to well past it: the
    tail's 32 .. 40 rows land on slots whose old rows the next real tick still reads -- at 755 from the second tick of the tail on -- so a peek that did not put them back
    changes the logits behind it."""
    m = tiny; x = _clip(pkg, 33.0, 33); t = _t(pkg, m)
    cuts = _pieces(len(x), 16000)
    at = (1, 9, 19, 22, 23, 24, 25, 28, 32)
    a = _walk(m, t, x, cuts, peek_after=at, enc_capacity_rows=cap)
    b = _walk(m, t, x, cuts, enc_capacity_rows=cap)
    assert b["end"]["encoder_position"] > cap + 150 and 4 * (37 + pkg.stream_schedule(cuts[19][1])[1]) < cap < 4 * (37 + pkg.stream_schedule(cuts[24][1])[1])
    _same_session(a, b, f"ring of {cap} rows")
    twin = _walk(m, t, x[:cuts[28][1]], cuts[:29], enc_capacity_rows=cap, gain=_gain(x))      # past the wrap the peek itself is still finish
    _peek_is_finish(a["peeks"][28], twin, f"ring of {cap} rows: peek after {cuts[28][1]} samples")


# ---- 4. decoder cache growth undone ---------------------------------------------------------------------------------------------------------------------------------------
def test_growth_inside_the_tail_is_undone(pkg, ctx, tiny):
    """166 s: a peek at each of the positions 1015 .. 1023 -- every tail crosses the cache's 1024 rows, so every peek grows the cache and takes the growth back -- then
    20 more positions, across the session's own growth.  The twin never peeks; info [5] differs by the save area alone: the cache is 1024 rows again after each peek."""
    m = tiny; x = _clip(pkg, 166.0, 61); t = _t(pkg, m)
    at = lambda pos: 2560 * pos + 40 - 97280      # samples at which decoder position `pos` becomes the next tick's
    n0 = at(1015); assert len(x) >= at(1044)
    cuts = _pieces(n0, 64000) + [(at(p), at(p + 1)) for p in range(1015, 1024)] + [(at(1024), at(1044))]
    first = len(_pieces(n0, 64000)) - 1
    peeks = range(first, first + 9)
    a = _walk(m, t, x, cuts, peek_after=peeks, tap=1100, finish=False)
    b = _walk(m, t, x, cuts, tap=1100, finish=False)
    assert a["info"]["positions"] == 1044 and all(a["peeks"][k][0].size >= 8 for k in peeks)
    _same_session(a, b, "peeks at positions 1015 .. 1023")
    twin = _walk(m, t, x[:at(1020)], _pieces(at(1020), 64000), tap=1100, gain=_gain(x))      # such a peek is finish's tail, growth included
    _peek_is_finish(a["peeks"][first + 5], twin, "peek at position 1020")


# ---- 5. capture rate and 16-bit PCM ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,s16", [(48000, False), (44100, True)])
def test_rate_and_pcm_streams(pkg, ctx, tiny, sr, s16):
    m = tiny; t = _t(pkg, m)
    rng = np.random.default_rng(900 + sr % 1000); n = int(2.5 * sr)
    f = 0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * (0.07 * 16000 / sr))
    x = np.clip(np.round(f * 20000), -32768, 32767).astype(np.int16) if s16 else f.astype(np.float32)
    cuts = _pieces(n, sr // 10)
    a = _walk(m, t, x, cuts, peek_after=[-1] + list(range(len(cuts))), scores=True, sample_rate=sr, twice=True)
    b = _walk(m, t, x, cuts, scores=True, sample_rate=sr)
    _same_session(a, b, f"{sr} Hz{' s16' if s16 else ''}: a peek after every push")
    for k in (-1, 6, len(cuts) - 1):      # nothing pushed, mid-block, the whole clip
        n_k = cuts[k][1] if k >= 0 else 0
        twin = _walk(m, t, x[:n_k], _pieces(n_k, sr // 4), scores=True, sample_rate=sr, gain=_gain(x))
        assert len(twin["fin"]) == pkg.stream_peek_ids(n_k, pkg.stream_schedule(n_k, sample_rate=sr)[1], sr)
        _peek_is_finish(a["peeks"][k], twin, f"{sr} Hz: peek after {n_k} samples")


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_are_finish_s_and_change_nothing(pkg, ctx, tiny):
    m = tiny; L = pkg.lib(); t = _t(pkg, m); x = _clip(pkg, 3.0, 31)
    twin = _walk(m, t, x, [(0, len(x))])
    st = m.create_stream(t, gain=_gain(x))
    try:
        st.push(x)
        due = len(twin["fin"]); n = C.c_int32(-1); ids = np.zeros(64, np.int32)
        before = st.info()
        assert L.vox_stream_peek(st.h, ids.ctypes.data, due - 1, C.byref(n), None) == 1 and b"capacity" in L.vox_last_error()      # cap one short
        assert st.info() == before
        assert L.vox_stream_peek(st.h, ids.ctypes.data, due, C.byref(n), None) == 0      # the same peek with room
        assert n.value == due and np.array_equal(ids[:due], twin["fin"])
        assert L.vox_stream_peek(st.h, None, 4, C.byref(n), None) == 1 and L.vox_stream_peek(st.h, ids.ctypes.data, 64, None, None) == 1
        assert np.array_equal(st.finish(), twin["fin"])
        before = st.info()
        with pytest.raises(pkg.VoxError, match="finished"):
            st.peek()
        assert st.info() == before
        st.reset()
        assert len(st.peek()) == 8      # the next utterance peeks again
    finally:
        st.close()
    small = m.create_stream(t, gain=_gain(x), max_positions=48)      # positions 37 .. 47 can be reached
    try:
        ks = [k for k in range(12) if pkg.stream_schedule(2560 * k + 40)[0] <= 48 and pkg.stream_schedule(2560 * k + 40, finished=True)[0] - 1 > 48]
        assert ks and ks[0] >= 2
        k = ks[0]; ref = _walk(m, t, x[:2560 * (k - 1) + 40], [(0, 2560 * (k - 1) + 40)], gain=_gain(x))
        small.push(x[:2560 * (k - 1) + 40])
        assert np.array_equal(small.peek(), ref["fin"])      # this tail still fits
        small.push(x[2560 * (k - 1) + 40:2560 * k + 40])
        before = small.info()
        with pytest.raises(pkg.VoxError, match="position"):
            small.peek()
        assert small.info() == before
        with pytest.raises(pkg.VoxError, match="position"):      # as finish is
            small.finish()
    finally:
        small.close()


# ---- 7. groups ------------------------------------------------------------------------------------------------------------------------------------------------------------
def _group_run(pkg, m, t, clips, rates, piece_s, peeks, stop_after=None, finish_at_stop=(), scored=(0,)):
    """A group's calls: member k starts in call k and is fed piece_s seconds of its clip per call; peeks: {call: members peeked behind it}.  stop_after: the run ends behind
    that call with advance({}, finish=finish_at_stop).  -> per-call ids, the peeks' results, each member's tap rows and info, the finishing ids and records at the stop."""
    n = len(clips)
    g = m.create_stream_group(t, n, gains=[_gain(c) for c in clips], max_positions=256, sample_rates=rates)
    out = dict(calls=[], peeks={}, taps=[], info=[], stop=None)
    try:
        for k in range(n):
            g.tap_arm(k, 128)
        for k in scored:
            g.set_scores(k, True)
        step = [int(piece_s * r) for r in rates]
        n_calls = max(k + -(-len(clips[k]) // step[k]) for k in range(n))
        for c in range(n_calls):
            feeds = {}; fin = []
            for k in range(n):
                lo = (c - k) * step[k]
                if c >= k and lo < len(clips[k]):
                    feeds[k] = clips[k][lo:lo + step[k]]
                    if lo + step[k] >= len(clips[k]) and stop_after is None:
                        fin.append(k)
            out["calls"].append(g.advance(feeds, finish=fin))
            if c in peeks:
                before = [g.info(k) for k in range(n)]
                out["peeks"][c] = g.peek(peeks[c], return_scores=True)
                after = [g.info(k) for k in range(n)]
                assert [_words(i) for i in before] == [_words(i) for i in after], c
            if c == stop_after:
                ids = g.advance({}, finish=list(finish_at_stop))
                out["stop"] = {k: (ids[k], g.scores(k)[len(g.scores(k)) - len(ids[k]):] if k in scored else None) for k in finish_at_stop}
                break
        out["info"] = [_words(g.info(k)) for k in range(n)]
        out["taps"] = [g.tap_fetch(k) for k in range(n)]
    finally:
        g.close()
    return out


def _same_group(a, b, label):
    assert len(a["calls"]) == len(b["calls"])
    for c, (u, v) in enumerate(zip(a["calls"], b["calls"])):
        assert u.keys() == v.keys() and all(np.array_equal(u[k], v[k]) for k in u), f"{label}: call {c} differs from the twin's"
    assert a["info"] == b["info"], (label, a["info"], b["info"])
    for k, (u, v) in enumerate(zip(a["taps"], b["taps"])):
        assert u.shape == v.shape and u.shape[0] >= 8 and np.array_equal(u, v), f"{label}: member {k}'s logits rows differ from the twin's"


def _group_checks(pkg, m, t, clips, rates, piece_s, peeks, at, label):
    a = _group_run(pkg, m, t, clips, rates, piece_s, peeks)
    b = _group_run(pkg, m, t, clips, rates, piece_s, {})
    assert sorted(a["peeks"]) == sorted(peeks)
    _same_group(a, b, label)      # later rounds of every member, the peeked and the others
    c = _group_run(pkg, m, t, clips, rates, piece_s, {}, stop_after=at, finish_at_stop=peeks[at])      # the twin whose members finish where the others peeked
    for k in peeks[at]:
        ids, rec = a["peeks"][at][k]; fids, frec = c["stop"][k]
        assert len(ids) >= 8 and np.array_equal(ids, fids), f"{label}: member {k}: peek {ids}, finishing advance {fids}"
        if frec is not None:
            assert rec.tobytes() == frec.tobytes(), f"{label}: member {k}: the peek's records differ from the finishing advance's"
        else:
            assert np.isnan(rec["logprob"]).all() and np.array_equal(rec["id"], ids)
    return a


def test_group_peek_tiny(pkg, ctx, tiny):
    """Three members, staggered starts, 16 kHz / 48 kHz / 44.1 kHz, max_positions 256; subsets peeked behind calls 1, 3, 4 and 6."""
    m = tiny; t = _t(pkg, m); rates = [16000, 48000, 44100]
    rng = np.random.default_rng(77)
    clips = [(0.4 * rng.standard_normal(int(s * r)) + 0.3 * np.sin(np.arange(int(s * r)) * (0.07 * 16000 / r))).astype(np.float32) for s, r in zip((3.1, 2.6, 2.2), rates)]
    peeks = {1: [1], 3: [0, 2], 4: [2, 1, 0], 6: [0]}
    _group_checks(pkg, m, t, clips, rates, 0.4, peeks, 3, "tiny group of three")
    g = m.create_stream_group(t, 3, max_positions=256, sample_rates=rates)
    try:
        L = pkg.lib(); ids = np.zeros(32, np.int32)
        arr = (pkg._lib.StreamFeed * 2)()
        for e in arr:
            e.member = 1; e.finish = 0; e.samples = None; e.n_samples = 0; e.out_ids = ids.ctypes.data; e.cap = 16; e.n_ids = -1
        before = [g.info(k) for k in range(3)]
        assert L.vox_stream_group_peek(g.h, arr, 2, None) == 1 and b"twice" in L.vox_last_error()
        arr[1].member = 2; arr[1].n_samples = 5; arr[1].samples = ids.ctypes.data
        assert L.vox_stream_group_peek(g.h, arr, 2, None) == 1 and b"peek" in L.vox_last_error()
        arr[1].n_samples = 0; arr[1].samples = None; arr[1].finish = 1
        assert L.vox_stream_group_peek(g.h, arr, 2, None) == 1 and b"peek" in L.vox_last_error()
        arr[1].finish = 0; arr[1].cap = 7
        assert L.vox_stream_group_peek(g.h, arr, 2, None) == 1 and b"capacity" in L.vox_last_error()
        assert [g.info(k) for k in range(3)] == before
        assert L.vox_stream_group_peek(g.h, arr, 0, None) == 0
        g.advance({}, finish=[2])
        with pytest.raises(pkg.VoxError, match="finished"):
            g.peek([2])
        assert len(g.peek([0, 1])[0]) == 8
    finally:
        g.close()


def test_group_ring_rows_are_restored(pkg, ctx, tiny):
    """Two members with rings of 755 rows, 33 s and 31 s in 1 s calls (positions up to 243 of 256): peeks from before the rings' first wrap (24 s) to well past it,
    of one member and of both.  Past the wrap the tails overwrite rows inside the 750-row window: the twin comparison fails unless the keep launch puts them back."""
    m = tiny; t = _t(pkg, m)
    clips = [_clip(pkg, 33.0, 33), _clip(pkg, 33.0, 34)[:31 * 16000]]
    n = len(clips)

    def run(peeks):
        g = m.create_stream_group(t, n, gains=[_gain(c) for c in clips], enc_capacity_rows=755, max_positions=256)
        out = dict(calls=[], peeks={})
        try:
            for k in range(n):
                g.tap_arm(k, 256)
            for c in range(33):
                feeds = {k: clips[k][16000 * c:16000 * (c + 1)] for k in range(n) if 16000 * c < len(clips[k])}
                out["calls"].append(g.advance(feeds, finish=[k for k in feeds if 16000 * (c + 1) >= len(clips[k])]))
                if c in peeks:
                    out["peeks"][c] = g.peek(peeks[c])
            out["info"] = [_words(g.info(k)) for k in range(n)]
            out["taps"] = [g.tap_fetch(k) for k in range(n)]
        finally:
            g.close()
        return out

    peeks = {5: [0, 1], 22: [1], 24: [0, 1], 25: [0], 27: [1, 0], 29: [0, 1], 31: [0]}
    a = run(peeks); b = run({})
    assert sorted(a["peeks"]) == sorted(peeks) and all(len(ids) >= 8 for p in a["peeks"].values() for ids in p.values())
    assert b["info"][0]["encoder_position"] > 755 + 150 and b["info"][1]["encoder_position"] > 755 + 100
    _same_group(a, b, "group with rings of 755 rows")


def test_group_peek_full(pkg, ctx, full_model):
    """Two full-size members, max_positions 256: member 0 peeked behind call 2, both behind call 4."""
    m = full_model; t = _t(pkg, m)
    clips = [_clip(pkg, 3.0, 31), _clip(pkg, 3.0, 503)[:40000]]
    _group_checks(pkg, m, t, clips, [16000, 16000], 0.5, {2: [0], 4: [0, 1]}, 4, "full-size group of two")
