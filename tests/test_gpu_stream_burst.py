"""Burst streams (vox_stream_create_burst, DESIGN.md section 8, "Bursts"): a solo live session that runs the due ticks of a pass in bursts of up to 16 -- one encoder
pass of 4 b rows with the burst ring attention, then the b decode steps -- against a plain stream on the same audio.

What is asserted, and against what:
 * fed one tick per call a burst stream IS a plain stream: ids and tapped logits bit for bit, burst_info shows no burst;
 * with a backlog its ids are the plain stream's by the rule of the group files (stream_helpers._held at TOL = 2e-4: equal outright before the reference's first
   near-tie, which lies at or beyond half of the ids -- a clip that does not meet the condition is swapped for another seed, the condition is never relaxed) and its
   tapped logits lie within 2e-4 of the largest teacher-forced logit, the group files' bound: the row count selects the GEMM kernels, as in a group;
 * burst_info and vox_debug_stream_attn_burst_launches count what ran: a pass's ticks are cut into min(due in the pass, 16, distance to the next stop).  A pass holds
   what the 65 536-sample ring takes, so 40 due ticks of a fresh stream are the passes 26 + 14 and the bursts 16, 10, 14 (_bursts_of restates the rule on the feed
   planner's own passes);
 * the front tap of a burst holds the ticks' frames bit for bit and their conv rows within the front-end tests' bound against float64 on the tapped mel;
 * a peek on a backlog (its tail runs in bursts) leaves the session what it was: ids per call, tapped rows, finish, info words and burst_info of a twin that never peeks;
 * with scores and alternatives on every record is vox_score_rows / vox_alternatives_rows of its tapped row, byte for byte;
 * an endless burst stream crosses its wrap inside one call: the burst is cut at ring_rows (3 + 16 + 3 ticks: three bursts where 16 + 6 would be two), ids by _held
   against a plain endless stream continued from the same snapshot;
 * a snapshot at a position reached by bursts continues in a plain stream by _held;
 * full size (the peaked synthetic model): 40 ticks in one call by _held.
Reaching the wrap of the 8192-position decoder window costs 8250 ticks, here run in bursts (about a second on the tiny model)."""
import ctypes as C
import os

import numpy as np
import pytest

from model_fixtures import gguf_conv_weights, teacher_forced_logits, tiny_gguf
from stream_helpers import _full_path, _gain, _held, _stop, _t
from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
TOL = 2e-4
TICK = 2560
B = 16


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gg(pkg):
    return __import__("importlib").import_module(pkg.__name__ + ".gguf")


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


def _n_for(pkg, positions):
    """The fewest samples after which `positions` decoder positions are determined (an unfinished 16 kHz stream)."""
    n = max(0, (positions - 38) * TICK)
    while pkg.stream_schedule(n)[0] < positions:
        n += 1
    assert pkg.stream_schedule(n)[0] == positions
    return n


def _passes(pkg, calls):
    """The feed planner's passes of a fresh 16 kHz session fed `calls` = [(samples, finish)]: [(call, ticks)]."""
    n = len(calls); ns = (C.c_size_t * n)(*[c[0] for c in calls]); fin = (C.c_int32 * n)(*[int(c[1]) for c in calls])
    rows = np.zeros((256, 5), np.int64); k = C.c_int32()
    assert pkg.lib().vox_debug_stream_feed_passes(16000, ns, fin, n, 0, rows.ctypes.data_as(C.POINTER(C.c_int64)), 256, C.byref(k)) == 0
    return [(int(r[0]), int(r[4])) for r in rows[:k.value]]


def _bursts_of(passes, burst=B):
    """The rule, restated for a session far from every stop: each pass's ticks in bursts of min(due, burst); -> (bursts with b >= 2, ticks in them, single ticks)."""
    nb = nt = single = 0
    for _, due in passes:
        while due > 0:
            b = min(due, burst); due -= b
            if b >= 2:
                nb += 1; nt += b
            else:
                single += 1
    return nb, nt, single


_PLAIN = {}      # clip key -> (ids, logits) of the plain stream: computed once, shared, read-only


def _plain(m, key, x, t):
    if key not in _PLAIN:
        st = m.create_stream(t, gain=_gain(x)); st.tap_arm(256)
        try:
            ids = np.concatenate([st.push(x), st.finish()]); lg = st.tap_fetch()      # (a plain stream's ids do not depend on the cuts, bit for bit)
        finally:
            st.close()
        assert lg.shape[0] == len(ids) and np.array_equal(lg.argmax(axis=1), ids)
        ids.setflags(write=False); lg.setflags(write=False)
        _PLAIN[key] = (ids, lg)
    return _PLAIN[key]


def _clip(pkg, m, t, seconds, seed):
    """synth_audio(seconds, seed), the seed moved on until the plain reference's first near-tie lies at or beyond half of the clip's ids."""
    for s in range(seed, seed + 12 * 1000, 1000):
        x = pkg.synth.synth_audio(seconds, seed=s)
        ids, lg = _plain(m, (id(m), seconds, s), x, t)
        if 2 * _stop(lg, TOL) >= len(ids):
            return x, ids, lg
        print(f"clip {seconds} s seed {s}: first near-tie at {_stop(lg, TOL)} of {len(ids)} ids: another seed")
    raise AssertionError(f"no seed from {seed} on gives a {seconds} s clip that can carry an ids claim")


def _bi(st):
    i = st.burst_info()
    return i["bursts"], i["burst_ticks"], i["single_ticks"]


def test_one_tick_per_call_is_a_plain_stream_bit_for_bit(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); x = pkg.synth.synth_audio(6.0, seed=311)
    cuts = [0, 40] + list(range(40 + TICK, len(x), TICK))      # the first tick is due at 40 samples, one more every 2560
    out = {}
    for name, kw in (("plain", {}), ("burst", {"burst": B})):
        st = m.create_stream(t, gain=_gain(x), **kw); st.tap_arm(128)
        try:
            per = [st.push(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
            assert all(len(p) <= 1 for p in per) and sum(len(p) for p in per) >= 30
            info = st.burst_info()
            out[name] = (np.concatenate(per), st.tap_fetch(), info)
        finally:
            st.close()
    ids, lg, info = out["burst"]
    assert info == {"burst": B, "bursts": 0, "burst_ticks": 0, "single_ticks": len(ids)}, info
    assert out["plain"][2] == {**info, "burst": 1}
    assert np.array_equal(ids, out["plain"][0]) and np.array_equal(lg.view(np.uint32), out["plain"][1].view(np.uint32))


def test_default_ring_capacity_and_the_refusal_of_a_small_one(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); w = m.config.enc_window
    assert w == 750
    for burst, cap in ((1, 768), (4, 832), (16, 832)):
        st = m.create_stream(t, burst=burst)
        try:
            st.push(np.zeros(TICK * 230, np.float32))      # 920 encoder rows: the ring is full
            assert st.info()["ring_rows"] == cap == (max(w + 4 * burst + 4, 148) + 63) // 64 * 64
        finally:
            st.close()
    with pytest.raises(pkg.VoxError) as e:
        m.create_stream(t, burst=16, enc_capacity_rows=w + 64)
    assert e.value.code == 1 and str(w + 64) in str(e.value) and "burst_ticks" in str(e.value), e.value
    m.create_stream(t, burst=16, enc_capacity_rows=w + 65).close()


def test_forty_ticks_in_one_call(pkg, ctx, gg, tiny):
    m = tiny; t = _t(pkg, m); EL = m.config.enc_layers
    x, rids, rlg = _clip(pkg, m, t, 8.0, 520)
    n40 = _n_for(pkg, 77)      # positions 37 .. 76: 40 ticks, 40 ids
    st = m.create_stream(t, gain=_gain(x), burst=B); st.tap_arm(256)
    try:
        a0 = gg.stream_attn_burst_launches()
        first = st.push(x[:n40])
        got = _bi(st); want = _bursts_of(_passes(pkg, [(n40, 0)]))
        print(f"40 ticks due in one call: passes {_passes(pkg, [(n40, 0)])}, bursts {got}")
        assert len(first) == 40 and got == want == (3, 40, 0)
        assert gg.stream_attn_burst_launches() - a0 == 3 * EL
        ids = np.concatenate([first, st.push(x[n40:]), st.finish()]); lg = st.tap_fetch()
    finally:
        st.close()
    same = _held(ids, rids, rlg, "burst stream, 40 ticks in one call", TOL)
    assert lg.shape[0] == len(ids) and np.array_equal(lg.argmax(axis=1), ids)
    ref = teacher_forced_logits(pkg, ctx, m, x, t, ids)
    err = float(np.abs(lg - ref).max()); bar = TOL * float(np.abs(ref).max())
    print(f"burst stream: {same} of {len(rids)} ids equal to the plain stream's; tapped logits vs teacher-forced: max error {err:.3e}, bar {bar:.3e}")
    assert err <= bar


def test_front_tap_of_a_burst(pkg, ctx, tiny):
    import frontend_ref as F
    from linear_ref import EPI_GELU, carry_bound
    m = tiny; t = _t(pkg, m)
    x = F.make_clip("noise", 9, 3.0); ticks = F.pad_len(len(x)) // TICK - 1 - 37
    out = {}
    for name, kw in (("plain", {}), ("burst", {"burst": B})):
        st = m.create_stream(t, gain=_gain(x), **kw); st.front_tap_arm(ticks + 3)
        try:
            st.push(x); st.finish(); info = st.burst_info()
            mel, conv = st.front_tap_fetch()
        finally:
            st.close()
        assert mel.shape[0] == conv.shape[0] == ticks
        out[name] = (np.ascontiguousarray(mel.reshape(ticks * 16, -1).T), conv.reshape(ticks * 4, -1), info)
    mel, conv, info = out["burst"]
    assert info["bursts"] >= 2 and info["burst_ticks"] + info["single_ticks"] == ticks
    assert np.array_equal(mel.view(np.uint32), out["plain"][0].view(np.uint32)), "the burst's mel frames are not the ticks' frames"
    w1, b1, w2, b2 = gguf_conv_weights(pkg, tiny_gguf()[0], m.config.enc_dim, m.config.n_mels)
    full = np.full((128, 592 + mel.shape[1]), np.float32(F.FLOOR), np.float32); full[:, 592:] = mel
    ref, pre = F.conv_stem(full, w1, b1, w2, b2)
    ref, pre = ref[148:], pre[148:]
    assert ref.shape == conv.shape
    bound = carry_bound(pre, 2e-5 * np.abs(pre).max(axis=1)[:, None], EPI_GELU)
    err = np.abs(conv - ref); ratio = float((err / bound).max())
    print(f"burst conv rows: worst error {err.max():.2e}, {ratio:.3f} x the bound; bit-equal to the plain stream's: {np.array_equal(conv, out['plain'][1])}")
    assert (err <= bound).all(), f"conv row {148 + int(np.argmax((err / bound).max(axis=1)))} is {ratio:.2f} x its bound"


def test_cuts_that_force_bursts_of_2_3_and_5(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    x, rids, rlg = _clip(pkg, m, t, 8.0, 520)
    st = m.create_stream(t, gain=_gain(x), burst=B)
    try:
        ids = []; at = 0; seen = []
        for due in (1, 2, 3, 1, 5, 2):
            n = _n_for(pkg, st.info()["positions"] + due); before = _bi(st)
            ids.append(st.push(x[at:n])); at = n
            seen.append(tuple(a - b for a, b in zip(_bi(st), before)))
        assert seen == [(0, 0, 1), (1, 2, 0), (1, 3, 0), (0, 0, 1), (1, 5, 0), (1, 2, 0)], seen
        ids += [st.push(x[at:]), st.finish()]
    finally:
        st.close()
    _held(np.concatenate(ids), rids, rlg, "bursts of 2, 3 and 5", TOL)


def test_a_peek_on_a_backlog_leaves_the_session_as_it_was(pkg, ctx, tiny):
    """Two burst streams fed the same calls (a backlog in each), one of which peeks twice on the way -- the peek's tail runs in bursts: the peeking session's ids
    per call, its tapped logits rows, its finish, its info words (all but the bytes, which grow by the first peek's save area) and its burst_info are the twin's,
    bit for bit (the method of tests/test_gpu_stream_peek.py); the peeked ids are those of the utterance that ends there, by _held."""
    m = tiny; t = _t(pkg, m)
    x, rids, rlg = _clip(pkg, m, t, 8.0, 520)
    cut = 16000 * 5 + 123; cuts = [(0, 30000), (30000, cut), (cut, 110000), (110000, len(x))]
    out = {}
    for name in ("twin", "peeks"):
        st = m.create_stream(t, gain=_gain(x), burst=B); st.tap_arm(256)
        try:
            per = []; peeked = None
            for a, b in cuts:
                per.append(st.push(x[a:b]))
                if name == "peeks" and b in (cut, 110000):
                    words = lambda: ({k: v for k, v in st.info().items() if k != "bytes"}, st.burst_info())
                    before = words(); got = st.peek()
                    assert words() == before
                    peeked = got if b == cut else peeked
            per.append(st.finish())
            words = {k: v for k, v in st.info().items() if k != "bytes"}
            out[name] = (per, st.tap_fetch(), words, st.burst_info(), peeked)
        finally:
            st.close()
    per, lg, words, bi, peeked = out["peeks"]
    assert bi["bursts"] >= 6 and len(peeked) >= 8      # the tail: the right pad's ticks, several due in one pass
    assert len(per) == len(out["twin"][0]) and all(np.array_equal(a, b) for a, b in zip(per, out["twin"][0]))
    assert np.array_equal(lg.view(np.uint32), out["twin"][1].view(np.uint32)) and words == out["twin"][2] and bi == out["twin"][3]
    _held(np.concatenate(per), rids, rlg, "burst stream around its peeks", TOL)
    pids, plg = _peek_ref(m, t, x, cut)      # the utterance that ends at the cut: what the peek answers for
    _held(np.concatenate(per[:2] + [peeked]), pids, plg, "peeked ids", TOL)


def _peek_ref(m, t, x, cut):
    """(ids, logits) of a plain stream fed x[:cut] and finished: what a peek at `cut` returns behind the ids handed out, with the rows behind them."""
    key = ("peek", id(m), cut)
    if key not in _PLAIN:
        st = m.create_stream(t, gain=_gain(x)); st.tap_arm(256)
        try:
            ids = np.concatenate([st.push(x[:cut]), st.finish()]); lg = st.tap_fetch()
        finally:
            st.close()
        _PLAIN[key] = (ids, lg)
    return _PLAIN[key]


def test_scores_and_alternatives_are_the_records_of_the_tapped_rows(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); x = pkg.synth.synth_audio(6.0, seed=311)
    st = m.create_stream(t, gain=_gain(x), burst=B)
    try:
        st.tap_arm(128); st.set_scores(True); st.set_alternatives(3)
        ids = np.concatenate([st.push(x), st.finish()]); lg = st.tap_fetch()
        sc, al = st.scores(), st.alternatives()
        assert st.burst_info()["bursts"] >= 2
    finally:
        st.close()
    assert len(ids) == len(sc) == len(al) == lg.shape[0] >= 30 and np.array_equal(sc["id"], ids)
    assert sc.tobytes() == pkg.score_rows(ctx, lg, ids).tobytes()
    assert al.tobytes() == pkg.alternatives_rows(ctx, lg, 3).tobytes()


@pytest.fixture(scope="module")
def endless_run(tmp_path_factory):
    r = run_worker("stream_burst_endless_worker.py", tmp_path_factory.mktemp("burst_endless"), 600)
    print(r[1][-1500:])
    return r


def test_an_endless_burst_stream_is_cut_at_its_wrap(endless_run):
    """tests/stream_burst_endless_worker.py, in a process of its own: past its wrap an endless session launches the ring decode attention, whose slot of
    vox_debug_attn_launches other tests of the suite hold to 0 in their process."""
    check(endless_run, "test_an_endless_burst_stream_is_cut_at_its_wrap")
    assert set(endless_run[0]) == {"test_an_endless_burst_stream_is_cut_at_its_wrap"}


def test_a_snapshot_reached_by_bursts_continues_in_a_plain_stream(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    x, rids, rlg = _clip(pkg, m, t, 8.0, 520)
    n40 = _n_for(pkg, 77)
    sb = m.create_stream(t, gain=_gain(x), burst=B); sp = m.create_stream(t, gain=_gain(x))
    try:
        head = sb.push(x[:n40])
        assert _bi(sb)[0] == 3
        sp.restore(sb.snapshot())
        assert sp.info()["positions"] == 77 and sp.burst_info()["burst"] == 1
        ids = np.concatenate([head, sp.push(x[n40:]), sp.finish()])
        assert sp.burst_info()["bursts"] == 0
    finally:
        sb.close(); sp.close()
    _held(ids, rids, rlg, "a plain stream restored from a burst stream's snapshot", TOL)


def test_full_size_forty_ticks_in_one_call(pkg, ctx, full_model):
    m = full_model; t = _t(pkg, m)
    x = pkg.synth.synth_audio(16.0, seed=7049)
    rids, rlg = _plain(m, ("full", 7049), x, t)
    assert 2 * _stop(rlg, TOL) >= len(rids)
    n40 = _n_for(pkg, 77)
    st = m.create_stream(t, gain=_gain(x), burst=B)
    try:
        first = st.push(x[:n40])
        assert len(first) == 40 and _bi(st) == (3, 40, 0)
        ids = np.concatenate([first, st.push(x[n40:]), st.finish()])
    finally:
        st.close()
    same = _held(ids, rids, rlg, "full size, 40 ticks in one call", TOL)
    print(f"full size: {same} of {len(rids)} ids equal to the plain stream's")


def test_cli_live_burst_prints_a_line(pkg, tmp_path):
    """--live --live-burst 16 fed in 1 s chunks (6 ticks due per push) prints a line as --live does; the flag is refused without --live, with --live-group and out of range."""
    import base64, contextlib, io, json, wave
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)
    vocab = [{"rank": i, "token_bytes": base64.b64encode(f" w{i}".encode()).decode(), "token_str": f" w{i}"} for i in range(1200)]
    tok = str(tmp_path / "tekken.json")
    json.dump({"config": {"pattern": "", "num_vocab_tokens": 1200, "default_vocab_size": 131072, "default_num_special_tokens": 1000, "version": "v7"}, "vocab": vocab}, open(tok, "w"))
    wav = str(tmp_path / "clip.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(S.synth_audio(8.0, seed=1234), -1, 1) * 32767).astype("<i2").tobytes())

    def run_cli(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok, "--audio", wav, "--live", "--live-chunk-ms", "1000"] + extra)
        return rc, buf.getvalue()

    rc0, out0 = run_cli([])
    rc1, out1 = run_cli(["--live-burst", "16"])
    assert rc0 == 0 and rc1 == 0 and out0.strip() and out1.strip(), (out0, out1)
    for bad in (["--live-burst", "17"], ["--live-burst", "4", "--live-group", "2"]):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            run_cli(bad)
    with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
        cli.main(["--gguf", gguf, "--tokenizer", tok, "--audio", wav, "--live-burst", "4"])
