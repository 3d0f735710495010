"""Worker of tests/test_gpu_stream_group_endless.py: its tests run through pytest in a process of their own (worker_tests.run_worker) -- they launch the paged attention on ring
page tables, whose launch counts (vox_debug_attn_launches [14] [15]) the suite's other tests hold to 0 in their own process.  Not collected by the suite (no test_ prefix).

Endless paged stream groups (vox_stream_group_create_endless, DESIGN.md section 8 "Endless paged groups"): the members of a paged group go on past 16 384 positions.

The reference of every comparison is the BOUNDED paged group of the same build under the identical sequence of calls: every round then has the same width and picks
the same GEMM kernels, and the paged attention's bits depend on the logical key index alone.  So every claim is np.array_equal -- on ids, on f32 logits viewed as
uint32, on the records' bytes -- with no tolerance anywhere in this file.  An endless group reads its member RoPE rings and its ring page tables at EVERY position, so
the runs below 16 384 exercise the code that runs above it; past the limit there is no bounded reference, and the last test says what stands behind its values."""
import base64
import contextlib
import ctypes as C
import io
import json
import time
import wave

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _t

pytestmark = pytest.mark.gpu
TICK = 2560
LISTS_START = 2048      # positions a member's token row and records start with (include/voxtral_hip.h, ENDLESS PAGED GROUPS)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def models(pkg, ctx):
    """the per-head model (4 heads on 2 KV heads) and the GQA one (8 on 2: G = 4), loaded when first asked for"""
    held = {}

    def get(kind):
        if kind not in held:
            held[kind] = pkg.Q4ModelLoader.from_file(tiny_gguf(**({"dec_heads": 8} if kind == "gqa" else {}))[0]).load(ctx)
        return held[kind]
    yield get
    for m in held.values():
        m.close()


def _counts(pkg):
    a = (C.c_uint64 * 16)()
    assert pkg.lib().vox_debug_attn_launches(a, 16) == 0
    return [int(x) for x in a]


def _same(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    va = a.view(np.uint32) if a.dtype == np.float32 else np.frombuffer(a.tobytes(), np.uint8)
    vb = b.view(np.uint32) if b.dtype == np.float32 else np.frombuffer(b.tobytes(), np.uint8)
    assert np.array_equal(va, vb), f"{what}: differs from the bounded paged group's at {np.argwhere(va != vb)[:4].tolist()}"


def _pool_ok(g):
    p = g.pool()
    assert p["free"] + sum(p["held"]) == p["pool_pages"], p
    every = [q for k in range(g.n_members) for q in g.pages(k)]
    assert len(every) == sum(p["held"]) and len(set(every)) == len(every) and all(0 <= q < p["pool_pages"] for q in every)      # no page in two tables
    return p


def _pcm(x):
    return (np.clip(x, -1, 1) * 32767).astype(np.int16)


# ---- 4. endless == bounded paged: three interleaving members, every feature on -------------------------------------------------------------------------------------------
def _three(pkg, g):
    """Clips of 24, 9 and 5 s start in calls 0, 2 and 5 (the staggered feeding of the paged group's file), every member fed 16-bit PCM -- member 1 at 48 kHz --, scores
    and k = 3 alternatives on, the logits tapped; member 2 is reset when its clip ends and reused for a 6 s clip; one peek of the busy members behind call 6.
    -> everything the calls handed back, and pool() after every call."""
    S = pkg.synth
    clips = [_pcm(S.synth_audio(24.0, seed=910)), _pcm(S.synth_audio(9.0, seed=911, sample_rate=48000)), _pcm(S.synth_audio(5.0, seed=912))]
    again = _pcm(S.synth_audio(6.0, seed=913))
    rate = [16000, 48000, 16000]; starts = [0, 2, 5]; step = [3200, 9600, 3200]
    for k in range(3):
        g.set_scores(k, True); g.set_alternatives(k, 3); g.tap_arm(k, 256)
    out = {"ids": [[] for _ in range(4)], "pools": [], "peek": None}
    off = [0, 0, 0]; done = [False] * 3; first2 = None; c = 0
    while not all(done):
        feeds = {}; fin = []
        for k in range(3):
            if c >= starts[k] and not done[k]:
                feeds[k] = clips[k][off[k]:off[k] + step[k]]
                if off[k] + step[k] >= len(clips[k]):
                    fin.append(k)
        for k, v in g.advance(feeds, finish=fin).items():
            out["ids"][3 if (k == 2 and first2 is not None) else k].extend(v); off[k] += step[k]
        out["pools"].append(_pool_ok(g))
        for k in fin:
            if k == 2 and first2 is None:      # the member's next connection: its records and its tap start over, its pages went back
                first2 = (g.scores(2).copy(), g.alternatives(2).copy(), g.tap_fetch(2))
                g.reset(2, _gain(again)); g.tap_arm(2, 256)
                clips[2] = again; off[2] = 0
                out["pools"].append(_pool_ok(g))
            else:
                done[k] = True
        if c == 6:
            before = (g.pool(), [g.pages(k) for k in range(3)], [{a: b for a, b in g.info(k).items() if a != "bytes"} for k in range(3)])
            pk = g.peek([0, 1], return_scores=True)
            out["peek"] = (pk[0][0], pk[0][1], pk[1][0], pk[1][1], g.peeked_alternatives(0).copy(), g.peeked_alternatives(1).copy())
            assert (g.pool(), [g.pages(k) for k in range(3)], [{a: b for a, b in g.info(k).items() if a != "bytes"} for k in range(3)]) == before
            assert len(pk[0][0]) > 0 and len(pk[1][0]) > 0
        c += 1
    out["ids"] = [np.array(v, np.int32) for v in out["ids"]]
    # (slot 2: member 2's first connection, slot 3: its second)
    out["scores"] = [g.scores(0).copy(), g.scores(1).copy(), first2[0], g.scores(2).copy()]
    out["alts"] = [g.alternatives(0).copy(), g.alternatives(1).copy(), first2[1], g.alternatives(2).copy()]
    out["taps"] = [g.tap_fetch(0), g.tap_fetch(1), first2[2], g.tap_fetch(2)]
    out["positions"] = [g.info(k)["positions"] for k in range(3)]
    return out


@pytest.mark.parametrize("kind,slot,flat_slot", [("head", 14, 11), ("gqa", 15, 12)])
def test_endless_group_equals_the_bounded_paged_group_bit_for_bit(pkg, ctx, models, kind, slot, flat_slot):
    m = models(kind); t = _t(pkg, m)
    assert (m.config.dec_heads == 4 * m.config.dec_kv_heads) == (kind == "gqa")
    kw = dict(gains=[0.9, 1.1, 1.0], sample_rates=[16000, 48000, 16000], page_rows=16, pool_pages=40)
    res = []
    for endless in (False, True):
        g = m.create_stream_group(t, 3, **kw, **({"endless": True} if endless else {"max_positions": 256}))
        try:
            assert g.pool() == {"page_rows": 16, "pool_pages": 40, "free": 40 - 9, "peak": 9, "held": [3, 3, 3]}
            c0 = _counts(pkg); res.append(_three(pkg, g)); c1 = _counts(pkg)
        finally:
            g.close()
        d = [b - a for a, b in zip(c0, c1)]
        print(f"{kind}, endless {endless}: attention launches [11..15] {d[11:]}")
        if endless:      # every decode attention of the endless group is the ring-table form; the flat forms' slots do not move
            assert d[slot] > 0 and d[11] == 0 and d[12] == 0 and d[13] == 0 and d[29 - slot] == 0
        else:
            assert d[flat_slot] > 0 and d[14] == 0 and d[15] == 0
    b, e = res
    assert b["positions"][0] >= 187 and min(len(v) for v in b["ids"]) >= 20      # the RoPE rings of 64 rows wrapped, the page tables did not (40 entries, 12 pages)
    assert e["positions"] == b["positions"] and e["pools"] == b["pools"] and len(b["pools"]) > 40
    for i in range(4):
        who = f"member {min(i, 2)}" + (" after its reset" if i == 3 else "")
        _same(e["ids"][i], b["ids"][i], f"{who} ids"); _same(e["taps"][i], b["taps"][i], f"{who} logits")
        _same(e["scores"][i], b["scores"][i], f"{who} scores"); _same(e["alts"][i], b["alts"][i], f"{who} alternatives")
        assert len(b["ids"][i]) == b["taps"][i].shape[0] == len(b["scores"][i]) == len(b["alts"][i]) > 0
        assert np.isfinite(b["scores"][i]["logprob"]).all()
    for j, (x, y) in enumerate(zip(e["peek"], b["peek"])):
        _same(x, y, f"the peek's part {j}")


# ---- 5. across the window and across the table wrap -----------------------------------------------------------------------------------------------------------------------
def test_past_the_window_and_across_the_table_wrap(pkg, ctx, models):
    """One member of the GQA model from position 37 to beyond 8192 + 200 in calls of 64 ticks on pages of 64 rows, the pool the 130 pages the largest call holds
    (test_past_the_window_on_a_pool_smaller_than_the_run's shape).  The endless group's table has 130 entries: logical page 130 -- position 8320, inside the run -- is
    the first to share an entry with a page that went back.  Against the bounded paged group (max_positions 8448): ids and every tapped logits row.  The member's lists
    grow from 2048 positions by doubling to 16 384: info bytes rise by the rows x (4 + 16 + 72) bytes of it and are constant over the last 200 ticks.
    The cost of test_past_the_window_on_a_pool_smaller_than_the_run (12.8 s there); the seconds are printed."""
    m = models("gqa"); t = _t(pkg, m); W = m.config.dec_window
    assert W == 8192
    t0 = time.time()
    piece = pkg.synth.synth_audio(4.0, seed=951); gain = _gain(piece)
    per = 64 * TICK; goal = 8192 + 200
    n_calls = 0; total = 0; pos = [37]
    while pos[-1] < goal:
        n_calls += 1; total += per; pos.append(pkg.stream_schedule(total)[0])
    x = np.ascontiguousarray(np.tile(piece, total // len(piece) + 1)[:total])
    held = []
    for a, b in zip(pos, pos[1:]):
        fa, _ = pkg.stream_group_pages_for(a, 64, W); fb, nb = pkg.stream_group_pages_for(b, 64, W)
        held.append(fb + nb - fa)
    pool_pages = max(held)
    assert pool_pages == 130 and -(-pos[-1] // 64) > 130 and pos[-1] <= 8448 and 130 * 64 == 8320 < pos[-1]
    res = []
    for endless in (False, True):
        g = m.create_stream_group(t, 1, gains=[gain], page_rows=64, pool_pages=pool_pages, **({"endless": True} if endless else {"max_positions": 8448}))
        try:
            g.set_scores(0, True); g.set_alternatives(0, 3); g.tap_arm(0, pos[-1] - 37)
            ids = []; infos = [g.info(0)]
            for c in range(n_calls):
                ids.extend(g.advance({0: x[c * per:(c + 1) * per]})[0])
                infos.append(g.info(0)); assert infos[-1]["positions"] == pos[c + 1]
            p = _pool_ok(g)
            assert p["peak"] == pool_pages and p["held"] == [pkg.stream_group_pages_for(pos[-1], 64, W)[1]]      # pool() is conserved, and what pages_for says
            res.append((np.array(ids, np.int32), g.tap_fetch(0), g.scores(0)[-300:].copy(), g.alternatives(0)[-300:].copy(), infos))
        finally:
            g.close()
    (bi, bt, bs, ba, _), (ei, et, es, ea, infos) = res
    assert len(bi) == pos[-1] - 37 == bt.shape[0]
    _same(ei, bi, "ids"); _same(et, bt, "logits"); _same(es, bs, "scores"); _same(ea, ba, "alternatives")
    cap = LISTS_START
    while cap < pos[-1]:
        cap *= 2
    assert cap == 16384      # grown three times
    assert infos[-1]["bytes"] - infos[0]["bytes"] == (cap - LISTS_START) * (4 + 16 + 72), (infos[0]["bytes"], infos[-1]["bytes"])
    last = [i["bytes"] for i in infos if i["positions"] >= pos[-1] - 200]
    assert len(last) >= 4 and len(set(last)) == 1
    print(f"{n_calls} calls to position {pos[-1]}, both groups: {time.time() - t0:.1f} s")


# ---- 5b. a changed entry range that wraps: two copies ---------------------------------------------------------------------------------------------------------------------
def test_a_call_that_enters_two_pages_across_the_table_wrap_and_a_reset_of_a_wrapped_range(pkg, ctx, models):
    """group_table_upload's second copy.  The run above takes one page per call, so no changed entry range wraps there.  Here the calls have 96 ticks: the pool is the
    131 pages the largest call holds, the endless table has 131 entries, and the call from position 8293 to 8389 enters logical pages 130 and 131 -- entries 130 and
    0 -- in ONE take: a range that wraps, uploaded as two copies, both read by that call's ticks.  Then the member, whose held pages now wrap the table (release_all's
    range wraps as well), is reset and runs a 6 s clip.  Ids and tapped logits against the bounded paged group (max_positions 8704) under the same calls; pool() equal.
    A table wraps only past the window (until then a member gives nothing back), so no smaller shape reaches this; the seconds are printed."""
    m = models("gqa"); t = _t(pkg, m); W = m.config.dec_window
    assert W == 8192
    t0 = time.time()
    piece = pkg.synth.synth_audio(4.0, seed=971); gain = _gain(piece); again = pkg.synth.synth_audio(6.0, seed=972)
    per = 96 * TICK; pos = [37]; total = 0
    while pos[-1] < 8192 + 208:
        total += per; pos.append(pkg.stream_schedule(total)[0])
    n_calls = len(pos) - 1
    x = np.ascontiguousarray(np.tile(piece, total // len(piece) + 1)[:total])
    held = []
    for a, b in zip(pos, pos[1:]):
        fa, _ = pkg.stream_group_pages_for(a, 64, W); fb, nb = pkg.stream_group_pages_for(b, 64, W)
        held.append(fb + nb - fa)
    L = max(held)
    across = [(a, b) for a, b in zip(pos, pos[1:]) if -(-a // 64) <= L - 1 and -(-b // 64) >= L + 1]      # a call whose new pages include L - 1 and L: entries L - 1 and 0
    assert L == 131 and across == [(8293, 8389)] and pos[-1] <= 8704
    first, n = pkg.stream_group_pages_for(pos[-1], 64, W)
    assert first % L > (first + n - 1) % L      # at the end the held range wraps the table: the reset returns a wrapped range
    res = []
    for endless in (False, True):
        g = m.create_stream_group(t, 1, gains=[gain], page_rows=64, pool_pages=L, **({"endless": True} if endless else {"max_positions": 8704}))
        try:
            g.tap_arm(0, pos[-1] - 37); ids = []; pools = []
            for c in range(n_calls):
                ids.extend(g.advance({0: x[c * per:(c + 1) * per]})[0]); pools.append(_pool_ok(g))
                assert g.info(0)["positions"] == pos[c + 1]
            taps = g.tap_fetch(0)
            g.reset(0, _gain(again)); g.tap_arm(0, 256); pools.append(_pool_ok(g))
            assert pools[-1]["held"] == [1] and g.pages(0) == g.pages(0)[:1]
            ids2 = list(g.advance({0: again[:50000]})[0]) + list(g.advance({0: again[50000:]}, finish=[0])[0]); pools.append(_pool_ok(g))
            res.append((np.array(ids, np.int32), taps, np.array(ids2, np.int32), g.tap_fetch(0), pools))
        finally:
            g.close()
    b, e = res
    assert len(b[0]) == pos[-1] - 37 == b[1].shape[0] and len(b[2]) == b[3].shape[0] >= 30
    _same(e[0], b[0], "ids"); _same(e[1], b[1], "logits"); _same(e[2], b[2], "ids after the reset"); _same(e[3], b[3], "logits after the reset")
    assert e[4] == b[4]
    print(f"{n_calls} calls of 96 ticks to position {pos[-1]}, a reset and a 6 s clip, both groups: {time.time() - t0:.1f} s")


# ---- 6. past 16 384 ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_two_members_past_16384_positions(pkg, ctx, models):
    """The one long test: no smaller shape crosses the limit, which is the load-time RoPE tables' length, and the model's window is 8192.  An endless group of two members
    of the GQA model, pages of 64 rows, from position 37 to beyond 16 384 + 264, both members fed the same device-resident samples in the same calls of 64 ticks.
    Asserted: no call is refused; positions follow stream_schedule; ids = positions - 37; the tapped rows of the last 400 positions (they straddle 16 384) are finite and
    differ from one another; the two members -- different physical pages, different RoPE ring offsets, the same inputs -- agree bit for bit on ids and on those rows; each
    holds exactly pages_for(pos) pages at the end; info bytes are constant over the last 200 ticks.  A bounded paged group fed the same calls is refused at 16 384 with
    the session-limit message, and up to there its ids are the endless group's.
    There is NO bounded reference past the limit, so no value is compared with one there.  What stands behind the values: the two tests above (an endless group runs the
    same code path at every position, compared bit for bit below the limit), tests/test_stream_endless_cpu.py (the RoPE rows past the tables against float64: it
    goes through vox_debug_rope_rows into rope_rows_fill, whose rows are rope_row_fill's -- the function the group's per-pass fill calls for every row) and
    tests/test_gpu_attn_decode_paged_ring.py (the ring table's addresses up to position 2^24 - 1).
    About 16 700 rounds of two members and as many of the bounded group's; the seconds are printed."""
    m = models("gqa"); t = _t(pkg, m); W = m.config.dec_window; L = pkg.lib()
    assert W == 8192
    t0 = time.time()
    per = 64 * TICK; goal = 16384 + 264; n_var = 8
    base = pkg.synth.synth_audio(per * n_var / 16000.0, seed=961); gain = _gain(base)
    assert len(base) == per * n_var
    dev = C.c_void_p(); pkg._lib.check(L.vox_dev_alloc(ctx.h, base.nbytes, C.byref(dev))); pkg._lib.check(L.vox_dev_upload(ctx.h, dev, base.ctypes.data, base.nbytes))
    piece = lambda c: (dev.value + 4 * per * (c % n_var), per)      # call c's samples: device-resident, the same for both members
    pos = [37]; total = 0
    while pos[-1] < goal:
        total += per; pos.append(pkg.stream_schedule(total)[0])
    n_calls = len(pos) - 1
    arm_at = next(c for c in range(n_calls) if pos[c + 1] >= pos[-1] - 464)      # the tap is armed behind this call: it then holds more than the last 400 rows
    try:
        g = m.create_stream_group(t, 2, gains=[gain, gain], page_rows=64, pool_pages=2 * 130, endless=True)      # 130: the pages a call of 64 ticks holds past the window
        try:
            ids = [[], []]; infos = []
            for c in range(n_calls):
                out = g.advance({0: piece(c), 1: piece(c)}, device=True)      # (a refusal raises)
                ids[0].extend(out[0]); ids[1].extend(out[1])
                infos.append((g.info(0), g.info(1)))
                assert infos[-1][0]["positions"] == infos[-1][1]["positions"] == pos[c + 1]
                if c == arm_at:
                    g.tap_arm(0, 600); g.tap_arm(1, 600)
            taps = [g.tap_fetch(k)[-400:] for k in range(2)]
            p = _pool_ok(g)
            assert p["held"] == [pkg.stream_group_pages_for(pos[-1], 64, W)[1]] * 2 and set(g.pages(0)).isdisjoint(g.pages(1))
            for k in range(2):
                assert len(ids[k]) == pos[-1] - 37 and infos[-1][k]["ids"] == pos[-1] - 37
                last = [i[k]["bytes"] for i in infos if i[k]["positions"] >= pos[-1] - 200]
                assert len(last) >= 4 and len(set(last)) == 1
        finally:
            g.close()
        assert pos[-1] - 400 < 16384 < pos[-1] and taps[0].shape == (400, m.config.vocab)
        assert np.isfinite(taps[0]).all() and len({r.tobytes() for r in taps[0]}) == 400
        _same(np.array(ids[1], np.int32), np.array(ids[0], np.int32), "member 1's ids against member 0's"); _same(taps[1], taps[0], "member 1's rows against member 0's")
        t1 = time.time()
        # the contrast: a bounded paged group (max_positions 0: the session limit) under the same calls
        b = m.create_stream_group(t, 2, gains=[gain, gain], page_rows=64, pool_pages=2 * 132)
        try:
            bids = []; refused_at = None
            for c in range(n_calls):
                try:
                    bids.extend(b.advance({0: piece(c), 1: piece(c)}, device=True)[0])
                except pkg.VoxError as e:
                    refused_at = c; msg = str(e)
                    break
            assert refused_at is not None and pos[refused_at] <= 16384 < pos[refused_at + 1]
            assert e_code(msg) and "16384" in msg and "reset" in msg, msg
            assert b.info(0)["positions"] == pos[refused_at]      # nothing changed
            _same(np.array(ids[0][:len(bids)], np.int32), np.array(bids, np.int32), "ids below the limit")
        finally:
            b.close()
    finally:
        pkg._lib.check(L.vox_dev_free(ctx.h, dev))
    print(f"{n_calls} calls of two members to position {pos[-1]}: {t1 - t0:.1f} s; the bounded group to its refusal at call {refused_at}: {time.time() - t1:.1f} s")


def e_code(msg):
    return "would reach decoder position" in msg and "of a session created for" in msg


# ---- 7. the CLI ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _tekken(n=1200):
    vocab = [{"rank": i, "token_bytes": base64.b64encode(f" w{i}".encode()).decode(), "token_str": f" w{i}"} for i in range(n)]
    return {"config": {"pattern": "", "num_vocab_tokens": n, "default_vocab_size": 131072, "default_num_special_tokens": 1000, "version": "v7"}, "vocab": vocab}


def test_cli_live_group_endless_prints_the_paged_group_lines(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wavs = []
    for i, secs in enumerate((8.0, 5.0, 6.0)):
        wavs.append(str(tmp_path / f"clip{i}.wav"))
        with wave.open(wavs[-1], "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
            w.writeframes((np.clip(S.synth_audio(secs, seed=1234 + i), -1, 1) * 32767).astype("<i2").tobytes())

    def run_cli(extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok, "--live", "--live-chunk-ms", "400", "--live-group", "2"] + [a for w in wavs for a in ("--audio", w)] + extra)
        return rc, buf.getvalue(), err.getvalue()

    rc0, out0, err0 = run_cli(["--live-page-rows", "256"])
    rc1, out1, err1 = run_cli(["--live-endless"])
    assert rc0 == 0 and rc1 == 0 and out0.count("\n") == 3 and out0.strip() and out1 == out0, (out0, out1, err1)
    assert "Error in the stream group" not in err0 and "Error in the stream group" not in err1      # neither run fell back to one session per file
    lines = lambda err: [l for l in err.split("\n") if l.startswith("  [")]
    assert lines(err1) == lines(err0) and lines(err0)
    rc2, out2, err2 = run_cli(["--live-endless", "--live-page-rows", "16", "--live-pool-pages", "64"])      # the paged group's flags apply to an endless one
    assert rc2 == 0 and out2 == out0 and "Error in the stream group" not in err2
