"""Worker of tests/test_gpu_stream_group_kv.py: its tests run through pytest in a process of their own (worker_tests.run_worker) -- a bf16 group's decode attention
counts in vox_debug_attn_launches [16] .. [19], which other tests of the suite hold to 0 in their own process.  Not collected by the suite (no test_ prefix).

Paged stream groups with a bf16 K/V pool (vox_stream_group_create_kv, VOX_KV_BF16; DESIGN.md section 8 "A bf16 K/V pool") end to end on the tiny models.

What is exact and what is not.  The allocator does not know the dtype: pool() and pages() of a bf16 group equal the f32 paged group's after every call.  Rows are
rounded where they are appended and nowhere else, and layer 0's K / V rows depend on the step's input row alone: while the ids agree, the bf16 member's layer-0 rows
are the RNE-rounded rows of the f32 member, word for word (read back through session blobs, which hold f32 rows whatever the container).  A blob of a bf16 member
restored into a bf16 group continues bit for bit.  The ids and logits of a bf16 group are NOT the f32 group's: every stored value moved by up to 2^-9 of itself, and
how that propagates through the softmax and the layers above is not derived here but MEASURED, on an MI355X, as the largest |delta logit| / max(1, max |logit|) over
the rows up to each member's first differing id:

    tiny per-head model (seed 7)    3.2278e-04   (no id differs over the 158 + 65 + 40 ids of the three members)
    tiny GQA model (seed 7)         2.9919e-04   (the same)
    full-size peaked model          6.9858e-04   (6 s clip of seed 7049; no id differs over 3 x 46 ids.  Seeds 8049 .. 14049: 6.3e-04 .. 8.4e-04, no id differs;
                                                 the test's own clip, seed 11049 -- the first whose f32 reference meets _held's half rule --: 6.6436e-04)

(MEASURED below; profiles/stream_group_kv_bf16.txt, which also lists seeds 8 .. 11: 2.1e-04 .. 4.0e-04, and which of them meet _held's half rule at 4x their gap).  The tests assert 4x the larger tiny value (4x the full-size value there): the factor covers other seeds and
box-to-box differences.  The ids follow the group files' rule (stream_helpers._held) at that tolerance against the f32 paged group's ids and logits."""
import ctypes as C

import numpy as np
import pytest

import snapshot_group_cases as SG
from model_fixtures import tiny_gguf
from stream_helpers import _full_path, _gain, _held, _stop, _t

pytestmark = pytest.mark.gpu
N_SLOTS = 20
SLOT = {("head", False): 16, ("gqa", False): 17, ("head", True): 18, ("gqa", True): 19}      # (model kind, ring table) -> the bf16 form's counter slot
F32_DECODE_SLOTS = (3, 4, 5, 11, 12, 13, 14, 15)                                              # every f32 decode form: none of them may move under a bf16 group
MEASURED = {"head": 3.2278e-04, "gqa": 2.9919e-04, "full": 6.9858e-04}      # on an MI355X; see the docstring
TOL = 4 * max(MEASURED["head"], MEASURED["gqa"])
TOL_FULL = 4 * MEASURED["full"]
SEED = {"head": 7, "gqa": 7}      # tiny_gguf seeds whose f32 paged group meets _held's rule (first near-tie at or beyond half of the ids) at TOL
KW = dict(max_positions=256, page_rows=16, pool_pages=32)


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
            held[kind] = pkg.Q4ModelLoader.from_file(tiny_gguf(seed=SEED[kind], **({"dec_heads": 8} if kind == "gqa" else {}))[0]).load(ctx)
        return held[kind]
    yield get
    for m in held.values():
        m.close()


def _counts(pkg):
    a = (C.c_uint64 * N_SLOTS)()
    assert pkg.lib().vox_debug_attn_launches(a, N_SLOTS) == 0
    return [int(x) for x in a]


def _only_bf16(before, after, slot):
    d = [b - a for a, b in zip(before, after)]
    assert d[slot] > 0, d
    assert all(d[i] == 0 for i in F32_DECODE_SLOTS) and all(d[i] == 0 for i in range(16, N_SLOTS) if i != slot), d


def _state(g):
    p = dict(g.pool()); p.pop("kv_dtype", None)
    assert p["free"] + sum(p["held"]) == p["pool_pages"], p
    return p, [g.pages(k) for k in range(g.n_members)]


def _staggered(g, clips, starts, step=3200, after=None):
    """Member k starts in call starts[k], is fed `step` samples per call and finishes with its last piece -> the ids per member.  after(g, call): a hook behind each call."""
    n = len(clips); ids = [[] for _ in range(n)]; c = 0
    while True:
        feeds = {}; fin = []
        for k in range(n):
            i = c - starts[k]
            if i >= 0 and i * step < len(clips[k]):
                feeds[k] = clips[k][i * step:(i + 1) * step]
                if (i + 1) * step >= len(clips[k]):
                    fin.append(k)
        if not feeds and c > max(starts):
            break
        for k, v in g.advance(feeds, finish=fin).items():
            ids[k].extend(v)
        if after:
            after(g, c)
        c += 1
    return [np.array(v, np.int32) for v in ids]


def _clips3(pkg):
    return [pkg.synth.synth_audio(s, seed=910 + i) for i, s in enumerate((24.0, 9.0, 5.0))]


def _run3(pkg, m, kv_dtype, blob_at=None):
    """The three staggered members (24 s, 9 s, 5 s) on a paged group of the given dtype (None: vox_stream_group_create_paged) -> ids, taps, the state after every
    call and, with blob_at = c, member 0's blob behind call c."""
    t = _t(pkg, m); clips = _clips3(pkg)
    g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], **KW, **({"kv_dtype": kv_dtype} if kv_dtype else {}))
    states = []; blob = {}
    try:
        p0 = g.pool()
        assert ("kv_dtype" in p0) == (kv_dtype is not None) and p0.get("kv_dtype", kv_dtype) == kv_dtype
        for k in range(3):
            g.tap_arm(k, 256)

        def after(g, c):
            states.append(_state(g))
            if c == blob_at:
                blob[0] = g.snapshot(0); blob["pos"] = g.info(0)["positions"]; blob["ids"] = g.info(0)["ids"]
        ids = _staggered(g, clips, (0, 2, 5), after=after)
        taps = [g.tap_fetch(k) for k in range(3)]
        nbytes = g.info(0)["bytes"]
    finally:
        g.close()
    return dict(ids=ids, taps=taps, states=states, blob=blob, bytes=nbytes)


_F32 = {}      # kind -> the f32 paged group's run: computed once per model, read-only


def _f32_run(pkg, m, kind):
    if kind not in _F32:
        r = _run3(pkg, m, None, blob_at=8)
        for a in r["ids"] + r["taps"]:
            a.setflags(write=False)
        _F32[kind] = r
    return _F32[kind]


def _logit_gap(ids, taps, rids, rtaps):
    """-> (the largest |delta logit| / max(1, max |logit|) over the rows up to each member's first differing id, those first indices)"""
    worst = 0.0; firsts = []
    for a, la, b, lb in zip(ids, taps, rids, rtaps):
        assert len(a) == len(b) == la.shape[0] == lb.shape[0] > 0
        diff = np.flatnonzero(a != b); n = int(diff[0]) + 1 if len(diff) else len(a)      # the row behind the first differing id saw the same ids: it still compares
        firsts.append(int(diff[0]) if len(diff) else None)
        worst = max(worst, float(np.abs(la[:n].astype(np.float64) - lb[:n]).max() / max(1.0, float(np.abs(lb[:n]).max()))))
    return worst, firsts


# ---- 1. against the f32 paged group ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head", "gqa"])
def test_bf16_group_against_the_f32_paged_group(pkg, ctx, models, kind):
    m = models(kind)
    assert (m.config.dec_heads == 4 * m.config.dec_kv_heads) == (kind == "gqa")
    ref = _f32_run(pkg, m, kind)
    c0 = _counts(pkg)
    got = _run3(pkg, m, "bf16")
    c1 = _counts(pkg)
    _only_bf16(c0, c1, SLOT[(kind, False)])
    assert got["states"] == ref["states"]      # pool() and pages(member) after every call: the allocator does not know the dtype
    assert any(b != a + 1 for _, pages in got["states"] for p in pages for a, b in zip(p, p[1:]))      # the members interleave their pages
    gap, firsts = _logit_gap(got["ids"], got["taps"], ref["ids"], ref["taps"])
    print(f"MEASURED {kind} {gap:.6e} first differing ids {firsts} of {[len(v) for v in ref['ids']]}")
    assert gap <= TOL, (gap, TOL)
    assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got["taps"], ref["taps"]))      # (a bf16 group is not the f32 group: the rows did move)
    for k in range(3):
        _held(got["ids"][k], ref["ids"][k], ref["taps"][k], f"{kind} member {k}", TOL)
    # the pool's memory: K and V halve, nothing else changes -- a member's share of the group's bytes drops by half the f32 pool's
    c = m.config; pool_f32 = 2 * c.dec_layers * KW["pool_pages"] * c.dec_kv_heads * KW["page_rows"] * c.dec_head_dim * 4
    assert abs((ref["bytes"] - got["bytes"]) * 3 - pool_f32 // 2) <= 3, (ref["bytes"], got["bytes"], pool_f32)


# ---- 2. layer 0: rows are rounded at the append (and the seed) and nowhere else ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head", "gqa"])
def test_layer0_rows_are_the_rounded_rows_of_the_f32_member(pkg, ctx, models, kind):
    m = models(kind); c = m.config
    ref = _f32_run(pkg, m, kind); got = _run3(pkg, m, "bf16", blob_at=8)
    fb, bb = ref["blob"], got["blob"]
    assert fb["pos"] == bb["pos"] > 48 and fb["ids"] == bb["ids"] > 0
    n = fb["ids"]
    assert np.array_equal(got["ids"][0][:n], ref["ids"][0][:n])      # the premise: the two members have emitted the same ids so far
    fi, bi = pkg.snapshot_info(fb[0]), pkg.snapshot_info(bb[0])
    assert fi["section_bytes"] == bi["section_bytes"] and fi["section_offset"] == bi["section_offset"] and len(fb[0]) == len(bb[0])      # the blob does not know its container
    D = fi["dec_rows"]
    assert 48 < D <= fb["pos"] and fi["section_bytes"][2] == c.dec_layers * c.dec_kv_heads * D * c.dec_head_dim * 4
    for sec in (2, 3):      # SEC_DEC_K, SEC_DEC_V: [layer][kv head][row][head_dim] f32
        o, nb = fi["section_offset"][sec], fi["section_bytes"][sec]
        f = fb[0][o:o + nb].view(np.uint32).reshape(c.dec_layers, c.dec_kv_heads, D, c.dec_head_dim)
        b = bb[0][o:o + nb].view(np.uint32).reshape(c.dec_layers, c.dec_kv_heads, D, c.dec_head_dim)
        assert not (b & 0xFFFF).any()      # every word of the bf16 member is a widened 16-bit value: rows were rounded
        assert (f & 0xFFFF).any()
        want = pkg.gguf.kv_round_bf16(f[0].view(np.float32)).astype(np.uint32) << 16
        assert np.array_equal(b[0], want), np.argwhere(b[0] != want)[:4].tolist()      # layer 0, the 37 seed rows included: exactly the rounded f32 rows
        if c.dec_layers > 1:      # (the layers above read rounded rows: theirs are close, not the rounded f32 rows)
            assert not np.array_equal(b[1], pkg.gguf.kv_round_bf16(f[1].view(np.float32)).astype(np.uint32) << 16)


# ---- 3. snapshot and resume --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["head", "gqa"])
def test_snapshot_reset_restore_of_a_bf16_member_continues_bit_for_bit(pkg, ctx, models, kind):
    """The same-slot case of the snapshot tests (snapshot_group_cases.run_group: member 1 snapshotted, reset and restored behind a call) on a bf16 paged group, behind
    call 18 -- position 60: ids per call, logits rows, records, pool() and pages held after every call equal the uninterrupted bf16 group's."""
    SG.KINDS["paged_bf16"] = dict(max_positions=256, page_rows=16, pool_pages=48, kv_dtype="bf16")
    m = models(kind); clips = SG.group_clips(pkg)
    c0 = _counts(pkg)
    a = SG.run_group(pkg, m, "paged_bf16", clips); b = SG.run_group(pkg, m, "paged_bf16", clips, suspend_after=18)
    _only_bf16(c0, _counts(pkg), SLOT[(kind, False)])
    assert sum(len(v) for v in a["ids"][1][19:]) >= 20      # the restored member has most of its utterance ahead
    for k in range(3):
        for c, (u, v) in enumerate(zip(b["ids"][k], a["ids"][k])):
            assert np.array_equal(u, v), f"member {k}, call {c}: {u}, the uninterrupted group's {v}"
        assert a["taps"][k].shape == b["taps"][k].shape and np.array_equal(a["taps"][k].view(np.uint32), b["taps"][k].view(np.uint32)), f"member {k}'s logits rows differ"
    assert a["rec"].tobytes() == b["rec"].tobytes() and a["alt"].tobytes() == b["alt"].tobytes()
    assert a["pools"] == b["pools"] and a["words"] == b["words"]      # pool() and the pages held per member, vox_stream_group_info words 0-4, after every call
    info = pkg.snapshot_info(b["blob"])
    assert 57 <= info["positions"] <= 63, info["positions"]      # position 60: member 1 is at 49 behind call 9 (snapshot_group_cases.same_slot_case) and every call of 3200 samples is 1.25 ticks of 2560
    o, nb = info["section_offset"][2], info["section_bytes"][2]
    assert not (b["blob"][o:o + nb].view(np.uint32) & 0xFFFF).any()


def test_endless_bf16_member_resumes_behind_the_table_wrap(pkg, ctx, models):
    """One member of the GQA model on an ENDLESS bf16 group, pages of 64 rows, a pool -- and so a table ring -- of 130 entries: 130 calls of 64 ticks take it to
    position 8357, logical page 130 = ring entry 0 (the ring has wrapped, the window has moved).  There it is snapshotted; one more call gives the uninterrupted tail.
    Then the member is reset and restored from the blob and runs the same call again: ids, logits rows and pool() equal the uninterrupted tail's, bit for bit."""
    m = models("gqa"); t = _t(pkg, m); W = m.config.dec_window
    assert W == 8192
    piece = pkg.synth.synth_audio(4.0, seed=951); gain = _gain(piece)
    per = 64 * 2560; n_calls = 131
    x = np.ascontiguousarray(np.tile(piece, n_calls * per // len(piece) + 1)[:n_calls * per])
    c0 = _counts(pkg)
    g = m.create_stream_group(t, 1, gains=[gain], page_rows=64, pool_pages=130, endless=True, kv_dtype="bf16")
    try:
        for c in range(n_calls - 1):
            g.advance({0: x[c * per:(c + 1) * per]})
        at = g.info(0)["positions"]
        assert at == pkg.stream_schedule((n_calls - 1) * per)[0] and at // 64 >= 130 and at - W > 64      # entry (at // 64) % 130 == 0: wrapped; the window's first page is not page 0 any more
        pool_at = g.pool()
        blob = g.snapshot(0)
        assert g.pool() == pool_at and g.info(0)["positions"] == at
        last = x[(n_calls - 1) * per:]
        g.tap_arm(0, 64)
        ids = g.advance({0: last})[0]; rows = g.tap_fetch(0); pool_end = g.pool(); words = g.info(0)
        assert len(ids) == 64 == rows.shape[0]
        g.reset(0, gain=0.5)
        assert g.pool()["held"] == [1]
        g.restore(0, blob)
        assert g.pool() == pool_at and g.info(0)["positions"] == at
        g.tap_arm(0, 64)
        ids2 = g.advance({0: last})[0]; rows2 = g.tap_fetch(0)
        assert np.array_equal(ids2, ids) and np.array_equal(rows2.view(np.uint32), rows.view(np.uint32))
        five = ("samples", "positions", "ids", "encoder_position", "ring_rows")      # vox_stream_group_info words 0-4 (the step counter restarts with the restored session)
        assert g.pool() == pool_end and [g.info(0)[w] for w in five] == [words[w] for w in five]
        assert pool_end["kv_dtype"] == "bf16" and pool_end["peak"] == 130
    finally:
        g.close()
    _only_bf16(c0, _counts(pkg), SLOT[("gqa", True)])


# ---- 4. reset and reuse, a refused call, a peek, the records ---------------------------------------------------------------------------------------------------------------
def test_reset_and_reuse_leave_nothing_behind(pkg, ctx, models):
    """Member 0 runs clip a, is reset and runs clip b in the pages it gave back; a fresh bf16 group runs clip b alone: the same ids and logits rows (no stale row is read),
    and the pool's states along the way are the f32 paged group's under the same calls."""
    m = models("head"); t = _t(pkg, m)
    a, b = pkg.synth.synth_audio(3.0, seed=921), pkg.synth.synth_audio(4.0, seed=922)

    def feed(g, x, states=None):
        ids = []
        for o in range(0, len(x), 3200):
            ids.extend(g.advance({0: x[o:o + 3200]}, finish=[0] if o + 3200 >= len(x) else [])[0])
            if states is not None:
                states.append(_state(g))
        return np.array(ids, np.int32)
    res = {}
    for name, kv in (("f32", None), ("bf16", "bf16")):
        g = m.create_stream_group(t, 2, gains=[_gain(a), 1.0], max_positions=256, page_rows=16, pool_pages=24, **({"kv_dtype": kv} if kv else {}))
        try:
            states = []
            feed(g, a, states); was = g.pages(0)
            g.reset(0, _gain(b)); states.append(_state(g))
            assert g.pages(0) == was[::-1][:3]      # LIFO: the seed sits in the pages returned last
            g.tap_arm(0, 256)
            ids = feed(g, b, states); res[name] = (ids, g.tap_fetch(0), states)
        finally:
            g.close()
    assert res["bf16"][2] == res["f32"][2]
    g = m.create_stream_group(t, 2, gains=[_gain(b), 1.0], max_positions=256, page_rows=16, pool_pages=24, kv_dtype="bf16")
    try:
        g.tap_arm(0, 256)
        ids = feed(g, b); rows = g.tap_fetch(0)
    finally:
        g.close()
    assert np.array_equal(res["bf16"][0], ids) and np.array_equal(res["bf16"][1].view(np.uint32), rows.view(np.uint32))


def test_a_refused_call_leaves_pool_and_tables_untouched(pkg, ctx, models):
    m = models("head"); t = _t(pkg, m); x = pkg.synth.synth_audio(6.0, seed=931)
    for kw, needle in [({"page_rows": 48}, "page_rows"), ({"page_rows": 16, "pool_pages": 5}, "pool"), ({"page_rows": 16, "max_positions": 1 << 20}, "max_positions")]:
        with pytest.raises(pkg.VoxError, match=needle):      # the f32 paged group's refusals
            m.create_stream_group(t, 2, kv_dtype="bf16", **kw)
    f = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=256, page_rows=16, pool_pages=8)
    g = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=256, page_rows=16, pool_pages=8, kv_dtype="bf16")
    try:
        first = {0: x[:2560 * 30]}
        f.advance(first); g.advance(first)
        assert g.info(0)["positions"] > 64 and _state(g) == _state(f) and g.pool()["free"] == 0
        state = lambda: ([g.info(k) for k in range(2)], g.pool(), [g.pages(k) for k in range(2)])
        before = state(); call = {1: x[:2560 * 20]}
        for _ in range(2):      # ... and again: the refused call changed nothing
            with pytest.raises(pkg.VoxError, match="pool") as ei:
                g.advance(call)
            assert "member 1" in str(ei.value) and " 0 are free" in str(ei.value), str(ei.value)
            assert state() == before
        g.reset(0, _gain(x)); f.reset(0, _gain(x))
        g.advance(call); f.advance(call)
        assert _state(g) == _state(f)
    finally:
        g.close(); f.close()


def test_a_peek_leaves_the_group_what_it_was(pkg, ctx, models):
    m = models("head"); t = _t(pkg, m); x = pkg.synth.synth_audio(8.0, seed=941); y = pkg.synth.synth_audio(5.0, seed=942)
    n0 = 2560 * 20 + 40
    res = []
    for peek in (False, True):
        g = m.create_stream_group(t, 2, gains=[_gain(x), _gain(y)], max_positions=256, page_rows=16, pool_pages=20, kv_dtype="bf16")
        try:
            for k in range(2):
                g.tap_arm(k, 256)
            ids = [list(v) for v in g.advance({0: x[:n0], 1: y[:n0 // 2]}).values()]
            pos = g.info(0)["positions"]
            assert pos % 16 >= 8      # the 8-to-10-tick tail of a peek enters the next page
            pk = None
            if peek:
                info = lambda k: {a: b for a, b in g.info(k).items() if a != "bytes"}      # (the peek's save area is the group's from the first peek on)
                state = lambda: (g.pool(), [g.pages(k) for k in range(2)], [info(k) for k in range(2)])
                before = state()
                pk = g.peek([0])[0]
                assert len(pk) >= 8 and state() == before
                assert (pos + len(pk) - 1) // 16 > (pos - 1) // 16      # the tail did enter a page the member does not hold
            out = g.advance({0: x[n0:], 1: y[n0 // 2:]}, finish=[0, 1])
            ids[0].extend(out[0]); ids[1].extend(out[1])
            res.append((pk, [np.array(v, np.int32) for v in ids], [g.tap_fetch(k) for k in range(2)]))
        finally:
            g.close()
    for k in range(2):      # the rows the peek's ticks wrote into borrowed pages are gone: what follows is the unpeeked group's, bit for bit
        assert np.array_equal(res[1][1][k], res[0][1][k]) and np.array_equal(res[1][2][k].view(np.uint32), res[0][2][k].view(np.uint32)), k


def test_scores_and_alternatives_are_functions_of_the_tapped_row(pkg, ctx, models):
    m = models("gqa"); t = _t(pkg, m); x = pkg.synth.synth_audio(6.0, seed=961)
    g = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=256, page_rows=16, pool_pages=24, kv_dtype="bf16")
    try:
        g.set_scores(1, True); g.set_alternatives(1, 3); g.tap_arm(1, 256)
        ids = []
        for o in range(0, len(x), 6400):
            ids.extend(g.advance({0: x[o:o + 6400], 1: x[o:o + 6400]}, finish=[0, 1] if o + 6400 >= len(x) else []).get(1, []))
        ids = np.array(ids, np.int32); rows = g.tap_fetch(1); rec = g.scores(1); alt = g.alternatives(1)
    finally:
        g.close()
    assert len(ids) == rows.shape[0] == len(rec) == len(alt) >= 40
    assert np.array_equal(rec["id"], ids)
    want = pkg.score_rows(ctx, rows, ids); walt = pkg.alternatives_rows(ctx, rows, 3)
    assert rec.tobytes() == want.tobytes() and alt.tobytes() == walt.tobytes()


# ---- 5. full size ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_full_size_three_members_against_the_f32_paged_group(pkg, ctx):
    """Three members fed the same 6 s clip, staggered.  The clip is chosen by the f32 paged group ALONE, as test_gpu_stream_group._clip chooses its clips: the seed
    moves on from 7049 until the first near-tie of every member's f32 logits (stream_helpers._stop at TOL_FULL) lies at or beyond half of its ids -- with seed 7049
    itself it lies at id 2 of 46, and such a clip cannot carry an ids claim.  The bf16 group then runs on that clip."""
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    try:
        t = _t(pkg, m); c = m.config
        assert c.dec_heads == 4 * c.dec_kv_heads

        def run(kv, x):
            g = m.create_stream_group(t, 3, gains=[_gain(x)] * 3, max_positions=256, page_rows=32, **({"kv_dtype": kv} if kv else {}))
            try:
                for k in range(3):
                    g.tap_arm(k, 128)
                states = []
                c0 = _counts(pkg)
                ids = _staggered(g, [x, x, x], (0, 1, 3), step=2560 * 4, after=lambda g, c: states.append(_state(g)))
                c1 = _counts(pkg)
                if kv:
                    _only_bf16(c0, c1, SLOT[("gqa", False)])
                else:
                    assert c1[12] > c0[12] and c1[16:] == c0[16:]
                return dict(ids=ids, taps=[g.tap_fetch(k) for k in range(3)], states=states, bytes=g.info(0)["bytes"], pool=g.pool())
            finally:
                g.close()
        for seed in range(7049, 7049 + 16 * 1000, 1000):
            x = pkg.synth.synth_audio(6.0, seed=seed); f = run(None, x)
            stops = [_stop(lg, TOL_FULL) for lg in f["taps"]]
            if all(2 * st >= len(v) for st, v in zip(stops, f["ids"])):
                break
            print(f"clip seed {seed}: the f32 group's first near-ties at {stops} of {[len(v) for v in f['ids']]} ids: another seed")
        else:
            raise AssertionError("no clip seed from 7049 on gives an f32 reference that can carry an ids claim at TOL_FULL")
        b = run("bf16", x)
        assert 25 <= len(f["ids"][0]) <= 60, len(f["ids"][0])      # about 40 ticks each
        assert b["states"] == f["states"]
        gap, firsts = _logit_gap(b["ids"], b["taps"], f["ids"], f["taps"])
        print(f"MEASURED full {gap:.6e} (clip seed {seed}) first differing ids {firsts} of {[len(v) for v in f['ids']]}")
        assert gap <= TOL_FULL, (gap, TOL_FULL)
        for k in range(3):
            _held(b["ids"][k], f["ids"][k], f["taps"][k], f"full-size member {k}", TOL_FULL)
        pool_f32 = 2 * c.dec_layers * f["pool"]["pool_pages"] * c.dec_kv_heads * 32 * c.dec_head_dim * 4      # K and V: [layer][page][kv head][32 rows][128] f32
        assert abs((f["bytes"] - b["bytes"]) * 3 - pool_f32 // 2) <= 3, (f["bytes"], b["bytes"], pool_f32)      # info word [5]: half the pool
    finally:
        m.close()
