"""Paged stream groups (vox_stream_group_create_paged, DESIGN.md section 8 "Paged decoder cache"): the members of a group grow into one pool of K / V pages.

The reference of every claim here is the SLAB group of the same build, driven by the identical sequence of calls: every round then has the same width and picks the same
GEMM kernels, and the paged attention reads the same rows in the same order through its page table.  So the claim is bit for bit -- np.array_equal on the ids and on
the tapped logits rows, no tolerance anywhere in this file.  Beside it: which attention form ran (the launch counters), the pool's conservation law after every call
(free + held == pool_pages), LIFO reuse after a reset, the refusals (nothing changed, the call can be repeated), a peek that borrows pages, and a run past the sliding
window on a pool smaller than the run's logical pages."""
import ctypes as C
import os

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _full_path, _gain, _t

pytestmark = pytest.mark.gpu
ATTN_FORMS = ("prefill_small", "prefill_mfma", "prefill_f32", "decode", "decode_spec", "decode_gqa", "attn_wo", "engine", "stream_ring", "group_resample", "stream_resample",
              "decode_paged", "decode_gqa_paged")


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


def _attn(pkg):
    a = (C.c_uint64 * len(ATTN_FORMS))()
    assert pkg.lib().vox_debug_attn_launches(a, len(ATTN_FORMS)) == 0
    return dict(zip(ATTN_FORMS, map(int, a)))


def _pool_ok(g):
    p = g.pool()
    assert p["free"] + sum(p["held"]) == p["pool_pages"], p
    for k, h in enumerate(p["held"]):
        assert len(g.pages(k)) == h
    every = [q for k in range(g.n_members) for q in g.pages(k)]
    assert len(set(every)) == len(every) and all(0 <= q < p["pool_pages"] for q in every)      # no page in two tables
    return p


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


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(a, b), f"{what}: differs from the slab group's at {np.argwhere(a != b)[:4].tolist() if a.shape == b.shape else (a.shape, b.shape)}"


# ---- 1 + 2. both attention forms, three members interleaving their pages ------------------------------------------------------------------------------------------------
_SLAB3 = {}      # kind -> (clips, ids, taps) of the slab group: computed once per model, read-only


def _slab3(pkg, m, kind):
    if kind not in _SLAB3:
        t = _t(pkg, m); clips = [pkg.synth.synth_audio(s, seed=910 + i) for i, s in enumerate((24.0, 9.0, 5.0))]
        g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], max_positions=256)
        try:
            for k in range(3):
                g.tap_arm(k, 256)
            ids = _staggered(g, clips, (0, 2, 5)); taps = [g.tap_fetch(k) for k in range(3)]
        finally:
            g.close()
        for a in clips + ids + taps:
            a.setflags(write=False)
        _SLAB3[kind] = (clips, ids, taps)
    return _SLAB3[kind]


@pytest.mark.parametrize("kind,form,other", [("head", "decode_paged", "decode"), ("gqa", "decode_gqa_paged", "decode_gqa")])
def test_paged_group_equals_the_slab_group_bit_for_bit(pkg, ctx, models, kind, form, other):
    m = models(kind); t = _t(pkg, m)
    assert (m.config.dec_heads == 4 * m.config.dec_kv_heads) == (kind == "gqa")
    clips, rids, rtaps = _slab3(pkg, m, kind)
    g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], max_positions=256, page_rows=16, pool_pages=32)
    scattered = []
    try:
        assert g.pool() == {"page_rows": 16, "pool_pages": 32, "free": 32 - 9, "peak": 9, "held": [3, 3, 3]}      # the 37 prefix rows: three pages of 16 each
        for k in range(3):
            g.tap_arm(k, 256)

        def after(g, c):
            _pool_ok(g)
            for k in range(3):
                p = g.pages(k)
                scattered.append(any(b != a + 1 for a, b in zip(p, p[1:])))
        a0 = _attn(pkg)
        ids = _staggered(g, clips, (0, 2, 5), after=after)
        a1 = _attn(pkg)
        taps = [g.tap_fetch(k) for k in range(3)]
        end = g.info(0)["positions"]
        assert end >= 187      # the 24 s member (187 with its last sample, its right pad behind): its 160 prefetched keys and the loop behind them both cross page boundaries
        assert g.pool()["held"][0] == -(-end // 16) >= 12
    finally:
        g.close()
    d = {k: a1[k] - a0[k] for k in a1 if a1[k] != a0[k]}
    print(f"{kind}: attention launches of the paged run {d}")
    assert d.get(form, 0) > 0 and other not in d and not {"decode", "decode_gqa", "decode_spec"} & set(d)
    assert any(scattered)      # the members interleave their allocations: some member's physical pages are not one run
    for k in range(3):
        _same(ids[k], rids[k], f"member {k} ids"); _same(taps[k], rtaps[k], f"member {k} logits")
        assert len(ids[k]) == taps[k].shape[0] > 0


# ---- 3. reset and reuse ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_reset_returns_the_pages_and_the_next_allocation_reuses_them(pkg, ctx, models):
    m = models("head"); t = _t(pkg, m)
    a, b = pkg.synth.synth_audio(3.0, seed=921), pkg.synth.synth_audio(4.0, seed=922); others = [pkg.synth.synth_audio(6.0, seed=923 + j) for j in range(2)]

    def run(g, paged):
        clips = [a, others[0], others[1]]; off = [0, 0, 0]; ids = [[], [], []]; first = None; seen = {}
        for k in range(3):
            g.tap_arm(k, 256)
        while any(off[k] < len(clips[k]) for k in range(3)):
            feeds = {k: clips[k][off[k]:off[k] + 3200] for k in range(3) if off[k] < len(clips[k])}
            fin = [k for k in feeds if off[k] + 3200 >= len(clips[k])]
            had = {k: g.pages(k) for k in range(3)} if paged else None
            for k, v in g.advance(feeds, finish=fin).items():
                ids[k].extend(v); off[k] += 3200
            if paged:
                _pool_ok(g)
                if "returned" in seen:      # the pages taken since the reset, in the order of their taking (entries are served in member order)
                    seen["taken"] += [(k, q) for k in range(3) for q in g.pages(k) if q not in had[k]]
            if 0 in fin and first is None:
                first = np.array(ids[0], np.int32); ids[0] = []; off[0] = 0; clips[0] = b
                if paged:
                    was = g.pages(0); free = g.pool()["free"]
                g.reset(0, _gain(b))
                if paged:
                    now = g.pages(0); p = _pool_ok(g)
                    assert len(was) > 3 and len(now) == 3 and p["free"] == free + len(was) - 3
                    assert now == was[::-1][:3]      # LIFO: the seed sits in the pages returned last
                    seen["returned"] = [q for q in was if q not in now]; seen["taken"] = []
        if paged:
            taken = seen["taken"]; back = seen["returned"][::-1]      # the stack above what the group never used: the returned pages, the last one on top
            assert any(k != 0 for k, _ in taken), taken
            assert [q for _, q in taken][:len(back)] == back[:len(taken)]      # every page taken next -- by the other members as well -- is a returned one, top first
        return [first] + [np.array(v, np.int32) for v in ids], [g.tap_fetch(k) for k in range(3)]
    gains = [_gain(a)] + [_gain(o) for o in others]
    res = []
    for paged in (False, True):
        g = m.create_stream_group(t, 3, gains=gains, max_positions=256, **({"page_rows": 16, "pool_pages": 24} if paged else {}))
        try:
            res.append(run(g, paged))
        finally:
            g.close()
    for i, (x, y) in enumerate(zip(res[1][0], res[0][0])):
        _same(x, y, f"ids list {i}")
    for k in range(3):
        _same(res[1][1][k], res[0][1][k], f"member {k} logits")      # member 0: the second clip's rows (its reset restarts the tap's count)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_pool_and_tables_untouched(pkg, ctx, models):
    m = models("head"); t = _t(pkg, m); x = pkg.synth.synth_audio(6.0, seed=931)
    for kw, needle in [({"page_rows": 48}, "page_rows"), ({"page_rows": 8}, "page_rows"), ({"page_rows": 2048}, "page_rows"), ({"page_rows": 16, "pool_pages": 5}, "pool"),
                       ({"page_rows": 16, "max_positions": 1 << 20}, "max_positions")]:
        with pytest.raises(pkg.VoxError, match=needle):
            m.create_stream_group(t, 2, **kw)
    slab = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=256)
    g = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=256, page_rows=16, pool_pages=8)
    try:
        with pytest.raises(pkg.VoxError, match="pool") as ei:
            slab.pool()
        assert ei.value.code == 5      # VOX_ERR_UNSUPPORTED
        first = {0: x[:2560 * 30]}
        r0 = slab.advance(first)[0]; _same(g.advance(first)[0], r0, "member 0")
        assert g.info(0)["positions"] > 64 and g.pool()["free"] == 0 and g.pool()["held"] == [5, 3]
        state = lambda: ([g.info(k) for k in range(2)], g.pool(), [g.pages(k) for k in range(2)])
        before = state(); call = {1: x[:2560 * 20]}
        with pytest.raises(pkg.VoxError, match="pool") as ei:
            g.advance(call)
        assert "member 1" in str(ei.value) and " 1 new" in str(ei.value) and " 0 are free" in str(ei.value), str(ei.value)
        assert state() == before
        with pytest.raises(pkg.VoxError, match="pool"):      # ... and again: the refused call changed nothing
            g.advance(call)
        assert state() == before
        g.reset(0, _gain(x)); slab.reset(0, _gain(x))
        assert g.pool()["free"] == 2
        _same(g.advance(call)[1], slab.advance(call)[1], "member 1 after the other member's reset")
        _pool_ok(g)
    finally:
        g.close(); slab.close()


# ---- 5. peek ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_peek_borrows_pages_and_returns_them(pkg, ctx, models):
    m = models("head"); t = _t(pkg, m); x = pkg.synth.synth_audio(8.0, seed=941); y = pkg.synth.synth_audio(5.0, seed=942)
    n0 = 2560 * 20 + 40
    res = []
    for paged in (False, True):
        g = m.create_stream_group(t, 2, gains=[_gain(x), _gain(y)], max_positions=256, **({"page_rows": 16, "pool_pages": 20} if paged else {}))
        try:
            for k in range(2):
                g.tap_arm(k, 256)
            ids = [list(v) for v in g.advance({0: x[:n0], 1: y[:n0 // 2]}).values()]
            pos = g.info(0)["positions"]
            assert pos % 16 >= 8      # the 8-to-10-tick tail of a peek enters the next page
            if paged:
                info = lambda k: {a: b for a, b in g.info(k).items() if a != "bytes"}      # (the peek's save area is the group's from the first peek on, as a slab group's)
                state = lambda: (g.pool(), [g.pages(k) for k in range(2)], [info(k) for k in range(2)])
                before = state()
            pk = g.peek([0])[0]
            assert len(pk) >= 8
            if paged:
                assert state() == before
                assert (pos + len(pk) - 1) // 16 > (pos - 1) // 16      # the tail did enter a page the member does not hold
            for a, b in ((n0, len(x)), ):
                out = g.advance({0: x[a:b], 1: y[n0 // 2:]}, finish=[0, 1])
                ids[0].extend(out[0]); ids[1].extend(out[1])
            res.append((pk, [np.array(v, np.int32) for v in ids], [g.tap_fetch(k) for k in range(2)]))
        finally:
            g.close()
    _same(res[1][0], res[0][0], "the peek's ids")
    for k in range(2):
        _same(res[1][1][k], res[0][1][k], f"member {k} ids after the peek"); _same(res[1][2][k], res[0][2][k], f"member {k} logits after the peek")
    # an empty pool: the member holds every page, its peek's tail needs one more
    g = m.create_stream_group(t, 1, gains=[_gain(x)], max_positions=256, page_rows=16, pool_pages=4)
    try:
        g.advance({0: x[:n0]})
        assert g.pool()["free"] == 0 and g.info(0)["positions"] % 16 >= 8
        before = (g.pool(), g.pages(0), g.info(0))
        with pytest.raises(pkg.VoxError, match="pool"):
            g.peek([0])
        assert (g.pool(), g.pages(0), g.info(0)) == before
    finally:
        g.close()


# ---- 6. past 2048, across the window, with recycling --------------------------------------------------------------------------------------------------------------------
def test_past_the_window_on_a_pool_smaller_than_the_run(pkg, ctx, models):
    """One member of the GQA model runs from position 37 to beyond 8192 + 200 in calls of 64 ticks on pages of 64 rows.  The pool has exactly the pages the largest call
    holds (vox_stream_group_pages_for over the run: 130), fewer than the run's 132 logical pages, so the run finishes only by reusing pages that left the window.
    About 16 800 tiny rounds over both groups: 12.8 s measured on an MI355X (the clip's synthesis and the 86 MB of samples included)."""
    m = models("gqa"); t = _t(pkg, m); W = m.config.dec_window
    assert W == 8192
    piece = pkg.synth.synth_audio(4.0, seed=951); gain = _gain(piece)
    per = 64 * 2560; goal = 8192 + 200
    n_calls = 0; total = 0; pos = [37]
    while pos[-1] < goal:
        n_calls += 1; total += per; pos.append(pkg.stream_schedule(total)[0])
    x = np.ascontiguousarray(np.tile(piece, total // len(piece) + 1)[:total])
    held = []
    for a, b in zip(pos, pos[1:]):      # during a call from a to b the member holds the pages of a's window up to b's last page
        fa, _ = pkg.stream_group_pages_for(a, 64, W); fb, nb = pkg.stream_group_pages_for(b, 64, W)
        held.append(fb + nb - fa)
    pool_pages = max(held); logical = -(-pos[-1] // 64)
    print(f"{n_calls} calls to position {pos[-1]}: pool of {pool_pages} pages for {logical} logical pages")
    assert pool_pages == 130 and logical == 132 and pool_pages < logical and pos[-1] <= 8448
    res = []
    for paged in (False, True):
        g = m.create_stream_group(t, 1, gains=[gain], max_positions=8448, **({"page_rows": 64, "pool_pages": pool_pages} if paged else {}))
        try:
            g.tap_arm(0, pos[-1] - 37)
            ids = []
            for c in range(n_calls):
                ids.extend(g.advance({0: x[c * per:(c + 1) * per]})[0])
                assert g.info(0)["positions"] == pos[c + 1]
            if paged:
                p = _pool_ok(g)
                assert p["peak"] == pool_pages and p["held"] == [list(pkg.stream_group_pages_for(pos[-1], 64, W))[1]]
                assert len(set(g.pages(0))) == p["held"][0]
            res.append((np.array(ids, np.int32), g.tap_fetch(0)))
        finally:
            g.close()
    assert len(res[0][0]) == pos[-1] - 37 == res[0][1].shape[0]
    _same(res[1][0], res[0][0], "ids"); _same(res[1][1], res[0][1], "logits")


# ---- 7. full size -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_full_size_three_members_equal_the_slab_group(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    try:
        x = pkg.synth.synth_audio(16.0, seed=7049); t = _t(pkg, m)
        assert m.config.dec_heads == 4 * m.config.dec_kv_heads
        res = []
        for paged in (False, True):
            g = m.create_stream_group(t, 3, gains=[_gain(x)] * 3, max_positions=256, **({"page_rows": 32} if paged else {}))
            try:
                g.tap_arm(1, 128)
                a0 = _attn(pkg)
                ids = _staggered(g, [x, x, x], (0, 1, 3), step=2560 * 4, after=(lambda g, c: _pool_ok(g)) if paged else None)
                a1 = _attn(pkg)
                res.append((ids, g.tap_fetch(1)))
                assert (a1["decode_gqa_paged"] > a0["decode_gqa_paged"]) == paged and (a1["decode_gqa"] > a0["decode_gqa"]) == (not paged)
            finally:
                g.close()
        assert len(res[0][0][0]) == 108
        for k in range(3):
            _same(res[1][0][k], res[0][0][k], f"member {k} ids")
        _same(res[1][1], res[0][1], "member 1 logits")
    finally:
        m.close()
