"""Stream groups (vox_stream_group): up to 16 live sessions advanced together, every weight matrix read once per tick for all members due.

What is asserted, and against what:
 * a member's ids are those of a solo LiveStream (its ids and its logits tap: the reference) with the same gain fed the same samples, in the project's usual sense:
   check_greedy_ids at TOL = 2e-4, equal outright before the reference's first near-tie; every such claim also asserts that this near-tie lies at or beyond half of the
   clip's ids (the condition of tests/test_gpu_stream.py).  A clip that does not meet the condition is swapped for another seed (_clip); the condition is never relaxed.
 * tapped logits against teacher_forced_logits at 2e-4 of the largest reference logit (the bar of test_batch_logits_every_step_form_vs_teacher_forced).
 * every advance hands each fed member exactly the ids vox_stream_schedule says became due.
Bit-identity with the solo stream is not claimed for a member: the width of a round selects the GEMM kernels.

The 16-member run feeds 3200 samples (two 1600-sample pieces) per member and call, the members' starts one 1600-sample piece apart.  With ONE piece per call only 10 of
16 members could ever tick together -- a tick is 1.6 pieces long, so in any call 3 of every 8 consecutive starts have no tick due -- and the widths above 10, where the
encoder's 4 n rows leave the 17..48-row kernels for the tile GEMM, would never run.  Two pieces make every fed member due in a call's first round."""
import ctypes as C
import os

import numpy as np
import pytest

from model_fixtures import GEMM_FORMS, teacher_forced_logits, tiny_gguf
from stream_helpers import _full_path, _gain, _held, _raw_advance, _stop, _t

pytestmark = pytest.mark.gpu
TOL = 2e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_16s_peaked_oracle.npz")
ATTN_FORMS = ("prefill_small", "prefill_mfma", "prefill_f32", "decode", "decode_spec", "decode_gqa", "attn_wo", "engine", "stream_ring")


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


_SOLO = {}      # clip key -> (ids, logits) of the solo LiveStream: computed once, shared, read-only


def _solo(m, key, x, t, **kw):
    if key not in _SOLO:
        st = m.create_stream(t, gain=_gain(x), **kw); st.tap_arm(256)
        try:
            per = [st.push(x[a:a + 3200]) for a in range(0, len(x), 3200)] + [st.finish()]      # (a solo stream's ids do not depend on the cuts, bit for bit)
            lg = st.tap_fetch()
        finally:
            st.close()
        ids = np.concatenate(per)
        assert lg.shape[0] == len(ids) and np.array_equal(lg.argmax(axis=1), ids)
        ids.setflags(write=False); lg.setflags(write=False)
        _SOLO[key] = (ids, lg)
    return _SOLO[key]


def _clip(pkg, m, t, seconds, seed, n=None, **kw):
    """synth_audio(seconds, seed) (cut to n samples), the seed moved on until the solo reference's first near-tie lies at or beyond half of the clip's ids."""
    for s in range(seed, seed + 12 * 1000, 1000):
        x = pkg.synth.synth_audio(seconds, seed=s)
        if n is not None:
            assert len(x) >= n
            x = np.ascontiguousarray(x[:n])
        ids, lg = _solo(m, (id(m), seconds, s, n, tuple(sorted(kw.items()))), x, t, **kw)
        if 2 * _stop(lg, TOL) >= len(ids):
            return x, ids, lg
        print(f"clip {seconds} s seed {s}: first near-tie at {_stop(lg, TOL)} of {len(ids)} ids: another seed")
    raise AssertionError(f"no seed from {seed} on gives a {seconds} s clip that can carry an ids claim")


def _counts(pkg):
    L = pkg.lib(); a = (C.c_uint64 * 9)(); g = (C.c_uint64 * len(GEMM_FORMS))()
    assert L.vox_debug_attn_launches(a, 9) == 0 and L.vox_debug_gemm_launches(g, len(GEMM_FORMS)) == 0
    return dict(zip(ATTN_FORMS, map(int, a))), dict(zip(GEMM_FORMS, map(int, g)))


def _delta(b, a):
    return {k: a[k] - b[k] for k in a if a[k] != b[k]}


# ---- 1 + 2. sixteen members across every dispatch edge; the schedule --------------------------------------------------------------------------------------------------
ENDS = [23] * 3 + [24] + [25] * 7 + [26] + [27] * 2 + [28] + [29]      # the call in which member k's clip ends: 16, 13, 12, 5, 4, 2, 1 members are fed as they finish


@pytest.fixture(scope="module")
def run16(pkg, ctx, tiny):
    """One run of 16 members, recorded: member k starts 1600 k samples after member 0 and is fed 3200 samples per call; its clip has 1600 (2 E_k - k) - 100 - 37 k samples
    (4.0 .. 4.6 s, all lengths distinct, none a multiple of the piece), so it ends in call E_k."""
    m = tiny; t = _t(pkg, m)
    lens = [1600 * (2 * ENDS[k] - k) - 100 - 37 * k for k in range(16)]
    assert len(set(lens)) == 16 and 3 * 16000 <= min(lens) and max(lens) <= 6 * 16000
    clips = [_clip(pkg, m, t, 6.0, 4100 + k, n=lens[k]) for k in range(16)]
    tapped = (0, 7, 15)      # the first to finish, one in the middle, the last
    g = m.create_stream_group(t, 16, gains=[_gain(c[0]) for c in clips])
    rec = {"ids": [[] for _ in range(16)], "widths": set(), "calls": [], "positions16": None}
    try:
        for k in tapped:
            g.tap_arm(k, 64)
        for c in range(max(ENDS) + 1):
            feeds = {}; fin = []
            for k in range(16):
                lo, hi = max(0, 1600 * (2 * c - 2 - k)), min(lens[k], 1600 * (2 * c - k))
                if hi > lo and c <= ENDS[k]:
                    feeds[k] = clips[k][0][lo:hi]
                    if hi == lens[k]:
                        fin.append(k)
            before = {k: g.info(k) for k in range(16)}
            out = g.advance(feeds, finish=fin)
            after = {k: g.info(k) for k in range(16)}
            assert set(out) == set(feeds)
            steps = {k: after[k]["positions"] - before[k]["positions"] for k in range(16)}
            for k in range(16):
                if k not in feeds:
                    assert after[k] == before[k]
                    continue
                pushed = before[k]["samples"] + len(feeds[k])
                assert after[k]["samples"] == pushed and after[k]["ids"] == before[k]["ids"] + len(out[k])
                rec["calls"].append((c, k, before[k]["ids"], len(out[k]), pushed, k in fin))
                rec["ids"][k].extend(out[k])
            for r in range(max(steps.values())):      # round r of the call served the members with more than r ticks due
                rec["widths"].add(sum(1 for d in steps.values() if d > r))
            if len(feeds) == 16 and rec["positions16"] is None and c >= 12:
                rec["positions16"] = sorted(before[k]["encoder_position"] for k in range(16))
        assert all(g.info(k)["samples"] == lens[k] for k in range(16))
        rec["taps"] = {k: g.tap_fetch(k) for k in tapped}
    finally:
        g.close()
    rec["clips"] = clips; rec["lens"] = lens; rec["t"] = t
    return rec


def test_sixteen_members_equal_solo_streams_across_every_dispatch_edge(pkg, ctx, tiny, run16):
    rec = run16
    print(f"round widths seen: {sorted(rec['widths'])}; encoder positions of the 16 members in one call: {rec['positions16']}")
    assert {16, 13, 12, 5, 4, 2, 1} <= rec["widths"]      # 64 and 52 encoder rows (tile GEMM), 48 and 20 (17..48 rows), 16 and 8 (5..16), 4 (GEMV)
    assert len(set(rec["positions16"])) >= 8             # the members are spread over the stream, not in lock-step
    same = [_held(np.array(rec["ids"][k], np.int32), rec["clips"][k][1], rec["clips"][k][2], f"member {k}", TOL) for k in range(16)]
    print(f"16 members: ids equal to the solo stream's on {same} of {[len(c[1]) for c in rec['clips']]}")
    for k, lg in rec["taps"].items():
        x, rids, _ = rec["clips"][k]; ids = np.array(rec["ids"][k], np.int32)
        assert lg.shape[0] == len(ids) and np.array_equal(lg.argmax(axis=1), ids)      # the tap holds the row behind each id
        ref = teacher_forced_logits(pkg, ctx, tiny, x, rec["t"], ids)
        err = float(np.abs(lg - ref).max()); bar = TOL * float(np.abs(ref).max())
        print(f"member {k}: tapped logits vs teacher-forced: max error {err:.3e}, bar {bar:.3e}")
        assert err <= bar


def test_every_advance_returns_what_the_schedule_says(pkg, run16):
    rec = run16
    assert len(rec["calls"]) > 300
    for c, k, had, got, pushed, finished in rec["calls"]:
        assert had + got == pkg.stream_schedule(pushed, finished=finished)[1], (c, k, had, got, pushed, finished)
    for k in range(16):
        assert len(rec["ids"][k]) == pkg.stream_schedule(rec["lens"][k], finished=True)[1]


# ---- 3. full size, nothing forgiven -----------------------------------------------------------------------------------------------------------------------------------
def test_full_size_five_members_give_the_golden_ids(pkg, ctx, full_model):
    m = full_model; g0 = np.load(GOLDEN)
    x = pkg.synth.synth_audio(16.0, seed=7049); t = _t(pkg, m)
    rids, top1, amax = g0["ids"], g0["top1"], float(g0["logit_absmax"])
    assert len(rids) == 108
    pieces = [(a, min(len(x), a + 2560)) for a in range(0, len(x), 2560)]
    g = m.create_stream_group(t, 5, gains=[_gain(x)] * 5)
    ids = [[] for _ in range(5)]
    try:
        for k in range(5):
            g.tap_arm(k, 128)
        for c in range(len(pieces) + 4):
            feeds = {k: x[pieces[c - k][0]:pieces[c - k][1]] for k in range(5) if 0 <= c - k < len(pieces)}      # member k is k pieces behind member 0
            for k, v in g.advance(feeds, finish=[k for k in feeds if c - k == len(pieces) - 1]).items():
                ids[k].extend(v)
        for k in range(5):
            lg = g.tap_fetch(k); got = np.array(ids[k], np.int32)
            assert np.array_equal(got, rids), f"member {k}: ids differ from the oracle's at {np.flatnonzero(got != rids)[:8]}"
            assert lg.shape[0] == 108 and np.array_equal(lg.argmax(axis=1), got)
            err = float(np.abs(np.sort(lg, axis=1)[:, -1] - top1).max())
            print(f"full size, member {k} of 5: 108 / 108 ids, max top-logit error {err:.3e} at |logit| max {amax:.1f}")
            assert err <= 1e-2 * amax      # the bound of test_full_peaked_golden_all_ids
    finally:
        g.close()


# ---- 4. ring wrap inside a group --------------------------------------------------------------------------------------------------------------------------------------
def test_ring_wrap_inside_a_group(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    xl, lids, llg = _clip(pkg, m, t, 33.0, 33, enc_capacity_rows=760)      # 990 encoder rows: the 760-row ring wraps
    short = [_clip(pkg, m, t, 3.0 + 0.25 * j, 5200 + j) for j in range(3)]
    g = m.create_stream_group(t, 4, gains=[_gain(xl)] + [_gain(s[0]) for s in short], enc_capacity_rows=760)
    try:
        got = []; off = [0, 0, 0, 0]; runs = [0, 0, 0]; cur = [[], [], []]; done = []
        clips = [xl] + [s[0] for s in short]
        while off[0] < len(xl):
            feeds = {0: xl[off[0]:off[0] + 3200]}
            for j in range(3):
                if runs[j] < 3:
                    feeds[j + 1] = clips[j + 1][off[j + 1]:off[j + 1] + 3200]
            fin = [k for k in feeds if off[k] + 3200 >= len(clips[k])]
            out = g.advance(feeds, finish=fin)
            got.extend(out[0])
            for k in feeds:
                off[k] += 3200
            for j in range(3):
                if j + 1 in feeds:
                    cur[j].extend(out[j + 1])
                    if j + 1 in fin:      # the short member finished: its ids, then the next connection on the same member
                        done.append((j, runs[j], np.array(cur[j], np.int32))); cur[j] = []; runs[j] += 1; off[j + 1] = 0
                        g.reset(j + 1, _gain(clips[j + 1]))
        info = g.info(0)
        assert info["encoder_position"] == 4 * info["positions"] and info["ring_rows"] == 760 and info["encoder_position"] > 760
        assert runs == [3, 3, 3] and len(done) == 9
        print(f"long member next to 9 short runs: {_held(np.array(got, np.int32), lids, llg, 'the 33 s member', TOL)} of {len(lids)} ids equal to the solo stream's")
        for j, r, ids in done:
            _held(ids, short[j][1], short[j][2], f"short member {j + 1}, run {r}", TOL)
    finally:
        g.close()


# ---- 5. reset and reuse -----------------------------------------------------------------------------------------------------------------------------------------------
def test_reset_and_reuse_of_a_member(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    a = _clip(pkg, m, t, 3.0, 6100); b = _clip(pkg, m, t, 4.0, 6200); others = [_clip(pkg, m, t, 6.0, 6300 + j) for j in range(2)]
    b = (np.ascontiguousarray(0.5 * b[0]), b[1], b[2])      # half as loud: the reset's gain (twice the first clip's class) must reach the mel, the ids stay the clip's
    assert abs(_gain(b[0]) / _gain(a[0]) - 1) > 0.2
    g = m.create_stream_group(t, 3, gains=[_gain(a[0])] + [_gain(o[0]) for o in others])
    try:
        clips = [a[0], others[0][0], others[1][0]]; off = [0, 0, 0]; ids = [[], [], []]; first = None; mid_utterance = None
        while any(off[k] < len(clips[k]) for k in range(3)):
            feeds = {k: clips[k][off[k]:off[k] + 3200] for k in range(3) if off[k] < len(clips[k])}
            fin = [k for k in feeds if off[k] + 3200 >= len(clips[k])]
            for k, v in g.advance(feeds, finish=fin).items():
                ids[k].extend(v); off[k] += 3200
            if 0 in fin and first is None:
                first = np.array(ids[0], np.int32); ids[0] = []; off[0] = 0; clips[0] = b[0]
                with pytest.raises(pkg.VoxError, match="finished"):
                    g.advance({0: b[0][:100]})
                g.reset(0, _gain(b[0]))
                mid_utterance = [0 < g.info(k)["samples"] < len(clips[k]) for k in (1, 2)]
                assert g.info(0) == {**g.info(0), "samples": 0, "positions": 37, "ids": 0}
        assert mid_utterance == [True, True]
        _held(first, a[1], a[2], "member 0, first clip", TOL)
        # the solo reference of the second clip at ITS gain: 0.5 x with twice the gain is the clip the reference saw, to the last bit of the product
        _held(np.array(ids[0], np.int32), b[1], b[2], "member 0 after its reset, second clip", TOL)
        for k in (1, 2):
            _held(np.array(ids[k], np.int32), others[k - 1][1], others[k - 1][2], f"member {k}, mid-utterance during the reset", TOL)
    finally:
        g.close()


# ---- 6. weights once per round ----------------------------------------------------------------------------------------------------------------------------------------
def test_weights_once_per_round(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); x = pkg.synth.synth_audio(12.0, seed=88); EL = m.config.enc_layers
    res = {}
    for n in (8, 1):
        g = m.create_stream_group(t, n, gains=[_gain(x)] * n)
        try:
            g.advance({k: x[:2560 * 8] for k in range(n)})      # 8 warm-up ticks: every lazily built table exists
            a0, g0 = _counts(pkg)
            out = g.advance({k: x[2560 * 8:2560 * 58] for k in range(n)})
            a1, g1 = _counts(pkg)
        finally:
            g.close()
        assert all(len(v) == 50 for v in out.values()) and len(out) == n
        res[n] = (_delta(a0, a1), _delta(g0, g1))
        print(f"{n} member(s), 50 steady rounds: attention {res[n][0]}, linear {res[n][1]}")
    st = m.create_stream(t, gain=_gain(x))
    try:
        st.push(x[:2560 * 8]); a0, g0 = _counts(pkg); st.push(x[2560 * 8:2560 * 58]); a1, g1 = _counts(pkg)
    finally:
        st.close()
    solo = (_delta(a0, a1), _delta(g0, g1))
    print(f"solo stream, 50 steady ticks: attention {solo[0]}, linear {solo[1]}")
    da, dg = res[8]
    assert da["stream_ring"] == 50 * EL      # one ring-attention launch per layer and ROUND, not per member
    assert dg["dense2"] == 2 * 50            # the conv stem: two im2col GEMMs per round
    assert not [k for k in dg if k.startswith("gemv_")]      # 32 encoder rows, 8 adapter and decoder rows: no GEMV anywhere
    assert not {"prefill_small", "prefill_mfma", "prefill_f32", "engine", "attn_wo"} & set(da)
    # a group of one runs the solo stream's encoder half launch for launch: the ring attention, the conv stem, and no prefill or tile form; its decode half is the
    # batched step's chain at one row (skinny GEMMs) where the solo stream runs its engine or its per-operator step
    da1, dg1 = res[1]
    assert da1["stream_ring"] == solo[0]["stream_ring"] == 50 * EL and dg1["dense2"] == solo[1]["dense2"] == 2 * 50
    assert not {"prefill_small", "prefill_mfma", "prefill_f32"} & set(da1)
    assert not {"big", "big_rope", "wide", "skinny_mt", "skinny_mt2", "tile_11", "tile_12", "tile_21", "tile_22"} & set(dg1)


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_group_untouched(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    x, rids, rlg = _clip(pkg, m, t, 3.0, 31)
    due = pkg.stream_schedule(len(x))[1]; assert due > 2
    g = m.create_stream_group(t, 2, gains=[_gain(x)] * 2)
    try:
        infos = lambda: [g.info(k) for k in range(2)]
        half = x[:len(x) // 2]
        assert _raw_advance(pkg, g, [(1, 0, half, half.size, 64)])[0] == 0      # member 1 is mid-utterance throughout
        before = infos()
        for entries, kind, needle in [([(0, 0, x, x.size, due - 1)], 0, "capacity"), ([(1, 0, half, half.size, 64), (0, 0, x, x.size, due - 1)], 0, "capacity"),
                                      ([(0, 0, x, x.size, due), (0, 0, x, x.size, due)], 0, "twice"), ([(2, 0, x, x.size, due)], 0, "member"), ([(-1, 0, x, x.size, due)], 0, "member"),
                                      ([(0, 0, x, x.size, due)], 7, "mem_kind")]:
            code, msg, _ = _raw_advance(pkg, g, entries, mem_kind=kind)
            assert code == 1 and needle in msg, (entries[0][:2], msg)
            assert infos() == before
        code, msg, out = _raw_advance(pkg, g, [(0, 0, x, x.size, due)])      # the repeated call with room
        assert code == 0 and np.array_equal(out[0], rids[:due])
        before = infos()
        code, msg, _ = _raw_advance(pkg, g, [(0, 1, x[:0], 0, 1)])       # finish with too small a buffer
        assert code == 1 and "capacity" in msg and infos() == before
        rest = g.advance({}, finish=[0])[0]
        _held(np.concatenate([out[0], rest]), rids, rlg, "member 0 after the refused calls", TOL)
        before = infos()
        for fin in (0, 1):      # a finished member is refused until its reset
            code, msg, _ = _raw_advance(pkg, g, [(0, fin, x[:100], 100, 64)])
            assert code == 1 and "finished" in msg and infos() == before
        g.reset(0, _gain(x))
        again = np.concatenate([g.advance({0: x})[0], g.advance({}, finish=[0])[0]])
        _held(again, rids, rlg, "member 0 after its reset", TOL)
        rest1 = np.concatenate([g.advance({1: x[len(x) // 2:]})[1], g.advance({}, finish=[1])[1]])
        assert g.info(1)["ids"] == len(rids) and len(rest1) + pkg.stream_schedule(len(half))[1] == len(rids)
    finally:
        g.close()
    with pytest.raises(pkg.VoxError, match="window"):
        m.create_stream_group(t, 2, enc_capacity_rows=m.config.enc_window + 4)
    with pytest.raises(pkg.VoxError, match="max_positions"):
        m.create_stream_group(t, 2, max_positions=1 << 20)
    for bad in (0, 17):
        with pytest.raises(pkg.VoxError, match="n_members"):
            m.create_stream_group(t, bad)
    small = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=48)      # positions 37 .. 47 can be reached: 11 ids
    try:
        a = small.advance({0: x[:2560 * 10 + 40], 1: x[:2560 * 4 + 40]})
        assert len(a[0]) == 11 and np.array_equal(a[0], rids[:11]) and np.array_equal(a[1], rids[:5])      # (11 ids lie before the reference's first near-tie: asserted below)
        assert _stop(rlg, TOL) >= 11
        before = [small.info(k) for k in range(2)]
        with pytest.raises(pkg.VoxError, match="position"):
            small.advance({1: x[2560 * 4 + 40:2560 * 5 + 40], 0: x[2560 * 10 + 40:2560 * 11 + 40]})
        assert [small.info(k) for k in range(2)] == before
        with pytest.raises(pkg.VoxError, match="position"):
            small.advance({}, finish=[0])
        assert [small.info(k) for k in range(2)] == before
        b = small.advance({1: x[2560 * 4 + 40:2560 * 10 + 40]})[1]      # the other member goes on to the same limit
        assert np.array_equal(np.concatenate([a[1], b]), rids[:11])
        small.reset(0, _gain(x))
        assert np.array_equal(small.advance({0: x[:2560 * 10 + 40]})[0], rids[:11])
    finally:
        small.close()


# ---- 8. sample sources ------------------------------------------------------------------------------------------------------------------------------------------------
def test_device_and_host_samples_and_a_push_larger_than_the_ring(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    xd, dids, dlg = _clip(pkg, m, t, 5.0, 7100); xh, hids, hlg = _clip(pkg, m, t, 6.0, 7200)
    assert len(xh) > 70000 > 65536
    g = m.create_stream_group(t, 2, gains=[_gain(xd), _gain(xh)])
    dev = C.c_void_p(); pkg._lib.check(pkg.lib().vox_dev_alloc(ctx.h, len(xd) * 4, C.byref(dev)))
    try:
        pkg._lib.check(pkg.lib().vox_dev_upload(ctx.h, dev, xd.ctypes.data, len(xd) * 4))
        got_d = []; got_h = []
        cuts = [(a, min(len(xd), a + 4800)) for a in range(0, len(xd), 4800)]
        for i, (a, b) in enumerate(cuts):
            got_d.extend(g.advance({0: (dev.value + 4 * a, b - a)}, device=True)[0])
            if i == 3:
                got_h.extend(g.advance({1: xh[:70000]})[1])      # one host push larger than the 65 536-sample ring, between two device calls
        got_d.extend(g.advance({}, finish=[0], device=True)[0])
        got_h.extend(g.advance({1: xh[70000:]}, finish=[1])[1])
        _held(np.array(got_d, np.int32), dids, dlg, "the member fed from device memory", TOL)
        _held(np.array(got_h, np.int32), hids, hlg, "the member fed from host memory", TOL)
    finally:
        pkg._lib.check(pkg.lib().vox_dev_free(ctx.h, dev)); g.close()

