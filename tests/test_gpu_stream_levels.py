"""Level records of the live sessions (vox_tick_level; DESIGN.md section 8, "Levels") end to end on the tiny model: what a solo stream, a stream group, their burst
forms, a rate stream and an endless stream hand out, against the float64 reference of tests/level_ref.py computed from the pushed array (peak bit for bit,
mean_square within the derived bound) and, between the forms, bit for bit.  Utterances of 2 to 3 s: speech-like noise, 0.8 s of exact zeros, noise again."""
import ctypes as C
import time

import numpy as np
import pytest

import level_ref as R
from model_fixtures import tiny_gguf
from stream_helpers import _gain, _pieces, _t

pytestmark = pytest.mark.gpu
F32 = np.float32
TICK = R.TICK
ZERO0, ZERO1 = 14400, 27200      # the zero stretch of every clip: 0.9 s .. 1.7 s


def _clip(seconds, seed):
    rng = np.random.default_rng(seed); n = int(seconds * 16000)
    x = (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * 0.07)).astype(F32)
    x[ZERO0:ZERO1] = 0
    return x


CLIPS = [(_clip(2.6, 41), None), (_clip(2.2, 42), 0.37), (_clip(3.0, 43), -2.0)]      # (samples, gain; None: the clip's peak scale)


def _bits(a, b):
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


def _run(st, x, cuts):
    out = [st.push(x[a:b]) for a, b in cuts] + [st.finish()]
    return np.concatenate(out).astype(np.int32)


@pytest.fixture(scope="module")
def solo(pkg, tiny):
    """Every clip through a plain solo stream in ONE push, levels on, the logits tap armed: (gain, ids, records, tapped logits) -- the records every other form is held to."""
    t = _t(pkg, tiny); res = []
    for x, g in CLIPS:
        g = _gain(x) if g is None else g
        st = tiny.create_stream(t, gain=g)
        try:
            st.set_levels(True); st.tap_arm(64)
            ids = _run(st, x, [(0, len(x))]); res.append((g, ids, st.levels(), st.tap_fetch()))
        finally:
            st.close()
    return res


def test_solo_records_equal_the_reference(pkg, solo):
    """One record per id, finish's included; record 0 is (0, 0); peak exact and mean_square within the bound against float64 on f32(gain x); the zero stretch's windows
    are exactly (0, 0)."""
    for (x, _), (g, ids, lv, _) in zip(CLIPS, solo):
        n = pkg.stream_schedule(len(x), finished=True)[1]
        assert len(ids) == len(lv) == n >= 14
        pk, ms = R.levels(x, g, n)
        worst = R.check(lv, pk, ms, f"solo stream, gain {g}")
        assert lv[0]["peak"] == 0 and lv[0]["mean_square"] == 0
        assert (lv["peak"][7:11] == 0).all() and (lv["mean_square"][7:11] == 0).all() and (lv["peak"][[6, 11]] > 0.01).all()      # windows 7 .. 10 lie inside the zeros
        assert n * TICK > len(x) and (lv["peak"][-1] == pk[-1])      # the last windows reach into finish's pad
        print(f"gain {g}: largest |mean_square - ref| / bound = {worst:.3f}")


@pytest.mark.parametrize("cut", ["160", "odd"])
def test_solo_records_do_not_depend_on_the_cuts(pkg, tiny, solo, cut):
    x = CLIPS[0][0]; g, ids, lv, _ = solo[0]
    if cut == "160":
        cuts = _pieces(len(x), 160)
    else:
        sizes = [1, 977, 2559, 2561, 39, 5121, 3]; cuts = []; a = 0
        while a < len(x):
            b = min(len(x), a + sizes[len(cuts) % len(sizes)]); cuts.append((a, b)); a = b
    st = tiny.create_stream(_t(pkg, tiny), gain=g)
    try:
        st.set_levels(True)
        ids2 = _run(st, x, cuts); lv2 = st.levels()
        assert _bits(st.levels(3, 5), lv2[3:8]) and len(st.levels(len(ids2), 0)) == 0
    finally:
        st.close()
    assert np.array_equal(ids2, ids) and _bits(lv2, lv)


def test_levels_change_neither_ids_nor_logits_and_cost_only_their_records(pkg, tiny, solo):
    """The same clip with levels never turned on: the ids and the tapped logits rows have the bits of the run with levels on; the first set_levels(True) adds exactly
    the records' bytes (8 per position + 2), toggling adds nothing; reading with levels off is refused."""
    x = CLIPS[0][0]; g, ids, lv, lg = solo[0]; L = pkg.lib()
    st = tiny.create_stream(_t(pkg, tiny), gain=g, max_positions=256)
    try:
        b0 = st.info()["bytes"]; st.tap_arm(64)
        ids2 = _run(st, x, _pieces(len(x), TICK)); lg2 = st.tap_fetch()
        assert st.info()["bytes"] == b0      # (the tap is gone again) a stream that never turns levels on allocates nothing
        assert np.array_equal(ids2, ids) and _bits(lg2, lg)
        buf = np.full(4, -7, dtype=pkg.LEVEL_DTYPE); before = buf.tobytes(); q = C.c_int32(-7)
        assert L.vox_stream_levels(st.h, 0, 1, buf.ctypes.data) == 1 and "levels are off" in L.vox_last_error().decode()
        assert L.vox_stream_quiet(st.h, 0.01, C.byref(q)) == 1 and "levels are off" in L.vox_last_error().decode()
        st.set_levels(True); b1 = st.info()["bytes"]
        assert b1 - b0 == (256 + 2) * 8
        assert np.isnan(st.levels()["peak"]).all() and len(st.levels()) == len(ids)      # the ids handed out before the first on
        st.set_levels(False); st.set_levels(True)
        assert st.info()["bytes"] == b1
        n = len(ids)
        for first, cnt in ((0, n + 1), (n, 1), (-1, 2), (2, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert L.vox_stream_levels(st.h, first, cnt, buf.ctypes.data) == 1 and "handed out" in L.vox_last_error().decode(), (first, cnt)
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert L.vox_stream_quiet(st.h, bad, C.byref(q)) == 1 and "peak_below" in L.vox_last_error().decode()
        assert buf.tobytes() == before and q.value == -7
    finally:
        st.close()


def test_quiet_ticks_climb_through_the_zero_stretch_and_drop_behind_it(pkg, tiny, solo):
    """160 ms pushes: after push p the ids 0 .. p - 1 are out, and quiet_ticks() is the pure function on the records so far -- 1, 2, 3, 4 as windows 7 .. 10 (inside the
    zeros) arrive, 0 again with window 11."""
    x = CLIPS[0][0]; g, ids, lv, _ = solo[0]
    st = tiny.create_stream(_t(pkg, tiny), gain=g)
    try:
        st.set_levels(True); got = []
        for p, (a, b) in enumerate(_pieces(len(x), TICK), 1):
            st.push(x[a:b]); n = st.info()["ids"]
            assert n == p      # id k is due at 2560 k + 40 samples
            got.append(st.quiet_ticks()); assert got[-1] == pkg.quiet_ticks(lv[:n], -50.0)
        assert got[5:12] == [0, 0, 1, 2, 3, 4, 0] and max(got) == 4 and got[-1] == 0
        assert st.quiet_ticks(db=0.0) >= 1 and st.quiet_ticks(db=-120.0) == 0      # the threshold is the caller's
    finally:
        st.close()


def test_stream_at_48k_s16_equals_the_stream_fed_the_resampled_samples(pkg, ctx, tiny):
    """A 48 kHz stream pushed 16-bit PCM in odd pieces against a 16 kHz stream pushed vox_resample of the same audio: the records are taken on the 16 kHz samples the
    resampler produced, so they have the same bits; and they are the reference's on those samples."""
    t = _t(pkg, tiny); rng = np.random.default_rng(48); n = int(48000 * 2.3) + 5
    pcm = np.clip(np.round(9000.0 * rng.standard_normal(n) + 7000.0 * np.sin(np.arange(n) * 0.023)), -32768, 32767).astype(np.int16)
    pcm[3 * ZERO0:3 * ZERO1] = 0
    x16 = pkg.resample(ctx, pcm.astype(F32) / F32(32768), 48000); g = _gain(x16)
    a = tiny.create_stream(t, gain=g, sample_rate=48000); b = tiny.create_stream(t, gain=g)
    try:
        a.set_levels(True); b.set_levels(True)
        ia = _run(a, pcm, _pieces(len(pcm), 7001)); ib = _run(b, x16, _pieces(len(x16), 2560))
        la, lb = a.levels(), b.levels()
    finally:
        a.close(); b.close()
    assert len(ia) >= 12 and np.array_equal(ia, ib) and _bits(la, lb)
    pk, ms = R.levels(x16, g, len(lb)); R.check(lb, pk, ms, "16 kHz stream fed the resampled samples")


def _irregular_group_run(pkg, g, clips, finish_all=True):
    """The three clips fed in calls of different sizes per member, one member idle every third call."""
    off = [0, 0, 0]; step = [2560 * 3 + 17, 1600, 7777]; ids = {k: [] for k in range(3)}; c = 0
    while any(off[k] < len(clips[k]) for k in range(3)):
        feeds = {}
        for k in range(3):
            if off[k] < len(clips[k]) and (c + k) % 3 != 2:
                feeds[k] = clips[k][off[k]:off[k] + step[k]]; off[k] += step[k]
        fin = [k for k in feeds if off[k] >= len(clips[k])] if finish_all else []
        for k, v in g.advance(feeds, finish=fin).items():
            ids[k].extend(v)
        c += 1
    return {k: np.array(v, np.int32) for k, v in ids.items()}


def test_group_members_have_the_solo_streams_bits_and_an_unleveled_member_is_refused(pkg, tiny, solo):
    t = _t(pkg, tiny); L = pkg.lib(); clips = [x for x, _ in CLIPS]
    g = tiny.create_stream_group(t, 3, gains=[s[0] for s in solo])
    try:
        b0 = [g.info(k)["bytes"] for k in range(3)]
        g.set_levels(0, True); g.set_levels(2, True)
        b1 = [g.info(k)["bytes"] for k in range(3)]
        assert b1[1] == b0[1] and b1[0] - b0[0] == b1[2] - b0[2] == (2048 + 2) * 8      # the member's own records, nothing for a member with levels off
        ids = _irregular_group_run(pkg, g, clips)
        for k in (0, 2):
            assert len(ids[k]) == len(solo[k][1]) and _bits(g.levels(k), solo[k][2]), k
            assert g.quiet_ticks(k) == pkg.quiet_ticks(solo[k][2])
        buf = np.full(2, -7, dtype=pkg.LEVEL_DTYPE); before = buf.tobytes(); q = C.c_int32(-7)
        assert L.vox_stream_group_levels(g.h, 1, 0, 1, buf.ctypes.data) == 1 and "levels are off" in L.vox_last_error().decode()
        assert L.vox_stream_group_quiet(g.h, 1, 0.01, C.byref(q)) == 1 and "levels are off" in L.vox_last_error().decode()
        assert L.vox_stream_group_levels(g.h, 3, 0, 1, buf.ctypes.data) == 1 and L.vox_stream_group_levels(g.h, 0, len(ids[0]), 1, buf.ctypes.data) == 1 and buf.tobytes() == before
        with pytest.raises(pkg.VoxError):
            g.levels(1)
        g.reset(0, solo[0][0])      # the member's next connection: the records start over, the flag stays
        assert len(g.levels(0)) == 0
        again = g.advance({0: clips[0]}, finish=[0])[0]
        assert len(again) == len(solo[0][1]) and _bits(g.levels(0), solo[0][2])
    finally:
        g.close()


def test_burst_stream_and_burst_group_have_the_plain_bits(pkg, tiny, solo):
    """A burst stream (B = 4) and a burst group, each given a 9-tick backlog in ONE call (bursts of 4, 4 and a tick; a ragged round in the group, whose members get 9, 5
    and 2 ticks), then the rest: the records of the plain solo streams, bit for bit; the counters say the bursts ran."""
    t = _t(pkg, tiny); clips = [x for x, _ in CLIPS]; cut = 8 * TICK + 40
    st = tiny.create_stream(t, gain=solo[0][0], burst=4)
    try:
        st.set_levels(True)
        first = st.push(clips[0][:cut]); assert len(first) == 9
        bi = st.burst_info(); assert bi["bursts"] == 2 and bi["burst_ticks"] == 8 and bi["single_ticks"] == 1
        assert _bits(st.levels(), solo[0][2][:9])
        st.push(clips[0][cut:]); st.finish()
        assert _bits(st.levels(), solo[0][2])
    finally:
        st.close()
    g = tiny.create_stream_group(t, 3, gains=[s[0] for s in solo], burst=4)
    try:
        for k in range(3):
            g.set_levels(k, True)
        cuts = [cut, 4 * TICK + 40, 1 * TICK + 40]
        out = g.advance({k: clips[k][:cuts[k]] for k in range(3)})
        assert [len(out[k]) for k in range(3)] == [9, 5, 2] and g.burst_info()["burst_rounds"] >= 2
        for k in range(3):
            assert _bits(g.levels(k), solo[k][2][:len(out[k])]), k
        g.advance({k: clips[k][cuts[k]:] for k in range(3)}, finish=[0, 1, 2])
        for k in range(3):
            assert _bits(g.levels(k), solo[k][2]), k
    finally:
        g.close()


def _counted(pkg):
    """The library's counted launch forms (attention and linear kernels), as tools/stream_bench.py reads them."""
    a = (C.c_uint64 * 20)(); g = (C.c_uint64 * 20)(); L = pkg.lib()
    assert L.vox_debug_attn_launches(a, 20) == 0 and L.vox_debug_gemm_launches(g, 20) == 0
    return list(a), list(g)


def test_levels_off_sessions_count_and_hold_what_they_did(pkg, tiny, solo):
    """Sessions that never turn levels on, given the 9-tick backlog of the burst test: a burst stream's burst_info() is the burst arithmetic's (4, 4 and a tick), its
    bytes those of the twin with levels on less the records; a burst group's burst_info(), its counted launch forms over the call and its members' bytes are those of
    the twin group with levels on (less the records): the level kernel is one uncounted launch, and nothing else moves."""
    t = _t(pkg, tiny); clips = [x for x, _ in CLIPS]; cut = 8 * TICK + 40; gains = [s[0] for s in solo]
    off = tiny.create_stream(t, gain=gains[0], burst=4, max_positions=256); on = tiny.create_stream(t, gain=gains[0], burst=4, max_positions=256)
    try:
        on.set_levels(True); b0 = off.info()["bytes"]
        ids_off = off.push(clips[0][:cut]); ids_on = on.push(clips[0][:cut])
        assert off.burst_info() == on.burst_info() == {"burst": 4, "bursts": 2, "burst_ticks": 8, "single_ticks": 1} and np.array_equal(ids_off, ids_on)
        assert off.info()["bytes"] == b0 == on.info()["bytes"] - (256 + 2) * 8
    finally:
        off.close(); on.close()
    cuts = [cut, 4 * TICK + 40, 1 * TICK + 40]; res = []
    for levels in (False, True):
        g = tiny.create_stream_group(t, 3, gains=gains, burst=4)
        try:
            b0 = [g.info(k)["bytes"] for k in range(3)]
            for k in range(3 if levels else 0):
                g.set_levels(k, True)
            c0 = _counted(pkg); out = g.advance({k: clips[k][:cuts[k]] for k in range(3)}); c1 = _counted(pkg)
            delta = [[y - x for x, y in zip(u, v)] for u, v in zip(c0, c1)]
            res.append((g.burst_info(), delta, [g.info(k)["bytes"] - b0[k] for k in range(3)], [out[k] for k in range(3)]))
        finally:
            g.close()
    (bi0, d0, grew0, ids0), (bi1, d1, grew1, ids1) = res
    rounds = pkg.stream_group_burst_rounds([9, 5, 2], 4)      # the host arithmetic of the burst groups: (4, 4, 2), (4, 1), then a round of ones, which is a plain round
    assert [list(r) for r in rounds] == [[4, 4, 2], [4, 1], [1]]
    assert bi0 == bi1 == {"burst": 4, "burst_rounds": 2, "burst_member_ticks": 15, "plain_rounds": 1}
    assert d0 == d1 and sum(d0[0]) > 0 and sum(d0[1]) > 0
    assert grew0 == [0, 0, 0] and grew1 == [(2048 + 2) * 8] * 3 and all(np.array_equal(u, v) for u, v in zip(ids0, ids1))


def test_off_and_on_again_reset_and_peek(pkg, tiny, solo):
    x = CLIPS[2][0]; g, ids, lv, _ = solo[2]; t = _t(pkg, tiny)
    st = tiny.create_stream(t, gain=g)
    try:
        # on -> off -> on across pushes: NaN records for exactly the ids in between
        st.set_levels(True)
        a, b = 5 * TICK + 40, 11 * TICK + 40
        n_a = len(st.push(x[:a])); st.set_levels(False)
        n_b = n_a + len(st.push(x[a:b])); st.set_levels(True)
        st.push(x[b:]); st.finish()
        got = st.levels()
        assert (n_a, n_b) == (6, 12) and len(got) == len(ids)
        off = np.r_[n_a:n_b]; on = np.r_[0:n_a, n_b:len(ids)]
        assert np.isnan(got["peak"][off]).all() and np.isnan(got["mean_square"][off]).all() and _bits(got[on], lv[on])
        assert st.quiet_ticks(db=40.0) == len(ids) - n_b      # (a threshold above every sample) the run ends at the NaN records
        # reset: the records start over, the flag stays
        st.reset()
        assert len(st.levels()) == 0 and st.quiet_ticks() == 0
        # a peek after every push: the list is not extended, and the later records are those of a session that never peeked
        for p0, p1 in _pieces(len(x), 3 * TICK + 7):
            st.push(x[p0:p1]); n = st.info()["ids"]; before = st.levels()
            tail = st.peek()
            assert len(tail) > 0 and st.info()["ids"] == n and _bits(st.levels(), before) and _bits(before, lv[:n])
        st.finish()
        assert _bits(st.levels(), lv)
    finally:
        st.close()


def test_snapshot_and_restore_carry_no_level_records(pkg, tiny, solo):
    """A session snapshotted mid-utterance and restored into a fresh stream with levels on: the ids handed out before have (NaN, NaN), the later ids the bits of the
    uninterrupted session; the blob is what it is without levels (the flag is not in it)."""
    x = CLIPS[0][0]; g, ids, lv, _ = solo[0]; t = _t(pkg, tiny); cut = 6 * TICK + 1000
    a = tiny.create_stream(t, gain=g); plain = tiny.create_stream(t, gain=g); b = tiny.create_stream(t, gain=1.0)
    try:
        a.set_levels(True)
        n0 = len(a.push(x[:cut])); plain.push(x[:cut])
        blob = a.snapshot()
        assert blob.tobytes() == plain.snapshot().tobytes()      # format and content as without the feature
        b.set_levels(True); b.restore(blob)
        assert len(b.levels()) == n0 == 7 and np.isnan(b.levels()["peak"]).all() and b.quiet_ticks() == 0
        rest = np.concatenate([b.push(x[cut:]), b.finish()])
        assert np.array_equal(rest, ids[n0:])
        got = b.levels()
        assert np.isnan(got["peak"][:n0]).all() and np.isnan(got["mean_square"][:n0]).all() and _bits(got[n0:], lv[n0:])
    finally:
        a.close(); plain.close(); b.close()


def test_endless_stream_keeps_every_record_across_the_lists_doubling(pkg, tiny):
    """An endless stream with the smallest decoder ring (8256 rows, the geometry of tests/test_gpu_stream_endless.py: an 8192-position window) starts with lists of
    8256 positions; run to 8300 ids in large pushes it doubles them at position 8256 -- the level list with the token list.  Every record, on both sides of the growth,
    is the reference's.  The slow one of this file: 8300 ticks of the tiny model are what reaching the doubling costs, about 4 s on an MI355X (printed)."""
    rows = 8192 + 1 + 63; n_ids = 8300; t0 = time.time()
    rng = np.random.default_rng(8256); n = TICK * (n_ids - 1) + 40
    amp = (0.02 + 0.5 * rng.random(n_ids)).astype(F32); amp[rng.integers(0, n_ids, 400)] = 0
    x = (rng.standard_normal(n, dtype=F32) * np.repeat(amp, TICK)[:n]).astype(F32)
    st = tiny.create_stream(_t(pkg, tiny), gain=0.37, endless=True, dec_ring_rows=rows)
    try:
        st.set_levels(True); b0 = st.info()["bytes"]; got = 0
        for a, b in _pieces(n, 1000 * TICK):
            got += len(st.push(x[a:b]))
        assert got == n_ids == st.info()["ids"] and st.info()["positions"] == n_ids + 37 > rows
        assert st.info()["bytes"] - b0 >= rows * (4 + 8)      # the token list and the level list doubled
        lv = st.levels()
    finally:
        st.close()
    pk, ms = R.levels(x, 0.37, n_ids)
    R.check(lv, pk, ms, "endless stream")
    assert (lv["peak"][8200:8300] == pk[8200:8300]).all() and (pk[8200:8300] > 0).sum() > 80      # behind the growth (id 8219 is the first there)
    print(f"{n_ids} ticks of an endless tiny stream: {time.time() - t0:.1f} s")
