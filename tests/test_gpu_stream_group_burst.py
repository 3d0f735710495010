"""Burst groups (vox_stream_group_create_burst, DESIGN.md section 8, "Bursts in stream groups"): a stream group that runs the due ticks of a pass as burst rounds -- one
encoder pass of 4 sum b_z rows with the ragged burst attention for every due member's next b_z = min(ticks still due, B) ticks, then max b_z decode rounds.

What is asserted, and against what:
 * fed one tick per call a burst group IS the plain group of the same ring capacity: ids, tapped logits, score and alternatives records, pool() and pages() after
   every call, bit for bit; burst_info shows no burst round;
 * a B = 1 group made by the new creator runs a backlog with a plain group's launch counts (every attention and GEMM form, no burst launch) and bits;
 * three members with 40, 7 and 1 ticks due in ONE call: ids by the rule of the group files (stream_helpers._held at TOL = 2e-4 against solo plain streams; a clip
   that does not meet the rule's condition is swapped for another seed, the condition is never relaxed); burst_info equals what stream_group_burst_rounds gives for
   the passes vox_debug_stream_feed_passes reports ((26, 7, 1) then (14): rounds (16, 7, 1), (10), (14)); the burst attention launches are enc_layers x burst rounds.
   The symbols do not exist on the parent commit;
 * the slab, the paged and the endless burst group agree bit for bit, the bf16 pool is held by tests/stream_group_kv_worker.py's rule: in a process of their own
   (tests/stream_group_burst_worker.py);
 * a peek on a backlog (its tail runs burst rounds) leaves the group what it was: ids per call, tapped logits, pool() and pages(), info words and burst_info of a
   twin that never peeks;
 * a blob taken after burst rounds continues in a plain group's slot, ids by _held;
 * scores and alternatives are vox_score_rows / vox_alternatives_rows of the tapped rows, byte for byte;
 * a member fed 48 kHz 16-bit PCM with a backlog: ids by _held against the solo plain stream at that rate;
 * a ring capacity of window + 4 B is refused and the device's free memory is what it was (within 1 MiB, where any group takes tens);
 * full size (the peaked synthetic model), once: two members with 40 and 5 ticks due in one call, by _held against the plain group given the same calls."""
import ctypes as C

import numpy as np
import pytest

from model_fixtures import GEMM_FORMS, tiny_gguf
from stream_helpers import _full_path, _gain, _held, _stop, _t
from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
TOL = 2e-4
TICK = 2560
B = 16
ATTN_SLOTS = 20


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


def _n_for(pkg, positions, rate=16000):
    """The fewest samples at `rate` after which `positions` decoder positions are determined (an unfinished stream)."""
    n = max(0, (positions - 38) * TICK * rate // 16000)
    while pkg.stream_schedule(n, False, rate)[0] < positions:
        n += 1
    assert pkg.stream_schedule(n, False, rate)[0] == positions
    return n


def _passes(pkg, calls, rate=16000):
    """The feed planner's passes of a fresh session at `rate` fed `calls` = [(samples, finish)]: per call the list of its passes' ticks."""
    n = len(calls); ns = (C.c_size_t * n)(*[c[0] for c in calls]); fin = (C.c_int32 * n)(*[int(c[1]) for c in calls])
    rows = np.zeros((256, 5), np.int64); k = C.c_int32()
    assert pkg.lib().vox_debug_stream_feed_passes(rate, ns, fin, n, 0, rows.ctypes.data_as(C.POINTER(C.c_int64)), 256, C.byref(k)) == 0
    out = [[] for _ in range(n)]
    for r in rows[:k.value]:
        out[int(r[0])].append(int(r[4]))
    return out


def _rounds_of(gg, member_passes, burst):
    """What a group's call runs: group pass p holds the members' p-th passes; its rounds are stream_group_burst_rounds of their ticks, sorted descending.
    -> (burst rounds, member-ticks inside them, plain rounds)"""
    nb = nt = plain = 0
    for p in range(max(len(v) for v in member_passes)):
        due = sorted((v[p] for v in member_passes if p < len(v) and v[p] > 0), reverse=True)
        for r in (gg.stream_group_burst_rounds(due, burst) if due else []):
            if max(r) >= 2:
                nb += 1; nt += sum(r)
            else:
                plain += 1
    return nb, nt, plain


def _bi(g):
    i = g.burst_info()
    return i["burst_rounds"], i["burst_member_ticks"], i["plain_rounds"]


_SOLO = {}      # clip key -> (ids, logits) of the solo plain stream: computed once, shared, read-only


def _solo(m, key, x, t, **kw):
    if key not in _SOLO:
        st = m.create_stream(t, gain=_gain(x), **kw); st.tap_arm(256)
        try:
            ids = np.concatenate([st.push(x), st.finish()]); lg = st.tap_fetch()      # (a plain stream's ids do not depend on the cuts, bit for bit)
        finally:
            st.close()
        assert lg.shape[0] == len(ids) and np.array_equal(lg.argmax(axis=1), ids)
        ids.setflags(write=False); lg.setflags(write=False)
        _SOLO[key] = (ids, lg)
    return _SOLO[key]


def _clip(pkg, m, t, seconds, seed, make=None, **kw):
    """synth_audio(seconds, seed) (through `make`), the seed moved on until the solo reference's first near-tie lies at or beyond half of the clip's ids."""
    for s in range(seed, seed + 12 * 1000, 1000):
        x = pkg.synth.synth_audio(seconds, seed=s)
        x = make(x) if make else x
        ids, lg = _solo(m, (id(m), seconds, s, make is not None, tuple(sorted(kw.items()))), x, t, **kw)
        if 2 * _stop(lg, TOL) >= len(ids):
            return x, ids, lg
        print(f"clip {seconds} s seed {s}: first near-tie at {_stop(lg, TOL)} of {len(ids)} ids: another seed")
    raise AssertionError(f"no seed from {seed} on gives a {seconds} s clip that can carry an ids claim")


def _counts(pkg):
    L = pkg.lib(); a = (C.c_uint64 * ATTN_SLOTS)(); g = (C.c_uint64 * len(GEMM_FORMS))()
    assert L.vox_debug_attn_launches(a, ATTN_SLOTS) == 0 and L.vox_debug_gemm_launches(g, len(GEMM_FORMS)) == 0
    return [int(x) for x in a] + [int(x) for x in g]


def _state(g):
    return g.pool(), [g.pages(k) for k in range(g.n_members)], [{a: b for a, b in g.info(k).items() if a != "bytes"} for k in range(g.n_members)]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


PAGED = dict(max_positions=256, page_rows=16, pool_pages=32)


def test_one_tick_per_call_is_the_plain_group_bit_for_bit(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    clips = [pkg.synth.synth_audio(5.0 - 0.5 * k, seed=311 + k) for k in range(3)]
    cuts = [0, 40] + list(range(40 + TICK, 80000, TICK))      # the first tick is due at 40 samples, one more every 2560
    out = {}
    for name, kw in (("plain", {}), ("burst", {"burst": B})):
        g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], enc_capacity_rows=832, **PAGED, **kw)
        try:
            for k in range(3):
                g.tap_arm(k, 128)
            g.set_scores(0, True); g.set_alternatives(2, 3)
            ids = [[] for _ in range(3)]; states = []
            for c, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
                feeds = {k: clips[k][a:b] for k in range(3) if c >= 2 * k and b <= len(clips[k])}      # member k joins 2 k calls late and leaves early: rounds of 1, 2 and 3 members
                got = g.advance(feeds)      # (no finish: its right pad makes several ticks due in one pass)
                assert all(len(v) <= 1 for v in got.values())
                for k, v in got.items():
                    ids[k].extend(v)
                states.append(_state(g))
            out[name] = (ids, [g.tap_fetch(k) for k in range(3)], g.scores(0).copy(), g.alternatives(2).copy(), states, g.burst_info())
        finally:
            g.close()
    p, b = out["plain"], out["burst"]
    assert b[5]["burst"] == B and b[5]["burst_rounds"] == 0 and b[5]["burst_member_ticks"] == 0 and b[5]["plain_rounds"] >= 30
    assert p[5] == {**b[5], "burst": 1}
    for k in range(3):
        assert len(p[0][k]) >= 20 and p[0][k] == b[0][k] and np.array_equal(_words(p[1][k]), _words(b[1][k])), f"member {k}"
    assert p[2].tobytes() == b[2].tobytes() and p[3].tobytes() == b[3].tobytes() and p[4] == b[4]


def test_a_burst_of_one_group_has_a_plain_groups_launch_counts(pkg, ctx, gg, tiny):
    m = tiny; t = _t(pkg, m)
    clips = [pkg.synth.synth_audio(4.0, seed=411 + k) for k in range(3)]
    at = [_n_for(pkg, 37 + d) for d in (12, 5, 1)]
    out = {}
    for name, kw in (("plain", {}), ("one", {"burst": 1})):
        g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], **kw)
        try:
            g.tap_arm(0, 128)
            c0 = _counts(pkg); a0 = gg.stream_attn_burst_launches()
            ids = g.advance({k: clips[k][:at[k]] for k in range(3)})
            rest = g.advance({k: clips[k][at[k]:] for k in range(3)}, finish=[0, 1, 2])
            c1 = _counts(pkg)
            assert gg.stream_attn_burst_launches() == a0
            out[name] = ([int(b - a) for a, b in zip(c0, c1)], [np.concatenate([ids[k], rest[k]]) for k in range(3)], g.tap_fetch(0), g.burst_info(), [g.info(k)["bytes"] for k in range(3)])
        finally:
            g.close()
    p, o = out["plain"], out["one"]
    assert sum(p[0]) > 100 and p[0] == o[0], (p[0], o[0])
    assert o[3]["burst"] == 1 and o[3]["burst_rounds"] == 0 and o[3] == p[3] and p[3]["plain_rounds"] >= 12
    assert all(np.array_equal(a, b) for a, b in zip(p[1], o[1])) and np.array_equal(_words(p[2]), _words(o[2]))
    assert p[4] == o[4]      # the same allocations


def test_backlogs_of_40_7_and_1_ticks_in_one_call(pkg, ctx, gg, tiny):
    m = tiny; t = _t(pkg, m); EL = m.config.enc_layers
    clips = [_clip(pkg, m, t, 8.0, 520 + k) for k in range(3)]
    at = [_n_for(pkg, 37 + d) for d in (40, 7, 1)]
    g = m.create_stream_group(t, 3, gains=[_gain(c[0]) for c in clips], burst=B)
    try:
        a0 = gg.stream_attn_burst_launches()
        first = g.advance({k: clips[k][0][:at[k]] for k in range(3)})
        got = _bi(g); passes = [_passes(pkg, [(at[k], 0)])[0] for k in range(3)]
        want = _rounds_of(gg, passes, B)
        print(f"40, 7 and 1 ticks due in one call: passes {passes}, burst_info {got}")
        assert [len(first[k]) for k in range(3)] == [40, 7, 1]
        assert passes == [[26, 14], [7], [1]] and got == want == (3, 48, 0)
        assert gg.stream_attn_burst_launches() - a0 == EL * got[0]
        assert [g.info(k)["operator_steps"] for k in range(3)] == [40, 7, 1]
        rest = g.advance({k: clips[k][0][at[k]:] for k in range(3)}, finish=[0, 1, 2])
        calls = [[(at[k], 0), (len(clips[k][0]) - at[k], 1)] for k in range(3)]
        per_call = [_rounds_of(gg, [_passes(pkg, calls[k])[c] for k in range(3)], B) for c in range(2)]
        assert _bi(g) == tuple(sum(v) for v in zip(*per_call)), (_bi(g), per_call)
    finally:
        g.close()
    for k in range(3):
        same = _held(np.concatenate([first[k], rest[k]]), clips[k][1], clips[k][2], f"member {k} of the burst group", TOL)
        print(f"member {k}: {same} of {len(clips[k][1])} ids equal to the solo plain stream's")


@pytest.fixture(scope="module")
def worker_run(tmp_path_factory):
    r = run_worker("stream_group_burst_worker.py", tmp_path_factory.mktemp("group_burst"), 600)
    print(r[1][-1500:])
    return r


@pytest.mark.parametrize("name", ["test_slab_paged_and_endless_burst_groups_agree_bit_for_bit", "test_bf16_burst_group_against_the_f32_paged_burst_group"])
def test_worker_case(worker_run, name):
    """tests/stream_group_burst_worker.py, in a process of its own (the endless and the bf16 group's attention forms count in slots other tests hold to 0)."""
    check(worker_run, name)


def test_every_case_of_the_worker_is_asserted_here(worker_run):
    assert set(worker_run[0]) == {"test_slab_paged_and_endless_burst_groups_agree_bit_for_bit", "test_bf16_burst_group_against_the_f32_paged_burst_group"}


def test_a_peek_on_a_backlog_leaves_the_group_as_it_was(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    clips = [_clip(pkg, m, t, 8.0, 520 + k) for k in range(2)]
    cuts = [(0, 30000), (30000, 80123), (80123, 110000), (110000, 128000)]
    out = {}
    for name in ("twin", "peeks"):
        g = m.create_stream_group(t, 2, gains=[_gain(c[0]) for c in clips], burst=B, **PAGED)
        try:
            g.tap_arm(0, 256); g.tap_arm(1, 256)
            per = []; peeked = None
            for a, b in cuts:
                per.append(g.advance({0: clips[0][0][a:b], 1: clips[1][0][a:b]}, finish=[0, 1] if b == 128000 else []))
                if name == "peeks" and b in (80123, 110000):
                    before = (_state(g), g.burst_info()); got = g.peek([0, 1])
                    assert (_state(g), g.burst_info()) == before
                    peeked = got if b == 80123 else peeked
            out[name] = (per, [g.tap_fetch(0), g.tap_fetch(1)], _state(g), g.burst_info(), peeked)
        finally:
            g.close()
    per, lg, state, bi, peeked = out["peeks"]; tw = out["twin"]
    assert bi["burst_rounds"] >= 4 and len(peeked[0]) >= 8 and len(peeked[1]) >= 8      # every call ran a burst round; the tail: the right pad's ticks, several due in one pass
    assert all(np.array_equal(a[k], b[k]) for a, b in zip(per, tw[0]) for k in (0, 1))
    assert all(np.array_equal(_words(a), _words(b)) for a, b in zip(lg, tw[1])) and state == tw[2] and bi == tw[3]
    for k in (0, 1):
        _held(np.concatenate([p[k] for p in per]), clips[k][1], clips[k][2], f"member {k} around the peeks", TOL)
        assert len(per[0][k]) + len(per[1][k]) + len(peeked[k]) == pkg.stream_schedule(80123, True)[1]      # the utterance that ends at the cut


def test_a_blob_taken_after_burst_rounds_continues_in_a_plain_group(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    x, rids, rlg = _clip(pkg, m, t, 8.0, 520)
    n40 = _n_for(pkg, 77)
    gb = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, burst=B); gp = m.create_stream_group(t, 2)
    try:
        head = gb.advance({0: x[:n40], 1: x[:_n_for(pkg, 40)]})[0]
        assert _bi(gb)[0] == 3 and len(head) == 40
        gp.restore(1, gb.snapshot(0))
        assert gp.info(1)["positions"] == 77 and gp.burst_info()["burst"] == 1
        ids = np.concatenate([head, gp.advance({1: x[n40:]}, finish=[1])[1]])
        assert gp.burst_info()["burst_rounds"] == 0 and gp.burst_info()["plain_rounds"] == len(ids) - 40 >= 10      # (a plain round per tick, an id per tick)
    finally:
        gb.close(); gp.close()
    _held(ids, rids, rlg, "a plain group's member restored from a burst group's blob", TOL)


def test_scores_and_alternatives_are_the_records_of_the_tapped_rows(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); xs = [pkg.synth.synth_audio(6.0 - k, seed=311 + k) for k in range(2)]
    g = m.create_stream_group(t, 2, gains=[_gain(x) for x in xs], burst=B)
    try:
        for k in (0, 1):
            g.tap_arm(k, 128); g.set_scores(k, True); g.set_alternatives(k, 3)
        out = g.advance({0: xs[0], 1: xs[1]}, finish=[0, 1])
        assert g.burst_info()["burst_rounds"] >= 2
        for k in (0, 1):
            ids, lg, sc, al = out[k], g.tap_fetch(k), g.scores(k), g.alternatives(k)
            assert len(ids) == len(sc) == len(al) == lg.shape[0] >= 30 and np.array_equal(sc["id"], ids) and np.array_equal(lg.argmax(axis=1), ids)
            assert sc.tobytes() == pkg.score_rows(ctx, lg, ids).tobytes()
            assert al.tobytes() == pkg.alternatives_rows(ctx, lg, 3).tobytes()
    finally:
        g.close()


def test_a_member_fed_48_khz_pcm_with_a_backlog(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    pcm = lambda x: (np.clip(x, -1, 1) * 32767).astype(np.int16)
    x48, rids, rlg = _clip(pkg, m, t, 24.0, 7520, make=pcm, sample_rate=48000)      # 24 s of 16 kHz samples played as 8 s at 48 kHz
    x16, sids, slg = _clip(pkg, m, t, 8.0, 521, make=pcm)
    g = m.create_stream_group(t, 2, gains=[_gain(x48), _gain(x16)], sample_rates=[48000, 16000], burst=B)
    try:
        n48 = 3 * 48000 + 77; n16 = _n_for(pkg, 38)
        first = g.advance({0: x48[:n48], 1: x16[:n16]})      # every fed array is int16: the 16-bit call
        assert len(first[0]) >= 15 and len(first[1]) == 1 and _bi(g)[0] >= 2
        rest = g.advance({0: x48[n48:], 1: x16[n16:]}, finish=[0, 1])
    finally:
        g.close()
    _held(np.concatenate([first[0], rest[0]]), rids, rlg, "the 48 kHz member", TOL)
    _held(np.concatenate([first[1], rest[1]]), sids, slg, "the 16 kHz member", TOL)


def _device_free_bytes():
    hip = C.CDLL("libamdhip64.so"); free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_default_ring_capacity_and_the_refusal_of_a_small_one(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); w = m.config.enc_window
    assert w == 750
    before = _device_free_bytes()
    for kw in ({}, PAGED, dict(page_rows=16, pool_pages=32, endless=True)):
        with pytest.raises(pkg.VoxError) as e:
            m.create_stream_group(t, 16, burst=16, enc_capacity_rows=w + 64, **kw)
        assert e.value.code == 1 and str(w + 64) in str(e.value) and "burst_ticks" in str(e.value), e.value
    after = _device_free_bytes()
    assert abs(after - before) <= 1 << 20, (before, after)
    g = m.create_stream_group(t, 16, burst=16, enc_capacity_rows=w + 65)
    took = after - _device_free_bytes(); g.close()
    print(f"a refused create moved the free memory by {after - before} bytes; a 16-member B = 16 group of the tiny model takes {took >> 20} MiB")
    assert took > 8 << 20
    for burst, cap in ((1, 768), (4, 832), (16, 832)):
        g = m.create_stream_group(t, 1, burst=burst)
        try:
            g.advance({0: np.zeros(TICK * 230, np.float32)})      # 920 encoder rows: the ring is full
            assert g.info(0)["ring_rows"] == cap == (max(w + 4 * burst + 4, 148) + 63) // 64 * 64
        finally:
            g.close()


def test_full_size_40_and_5_ticks_in_one_call(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    try:
        t = _t(pkg, m); x = pkg.synth.synth_audio(16.0, seed=7049)
        at = [_n_for(pkg, 77), _n_for(pkg, 42)]
        out = {}
        for name, kw in (("plain", {}), ("burst", {"burst": B})):
            g = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, enc_capacity_rows=832, **kw)
            try:
                g.tap_arm(0, 128); g.tap_arm(1, 128)
                first = g.advance({0: x[:at[0]], 1: x[:at[1]]})
                assert [len(first[k]) for k in (0, 1)] == [40, 5]
                assert _bi(g) == ((3, 45, 0) if name == "burst" else (0, 0, 40))
                rest = g.advance({0: x[at[0]:], 1: x[at[1]:]}, finish=[0, 1])
                out[name] = ([np.concatenate([first[k], rest[k]]) for k in (0, 1)], [g.tap_fetch(0), g.tap_fetch(1)])
            finally:
                g.close()
    finally:
        m.close()
    for k in (0, 1):
        rids, rlg = out["plain"][0][k], out["plain"][1][k]
        assert rlg.shape[0] == len(rids) and np.array_equal(rlg.argmax(axis=1), rids)
        same = _held(out["burst"][0][k], rids, rlg, f"full size, member {k}", TOL)
        print(f"full size, member {k}: {same} of {len(rids)} ids equal to the plain group's")
