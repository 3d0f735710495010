"""Stream groups with a delay (t_embed) per member (vox_stream_group_create_t_embeds, vox_stream_group_reset_t_embed, vox_stream_group_t_embed; DESIGN.md section 8,
"A delay per member") on the tiny model.  The symbols do not exist on the parent commit.

Every comparison is == : ids and which call returns them, the tapped f32 logits rows as bits, score and alternatives records as bytes, pool() after every call.  No
tolerance anywhere.  The reference of member k of a mixed group G (delays 2, 6, 10) is member k of the uniform group U_k, every member at delay d_k, made by an
EXISTING creator and given the same calls -- so every round has the same width in all four groups and the same kernels run.

 * slab, paged, burst (a pass with due = (5, 1, 2) at burst 4, so that decode rounds serve a strict prefix of the order), endless paged and bf16 pool: G against U_k;
 * not vacuous: U_0 and U_2 (delays 2 and 10) differ in a logit bit within the first 10 ids of member 0;
 * three equal t_embeds through the new creator: the existing creator's group, bit for bit, member by member;
 * reset_t_embed(member 1, delay 10): its next utterance is member 1 of U_2's after a reset; refused resets change nothing (against an untouched twin);
 * a member's blob restores into its slot of the mixed group and continues bit for bit; into a member at another delay it is refused (VOX_ERR_INVALID, the member named);
 * offline vox_transcribe_audio calls at their own delays between the advances return what they return alone, and the group's ids are an undisturbed twin's."""
import ctypes as C

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _t

pytestmark = pytest.mark.gpu
TICK = 2560
DELAYS = (2.0, 6.0, 10.0)
KINDS = {"slab": {}, "paged": dict(max_positions=256, page_rows=16, pool_pages=32), "burst": dict(burst=4),
         "endless": dict(endless=True, page_rows=16, pool_pages=48), "bf16": dict(kv_dtype="bf16", max_positions=256, page_rows=16, pool_pages=32)}


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
def clips(pkg):
    xs = [pkg.synth.synth_audio(4.0 - 0.5 * k, seed=911 + k) for k in range(3)]
    for x in xs:
        x.setflags(write=False)
    return xs


def _n_for(pkg, positions):
    """The fewest 16 kHz samples after which `positions` decoder positions are determined (an unfinished stream)."""
    n = max(0, (positions - 38) * TICK)
    while pkg.stream_schedule(n, False)[0] < positions:
        n += 1
    return n


def _calls(pkg, clips):
    """The calls every group of a comparison gets: a first one that leaves 5, 1 and 2 ticks due, one of three more ticks each, the rest with finish."""
    at = [_n_for(pkg, 37 + d) for d in (5, 1, 2)]
    return [({k: (0, at[k]) for k in range(3)}, ()), ({k: (at[k], at[k] + 3 * TICK) for k in range(3)}, ()),
            ({k: (at[k] + 3 * TICK, len(clips[k])) for k in range(3)}, (0, 1, 2))]


def _arm(g, members=(0, 1, 2)):
    for k in members:
        g.tap_arm(k, 128); g.set_scores(k, True); g.set_alternatives(k, 3)
    return g


def _feed(g, clips, calls, rec):
    """Run `calls` ([({member: (a, b)}, finish)]) on g; rec[k] collects member k's ids per call, rec["pool"] the pool after every call of a paged group."""
    for feeds, fin in calls:
        got = g.advance({k: clips[k][a:b] for k, (a, b) in feeds.items()}, finish=fin)
        for k in feeds:
            rec.setdefault(k, []).append([int(v) for v in got[k]])
        if g.paged:
            p = g.pool(); rec.setdefault("pool", []).append({a: (b.tolist() if isinstance(b, np.ndarray) else b) for a, b in p.items()})
    return rec


def _drain(g, rec, members=(0, 1, 2)):
    for k in members:
        rec[("lg", k)] = g.tap_fetch(k); rec[("sc", k)] = g.scores(k).tobytes(); rec[("al", k)] = g.alternatives(k).tobytes()
    return rec


def _run(m, clips, calls, kind, t_embed=None, **per_member):
    g = _arm(m.create_stream_group(t_embed, 3, gains=[_gain(x) for x in clips], **KINDS[kind], **per_member))
    try:
        rec = _drain(g, _feed(g, clips, calls, {}))
        rec["burst"] = g.burst_info()
        return rec
    finally:
        g.close()


def _member_equal(a, b, k, label):
    assert a[k] == b[k], f"{label}: member {k}: ids per call {a[k]} against {b[k]}"
    la, lb = a[("lg", k)], b[("lg", k)]
    assert la.shape == lb.shape and la.shape[0] == sum(len(c) for c in a[k]) >= 10, (label, k, la.shape, lb.shape)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), f"{label}: member {k}: logits rows {np.unique(np.nonzero(la.view(np.uint32) != lb.view(np.uint32))[0])[:8]} differ"
    assert a[("sc", k)] == b[("sc", k)], f"{label}: member {k}: score records differ"
    assert a[("al", k)] == b[("al", k)], f"{label}: member {k}: alternatives records differ"


_UNIFORM = {}      # (kind, delay) -> the record of the uniform group: computed once, shared, read-only


def _uniform(pkg, m, clips, calls, kind, delay):
    if (kind, delay) not in _UNIFORM:
        _UNIFORM[(kind, delay)] = _run(m, clips, calls, kind, t_embed=_t(pkg, m, delay))
    return _UNIFORM[(kind, delay)]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_mixed_group_is_the_uniform_groups_member_by_member(pkg, tiny, clips, kind):
    m = tiny; calls = _calls(pkg, clips)
    G = _run(m, clips, calls, kind, delays=DELAYS)
    for k, d in enumerate(DELAYS):
        U = _uniform(pkg, m, clips, calls, kind, d)
        _member_equal(G, U, k, f"{kind}: mixed against uniform at delay {d}")
        assert G.get("pool") == U.get("pool"), (kind, d)
        assert G["burst"] == U["burst"]
    if kind == "burst":      # the pass of the first call ran (4, 1, 2) then (1): a burst round whose late decode rounds serve a strict prefix of the order
        assert G["burst"]["burst"] == 4 and G["burst"]["burst_rounds"] >= 2 and G["burst"]["burst_member_ticks"] >= 7


def test_the_delay_decides_logit_bits_within_ten_ids(pkg, tiny, clips):
    calls = _calls(pkg, clips)
    a, b = _uniform(pkg, tiny, clips, calls, "slab", DELAYS[0]), _uniform(pkg, tiny, clips, calls, "slab", DELAYS[2])
    la, lb = a[("lg", 0)][:10], b[("lg", 0)][:10]
    assert la.shape == lb.shape and la.shape[0] == 10
    assert (la.view(np.uint32) != lb.view(np.uint32)).any(), "delays 2 and 10 give the same logits on this fixture: the mixed-group comparison would show nothing"


def test_equal_t_embeds_are_the_existing_creators_group(pkg, tiny, clips):
    m = tiny; calls = _calls(pkg, clips); t = _t(pkg, m, 6.0)
    for kind in ("slab", "paged"):
        U = _uniform(pkg, m, clips, calls, kind, 6.0)
        E = _run(m, clips, calls, kind, t_embeds=[t, t, t])
        for k in range(3):
            _member_equal(E, U, k, f"{kind}: three equal t_embeds")
        assert E.get("pool") == U.get("pool")


def test_t_embed_reads_a_members_back(pkg, tiny):
    m = tiny; ts = [_t(pkg, m, d) for d in DELAYS]
    g = m.create_stream_group(None, 3, delays=DELAYS)
    u = m.create_stream_group(ts[1], 2); v = m.create_stream_group(ts[0], 3)
    try:
        for k in range(3):
            assert np.array_equal(g.t_embed(k).view(np.uint32), ts[k].view(np.uint32))
        assert all(np.array_equal(u.t_embed(k).view(np.uint32), ts[1].view(np.uint32)) for k in range(2))
        with pytest.raises(pkg.VoxError) as e:
            u.reset(0, 1.0, delay=10.0)      # a group of one t_embed has no per-member delay
        assert e.value.code == 5
        assert g.info(0)["bytes"] - v.info(0)["bytes"] == m.config.dec_layers * m.config.dec_dim * 4      # the Ada block, per member
    finally:
        g.close(); u.close(); v.close()


def test_reset_to_another_delay(pkg, tiny, clips):
    m = tiny; calls = _calls(pkg, clips); L = pkg.lib()
    x = clips[1]; again = [({1: (0, len(x) // 2)}, ()), ({1: (len(x) // 2, len(x))}, (1,))]
    out = {}
    for name, kw in (("mixed", dict(delays=DELAYS)), ("twin", dict(delays=DELAYS)), ("u2", dict(t_embed=_t(pkg, m, DELAYS[2])))):
        g = _arm(m.create_stream_group(kw.pop("t_embed", None), 3, gains=[_gain(c) for c in clips], **kw))
        try:
            rec = _feed(g, clips, calls[:2], {})
            if name == "mixed":      # refused resets: the member, its delay and its state stay
                te = np.ascontiguousarray(_t(pkg, m, 10.0))
                before = [g.info(k) for k in range(3)]
                assert L.vox_stream_group_reset_t_embed(g.h, 1, 1.0, 0, None) == 1
                assert L.vox_stream_group_reset_t_embed(g.h, 3, 1.0, 0, te.ctypes.data_as(C.c_void_p)) == 1
                assert L.vox_stream_group_reset_t_embed(g.h, 1, 1.0, 44101, te.ctypes.data_as(C.c_void_p)) == 5
                assert L.vox_stream_group_reset_t_embed(g.h, 1, float("nan"), 0, te.ctypes.data_as(C.c_void_p)) == 1
                assert [g.info(k) for k in range(3)] == before
                assert np.array_equal(g.t_embed(1).view(np.uint32), _t(pkg, m, DELAYS[1]).view(np.uint32))
            _feed(g, clips, calls[2:], rec); _drain(g, rec)
            out[name] = rec
            if name != "twin":      # member 1's next utterance, alone: at delay 10 in both groups
                if name == "mixed":
                    g.reset(1, _gain(x), delay=10.0)
                    assert np.array_equal(g.t_embed(1).view(np.uint32), _t(pkg, m, 10.0).view(np.uint32))
                else:
                    g.reset(1, _gain(x))
                g.tap_arm(1, 128)
                out[name + "/next"] = _drain(g, _feed(g, clips, again, {}), members=(1,))
        finally:
            g.close()
    for k in range(3):
        _member_equal(out["mixed"], out["twin"], k, "after the refused resets against an untouched twin")
    _member_equal(out["mixed/next"], out["u2/next"], 1, "member 1 reset to delay 10 against the uniform group at delay 10")
    assert out["mixed/next"][1] != out["mixed"][1] or not np.array_equal(out["mixed/next"][("lg", 1)], out["mixed"][("lg", 1)])      # the delay took effect


def test_snapshot_and_restore_in_a_mixed_group(pkg, tiny, clips):
    m = tiny; calls = _calls(pkg, clips)
    out = {}
    for name in ("twin", "mixed"):
        g = _arm(m.create_stream_group(None, 3, gains=[_gain(c) for c in clips], delays=DELAYS))
        try:
            rec = _feed(g, clips, calls[:2], {})
            if name == "mixed":
                blob = g.snapshot(1)
                before = [g.info(k) for k in range(3)]
                with pytest.raises(pkg.VoxError) as e:      # member 0 runs at delay 2, the blob's session at delay 6
                    g.restore(0, blob)
                assert e.value.code == 1 and "member 0" in str(e.value) and "t_embed" in str(e.value), str(e.value)
                assert [g.info(k) for k in range(3)] == before
                head = {k: (g.tap_fetch(k), g.scores(k), g.alternatives(k)) for k in (1,)}      # member 1's rows so far: a reset starts its records over
                g.reset(1, 1.0); g.restore(1, blob); g.tap_arm(1, 128)
            _feed(g, clips, calls[2:], rec); _drain(g, rec)
            if name == "mixed":
                rec[("lg", 1)] = np.concatenate([head[1][0], rec[("lg", 1)]])
            out[name] = rec
        finally:
            g.close()
    for k in range(3):
        _member_equal(out["mixed"], out["twin"], k, "restored into its slot of the mixed group")


def test_offline_calls_between_the_advances_leave_the_group_alone(pkg, tiny, clips):
    m = tiny; calls = _calls(pkg, clips)
    off = [(clips[2], _t(pkg, m, 3.0)), (clips[0], _t(pkg, m, 8.0))]
    alone = [m.transcribe_audio(x, t).copy() for x, t in off]
    assert all(len(a) >= 10 for a in alone)
    twin = _run(m, clips, calls, "slab", delays=DELAYS)
    g = _arm(m.create_stream_group(None, 3, gains=[_gain(c) for c in clips], delays=DELAYS))
    try:
        rec = {}
        for i, call in enumerate(calls):
            x, t = off[i % 2]
            assert np.array_equal(m.transcribe_audio(x, t), alone[i % 2]), f"offline call {i}"
            _feed(g, clips, [call], rec)
        assert np.array_equal(m.transcribe_audio(*off[1]), alone[1])
        _drain(g, rec)
    finally:
        g.close()
    for k in range(3):
        _member_equal(rec, twin, k, "offline calls interleaved")
