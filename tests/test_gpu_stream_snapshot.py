"""Snapshot and resume of a solo live session (vox_stream_snapshot, vox_stream_restore; include/voxtral_hip.h, SNAPSHOT AND RESUME) on the tiny model.

Every comparison is == on ids (and on which call returns them), on tapped f32 logits rows, on score and alternatives records and on vox_stream_info words 0-3
(word 4 is the fill of the stream's OWN encoder ring, min(word 3, its capacity): checked against the restored stream's capacity): no tolerance anywhere.  The
reference is a twin session on the same model that is never interrupted and is fed the same calls; the interrupted session is snapshotted at a cut, FREED, created
anew -- with another encoder ring capacity (760 rows), so that the ring rows land at other slots -- and restored.  All sessions run with the logits tap, scores on
and alternatives at k = 3, and are fed from one device-resident clip.  The position-1030 case takes about a second on the GPU and runs in-process."""
import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _t

pytestmark = pytest.mark.gpu

TICK = 2560      # 16 kHz samples per decoder position


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
def clip(pkg, ctx):
    """(host samples, device pointer, gain): 172 s, enough for position 1030 and a tail"""
    x = pkg.synth.synth_audio(172.0, seed=31); x.setflags(write=False)
    p = ctx.upload(x)
    yield x, p, _gain(x)
    ctx.free(p)


def _arm(st, tap=1200):
    st.tap_arm(tap); st.set_scores(True); st.set_alternatives(3)
    return st


def _words(st):
    """vox_stream_info words 0-3; word 4, the rows held in the encoder ring, is min(word 3, the stream's OWN ring capacity) and is checked where the capacity is known"""
    i = st.info()
    return [i[k] for k in ("samples", "positions", "ids", "encoder_position")]


class Walk:
    """One session's record: ids per call, logits rows, info words after every call"""

    def __init__(self):
        self.per, self.words, self.rows = [], [], []

    def call(self, st, ids):
        self.per.append(ids); self.words.append(_words(st))

    def drain(self, st):
        self.rows.append(st.tap_fetch())

    def lg(self):
        return np.concatenate(self.rows)


def _push(st, dev, a, b, sample=4, dtype=None):
    return st.push(device_ptr=dev + sample * a, n_samples=b - a, dtype=dtype)


def _run(st, dev, pieces, finish=True, w=None, **kw):
    """push the pieces (sample ranges), then finish; -> the Walk (extended when given)"""
    w = w or Walk()
    for a, b in pieces:
        w.call(st, _push(st, dev, a, b, **kw))
    if finish:
        w.call(st, st.finish())
    return w


def _same(a, b, label, words=True):
    assert len(a.per) == len(b.per), label
    for k, (u, v) in enumerate(zip(a.per, b.per)):
        assert np.array_equal(u, v), f"{label}: call {k} returned {u}, the uninterrupted session's {v}"
    assert not words or a.words == b.words, (label, a.words, b.words)
    la, lb = a.lg(), b.lg()
    assert la.shape == lb.shape and len(la) == sum(len(p) for p in a.per), (label, la.shape, lb.shape)
    assert np.array_equal(la, lb), f"{label}: logits rows {np.unique(np.nonzero(la != lb)[0])[:8]} differ from the uninterrupted session's"
    assert a.rec.tobytes() == b.rec.tobytes(), f"{label}: score records differ"
    assert a.alt.tobytes() == b.alt.tobytes(), f"{label}: alternatives records differ"


def _close(st, w):
    w.drain(st); w.rec = st.scores(); w.alt = st.alternatives()
    st.close()
    return w


def _pieces(cut, end):
    """two calls up to the cut (none for cut 0), two behind it"""
    head = [(0, cut // 2), (cut // 2, cut)] if cut else []
    return head, [(cut, (cut + end) // 2), ((cut + end) // 2, end)]


def _uninterrupted(m, t, clip, cut, end):
    _, dev, gain = clip
    head, tail = _pieces(cut, end)
    st = _arm(m.create_stream(t, gain=gain))
    return _close(st, _run(st, dev, head + tail))


def _interrupted(pkg, m, t, clip, cut, end, make=None, via_device=None):
    """push to the cut, snapshot (twice: the blobs are identical), free, create anew, restore, go on.  -> (Walk, blob)"""
    _, dev, gain = clip
    head, tail = _pieces(cut, end)
    st = _arm(m.create_stream(t, gain=gain))
    w = _run(st, dev, head, finish=False)
    before = st.info()
    blob = st.snapshot()
    assert st.info() == before      # words, steps and info[5]: the staging area is gone
    assert st.snapshot().tobytes() == blob.tobytes()
    info = pkg.snapshot_info(blob)
    assert info["total_bytes"] == blob.size == pkg.snapshot_bytes_for(m.config, before["positions"], 16000, before["samples"], scores=True, alternatives=True)
    assert (info["positions"], info["ids"], info["samples_pushed"], info["scores"], info["alternatives"]) == (before["positions"], before["ids"], cut, 1, 3)
    if via_device is not None:      # the same blob written to device memory, byte for byte, and restored from there
        p = via_device.alloc(blob.size)
        assert st.snapshot(device_ptr=p) == blob.size
        assert via_device.download(p, blob.size, np.uint8).tobytes() == blob.tobytes()
    w.drain(st); st.close()
    st2 = _arm((make or (lambda: m.create_stream(t, gain=0.123, enc_capacity_rows=760)))())      # (the restore takes the blob's gain)
    if via_device is not None:
        st2.restore(device_ptr=p, nbytes=blob.size); via_device.synchronize(); via_device.free(p)
    else:
        st2.restore(blob)
    assert _words(st2) == [before[k] for k in ("samples", "positions", "ids", "encoder_position")]
    assert make is not None or st2.info()["ring_rows"] == min(before["encoder_position"], 760)
    return _close(st2, _run(st2, dev, tail, w=w)), blob


CUTS = {"cut0": (0, 60 * TICK), "mid_tick": (40 * TICK + 777, 70 * TICK + 5), "ring_wrapped": (200 * TICK + 1, 230 * TICK)}


@pytest.mark.parametrize("case", list(CUTS))
def test_restore_continues_bit_for_bit(pkg, tiny, clip, case):
    cut, end = CUTS[case]
    t = _t(pkg, tiny)
    a = _uninterrupted(tiny, t, clip, cut, end)
    b, _ = _interrupted(pkg, tiny, t, clip, cut, end)
    assert sum(len(p) for p in a.per) >= 20
    _same(b, a, case)
    if case == "ring_wrapped":
        assert a.words[1][3] > 760      # the 760-row ring of the restored session had wrapped at the cut


def test_restore_past_the_cache_doubling_and_the_engine_hand_over(pkg, tiny, clip):
    """position 1030, reached by ONE bulk push: the decoder cache has doubled to 2048 rows and the steps have left the decode engine; the restored session gets the
    2048-row cache the rule gives and goes on on the per-operator path"""
    t = _t(pkg, tiny)
    cut = next(n for n in range(900 * TICK, 1040 * TICK, 128) if pkg.stream_schedule(n)[0] >= 1030); end = cut + 12 * TICK
    _, dev, gain = clip

    def run(interrupt):
        st = _arm(tiny.create_stream(t, gain=gain)); w = _run(st, dev, [(0, cut)], finish=False)
        assert st.info()["positions"] in (1030, 1031)
        if interrupt:
            blob = st.snapshot(); w.drain(st); st.close()
            st = _arm(tiny.create_stream(t, gain=gain, enc_capacity_rows=760)); st.restore(blob)
        w = _run(st, dev, [(cut, end)], w=w)
        steps = st.info()
        return _close(st, w), steps

    (a, sa), (b, sb) = run(False), run(True)
    _same(b, a, "position 1030")
    assert sb["engine_steps"] == 0 and sb["operator_steps"] == len(b.per[1]) + len(b.per[2])      # behind position 1024 no step is the engine's, restored or not
    assert sa["operator_steps"] >= sb["operator_steps"]


def test_a_48k_16_bit_stream_cut_inside_a_resampling_block(pkg, ctx, tiny):
    t = _t(pkg, tiny)
    fi = pkg.resample_plan(48000, 16000)[0]
    x = (pkg.synth.synth_audio(40.0, seed=5) * 20000).astype(np.int16)      # 13.3 s at 48 kHz
    cut = (4 * 48000 // fi) * fi + fi // 2 + 1; end = 12 * 48000
    assert cut % fi not in (0, fi - 1) and cut > 3 * 48000
    dev = ctx.upload(x); gain = _gain(x)
    head, tail = _pieces(cut, end)
    try:
        def make(**kw):
            return _arm(tiny.create_stream(t, gain=gain, sample_rate=48000, **kw))
        sa = make(); a = _close(sa, _run(sa, dev, head + tail, sample=2, dtype="s16"))
        sb = make(); w = _run(sb, dev, head, finish=False, sample=2, dtype="s16")
        blob = sb.snapshot(); w.drain(sb); sb.close()
        info = pkg.snapshot_info(blob)
        ring = 1
        while ring < 2 * fi + (1 << 15):      # the input ring: a power of two holding two blocks and a feed chunk
            ring *= 2
        assert info["sample_rate"] == 48000 and info["samples_in"] == cut and info["section_bytes"][5] == 4 * min(cut, ring) and info["samples_16k"] < cut // 3
        sb = make(enc_capacity_rows=760); sb.restore(blob)
        b = _close(sb, _run(sb, dev, tail, w=w, sample=2, dtype="s16"))
        _same(b, a, "48 kHz s16")
    finally:
        ctx.free(dev)


def test_a_bounded_blob_into_an_endless_session_below_its_wrap(pkg, tiny, clip):
    cut, end = CUTS["mid_tick"]
    t = _t(pkg, tiny); gain = clip[2]
    a = _uninterrupted(tiny, t, clip, cut, end)
    b, _ = _interrupted(pkg, tiny, t, clip, cut, end, make=lambda: tiny.create_stream(t, gain=gain, enc_capacity_rows=760, endless=True))
    _same(b, a, "bounded -> endless")


def test_a_fork_and_a_device_blob(pkg, ctx, tiny, clip):
    """one blob into two streams (one of them from device memory), both fed the same tail: equal to each other and to the uninterrupted session"""
    cut, end = CUTS["mid_tick"]
    t = _t(pkg, tiny); _, dev, gain = clip
    a = _uninterrupted(tiny, t, clip, cut, end)
    b, blob = _interrupted(pkg, tiny, t, clip, cut, end, via_device=ctx)
    _same(b, a, "device blob")
    forks = [_arm(tiny.create_stream(t, gain=gain, enc_capacity_rows=c)) for c in (0, 900)]
    walks = []
    for st in forks:
        st.restore(blob)
    for st in forks:      # (interleaved: neither depends on the other)
        walks.append(_run(st, dev, _pieces(cut, end)[1][:1], finish=False))
    for st, w in zip(forks, walks):
        _close(st, _run(st, dev, _pieces(cut, end)[1][1:], w=w))
    n_head = len(_pieces(cut, end)[0]); rows_head = sum(len(p) for p in a.per[:n_head])
    for w in walks:
        assert all(np.array_equal(u, v) for u, v in zip(w.per, a.per[n_head:])) and len(w.per) == len(a.per) - n_head
        assert np.array_equal(w.lg(), a.lg()[rows_head:]) and w.rec.tobytes() == a.rec.tobytes() and w.alt.tobytes() == a.alt.tobytes()
        assert w.words == a.words[n_head:]


def test_snapshots_change_nothing(pkg, tiny, clip):
    """a session that snapshots after every call -- to host memory, so through the staging area -- gives the uninterrupted session's bits and reports the same footprint"""
    cut, end = CUTS["mid_tick"]
    t = _t(pkg, tiny); _, dev, gain = clip
    a = _uninterrupted(tiny, t, clip, cut, end)
    st = _arm(tiny.create_stream(t, gain=gain)); w = Walk(); blobs = []
    head, tail = _pieces(cut, end)
    for pa, pb in head + tail:
        w.call(st, _push(st, dev, pa, pb))
        before = st.info(); blobs.append(st.snapshot()); blobs.append(st.snapshot())
        assert st.info() == before and blobs[-1].tobytes() == blobs[-2].tobytes()      # info[5] included: the staging area was freed
    w.call(st, st.finish())
    with pytest.raises(pkg.VoxError, match="finished"):      # a finished source
        st.snapshot()
    _same(_close(st, w), a, "snapshot after every call")
    assert len({b.size for b in blobs}) == len(head + tail)      # the blob grows with the session


def test_refused_restores_leave_the_target_as_it_was(pkg, ctx, tiny, clip):
    cut, end = CUTS["mid_tick"]
    t = _t(pkg, tiny); x, dev, gain = clip
    a = _uninterrupted(tiny, t, clip, cut, end)
    head, tail = _pieces(cut, end)
    src = _arm(tiny.create_stream(t, gain=gain)); _run(src, dev, head, finish=False)
    blob = src.snapshot(); n = blob.size
    with pytest.raises(pkg.VoxError, match="capacity"):      # cap one byte short: nothing is written
        src.snapshot(cap=n - 1)
    bad = {}
    bad["truncated by a byte"] = (blob[:-1], "bytes")
    bad["truncated to 100 bytes"] = (blob[:100], "shorter than")
    flipped = blob.copy(); flipped[0] ^= 1
    bad["flipped magic"] = (flipped, "bad magic")
    other = pkg.Q4ModelLoader.from_file(tiny_gguf(seed=8)[0]).load(ctx)      # the tiny model at another seed
    try:
        so = other.create_stream(t, gain=gain); so.push(x[:cut]); bad["another model"] = (so.snapshot(), "another model"); so.close()
    finally:
        other.close()
    s5 = tiny.create_stream(_t(pkg, tiny, 5.0), gain=gain); s5.push(x[:cut]); bad["another t_embed"] = (s5.snapshot(), "another t_embed"); s5.close()
    s48 = tiny.create_stream(t, gain=gain, sample_rate=48000); s48.push(x[:cut]); bad["a rate mismatch"] = (s48.snapshot(), "48000 Hz"); s48.close()
    # the target: mid-utterance itself, so that a restore that wrote anything would show
    tgt = _arm(tiny.create_stream(t, gain=gain)); w = _run(tgt, dev, head[:1], finish=False)
    for label, (b, text) in bad.items():
        before = tgt.info()
        with pytest.raises(pkg.VoxError) as e:
            tgt.restore(b)
        assert text in str(e.value), (label, str(e.value))
        assert tgt.info() == before, label
    small = tiny.create_stream(t, gain=gain, max_positions=45); twin = tiny.create_stream(t, gain=gain, max_positions=45)      # a target with max_positions below D
    with pytest.raises(pkg.VoxError, match="created for 45"):
        small.restore(blob)
    assert np.array_equal(small.push(x[:5 * TICK]), twin.push(x[:5 * TICK])) and small.info() == twin.info()
    small.close(); twin.close()
    _same(_close(tgt, _run(tgt, dev, head[1:] + tail, w=w)), a, "after the refused restores")
    # ... and the source of all those snapshots is still the uninterrupted session
    ws = Walk(); ws.per = a.per[:len(head)]; ws.words = a.words[:len(head)]
    src.tap_fetch(); src.tap_arm(1200)
    s = _close(src, _run(src, dev, tail, w=ws))
    rows_head = sum(len(p) for p in a.per[:len(head)])
    assert all(np.array_equal(u, v) for u, v in zip(s.per, a.per)) and np.array_equal(s.lg(), a.lg()[rows_head:]) and s.rec.tobytes() == a.rec.tobytes()
