"""Stream-group members fed at their capture rate, as f32 or 16-bit PCM (vox_stream_group_create_rates, vox_stream_group_reset_rate, vox_stream_group_advance_s16;
DESIGN.md section 8, "Stream groups").

The invariant under test: a call in which every entry fits its rings in one pass runs exactly the rounds -- the same order, the same widths -- of a 16 kHz group fed, in
the same call, x16[a:b] per member, x16 = pkg.resample(ctx, x, sr), a and b the member's 16 kHz sample counts before and after the call (stream_schedule_rate's third
value; resample_len at finish).  Every 16 kHz sample a member consumes has vox_resample's bits, so every `==` here is bit for bit, on the ids AND on the tapped logits of
the compared members.  Only the push larger than both rings (other passes than the reference group's) uses the group's usual rule against the solo stream: _held at
TOL = 2e-4, the reference's first near-tie at or beyond half of the ids, otherwise another seed.  Every call must return exactly the ids the member's rate schedule says
became due.  Audio: noise plus a sine at the member's rate, the gain the peak gain of the resampled clip (as tests/test_gpu_stream_rate.py)."""
import ctypes as C

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _held, _raw_advance, _stop, _t

pytestmark = pytest.mark.gpu
TOL = 2e-4
RING16 = 65536      # a member's 16 kHz sample ring
RATES6 = [48000, 44100, 8000, 16000, 48000, 16000]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    yield m
    m.close()


def _loud(sr, n, seed):
    rng = np.random.default_rng(seed)
    return (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * (0.07 * 16000 / sr))).astype(np.float32)


def _pcm(sr, n, seed):
    rng = np.random.default_rng(seed)
    v = np.clip(np.round(9000.0 * rng.standard_normal(n) + 7000.0 * np.sin(np.arange(n) * (0.07 * 16000 / sr))), -32768, 32767).astype(np.int16)
    v[:4] = (-32768, 32767, -1, 1)      # the ends of the range
    return v


def _x16(pkg, ctx, x, sr):
    return pkg.resample(ctx, x, sr) if sr != 16000 else x


def _in_ring(pkg, sr):
    """The solo sizing rule: a power of two holding two blocks and a 32 768-sample feed chunk."""
    fft_in = pkg.resample_plan(sr)[0]; n = 1
    while n < 2 * fft_in + (1 << 15):
        n <<= 1
    return n


def _calls(lens, rates):
    """Every call feeds sr / 5 + 1 input samples per busy member (no multiple of any block, about 1.25 ticks); a member finishes with its last piece:
    [{member: (lo, hi, finish)}]."""
    calls = []; c = 0
    while True:
        call = {}
        for k, (n, sr) in enumerate(zip(lens, rates)):
            step = sr // 5 + 1; lo = c * step
            if lo < n:
                hi = min(n, lo + step); call[k] = (lo, hi, hi == n)
        if not call:
            return calls
        calls.append(call); c += 1


def _as16k(pkg, calls, rates):
    """The same calls for the 16 kHz reference group: member k is fed x16_k[a:b], a and b its 16 kHz sample counts before and after the call."""
    out = []
    for call in calls:
        out.append({k: (pkg.stream_schedule_rate(lo, rates[k])[2], pkg.stream_schedule_rate(hi, rates[k], finished=fin)[2], fin) for k, (lo, hi, fin) in call.items()})
    return out


def _run(pkg, g, rates, calls, feed, tap_rows=96):
    """The calls on group g, every member tapped: {ids, lg (per member), due (members that ticked, per call)}.  Every call is held to the members' schedules."""
    n = g.n_members
    for k in range(n):
        g.tap_arm(k, tap_rows)
    ids = [[] for _ in range(n)]; due = []
    for c, call in enumerate(calls):
        before = [g.info(k) for k in range(n)]
        out = feed(g, c, call)
        after = [g.info(k) for k in range(n)]
        assert set(out) == set(call)
        for k in range(n):
            if k not in call:
                assert after[k] == before[k]
                continue
            lo, hi, fin = call[k]
            assert before[k]["samples"] == lo and after[k]["samples"] == hi      # word [0] counts the samples as pushed, at the member's rate
            assert before[k]["ids"] + len(out[k]) == pkg.stream_schedule(hi, finished=fin, sample_rate=rates[k])[1] == after[k]["ids"], (c, k, lo, hi, fin)
            ids[k].extend(out[k])
        due.append(sum(1 for k in range(n) if after[k]["positions"] > before[k]["positions"]))
    lg = [g.tap_fetch(k) for k in range(n)]
    ids = [np.array(v, np.int32) for v in ids]
    for k in range(n):
        assert lg[k].shape[0] == len(ids[k]) and np.array_equal(lg[k].argmax(axis=1), ids[k])
    return dict(ids=ids, lg=lg, due=due)


def _host(clips):
    return lambda g, c, call: g.advance({k: clips[k][lo:hi] for k, (lo, hi, _) in call.items()}, finish=[k for k, v in call.items() if v[2]])


def _same(a, b, label, members=None):
    for k in (range(len(a["ids"])) if members is None else members):
        assert np.array_equal(a["ids"][k], b["ids"][k]), f"{label}, member {k}: ids differ ({len(a['ids'][k])} vs {len(b['ids'][k])})"
        assert a["lg"][k].shape == b["lg"][k].shape and np.array_equal(a["lg"][k], b["lg"][k]), f"{label}, member {k}: logits differ in rows {np.unique(np.nonzero(a['lg'][k] != b['lg'][k])[0])[:8]}"


def _pair(pkg, ctx, m, rates, clips):
    """(the rate group's run, the run of the 16 kHz group fed the resampled pieces in the same calls): the same gains, the same finish flags."""
    t = _t(pkg, m); x16 = [_x16(pkg, ctx, x, sr) for x, sr in zip(clips, rates)]; gains = [_gain(v) for v in x16]
    for x, v, sr in zip(clips, x16, rates):
        assert len(v) == pkg.stream_schedule_rate(len(x), sr, finished=True)[2]
    calls = _calls([len(x) for x in clips], rates)
    g = m.create_stream_group(t, len(rates), gains=gains, sample_rates=rates)
    try:
        assert [g.sample_rate(k) for k in range(len(rates))] == list(rates)
        a = _run(pkg, g, rates, calls, _host(clips))
    finally:
        g.close()
    r = m.create_stream_group(t, len(rates), gains=gains)
    try:
        b = _run(pkg, r, [16000] * len(rates), _as16k(pkg, calls, rates), _host(x16))
    finally:
        r.close()
    return a, b


def _lens6(extra=0):
    return [int(sr * (2.5 + 0.2 * k)) + 3 * k + 1 + extra for k, sr in enumerate(RATES6)]      # 2.5 .. 3.5 s, all distinct: the members finish in different calls


# ---- 1. equals the 16 kHz group of the resampled audio ----------------------------------------------------------------------------------------------------------------
def test_equals_the_16k_group_of_the_resampled_audio(pkg, ctx, model):
    lens = _lens6(); clips = [_loud(sr, n, 1200 + k) for k, (sr, n) in enumerate(zip(RATES6, lens))]
    ends = [-(-n // (sr // 5 + 1)) for n, sr in zip(lens, RATES6)]
    assert len(set(ends)) == 6      # every member finishes in a call of its own
    a, b = _pair(pkg, ctx, model, RATES6, clips)
    print(f"ids per member {[len(v) for v in a['ids']]}; members due per call {a['due']}")
    _same(a, b, "rate group vs the 16 kHz group of resample(x)")
    assert a["due"] == b["due"]
    assert all(len(v) >= 20 for v in a["ids"])
    assert max(a["due"]) >= 5 and 1 in a["due"]      # the encoder runs past 16 rows in one launch; a round of one


# ---- 2. both rings wrap -----------------------------------------------------------------------------------------------------------------------------------------------
def test_both_rings_wrap(pkg, ctx, model):
    rates = [48000, 44100, 8000]; secs = [5.0, 5.0, 9.0]
    clips = [_loud(sr, int(s * sr) + 11 * k + 1, 2200 + k) for k, (sr, s) in enumerate(zip(rates, secs))]
    for x, sr in zip(clips, rates):
        assert len(x) > _in_ring(pkg, sr) and pkg.resample_len(len(x), sr) > RING16, (sr, len(x), _in_ring(pkg, sr))
    a, b = _pair(pkg, ctx, model, rates, clips)
    _same(a, b, "rings wrapped: rate group vs the 16 kHz group of resample(x)")
    assert all(len(v) >= 20 for v in a["ids"])


# ---- 3. 16-bit PCM equals f32 -----------------------------------------------------------------------------------------------------------------------------------------
def test_s16_equals_f32(pkg, ctx, model):
    m = model; t = _t(pkg, m); L = pkg.lib(); rates = RATES6; lens = _lens6(5)
    pcm = [_pcm(sr, n, 3200 + k) for k, (sr, n) in enumerate(zip(rates, lens))]
    f32 = [v.astype(np.float32) / np.float32(32768) for v in pcm]
    gains = [_gain(_x16(pkg, ctx, x, sr)) for x, sr in zip(f32, rates)]
    calls = _calls(lens, rates)
    dev = [C.c_void_p() for _ in pcm]

    def run(feed):
        g = m.create_stream_group(t, 6, gains=gains, sample_rates=rates)
        try:
            return _run(pkg, g, rates, calls, feed), g.info(0)["bytes"]
        finally:
            g.close()

    def device(g, c, call):
        return g.advance({k: (dev[k].value + 2 * lo, hi - lo) for k, (lo, hi, _) in call.items()}, finish=[k for k, v in call.items() if v[2]], device=True, dtype="s16")

    ref, bytes_f32 = run(_host(f32))
    assert all(len(v) >= 20 for v in ref["ids"])
    host, bytes_s16 = run(_host(pcm))
    _same(host, ref, "int16 host arrays vs the same samples as float32")
    assert bytes_s16 > bytes_f32      # the staging area of the host 16-bit feeds is counted
    alt, _ = run(lambda g, c, call: (_host(pcm) if c % 2 else _host(f32))(g, c, call))
    _same(alt, ref, "advance and its 16-bit form alternating call by call")
    try:
        for d, v in zip(dev, pcm):
            pkg._lib.check(L.vox_dev_alloc(ctx.h, v.nbytes, C.byref(d))); pkg._lib.check(L.vox_dev_upload(ctx.h, d, v.ctypes.data, v.nbytes))
        got, bytes_dev = run(device)
    finally:
        for d in dev:
            if d.value:
                pkg._lib.check(L.vox_dev_free(ctx.h, d))
    _same(got, ref, "int16 device pointers vs float32")
    assert bytes_dev == bytes_f32      # device samples are read in place


# ---- 4. a push larger than both rings ---------------------------------------------------------------------------------------------------------------------------------
def _solo_clip(pkg, ctx, m, t, sr, n, seed):
    """(x, gain, ids, logits) of a solo stream at sr fed x whole; the seed moved on until the first near-tie lies at or beyond half of the ids."""
    for s in range(seed, seed + 12000, 1000):
        x = _loud(sr, n, s); gain = _gain(_x16(pkg, ctx, x, sr))
        st = m.create_stream(t, gain=gain, sample_rate=sr); st.tap_arm(256)
        try:
            ids = np.concatenate([st.push(x), st.finish()]); lg = st.tap_fetch()
        finally:
            st.close()
        assert lg.shape[0] == len(ids)
        if 2 * _stop(lg, TOL) >= len(ids):
            return x, gain, ids, lg
        print(f"{sr} Hz, seed {s}: first near-tie at {_stop(lg, TOL)} of {len(ids)} ids: another seed")
    raise AssertionError("no seed gives a clip that can carry an ids claim")


def test_a_push_larger_than_both_rings(pkg, ctx, model):
    m = model; t = _t(pkg, m)
    xa, ga, aids, alg = _solo_clip(pkg, ctx, m, t, 48000, 7 * 48000 + 5, 4100)
    xb, gb, bids, blg = _solo_clip(pkg, ctx, m, t, 16000, 3 * 16000 + 7, 4200)
    assert len(xa) > _in_ring(pkg, 48000) and pkg.resample_len(len(xa), 48000) > RING16
    g = m.create_stream_group(t, 2, gains=[ga, gb], sample_rates=[48000, 16000])
    try:
        cuts = [(a, min(len(xb), a + 3201)) for a in range(0, len(xb), 3201)]
        out = g.advance({0: xa, 1: xb[cuts[0][0]:cuts[0][1]]}, finish=[0])      # 336 005 samples in ONE call, with finish
        assert len(out[0]) == pkg.stream_schedule(len(xa), finished=True, sample_rate=48000)[1] and len(out[1]) == pkg.stream_schedule(cuts[0][1])[1]
        got = list(out[1])
        for a, b in cuts[1:]:
            ids = g.advance({1: xb[a:b]}, finish=[1] if b == len(xb) else [])[1]
            assert len(got) + len(ids) == pkg.stream_schedule(b, finished=b == len(xb))[1]
            got.extend(ids)
        assert g.info(0)["samples"] == len(xa) and g.info(1)["samples"] == len(xb)
        _held(out[0], aids, alg, "the 48 kHz member fed 7 s in one call", TOL)
        _held(np.array(got, np.int32), bids, blg, "the 16 kHz member next to it", TOL)
    finally:
        g.close()


# ---- 5. reset to another rate and reuse -------------------------------------------------------------------------------------------------------------------------------
def test_reset_to_another_rate_and_reuse(pkg, ctx, model):
    """Member 0 (16 kHz) is fed 40 samples in its first call and 2560 in every later one: exactly one tick per call wherever it is in its utterance, so a fresh group
    whose member 0 is fed the same way runs the rounds of the reused one."""
    m = model; t = _t(pkg, m)
    x0 = _loud(16000, 40 + 2560 * 80, 5100)
    xa = _loud(48000, int(2.5 * 48000) + 3, 5200); xb = _loud(8000, int(3.0 * 8000) + 5, 5300)
    g0 = _gain(x0); ga = _gain(_x16(pkg, ctx, xa, 48000)); gb = _gain(_x16(pkg, ctx, xb, 8000))
    fi8, fo8, _ = pkg.resample_plan(8000)[:3]; fi48, fo48, _ = pkg.resample_plan(48000)[:3]

    def utterance(g, x, sr, at):
        """x through member 1 in sr / 5 + 1-sample pieces while member 0 goes on from piece `at`: (member 1's ids, its logits, the next piece of member 0)."""
        g.tap_arm(1, 96); ids = []; step = sr // 5 + 1
        for lo in range(0, len(x), step):
            hi = min(len(x), lo + step)
            a = 0 if at == 0 else 40 + 2560 * (at - 1); b = 40 + 2560 * at; at += 1
            out = g.advance({0: x0[a:b], 1: x[lo:hi]}, finish=[1] if hi == len(x) else [])
            assert len(out[0]) == 1 and len(ids) + len(out[1]) == pkg.stream_schedule(hi, finished=hi == len(x), sample_rate=sr)[1]
            ids.extend(out[1])
        return np.array(ids, np.int32), g.tap_fetch(1), at

    g = m.create_stream_group(t, 2, gains=[g0, 1.0])
    try:
        plain = g.info(1)["bytes"]
        g.reset(1, ga, sample_rate=48000)
        assert g.sample_rate(1) == 48000 and g.info(1)["bytes"] >= plain + _in_ring(pkg, 48000) * 4 + fi48 * 2 * fo48 * 4      # the input ring and the block matrix
        assert g.info(0)["bytes"] == plain
        ids_a, lg_a, at = utterance(g, xa, 48000, 0)
        g.reset(1, gb, sample_rate=8000)
        assert g.sample_rate(1) == 8000 and g.info(1)["samples"] == 0 and g.info(0)["samples"] == 40 + 2560 * (at - 1)
        assert g.info(1)["bytes"] == plain + _in_ring(pkg, 8000) * 4 + fi8 * 2 * fo8 * 4      # the 48 kHz matrix went with its last member
        ids_b, lg_b, at = utterance(g, xb, 8000, at)
        g.reset(1, gb)      # no rate: the member keeps 8000
        assert g.sample_rate(1) == 8000 and g.info(1)["samples"] == 0
        ids_c, lg_c, at = utterance(g, xb, 8000, at)
        g.reset(1, 1.0, sample_rate=16000)
        assert g.sample_rate(1) == 16000 and g.info(1)["bytes"] <= plain
    finally:
        g.close()
    f = m.create_stream_group(t, 2, gains=[g0, gb], sample_rates=[16000, 8000])
    try:
        ids_f, lg_f, _ = utterance(f, xb, 8000, 0)
    finally:
        f.close()
    assert len(ids_a) >= 20 and len(ids_f) >= 20
    for ids, lg, label in ((ids_b, lg_b, "after the reset from 48 kHz to 8 kHz"), (ids_c, lg_c, "after a reset that keeps the rate")):
        assert np.array_equal(ids, ids_f) and np.array_equal(lg, lg_f), f"member 1 {label}: differs from a fresh group's member"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_group_untouched(pkg, ctx, model):
    m = model; t = _t(pkg, m); rates = [48000, 16000]
    xa = _loud(48000, int(2.5 * 48000) + 9, 6100); xb = _loud(16000, int(2.5 * 16000) + 4, 6200)
    gains = [_gain(_x16(pkg, ctx, xa, 48000)), _gain(xb)]
    half = len(xa) // 2; due = pkg.stream_schedule(half, sample_rate=48000)[1]
    assert due > 2 and due != pkg.stream_schedule(half)[1]
    far = np.zeros(8 * 48000, np.float32)      # 128 000 samples at 16 kHz: decoder position 65 of a group created for 64
    assert pkg.stream_schedule(len(far), sample_rate=48000)[0] > 64 >= pkg.stream_schedule(len(xa), finished=True, sample_rate=48000)[0]
    pcm = np.zeros(half, np.int16)

    def run(disturb):
        g = m.create_stream_group(t, 2, gains=gains, sample_rates=rates, max_positions=64)
        try:
            for k in range(2):
                g.tap_arm(k, 64)
            first = g.advance({1: xb[:len(xb) // 2]})[1]      # member 1 is mid-utterance throughout
            if disturb:
                infos = lambda: [g.info(k) for k in range(2)]
                before = infos()
                for rate, code in ((44101, 5), (0, 1)):      # VOX_ERR_UNSUPPORTED, VOX_ERR_INVALID
                    with pytest.raises(pkg.VoxError) as e:
                        g.reset(0, gains[0], sample_rate=rate)
                    assert e.value.code == code and infos() == before and g.sample_rate(0) == 48000
                for entries, s16, needle in [([(0, 0, xa, half, due - 1)], False, "capacity"), ([(1, 0, xb, 100, 64), (0, 0, xa, half, due - 1)], False, "capacity"),
                                             ([(0, 0, far, len(far), 512)], False, "position"), ([(0, 0, pcm, half, due - 1)], True, "capacity"),
                                             ([(0, 0, None, half, 64)], True, "null"), ([(1, 0, xb, 100, 64), (0, 0, None, half, 64)], True, "null")]:
                    code, msg, _ = _raw_advance(pkg, g, entries, s16)
                    assert code == 1 and needle in msg, msg
                    assert infos() == before
            code, msg, out = _raw_advance(pkg, g, [(0, 0, xa, half, due)])      # the correct call, with exactly the room the rate schedule asks for
            assert code == 0 and len(out[0]) == due, msg
            rest = g.advance({0: xa[half:], 1: xb[len(xb) // 2:]}, finish=[0, 1])
            ids = [np.concatenate([out[0], rest[0]]), np.concatenate([first, rest[1]])]
            return dict(ids=ids, lg=[g.tap_fetch(k) for k in range(2)])
        finally:
            g.close()

    calm = run(False); tried = run(True)
    assert len(calm["ids"][0]) == pkg.stream_schedule(len(xa), finished=True, sample_rate=48000)[1] >= 20
    _same(tried, calm, "after the refused calls vs an undisturbed run")
    with pytest.raises(pkg.VoxError, match="44101") as e:
        m.create_stream_group(t, 2, sample_rates=[16000, 44101])
    assert e.value.code == 5
    with pytest.raises(pkg.VoxError, match="rate") as e:
        m.create_stream_group(t, 2, sample_rates=[0, 16000])
    assert e.value.code == 1


# ---- 7. one ingest launch per pass ------------------------------------------------------------------------------------------------------------------------------------
def _ingest_launches(pkg):
    a = (C.c_uint64 * 11)()
    assert pkg.lib().vox_debug_attn_launches(a, 11) == 0
    return int(a[9]), int(a[10])      # the group's resampling kernel, the solo stream's


def test_one_ingest_launch_per_pass(pkg, ctx, model):
    m = model; t = _t(pkg, m); rates = [48000, 44100, 8000, 32000, 48000, 22050]
    g = m.create_stream_group(t, 6, sample_rates=rates)
    try:
        feeds = {k: _loud(sr, sr // 2 + k, 7100 + k) for k, sr in enumerate(rates)}      # half a second each: one pass, three ticks
        n0 = _ingest_launches(pkg)
        out = g.advance(feeds)
        n1 = _ingest_launches(pkg)
        assert all(len(out[k]) == pkg.stream_schedule(len(feeds[k]), sample_rate=rates[k])[1] for k in range(6)) and min(len(v) for v in out.values()) >= 1
        assert (n1[0] - n0[0], n1[1] - n0[1]) == (1, 0)
        out = g.advance({k: v.astype(np.int16) for k, v in feeds.items()})      # the 16-bit form: one pass again
        n2 = _ingest_launches(pkg)
        assert (n2[0] - n1[0], n2[1] - n1[1]) == (1, 0)
    finally:
        g.close()
    g = m.create_stream_group(t, 6)
    try:
        n0 = _ingest_launches(pkg)
        out = g.advance({k: _loud(16000, 8000 + k, 7200 + k) for k in range(6)})
        assert all(len(v) == pkg.stream_schedule(8000 + k)[1] >= 3 for k, v in out.items())
        assert _ingest_launches(pkg) == n0
    finally:
        g.close()
    st = m.create_stream(t, sample_rate=48000)      # the counters count: a solo rate stream moves the solo slot and only that one
    try:
        n0 = _ingest_launches(pkg); st.push(_loud(48000, 24000, 7300)); n1 = _ingest_launches(pkg)
        assert n1[0] == n0[0] and n1[1] > n0[1]
    finally:
        st.close()
