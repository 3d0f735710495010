"""Live sessions fed at the capture rate, as f32 or 16-bit PCM (vox_stream_create_rate, vox_stream_push_s16).

The contract is bit-identity against paths the suite already tests: a stream created for rate sr and fed x gives what a 16 kHz stream fed pkg.resample(ctx, x, sr) gives
with the same gain -- the ids, the logits behind them (the logits tap) and every tick's 16 log-mel frames and 4 conv-stem rows (the front tap) -- because every 16 kHz
sample it produces has vox_resample's bits.  So every assertion here is ==: no tolerance, no near-tie rule.  Every push must return exactly the ids
stream_schedule(pushed, sample_rate=sr) says were due."""
import ctypes as C
import os

import numpy as np
import pytest

from model_fixtures import cache_dir, tiny_gguf
from stream_helpers import _gain, _pieces, _t

pytestmark = pytest.mark.gpu
RATES = (48000, 44100, 8000)      # 513 -> 171; 882 -> 320; 512 -> 1024 (up-sampling: fft_in + 1 bins)
PIECE = 4801


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


def _loud(sr, seconds, seed):
    rng = np.random.default_rng(seed); n = int(seconds * sr)
    return (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * (0.07 * 16000 / sr))).astype(np.float32)


def _plan(pkg, sr):
    return pkg.resample_plan(sr)[:3]


def _run(pkg, st, x, cuts, push=None):
    """Push x[a:b] for every (a, b) of cuts, then finish: (all ids, ids per call).  Every call returns exactly what the schedule says was due."""
    sr = st.sample_rate; per = []; pushed = 0; had = 0
    for k, (a, b) in enumerate(cuts):
        ids = push(st, k, a, b) if push else st.push(x[a:b]); pushed += b - a
        assert had + len(ids) == pkg.stream_schedule(pushed, sample_rate=sr)[1], (sr, a, b, had, len(ids))
        had += len(ids); per.append(ids)
    assert st.info()["samples"] == pushed == len(x)      # slot 0 counts the samples as pushed, at the input rate
    ids = st.finish(); had += len(ids); per.append(ids)
    assert had == pkg.stream_schedule(len(x), finished=True, sample_rate=sr)[1]
    return np.concatenate(per), [len(p) for p in per]


def _tapped(pkg, m, t, x, sr, gain, cuts, push=None, st=None):
    """One utterance with both taps armed: {ids, per (ids per call), lg (logits rows), mel, conv (front tap)}."""
    own = st is None
    if own:
        st = m.create_stream(t, gain=gain, sample_rate=sr)
    try:
        st.tap_arm(128); st.front_tap_arm(128)
        ids, per = _run(pkg, st, x, cuts, push)
        lg = st.tap_fetch(); mel, conv = st.front_tap_fetch()
    finally:
        if own:
            st.close()
    assert lg.shape[0] == len(ids) and mel.shape[0] == conv.shape[0] == len(ids) and np.array_equal(lg.argmax(axis=1), ids)
    return dict(ids=ids, per=per, lg=lg, mel=mel, conv=conv)


def _same(a, b, label):
    assert np.array_equal(a["ids"], b["ids"]), f"{label}: ids differ at {np.flatnonzero(a['ids'] != b['ids'])[:8] if len(a['ids']) == len(b['ids']) else (len(a['ids']), len(b['ids']))}"
    for k, what in (("mel", "log-mel frames"), ("conv", "conv-stem rows"), ("lg", "logits")):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), f"{label}: {what} differ in ticks {np.unique(np.nonzero(a[k] != b[k])[0])[:8]}"


_REF = {}


def _clip(pkg, ctx, sr, seconds=2.5):
    """(x at sr, pkg.resample(ctx, x, sr), gain of the resampled clip): computed once per rate, never modified."""
    key = (sr, seconds)
    if key not in _REF:
        x = _loud(sr, seconds, 900 + sr % 1000); x16 = pkg.resample(ctx, x, sr)
        x.setflags(write=False); x16.setflags(write=False)
        _REF[key] = (x, x16, _gain(x16))
    return _REF[key]


def _stream_b(pkg, m, t, x16, gain):
    """The 16 kHz stream of the resampled audio, in 4801-sample pieces."""
    return _tapped(pkg, m, t, x16, 16000, gain, _pieces(len(x16), PIECE))


# ---- 1. equals the 16 kHz stream of the resampled audio ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_equals_the_16k_stream_of_the_resampled_audio(pkg, ctx, model, sr):
    m = model; t = _t(pkg, m)
    x, x16, gain = _clip(pkg, ctx, sr)
    assert len(x16) == pkg.resample_len(len(x), sr)
    a = _tapped(pkg, m, t, x, sr, gain, _pieces(len(x), PIECE))
    b = _stream_b(pkg, m, t, x16, gain)
    print(f"{sr} Hz: {len(x)} samples -> {len(x16)} at 16 kHz, {len(a['ids'])} ids, ids per call {a['per']}")
    assert len(a["ids"]) >= 20
    _same(a, b, f"{sr} Hz stream vs the 16 kHz stream of resample(x)")


# ---- 2. cuts -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [8000, 48000, 44100])
def test_cuts(pkg, ctx, model, sr):
    """Pieces of 1, 7, fft_in - 1, fft_in, fft_in + 1, 2 fft_in + 3 and one whole push.  Pieces of 1 over the whole clip are run at 8 kHz (16 000 pushes); at the higher
    rates (100 000 pushes) pieces of 1 cover the first three blocks and 5 samples -- every alignment of a push against a block boundary -- and pieces of 4801 the rest."""
    m = model; t = _t(pkg, m)
    x, x16, gain = _clip(pkg, ctx, sr, 2.0)
    n = len(x); fi = _plan(pkg, sr)[0]
    cuts = {"one push": [(0, n)], "7": _pieces(n, 7), "fft_in - 1": _pieces(n, fi - 1), "fft_in": _pieces(n, fi), "fft_in + 1": _pieces(n, fi + 1), "2 fft_in + 3": _pieces(n, 2 * fi + 3)}
    head = 3 * fi + 5
    cuts["1"] = _pieces(n, 1) if sr == 8000 else _pieces(head, 1) + [(head + a, head + b) for a, b in _pieces(n - head, PIECE)]
    st = m.create_stream(t, gain=gain, sample_rate=sr)
    try:
        out = {}
        for k, c in cuts.items():
            out[k] = _run(pkg, st, x, c)[0]; st.reset()      # (_run holds every call to the schedule)
    finally:
        st.close()
    ref = out["one push"]
    assert len(ref) == pkg.stream_schedule(n, finished=True, sample_rate=sr)[1] >= 16
    for k, v in out.items():
        assert np.array_equal(v, ref), f"{sr} Hz: ids of pieces of '{k}' differ from the one-push run at {np.flatnonzero(v != ref)[:8]}"


# ---- 3. ends -----------------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [48000, 8000])
def test_ends(pkg, ctx, model, sr):
    m = model; t = _t(pkg, m)
    x, _, _ = _clip(pkg, ctx, sr)
    fi = _plan(pkg, sr)[0]
    late = -(-40 * sr // 16000) + 1      # nothing is final yet, but the finished utterance has the 40 samples of the first id
    assert pkg.stream_schedule_rate(late, sr)[2] < 40 <= pkg.stream_schedule_rate(late, sr, finished=True)[2]
    for n in (0, 1, fi - 1, fi, fi + 1, 3 * fi, late):
        xs = x[:n]; x16 = pkg.resample(ctx, xs, sr) if n else np.zeros(0, np.float32)
        gain = _gain(x16) if n > 1 else 1.0
        a = _tapped(pkg, m, t, xs, sr, gain, [(0, n)] if n else [])
        b = _tapped(pkg, m, t, x16, 16000, gain, [(0, len(x16))] if len(x16) else [])
        due = pkg.stream_schedule(n, sample_rate=sr)[1]
        assert a["per"][:-1] == ([due] if n else []) and sum(a["per"]) == pkg.stream_schedule(n, finished=True, sample_rate=sr)[1] == len(b["ids"]) >= 8
        if n in (0, 1, fi - 1, late):
            assert due == 0      # nothing before finish: no block is complete
        _same(a, b, f"{sr} Hz, {n} samples")


# ---- 4. rings ----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_push_larger_than_both_rings(pkg, ctx, model):
    m = model; t = _t(pkg, m); sr = 48000
    x, x16, gain = _clip(pkg, ctx, sr, 6.0)
    assert len(x) == 288000 and len(x16) > 65536      # more than the 16 kHz ring (65 536) and the input ring hold
    whole = _tapped(pkg, m, t, x, sr, gain, [(0, len(x))])
    cut = _tapped(pkg, m, t, x, sr, gain, _pieces(len(x), PIECE))
    _same(whole, cut, "one push of 288 000 samples vs 4801-sample pieces")
    assert len(whole["ids"]) == pkg.stream_schedule(len(x), finished=True, sample_rate=sr)[1] >= 45


# ---- 5. 16-bit PCM -----------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", [16000, 48000])
def test_s16_equals_f32(pkg, ctx, model, sr):
    m = model; t = _t(pkg, m)
    rng = np.random.default_rng(sr + 5); n = int(2.5 * sr)
    v = np.clip(np.round(9000.0 * rng.standard_normal(n) + 7000.0 * np.sin(np.arange(n) * (0.07 * 16000 / sr))), -32768, 32767).astype(np.int16)
    v[:4] = (-32768, 32767, -1, 1)      # the ends of the range
    f = (v.astype(np.float32) / np.float32(32768))
    x16 = pkg.resample(ctx, f, sr); gain = _gain(x16)
    cuts = _pieces(n, PIECE)
    ref = _tapped(pkg, m, t, f, sr, gain, cuts)
    assert len(ref["ids"]) >= 20
    s16 = _tapped(pkg, m, t, v, sr, gain, cuts)
    _same(s16, ref, f"{sr} Hz: int16 pushes vs the same samples as float32")
    mixed = _tapped(pkg, m, t, v, sr, gain, cuts, push=lambda st, k, a, b: st.push(v[a:b]) if k % 2 else st.push(f[a:b]))
    _same(mixed, ref, f"{sr} Hz: alternating int16 and float32 pushes")
    whole = _tapped(pkg, m, t, v, sr, gain, [(0, n)])      # one host push: several rounds of the staging buffer
    _same(whole, ref, f"{sr} Hz: one int16 push")
    dev = C.c_void_p(); pkg._lib.check(pkg.lib().vox_dev_alloc(ctx.h, n * 2, C.byref(dev)))
    try:
        pkg._lib.check(pkg.lib().vox_dev_upload(ctx.h, dev, v.ctypes.data, n * 2))
        d = _tapped(pkg, m, t, v, sr, gain, cuts, push=lambda st, k, a, b: st.push(device_ptr=dev.value + 2 * a, n_samples=b - a, dtype="s16"))
    finally:
        pkg._lib.check(pkg.lib().vox_dev_free(ctx.h, dev))
    _same(d, ref, f"{sr} Hz: int16 pushes from device memory")


# ---- 6. isolation ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_rate_streams_offline_resampling_and_offline_calls_do_not_disturb_each_other(pkg, ctx, model):
    m = model; t = _t(pkg, m)
    xa, xa16, ga = _clip(pkg, ctx, 48000); xb, xb16, gb = _clip(pkg, ctx, 44100)
    z = _loud(22050, 1.0, 77); w = _loud(32000, 0.2, 78); xo = pkg.synth.synth_audio(3.0, seed=31)
    ca, cb = _pieces(len(xa), PIECE), _pieces(len(xb), 4410)
    solo_a = _tapped(pkg, m, t, xa, 48000, ga, ca); solo_b = _tapped(pkg, m, t, xb, 44100, gb, cb)
    z_before = pkg.resample(ctx, z, 22050); w_before = pkg.resample(ctx, w, 32000); off_before = m.transcribe_audio(xo, t)
    a = m.create_stream(t, gain=ga, sample_rate=48000); b = m.create_stream(t, gain=gb, sample_rate=44100)
    try:
        def push(which):
            def f(st, k, lo, hi):      # between the pushes: the context's resampler at two other rates (its matrix replaced each time), the other stream, an offline call
                assert np.array_equal(pkg.resample(ctx, z, 22050), z_before) and np.array_equal(pkg.resample(ctx, w, 32000), w_before)
                if k % 5 == 2:
                    assert np.array_equal(m.transcribe_audio(xo, t), off_before)
                if which == "a" and k < len(cb):
                    got_b.append(b.push(xb[cb[k][0]:cb[k][1]]))
                return st.push((xa if which == "a" else xb)[lo:hi])
            return f

        got_b = []
        b.tap_arm(128); b.front_tap_arm(128)
        ra = _tapped(pkg, m, t, xa, 48000, ga, ca, push=push("a"), st=a)
        for k in range(len(got_b), len(cb)):
            got_b.append(b.push(xb[cb[k][0]:cb[k][1]]))
        assert np.array_equal(pkg.resample(ctx, xa, 48000), xa16)      # the context's matrix is now the 48 kHz one; the 44.1 kHz stream finishes on its own
        got_b.append(b.finish())
        rb = dict(ids=np.concatenate(got_b), lg=b.tap_fetch()); rb["mel"], rb["conv"] = b.front_tap_fetch()
        assert [len(p) for p in got_b] == solo_b["per"]
        _same(ra, solo_a, "48 kHz stream, interleaved"); _same(rb, solo_b, "44.1 kHz stream, interleaved")
        a.reset(); b.reset()
        _same(_tapped(pkg, m, t, xa, 48000, ga, ca, st=a), solo_a, "48 kHz stream after reset")
        _same(_tapped(pkg, m, t, xb, 44100, gb, cb, st=b), solo_b, "44.1 kHz stream after reset")
    finally:
        a.close(); b.close()
    assert np.array_equal(pkg.resample(ctx, z, 22050), z_before) and np.array_equal(m.transcribe_audio(xo, t), off_before)


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, ctx, model):
    m = model; t = _t(pkg, m); L = pkg.lib(); sr = 48000
    with pytest.raises(pkg.VoxError, match="44101") as e:
        m.create_stream(t, sample_rate=44101)
    assert e.value.code == 5      # VOX_ERR_UNSUPPORTED
    with pytest.raises(pkg.VoxError, match="rate") as e:
        m.create_stream(t, sample_rate=0)
    assert e.value.code == 1      # VOX_ERR_INVALID
    x, x16, gain = _clip(pkg, ctx, sr)
    ref = _tapped(pkg, m, t, x, sr, gain, [(0, len(x))])["ids"]
    plain = m.create_stream(t, gain=gain)
    st = m.create_stream(t, gain=gain, sample_rate=sr)
    try:
        _, fo, _ = _plan(pkg, sr)
        assert st.info()["bytes"] >= plain.info()["bytes"] + 2 * 513 * 4 + 513 * 2 * fo * 4      # the input ring and the block matrix are counted
        n = C.c_int32(-1); ids = np.zeros(64, np.int32)
        due = pkg.stream_schedule(len(x), sample_rate=sr)[1]
        assert due > 2
        before = st.info()
        for fn, buf in ((L.vox_stream_push, x), (L.vox_stream_push_s16, np.zeros(len(x), np.int16))):
            assert fn(st.h, buf.ctypes.data, len(x), 0, ids.ctypes.data, due - 1, C.byref(n)) == 1 and b"capacity" in L.vox_last_error()
            assert st.info() == before
        pkg._lib.check(L.vox_stream_push(st.h, x.ctypes.data, len(x), 0, ids.ctypes.data, due, C.byref(n)))      # the repeated call with room
        assert n.value == due and np.array_equal(ids[:due], ref[:due])
        before = st.info()
        assert L.vox_stream_finish(st.h, ids.ctypes.data, 1, C.byref(n)) == 1 and st.info() == before
        assert np.array_equal(np.concatenate([ids[:due], st.finish()]), ref)
        with pytest.raises(pkg.VoxError, match="finished"):
            st.push(np.zeros(10, np.int16))
    finally:
        st.close(); plain.close()


# ---- 8. full size ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_full_size_48k(pkg, ctx):
    """The cached full-size peaked model of tests/test_gpu_stream.py: a 3 s clip at 48 kHz against the 16 kHz stream of the resampled clip."""
    path = os.path.join(cache_dir(), "full_q4_peaked_seed44.gguf")
    if not os.path.exists(path):
        S = pkg.synth
        S.write_synthetic_gguf(path + ".tmp", S.ModelDims(), seed=44, peaked=True); os.replace(path + ".tmp", path)
    m = pkg.Q4ModelLoader.from_file(path).load(ctx)
    try:
        t = _t(pkg, m); sr = 48000
        x, x16, gain = _clip(pkg, ctx, sr, 3.0)
        a = _tapped(pkg, m, t, x, sr, gain, _pieces(len(x), PIECE))
        b = _stream_b(pkg, m, t, x16, gain)
        assert len(a["ids"]) == 27
        assert np.array_equal(a["ids"], b["ids"]) and np.array_equal(a["lg"], b["lg"])
    finally:
        m.close()
