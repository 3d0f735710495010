"""The model-owned prefix state of transcribe_audio: encoder rows 0 .. 147 and decoder positions 0 .. 36 are computed once per model from a
silent mel, a call runs the encoder layers over the remaining rows and one ordinary decode step in place of the 38-token prefill.

Tolerance: the prefix path and the full computation differ by summation order only, so their ids must agree up to the first near-tie of the FULL path's own logits --
the rule of the neighbouring files (check_greedy_ids: top-2 margin below 10 x TOL x max|logit|), TOL = 2e-4.  The full path's logits come from the logits tap of
transcribe_streaming on the host-built mel of the same clip (the tap always runs the full computation)."""
import ctypes
import os

import numpy as np
import pytest

from model_fixtures import attn_launches, cache_dir, check_greedy_ids, fake_mel, gemm_launches, gemm_launches_since, launches_since, tiny_gguf

pytestmark = pytest.mark.gpu
TOL = 2e-4
# kernel forms that only the 38-row decoder prefill launches in a single-clip call of 10 s (every other GEMM of such a call has > 48 rows or exactly one)
PREFILL_GEMM_FORMS = ("skinny", "skinny_mt", "skinny_mt2", "xf_rows", "splitk_finish", "wide")


def _full_path():
    path = os.path.join(cache_dir(), "full_q4_seed42.gguf")
    if not os.path.exists(path):
        from __graft_entry__ import load_package
        S = load_package().synth
        S.write_synthetic_gguf(path + ".tmp", S.ModelDims(), seed=42); os.replace(path + ".tmp", path)
    return path


def _model_path(size):
    return tiny_gguf()[0] if size == "tiny" else _full_path()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["tiny", "full"])
def model(request, pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(_model_path(request.param)).load(ctx)
    yield m, request.param
    m.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    """Every test starts and ends with the model's defaults: prefix state on, decode engine on where the device allows it."""
    yield
    if "model" in request.fixturenames:
        m = request.getfixturevalue("model")[0]
        m.set_prefix_cache(True); m.set_decode_engine(True)


def _loud(seconds, seed):
    """Loud from sample 0 (no fade-in): the first mel frame, conv row and audio row that can differ between clips does."""
    rng = np.random.default_rng(seed); n = int(seconds * 16000)
    return (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * 0.07)).astype(np.float32)


def _clips(pkg):
    S = pkg.synth
    return {"3s": S.synth_audio(3.0, seed=31), "16s": S.synth_audio(16.0, seed=1234),
            "33s_past_window": S.synth_audio(33.0, seed=33),      # 990 encoder rows: the 750-row window starts inside the prefix for rows < 898, behind it from there on
            "loud_from_0": _loud(4.0, 5), "one_sample": np.array([0.3], np.float32)}


def _t(pkg, m, delay=6.0):
    return pkg.TimeEmbedding(m.config.dec_dim).embed(delay)


def _full_logits(pkg, ctx, m, x, t):
    """ids and per-step logits of the full computation: the logits tap on the host-built mel of the clip."""
    mel = pkg.MelSpectrogram.voxtral(ctx).compute_log(pkg.pad_audio(pkg.peak_normalize(x)))
    return m.transcribe_streaming(np.ascontiguousarray(mel.T)[None], t, return_logits=True)


def _stop(lg):
    """First step whose top-2 margin is a near-tie (len: none)."""
    srt = np.sort(lg, axis=1); safe = (srt[:, -1] - srt[:, -2]) > 10 * TOL * max(1.0, float(np.abs(lg).max()))
    return len(safe) if safe.all() else int(np.argmin(safe))


@pytest.mark.parametrize("clip", ["3s", "16s", "33s_past_window", "loud_from_0", "one_sample"])
def test_prefix_on_equals_off(pkg, ctx, model, clip):
    m, size = model
    x = _clips(pkg)[clip]; t = _t(pkg, m)
    assert m.set_prefix_cache(True)
    on = m.transcribe_audio(x, t)
    assert m.prefix_info()["built"]
    assert not m.set_prefix_cache(False)
    off = m.transcribe_audio(x, t)
    rids, rlg = _full_logits(pkg, ctx, m, x, t)
    stop = _stop(rlg)
    print(f"{size} {clip}: {len(on)} ids, on == off at {int((on == off).sum())}, first near-tie of the full path at {stop}")
    assert len(on) == len(off) == len(rids) and len(on) >= 9      # the shortest utterance: 76 + 1 + 17 pad tokens = 47 decoder positions
    assert (on[:stop] == off[:stop]).all()
    check_greedy_ids(on, rids, rlg, TOL); check_greedy_ids(off, rids, rlg, TOL)


def test_history_independence(pkg, ctx, model):
    """A fresh model's first call, its second, and a call after the state was dropped and rebuilt give the same ids, from host and from device samples: the state is
    built from the model alone, never from a clip."""
    _, size = model
    m = pkg.Q4ModelLoader.from_file(_model_path(size)).load(ctx)
    try:
        t = _t(pkg, m); x = _loud(5.0, 9); y = pkg.synth.synth_audio(3.0, seed=4)
        assert not m.prefix_info()["built"]
        first = m.transcribe_audio(x, t)
        assert m.prefix_info()["built"]
        other = m.transcribe_audio(y, t)
        second = m.transcribe_audio(x, t)
        m.set_prefix_cache(False); assert not m.prefix_info()["built"] and m.prefix_info()["bytes"] == 0
        m.set_prefix_cache(True)
        third = m.transcribe_audio(x, t)
        d = ctx.upload(x); dev = m.transcribe_audio(None, t, device_ptr=d, n_samples=x.size); ctx.free(d)
        assert (first == second).all() and (first == third).all() and (first == dev).all()
        assert (other == m.transcribe_audio(y, t)).all()
    finally:
        m.close()


def test_t_embed_change_rebuilds_the_decoder_part(pkg, ctx, model):
    """delay 6.0 -> 2.0 -> 6.0 on one model: at every delay the ids of a fresh model at that delay."""
    m, size = model
    x = pkg.synth.synth_audio(4.0, seed=12)
    fresh = {}
    for delay in (6.0, 2.0):
        f = pkg.Q4ModelLoader.from_file(_model_path(size)).load(ctx)
        try:
            fresh[delay] = f.transcribe_audio(x, _t(pkg, f, delay))
        finally:
            f.close()
    for delay in (6.0, 2.0, 6.0):
        ids = m.transcribe_audio(x, _t(pkg, m, delay))
        assert m.prefix_info()["built"] and (ids == fresh[delay]).all(), delay


def test_caller_supplied_mel_runs_the_full_computation(pkg, orc, ctx, model):
    """transcribe_streaming takes the caller's mel -- here one whose first 608 frames are NOT the silence floor -- and must not use the prefix state: equal to the oracle
    (tiny model) and the decoder-prefill kernel forms run; inside a prefix-on transcribe_audio none of them runs."""
    m, size = model
    t = _t(pkg, m); x = pkg.synth.synth_audio(10.0, seed=8)
    m.transcribe_audio(x, t)      # the state is built and in use
    assert m.prefix_info()["built"]
    mel = fake_mel(1144, seed=77)
    a0, g0 = attn_launches(pkg), gemm_launches(pkg)
    ids = m.transcribe_streaming(mel[None], t)
    a_str, g_str = launches_since(pkg, a0), gemm_launches_since(pkg, g0)
    print(f"{size} transcribe_streaming: attention {a_str}, linear {g_str}")
    assert a_str.get("prefill_small", 0) == m.config.dec_layers and a_str.get("prefill_mfma", 0) == m.config.enc_layers
    assert sum(g_str.get(k, 0) for k in PREFILL_GEMM_FORMS) > 0
    if size == "tiny":
        o = orc.Model(_model_path(size))
        try:
            rids, rlg = o.transcribe_streaming(mel, t, want_logits=True)
        finally:
            o.close()
        check_greedy_ids(ids, rids, rlg, TOL)
    a0, g0 = attn_launches(pkg), gemm_launches(pkg)
    m.transcribe_audio(x, t)
    a_on, g_on = launches_since(pkg, a0), gemm_launches_since(pkg, g0)
    print(f"{size} transcribe_audio, prefix on: attention {a_on}, linear {g_on}")
    assert "prefill_small" not in a_on and a_on.get("prefill_mfma", 0) == m.config.enc_layers
    assert not any(k in g_on for k in PREFILL_GEMM_FORMS)
    m.set_prefix_cache(False)
    a0 = attn_launches(pkg)
    m.transcribe_audio(x, t)
    assert launches_since(pkg, a0).get("prefill_small", 0) == m.config.dec_layers      # the switch brings the prefill back


def test_engine_off_serves_position_37_per_operator(pkg, ctx, model):
    """Prefix on, decode engine off: the per-operator step serves position 37 -- same ids as with the engine up to a near-tie of the full path's logits."""
    m, size = model
    t = _t(pkg, m); x = pkg.synth.synth_audio(5.0, seed=21)
    eng = m.set_decode_engine(True)
    a = m.transcribe_audio(x, t)
    assert not m.set_decode_engine(False)
    a0 = attn_launches(pkg)
    b = m.transcribe_audio(x, t)
    ran = launches_since(pkg, a0)
    assert "engine" not in ran and "prefill_small" not in ran
    rids, rlg = _full_logits(pkg, ctx, m, x, t)
    stop = _stop(rlg)
    print(f"{size}: engine {'on' if eng else 'not available'}; engine-off ids equal at {int((a == b).sum())} of {len(a)}, first near-tie at {stop}")
    assert (a[:stop] == b[:stop]).all()
    check_greedy_ids(b, rids, rlg, TOL)


def _device_free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_prefix_info_and_release(pkg):
    """Real geometry: 148 encoder rows, 37 decoder positions, the bytes of exactly those rows; switching off and close() give the memory back."""
    ctx = pkg.Context(0)
    try:
        x = pkg.synth.synth_audio(2.0, seed=3)
        held = []
        for cycle in range(2):      # the first cycle also loads kernels and fills the context's own scratch; the second is measured
            before = _device_free_bytes()
            m = pkg.Q4ModelLoader.from_file(_full_path()).load(ctx)
            c = m.config; t = pkg.TimeEmbedding(c.dec_dim).embed(6.0)
            assert m.prefix_info() == {"built": False, "encoder_rows": 148, "decoder_positions": 37, "bytes": 0}
            m.transcribe_audio(x, t)
            info = m.prefix_info()
            enc = c.enc_layers * 148 * 2 * c.enc_heads * c.enc_head_dim * 4      # k and v rows of every encoder layer
            dec = 2 * c.dec_layers * c.dec_kv_heads * 37 * c.dec_head_dim * 4 + 37 * c.dec_dim * 4      # decoder cache rows + the adapter rows they are rebuilt from
            assert info == {"built": True, "encoder_rows": 148, "decoder_positions": 37, "bytes": enc + dec}, info
            with_state = _device_free_bytes()
            m.set_prefix_cache(False)
            assert m.prefix_info()["bytes"] == 0 and _device_free_bytes() >= with_state + (enc + dec) * 3 // 4
            m.set_prefix_cache(True); m.transcribe_audio(x, t)
            assert m.prefix_info()["bytes"] == enc + dec
            m.close()
            held.append(before - _device_free_bytes())
        print(f"device bytes still held after close(): first cycle {held[0]}, second {held[1]}; the state is {enc + dec}")
        assert held[1] < (enc + dec) // 2
    finally:
        ctx.close()
