"""The bounds of the model-owned prefix state, pinned on the CPU oracle: vox_transcribe_audio pads every utterance on the left with 76 tokens of
silence, so mel frames 0 .. 606, conv-stem rows 0 .. 150 and audio rows 0 .. 36 do not depend on the utterance -- and the next frame / row does.  The library derives
148 encoder rows / 37 decoder positions from these; a change to the pad, the mel framing or the conv stem that moves them fails here."""
import numpy as np

from model_fixtures import tiny_gguf

MEL_FLOOR = np.float32(-0.625)      # (max(log10(1e-10), 1.5 - 8) + 4) / 4
LAST_CONST_FRAME, LAST_CONST_ROW, LAST_CONST_AUDIO_ROW = 606, 150, 36


def _loud_clip(seconds, seed):
    """Loud from sample 0: no fade-in, so the first frame that can differ does."""
    rng = np.random.default_rng(seed)
    n = int(seconds * 16000)
    return (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * (0.05 + 0.01 * seed))).astype(np.float32)


def _mel(orc, x):
    xn = x.copy(); orc.lib().orc_peak_normalize(xn, xn.size, 0.95)
    return orc.mel_compute_log(orc.pad_audio(xn))      # [T][128]


def test_pad_configuration_gives_the_bounds(pkg):
    """The library's own derivation (prefix_bounds in vox_api.cpp), restated on the pad the library lays down."""
    (left,) = pkg.pad_audio(np.ones(1, np.float32)).nonzero()[0].tolist()      # first sample of the utterance inside the padded signal
    assert left == 76 * 1280
    frames = (left - 200) // 160      # last mel frame whose 400-sample window ends inside the silence
    rows = (frames - 3) // 4 + 1
    assert (frames, rows, rows // 4 * 4, rows // 4) == (LAST_CONST_FRAME, LAST_CONST_ROW + 1, 148, 37)


def test_silent_pad_rows_do_not_depend_on_the_clip(orc):
    path, _ = tiny_gguf()
    o = orc.Model(path)
    try:
        a = _mel(orc, _loud_clip(3.0, 1)); b = _mel(orc, _loud_clip(5.0, 2))
        for mel in (a, b):
            assert (mel[:LAST_CONST_FRAME + 1] == MEL_FLOOR).all()
            assert (mel[LAST_CONST_FRAME + 1] != MEL_FLOOR).any()
        ca = o.encoder_conv(np.ascontiguousarray(a.T)); cb = o.encoder_conv(np.ascontiguousarray(b.T))
        assert np.array_equal(ca[:LAST_CONST_ROW + 1], cb[:LAST_CONST_ROW + 1])
        assert not np.array_equal(ca[LAST_CONST_ROW + 1], cb[LAST_CONST_ROW + 1])
        ea = o.encode_audio(np.ascontiguousarray(a.T)); eb = o.encode_audio(np.ascontiguousarray(b.T))
        assert np.array_equal(ea[:LAST_CONST_AUDIO_ROW + 1], eb[:LAST_CONST_AUDIO_ROW + 1])
        assert not np.array_equal(ea[LAST_CONST_AUDIO_ROW + 1], eb[LAST_CONST_AUDIO_ROW + 1])
    finally:
        o.close()
