"""Pins the float64 reference of the front-end tests (tests/frontend_ref.py) to the CPU oracle and to the reference project's own vectors (tests/golden/), so
tests/test_gpu_front_end.py and the front-end cases of tests/test_gpu_stream.py measure the kernels against those numbers and not against a reference of their own
making.  CPU only.

Log-mel: the oracle (f32 samples, f64-accumulated DFT) must lie within 1e-5 of the float64 reference on the five input classes the GPU tests draw from -- a tenth of
the GPU bar of 1e-4.  Measured here: 3 s noise 3.1e-7, 440 Hz tone 1.8e-6, noise with a -80 dB first half 2.7e-7, sparse impulses 7.0e-8, one sample 4.5e-8."""
import os

import numpy as np
import pytest

import frontend_ref as F
from model_fixtures import component_weight, golden, gguf_conv_weights, rel_err, tiny_gguf

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_python_components.npz")
ENC = "mm_streams_embeddings.embedding_module.whisper_encoder."


@pytest.fixture(scope="module")
def fb(pkg):
    return pkg.MelSpectrogram.mel_filterbank()


@pytest.fixture(scope="module")
def win(pkg):
    return pkg.MelSpectrogram.hann_window(400)


def test_window_table(orc, win):
    """The window is an f32 table by definition (audio/mel.rs:345-349): the oracle's and the library's agree to an ulp of cosf, and both are the periodic Hann window
    up to the f32 rounding of the angle (2 pi i / 400 near 6.28 carries 2.4e-7) -- the difference matters: on a pure tone it moves leakage bins by 1.4e-5."""
    ow = np.zeros(400, np.float32); orc.lib().orc_hann_window(400, ow)
    ideal = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(400) / 400))
    assert win.dtype == np.float32 and np.abs(win.astype(np.float64) - ow).max() <= 2.0 ** -23
    assert np.abs(win - ideal).max() <= 4e-7 and win[0] == 0.0


def _normalised(orc, x):
    xn = np.array(x, dtype=np.float32, copy=True); orc.lib().orc_peak_normalize(xn, xn.size, 0.95)
    return xn


def test_peak_scale_vs_oracle(orc):
    """peak_scale is the factor orc_peak_normalize multiplies by: x * scale in f32 reproduces the oracle's samples bit for bit; silence (below 1e-10) is left alone."""
    rng = np.random.default_rng(1)
    for k in range(40):
        x = (rng.standard_normal(int(rng.integers(1, 3000))) * 10.0 ** rng.uniform(-9, 1)).astype(np.float32)
        s = F.peak_scale(x)
        assert s.dtype == np.float32 and np.array_equal(_normalised(orc, x), x * s)
    for mx, exp in ((0.0, 1.0), (9e-11, 1.0), (1e-10, np.float32(0.95) / np.float32(1e-10)), (2e-10, np.float32(0.95) / np.float32(2e-10))):
        x = np.zeros(9, np.float32); x[4] = -mx
        assert F.peak_scale(x) == np.float32(exp)
        assert np.array_equal(_normalised(orc, x), x * F.peak_scale(x))


def test_pad_vs_oracle(pkg, orc):
    assert (F.SPT, F.LEFT) == (1280, 97280)
    pc = pkg.PadConfig.voxtral()
    for n in (0, 1, 159, 160, 1279, 1280, 1281, 3839, 3840, 3841, 48000, 144000):
        x = np.arange(1, n + 1, dtype=np.float32)
        ref = orc.pad_audio(x)
        assert F.pad_len(n) == ref.size == pc.padded_len(n) and ref.size % 1280 == 0
        assert np.array_equal(F.pad(x), ref.astype(np.float64))


@pytest.mark.parametrize("kind", ["noise", "tone", "quiet_half", "impulses", "one_sample"])
def test_log_mel_vs_oracle(orc, fb, win, kind):
    x = F.make_clip(kind)
    xn = _normalised(orc, x)
    ref = F.log_mel(F.pad(xn), fb, win)
    out = orc.mel_compute_log(orc.pad_audio(xn)).T
    assert ref.shape == out.shape == (128, F.pad_len(x.size) // 160)
    err = float(np.abs(out - ref).max())
    print(f"oracle vs float64 log-mel, {kind}: {err:.2e}")
    assert err <= 1e-5
    pad_only = ~F.clip_frames(x.size, ref.shape[1])
    assert (ref[:, pad_only] == F.FLOOR).all() and np.float32(F.FLOOR) == np.float32(-0.625)
    if kind in ("noise", "quiet_half"):
        assert (ref[:, ~pad_only] > F.FLOOR + 0.05).mean() >= 0.5


def test_log_mel_reproduces_reference_python_vector(fb, win):
    """The reference's own PyTorch front end on an already padded clip (in_mel_audio / out_log_mel), at the tolerance test_log_mel_matches_reference_python holds the
    oracle to: torch's f32 FFT rounds low-power bins next to the tones."""
    g = golden()
    ref = g["out_log_mel"]
    out = F.log_mel(g["in_mel_audio"], fb, win)
    assert out.shape == ref.shape
    d = np.abs(out - ref)
    assert d.max() < 5e-4 and (d > 1e-4).mean() < 1e-3, d.max()


def test_conv_stem_reproduces_reference_python_vector():
    """conv_input / conv_output of the reference's per-component script (real shapes 128 -> 1280 -> 1280), tolerance 2e-4 of the largest value as every comparison
    with those f32 PyTorch vectors."""
    g = np.load(G)
    w1, b1 = component_weight(ENC + "conv_layers.0.conv.weight"), component_weight(ENC + "conv_layers.0.conv.bias")
    w2, b2 = component_weight(ENC + "conv_layers.1.conv.weight"), component_weight(ENC + "conv_layers.1.conv.bias")
    out, pre = F.conv_stem(g["conv_input"][0], w1, b1, w2, b2)
    assert out.shape == pre.shape == (25, 1280)
    assert rel_err(out.T, g["conv_output"][0]) < 2e-4


@pytest.mark.parametrize("T", [1, 2, 16, 17, 18, 19, 67, 400])
def test_conv_stem_vs_oracle(pkg, orc, T):
    """Against orc_conv1d_gelu twice and against the oracle model's encoder_conv with the tensors gguf_conv_weights reads (the helper the GPU tests use): the oracle
    sums K = 3 C terms sequentially in f32, so it lies within K 2^-24 sum |x||w| (+ an f32 rounding of the value and of erff) of a float64 sum; 2e-5 of the largest
    value covers that at C <= 1280 and is the f32-class bar of the linear tests."""
    path, d = tiny_gguf()
    w1, b1, w2, b2 = gguf_conv_weights(pkg, path, d.enc_dim, d.n_mels)
    rng = np.random.default_rng(T)
    mel = (0.6 * rng.standard_normal((d.n_mels, T)) + 0.3).astype(np.float32)
    out, _ = F.conv_stem(mel, w1, b1, w2, b2)
    L = orc.lib()
    l1 = L.orc_conv_out_len(T); y1 = np.zeros((d.enc_dim, l1), np.float32); L.orc_conv1d_gelu(mel, d.n_mels, T, np.ascontiguousarray(w1), b1, d.enc_dim, y1)
    l2 = L.orc_conv_out_len(l1); y2 = np.zeros((d.enc_dim, l2), np.float32); L.orc_conv1d_gelu(y1, d.enc_dim, l1, np.ascontiguousarray(w2), b2, d.enc_dim, y2)
    assert out.shape == (l2, d.enc_dim) and rel_err(y2.T, out) < 2e-5
    m = orc.Model(path)
    try:
        assert rel_err(m.encoder_conv(mel), out) < 2e-5
    finally:
        m.close()
