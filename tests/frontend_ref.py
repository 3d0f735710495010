"""The float64 reference of the sample front end (tests/test_gpu_front_end.py, tests/test_gpu_stream.py): peak scale, pad, log-mel and the two-stage conv stem, written
from the definitions (audio/io.rs:59-68, audio/pad.rs, audio/mel.rs:128-244, models/layers/conv.rs:78-83) in numpy.  No project code: the two f32 tables the operation is defined
with, the Slaney filter bank and the periodic Hann window (an f32 table by definition, audio/mel.rs:345-349: 0.5 (1 - cos(2 pi i / 400)) evaluated in f32, up to 2.5e-7
off the ideal window), are passed in by the caller (vox_mel_filterbank, vox_hann_window; pinned in tests/test_frontend_ref.py); all arithmetic on them is float64.  tests/test_frontend_ref.py ties every function to the CPU oracle and to
the reference project's own vectors, so the GPU tests measure the kernels against those numbers and not against a reference of their own making."""
import math

import numpy as np

SAMPLE_RATE, FRAME_RATE, LEFT_TOKENS, RIGHT_TOKENS = 16000, 12.5, 76, 17      # PadConfig::voxtral (audio/pad.rs:32-46)
SPT = int(np.float32(SAMPLE_RATE) / np.float32(FRAME_RATE))                   # samples per token: 1280
LEFT = LEFT_TOKENS * SPT                                                      # 97 280 samples = 608 frames = 38 decoder positions of silence
HOP, NFFT, N_MELS = 160, 400, 128
FLOOR = (1.5 - 8.0 + 4.0) / 4.0                                               # -0.625: what every power below 10^-6.5 becomes (exact in f32 as well)

_erf = np.frompyfunc(math.erf, 1, 1)


def peak_scale(x):
    """peak_normalize(0.95)'s factor as the f32 arithmetic defines it: float32(0.95) / float32(max|x|), one correctly rounded f32 division; 1 when the maximum is
    below 1e-10 (compared in f32)."""
    x = np.asarray(x, dtype=np.float32)
    mx = np.float32(np.abs(x).max()) if x.size else np.float32(0)
    return np.float32(1.0) if mx < np.float32(1e-10) else np.float32(0.95) / mx


def pad_len(n):
    total = LEFT + n
    return total + (SPT - total % SPT) % SPT + RIGHT_TOKENS * SPT


def pad(x):
    """zeros(left) + x + zeros(right): 76 tokens in front, up to the next multiple of a token plus 17 tokens behind."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    out = np.zeros(pad_len(x.size), dtype=np.float64)
    out[LEFT:LEFT + x.size] = x
    return out


def log_mel(padded, fb, window):
    """[128][T], T = len / 160: frame f is the 400 samples around 160 f of the reflect-padded signal, times the periodic Hann `window` [400]; |rfft|^2 (201 bins); the
    128 x 201 bank `fb`; log10 (powers below 1e-10 clamped), floored at 1.5 - 8, (v + 4) / 4."""
    x = np.asarray(padded, dtype=np.float64).reshape(-1)
    T = x.size // HOP
    xp = np.pad(x, NFFT // 2, mode="reflect")
    frames = np.lib.stride_tricks.sliding_window_view(xp, NFFT)[::HOP][:T]
    win = np.asarray(window, dtype=np.float64).reshape(NFFT)
    power = np.abs(np.fft.rfft(frames * win[None, :], axis=1)) ** 2
    mel = power @ np.asarray(fb, dtype=np.float64).T
    v = np.maximum(np.log10(np.maximum(mel, 1e-10)), 1.5 - 8.0)
    return np.ascontiguousarray(((v + 4.0) / 4.0).T)


def clip_frames(n, T):
    """Mask [T] of the frames whose 400-sample window overlaps the clip's n samples inside the padded signal; every other frame sees only the pad's zeros."""
    f = np.arange(T)
    return (HOP * f + NFFT // 2 > LEFT) & (HOP * f - NFFT // 2 < LEFT + n)


def gelu64(v):
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + np.asarray(_erf(v / math.sqrt(2.0)), dtype=np.float64))


def conv1d_pre(x, w, b):
    """conv1d k3 s2 p1 before the activation: x [L][Cin] token-major, w [Cout][Cin][3], b [Cout] -> [(L - 1) // 2 + 1][Cout]; row t reads x rows 2 t - 1 .. 2 t + 1."""
    x = np.asarray(x, dtype=np.float64); w = np.asarray(w, dtype=np.float64)
    L, Cin = x.shape; Lo = (L + 2 - 3) // 2 + 1
    xp = np.zeros((L + 2, Cin)); xp[1:L + 1] = x
    cols = np.lib.stride_tricks.sliding_window_view(xp, 3, axis=0)[::2][:Lo]          # [Lo][Cin][3]
    return cols.reshape(Lo, Cin * 3) @ w.reshape(w.shape[0], Cin * 3).T + np.asarray(b, dtype=np.float64)[None, :]


def conv_stem(mel, w1, b1, w2, b2):
    """gelu(conv1d k3 s2 p1) twice (exact-erf GELU) on a log-mel [n_mels][T] -> (rows [S][enc_dim] token-major, the second stage's values before its GELU [S][enc_dim])."""
    c1 = gelu64(conv1d_pre(np.asarray(mel, dtype=np.float64).T, w1, b1))
    pre2 = conv1d_pre(c1, w2, b2)
    return gelu64(pre2), pre2


def make_clip(kind, seed=0, seconds=3.0):
    """The input classes of the front-end tests, float32 at 16 kHz.  (A pure tone plus 1e-4 noise is deliberately absent: its leakage bins sit just above the floor,
    where log10 is ill-conditioned -- the CPU oracle itself is 3.1e-5 off float64 there.)"""
    rng = np.random.default_rng([20261018, seed]); n = int(round(seconds * SAMPLE_RATE)); t = np.arange(n) / SAMPLE_RATE
    if kind == "noise":
        x = 0.3 * rng.standard_normal(n)
    elif kind == "tone":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t)
    elif kind == "tone_noise":
        x = 0.5 * np.sin(2 * np.pi * 440.0 * t) + 1e-2 * rng.standard_normal(n)
    elif kind == "quiet_half":
        x = 0.3 * rng.standard_normal(n); x[:n // 2] *= 1e-4
    elif kind == "impulses":
        x = np.zeros(n); k = rng.choice(n, size=max(n // 4000, 1), replace=False); x[k] = rng.uniform(-0.8, 0.8, k.size)
    elif kind == "one_sample":
        x = np.array([0.3])
    else:
        raise ValueError(kind)
    return x.astype(np.float32)
