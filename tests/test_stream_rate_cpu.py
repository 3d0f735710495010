"""Host side of live sessions fed at the capture rate (vox_stream_create_rate, vox_stream_push_s16, vox_stream_schedule_rate): the schedule against an independent
restatement, the finality bound it rests on against the CPU oracle's resampler, the exported symbols, argument checks.  No GPU.

The restatement: the resampler works on blocks of fft_in input samples that become fft_out output samples, delayed by fft_out / 2; output sample i reads block
(i + delay) / fft_out in full and the tail of the block before.  After n input samples floor(n / fft_in) blocks are complete, so the first
max(0, floor(n / fft_in) fft_out - delay) output samples are final; those are the 16 kHz samples the session holds, and the frame arithmetic of test_stream_cpu.py
applies to them.  Every assertion is ==."""
import ctypes as C
import math

import numpy as np
import pytest

LEFT = 97280
RATES = (48000, 44100, 32000, 24000, 22050, 11025, 8000, 96000)


def _plan(sr):
    """fft_in, fft_out, delay of the synchronous FFT resampler sr -> 16 kHz (chunk 1024, 2 sub-chunks): whole multiples of the reduced rates, at least 512 input samples"""
    g = math.gcd(sr, 16000); a, b = sr // g, 16000 // g
    k = -(-512 // a)
    return k * a, k * b, (k * b) // 2


def _avail16(sr, n):
    fi, fo, d = _plan(sr)
    return max(0, (n // fi) * fo - d)


def _schedule_rate(pkg, n, sr, finished):
    p = C.c_int32(-1); i = C.c_int32(-1); k = C.c_size_t(1 << 60)
    assert pkg.lib().vox_stream_schedule_rate(n, sr, 1 if finished else 0, C.byref(p), C.byref(i), C.byref(k)) == 0
    return p.value, i.value, k.value


def _schedule16(pkg, n, finished):
    p = C.c_int32(-1); i = C.c_int32(-1)
    assert pkg.lib().vox_stream_schedule(n, 1 if finished else 0, C.byref(p), C.byref(i)) == 0
    return p.value, i.value


def _lengths(sr):
    fi = _plan(sr)[0]
    ns = {0, 1, fi - 1, fi, fi + 1}
    for k in range(40):
        ns.update({k * fi - 1, k * fi + 1})
    rng = np.random.default_rng(sr)
    ns.update(int(v) for v in rng.integers(0, 30 * sr + 1, size=400))
    return sorted(n for n in ns if n >= 0)


def test_the_restated_plan_is_the_library_plan(pkg):
    expect = {48000: (513, 171), 44100: (882, 320), 8000: (512, 1024)}
    for sr in RATES:
        fi, fo, d, _, _ = pkg.resample_plan(sr)
        assert (fi, fo, d) == _plan(sr)
        if sr in expect:
            assert (fi, fo) == expect[sr]


@pytest.mark.parametrize("sr", RATES)
def test_unfinished_schedule_is_blocks_complete_minus_delay_then_frames(pkg, sr):
    prev = (0, 0, 0)
    for n in _lengths(sr):
        a = _avail16(sr, n)
        P = 0      # the positions whose last frame 16 P + 15 reads nothing beyond the 16 kHz samples that are final
        while 160 * (16 * P + 15) + 200 <= LEFT + a:
            P += 1
        got = _schedule_rate(pkg, n, sr, False)
        assert got == (P, max(P - 37, 0), a), (sr, n, got, P, a)
        assert got[:2] == _schedule16(pkg, a, False)
        assert got[0] >= prev[0] and got[1] >= prev[1] and got[2] >= prev[2]      # monotone in n (the lengths are sorted)
        fin = _schedule_rate(pkg, n, sr, True)
        assert got[0] <= fin[0] - 1 and got[1] <= fin[1] and got[2] <= fin[2]      # finish always has ticks left to run, and never fewer samples
        prev = got


@pytest.mark.parametrize("sr", RATES)
def test_finished_schedule_is_the_resampled_length_through_the_pad(pkg, sr):
    cfg = pkg.PadConfig.voxtral()
    for n in _lengths(sr):
        n16 = pkg.resample_len(n, sr)
        assert n16 == math.ceil(n * (16000 / sr))
        S = cfg.padded_len(n16) // 2560
        assert _schedule_rate(pkg, n, sr, True) == (S, S - 38, n16), (sr, n)
        assert _schedule_rate(pkg, n, sr, True)[:2] == _schedule16(pkg, n16, True)


def test_rate_16000_is_the_plain_schedule(pkg):
    for n in _lengths(16000) + [39, 40, 41, 2599, 2600, 2601]:
        for fin in (False, True):
            assert _schedule_rate(pkg, n, 16000, fin) == _schedule16(pkg, n, fin) + (n,)
            assert pkg.stream_schedule(n, finished=fin, sample_rate=16000) == pkg.stream_schedule(n, finished=fin) == _schedule16(pkg, n, fin)


def test_python_wrappers(pkg):
    assert pkg.stream_schedule(40) == (38, 1) and pkg.stream_schedule(0, finished=True) == (46, 8)      # what it returns today
    n = 5 * 513
    assert pkg.stream_schedule_rate(n, 48000) == _schedule_rate(pkg, n, 48000, False) and pkg.stream_schedule(n, sample_rate=48000) == _schedule_rate(pkg, n, 48000, False)[:2]
    assert pkg.stream_schedule_rate(n, 48000, finished=True) == _schedule_rate(pkg, n, 48000, True)
    assert pkg.stream_schedule_rate(513, 48000)[2] == 171 - 85 and pkg.stream_schedule_rate(512, 48000)[2] == 0


@pytest.mark.parametrize("sr", RATES)
def test_the_samples_the_schedule_counts_are_final_in_the_oracle(pkg, orc, sr):
    """orc.resample(x[:n])[:a] == orc.resample(x)[:a] bit for bit with a = samples_16k from the library: what the session produces after n samples never changes."""
    fi = _plan(sr)[0]
    N = int(1.3 * sr)
    rng = np.random.default_rng(1000 + sr)
    x = (0.4 * rng.standard_normal(N) + 0.3 * np.sin(np.arange(N) * 0.05)).astype(np.float32)
    full = orc.resample(x, sr)
    assert len(full) == _schedule_rate(pkg, N, sr, True)[2]
    for n in (1, fi - 1, fi, fi + 1, 2 * fi, 3 * fi + 5, N // 2, N - 1, N):
        a = _schedule_rate(pkg, n, sr, False)[2]
        part = orc.resample(x[:n], sr)
        assert a <= len(part), (sr, n, a, len(part))
        assert np.array_equal(part[:a], full[:a]), (sr, n, a)
    assert _schedule_rate(pkg, N, sr, False)[2] > 0      # (the comparison was not empty)


def test_symbols_and_argument_checks(pkg):
    L = pkg.lib()
    for name in ("vox_stream_create_rate", "vox_stream_push_s16", "vox_stream_schedule_rate"):
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES
    INVALID, UNSUPPORTED = 1, 5
    out = C.c_void_p(); t = np.zeros(8, np.float32); n = C.c_int32(); ids = np.zeros(4, np.int32); v = np.zeros(8, np.int16)
    p = C.c_int32(); i = C.c_int32(); k = C.c_size_t()

    def refused(code, want=INVALID):
        assert code == want
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    assert "null" in refused(L.vox_stream_create_rate(None, t.ctypes.data, 1.0, 0, 0, 48000, C.byref(out)))
    assert "null" in refused(L.vox_stream_push_s16(None, v.ctypes.data, 8, 0, ids.ctypes.data, 4, C.byref(n)))
    assert "rate" in refused(L.vox_stream_create_rate(None, t.ctypes.data, 1.0, 0, 0, 0, C.byref(out)))
    assert "mem_kind" in refused(L.vox_stream_push_s16(None, v.ctypes.data, 8, 7, ids.ctypes.data, 4, C.byref(n)))
    assert "null" in refused(L.vox_stream_schedule_rate(10, 48000, 0, None, C.byref(i), C.byref(k)))
    assert "null" in refused(L.vox_stream_schedule_rate(10, 48000, 0, C.byref(p), C.byref(i), None))
    assert "rate" in refused(L.vox_stream_schedule_rate(10, 0, 0, C.byref(p), C.byref(i), C.byref(k)))
    assert "44101" in refused(L.vox_stream_schedule_rate(10, 44101, 0, C.byref(p), C.byref(i), C.byref(k)), UNSUPPORTED)      # what the offline resampler refuses
    with pytest.raises(pkg.VoxError, match="rate"):
        pkg.stream_schedule(10, sample_rate=0)
