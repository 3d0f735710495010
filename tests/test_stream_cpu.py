"""Host side of the live streaming session (vox_stream): the schedule arithmetic against independent formulas, the exported symbols, argument checks.  No GPU.

The schedule (include/voxtral_hip.h): the left pad is 97 280 samples = 38 decoder positions of 2560 samples; mel frame f reads padded samples [160 f - 200, 160 f + 200);
decoder position p owns frames 16 p .. 16 p + 15, so it is determined once 160 (16 p + 15) + 200 <= 97 280 + n.  The step at position p yields tokens[p + 1] and the ids
are tokens[38 ...]: positions 0 .. 36 yield prefix tokens, position 37 the first id."""
import ctypes as C

import numpy as np

LEFT = 97280


def _conv(L):
    return (L + 2 - 3) // 2 + 1      # models/layers/conv.rs:47-48


def _schedule(pkg, n, finished):
    p = C.c_int32(-1); i = C.c_int32(-1)
    assert pkg.lib().vox_stream_schedule(n, 1 if finished else 0, C.byref(p), C.byref(i)) == 0
    return p.value, i.value


def _lengths():
    ns = {0, 1, 39, 40, 41, 2599, 2600, 2601, 256000}
    for k in range(0, 60):
        ns.update({1280 * k - 1, 1280 * k, 1280 * k + 1, 2560 * k + 39, 2560 * k + 40, 2560 * k + 41})
    rng = np.random.default_rng(2024)
    ns.update(int(v) for v in rng.integers(0, 30 * 16000 + 1, size=400))
    return sorted(n for n in ns if n >= 0)


def test_finished_schedule_is_the_offline_count(pkg):
    cfg = pkg.PadConfig.voxtral()
    for n in _lengths():
        total = cfg.padded_len(n)
        assert total % 1280 == 0
        T = C.c_size_t(); assert pkg.lib().vox_mel_num_frames(total, C.byref(T)) == 0
        assert T.value == total // 160 and T.value % 8 == 0      # neither conv reads its right zero pad
        S = total // 2560
        assert S == _conv(_conv(T.value)) // 4 and S >= 46
        assert _schedule(pkg, n, True) == (S, S - 38), n
    assert _schedule(pkg, 0, True)[0] == 46 and _schedule(pkg, 1, True)[0] == 47 and _schedule(pkg, 256000, True)[0] == 146


def test_unfinished_schedule_is_frame_arithmetic(pkg):
    cfg = pkg.PadConfig.voxtral()
    prev = (0, 0)
    for n in _lengths():
        # independent count: the positions whose last frame 16 p + 15 reads nothing beyond the samples pushed so far
        P = 0
        while 160 * (16 * P + 15) + 200 <= LEFT + n:
            P += 1
        got = _schedule(pkg, n, False)
        assert got == (P, max(P - 37, 0)), (n, got, P)
        assert got[0] >= prev[0] and got[1] >= prev[1]      # monotone in n (the lengths are sorted)
        fin = _schedule(pkg, n, True)
        assert got[0] <= fin[0] - 1 and got[1] <= fin[1]      # finish always has ticks left to run: the right pad is 17 tokens
        prev = got
    assert _schedule(pkg, 39, False)[1] == 0 and _schedule(pkg, 40, False)[1] == 1      # the first id is due after 40 samples,
    assert _schedule(pkg, 2599, False)[1] == 1 and _schedule(pkg, 2600, False)[1] == 2  # the second after 2 600
    assert cfg.left_pad_samples() == LEFT


def test_python_schedule_wrapper(pkg):
    assert pkg.stream_schedule(40) == (38, 1) and pkg.stream_schedule(0, finished=True) == (46, 8)


def test_symbols_and_argument_checks(pkg):
    L = pkg.lib()
    for name in ("vox_stream_create", "vox_stream_push", "vox_stream_finish", "vox_stream_reset", "vox_stream_free", "vox_stream_info", "vox_stream_schedule",
                 "vox_debug_stream_tap_arm", "vox_debug_stream_tap_fetch"):
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES
    INVALID = 1
    out = C.c_void_p(); t = np.zeros(8, np.float32); n = C.c_int32(); ids = np.zeros(4, np.int32); info = (C.c_int64 * 8)()

    def refused(code):
        assert code == INVALID
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    # without a model there is nothing to stream on: a machine without a GPU cannot load one (pkg.Context fails with "no HIP device"), so create can only be refused
    assert "null" in refused(L.vox_stream_create(None, t.ctypes.data, 1.0, 0, 0, C.byref(out)))
    refused(L.vox_stream_push(None, t.ctypes.data, 8, 0, ids.ctypes.data, 4, C.byref(n)))
    refused(L.vox_stream_finish(None, ids.ctypes.data, 4, C.byref(n)))
    refused(L.vox_stream_reset(None))
    refused(L.vox_stream_info(None, info))
    refused(L.vox_debug_stream_tap_arm(None, 4))
    refused(L.vox_debug_stream_tap_fetch(None, None, C.byref(n)))
    refused(L.vox_stream_schedule(10, 0, None, None))
    assert L.vox_stream_free(None) == 0      # like vox_cache_free: freeing nothing is fine
    assert L.vox_abi_version() == 1

