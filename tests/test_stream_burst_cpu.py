"""The device-free parts of the burst streams (vox_stream_create_burst; DESIGN.md section 8, "Bursts"): the new entries exist and are bound; vox_stream_burst_len --
where a burst is cut -- against a Python restatement; the creation refusals that are decided before the model or a device is touched; create_stream(burst=...)'s
argument checks.  No GPU, no model; every assertion is ==."""
import ctypes as C
import os
from importlib import import_module

import pytest

NEW_SYMBOLS = ("vox_stream_create_burst", "vox_stream_burst_info", "vox_stream_burst_len", "vox_debug_stream_attn_burst", "vox_debug_stream_attn_burst_launches")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voxtral_hip.h")


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def test_new_symbols_are_bound_and_declared(pkg):
    lib_mod = import_module(pkg.__name__ + "._lib")
    L = pkg.lib(); hdr = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert name in lib_mod.SIGNATURES, name
        assert getattr(L, name).argtypes is not None, name
        assert f" {name}(" in hdr, name
    assert "#define VOX_STREAM_BURST_MAX 16" in hdr


def burst_len(due, burst, pos, next_stop):
    """The rule, restated: the smallest of the ticks still due, B and the distance to the next stop -- and at least 1."""
    return max(1, min(due, burst, next_stop - pos))


def test_burst_len_against_the_restatement(gg):
    n = 0
    for burst in (1, 2, 4, 15, 16):
        for due in (0, 1, 2, 3, 5, 15, 16, 17, 26, 40, 1000):
            for pos in (37, 1000, 1023, 8255, (1 << 24) - 20):
                for dist in (0, 1, 2, 3, 15, 16, 17, 1024, 1 << 20):
                    got = gg.stream_burst_len(due, burst, pos, pos + dist)
                    assert got == burst_len(due, burst, pos, pos + dist), (due, burst, pos, dist, got)
                    assert 1 <= got <= 16 and (got == 1 or (got <= due and got <= burst and pos + got <= pos + dist))      # a burst never spans the stop
                    n += 1
    assert n == 5 * 11 * 5 * 9
    assert gg.stream_burst_len(40, 16, 37, 1024) == 16 and gg.stream_burst_len(8, 16, 37, 1024) == 8 and gg.stream_burst_len(40, 16, 1020, 1024) == 4
    assert gg.stream_burst_len(0, 16, 37, 1024) == 1 and gg.stream_burst_len(1, 16, 37, 1024) == 1 and gg.stream_burst_len(40, 16, 1023, 1024) == 1
    assert gg.stream_burst_len(40, 1, 37, 1024) == 1


def test_the_launch_counter_starts_at_zero_and_refuses_null(pkg, gg):
    assert gg.stream_attn_burst_launches() == 0      # (a process without a GPU launched nothing)
    assert pkg.lib().vox_debug_stream_attn_burst_launches(None) != 0 and b"null argument" in pkg.lib().vox_last_error()
    assert pkg.lib().vox_debug_stream_attn_burst(None, None, None, None, None, None) != 0 and b"null argument" in pkg.lib().vox_last_error()
    assert pkg.lib().vox_stream_burst_info(None, None) != 0 and b"null argument" in pkg.lib().vox_last_error()


def test_create_burst_refusals_without_a_device(pkg):
    L = pkg.lib(); out = C.c_void_p(); t = (C.c_float * 8)()
    for args in ((None, t, 1.0, 0, 0, 16000, 0, 0, 16, C.byref(out)), (None, None, 1.0, 0, 0, 16000, 0, 0, 16, None)):
        assert L.vox_stream_create_burst(*args) != 0
        assert b"null argument" in L.vox_last_error()
    fake = (C.c_char * 64)()      # stands for a model: burst_ticks is refused before the model is looked at
    for bad in (0, 17, -1):
        assert L.vox_stream_create_burst(C.addressof(fake), t, 1.0, 0, 0, 16000, 0, 0, bad, C.byref(out)) != 0
        msg = L.vox_last_error()
        assert f"burst_ticks {bad}".encode() in msg and b"1..16" in msg, msg
    assert L.vox_stream_create_burst(C.addressof(fake), t, 1.0, 0, 0, 0, 0, 0, 16, C.byref(out)) != 0 and b"sample rate" in L.vox_last_error()
    assert L.vox_stream_create_burst(C.addressof(fake), t, 1.0, 0, 0, 16000, 0, 8256, 16, C.byref(out)) != 0 and b"dec_ring_rows" in L.vox_last_error()
    assert out.value is None


def test_create_stream_checks_burst_before_anything_else(pkg, gg):
    for bad in (0, 17, -3, True, 1.5, "4"):
        with pytest.raises(gg.VoxError) as e:
            gg.LiveStream(None, [0.0] * 8, burst=bad)      # (no model: the refusal comes first)
        assert e.value.code == 1 and "burst" in str(e.value) and "1..16" in str(e.value)
    assert gg.STREAM_BURST_MAX == 16
