"""The device-free parts of the endless session: the new entry points exist and are bound, null arguments are refused without a device, and vox_debug_rope_rows -- the one function behind every RoPE table --
is held to float64 past the load-time table lengths, where the tables' f32 product pos * inv no longer carries the angle.

Bounds, from the number formats alone: a row past the table length is cos / sin of double(pos) * double(inv) rounded ONCE to f32, half an ulp of a value <= 1 (2^-25);
2^-23 leaves room for the double evaluation.  inv = 1 / powf(theta, 2 j / hd): the exponent is exact in f32 for hd a power of two, powf and the division round once
each, so 2 f32 ulp of the float64 power."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

NEW_SYMBOLS = ("vox_stream_create_endless", "vox_debug_attn_decode_ring", "vox_debug_rope_rows")
THETA = 1e6
TABLE_LEN = {128: 16384, 64: 65536}      # the decoder's load-time table, the streaming encoder's table (include/voxtral_hip.h)


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def test_new_symbols_are_bound(pkg):
    lib_mod = import_module(pkg.__name__ + "._lib")
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert name in lib_mod.SIGNATURES, name
        assert getattr(L, name).argtypes is not None, name


def test_attn_launches_has_a_ring_slot(pkg):
    """Slot [13] exists and is 0 in a process that ran no ring launch; entries past it are written as 0."""
    out = (C.c_uint64 * 16)(*([7] * 16))
    assert pkg.lib().vox_debug_attn_launches(out, 16) == 0
    assert out[13] == 0 and out[14] == 0 and out[15] == 0


def test_create_endless_refuses_null_arguments_without_a_device(pkg):
    L = pkg.lib(); out = C.c_void_p()
    t = (C.c_float * 8)()
    for args in ((None, t, 1.0, 0, 0, 16000, C.byref(out)), (None, None, 1.0, 0, 0, 16000, None)):
        assert L.vox_stream_create_endless(*args) != 0
        assert b"null argument" in L.vox_last_error()
    assert out.value is None


def test_ring_call_refuses_null_arguments_without_a_device(pkg):
    assert pkg.lib().vox_debug_attn_decode_ring(None, None, None, None, None, None) != 0
    assert b"null argument" in pkg.lib().vox_last_error()


def test_rope_rows_refusals(pkg, gg):
    for args in ((127, THETA, 0, 1), (128, THETA, -1, 1), (128, THETA, (1 << 24) - 1, 2), (128, 1.0, 0, 1), (128, THETA, 0, -1)):
        with pytest.raises(gg.VoxError):
            gg.rope_rows(*args)
    L = pkg.lib()
    assert L.vox_debug_rope_rows(128, THETA, 0, 1, None, None, None) != 0


@pytest.mark.parametrize("hd", (64, 128))
def test_rope_rows_past_the_tables(gg, hd):
    positions = (TABLE_LEN[hd], TABLE_LEN[hd] + 1, (1 << 20) + 3, (1 << 24) - 1)
    j = np.arange(hd // 2, dtype=np.float64)
    want_inv = np.float64(THETA) ** (-2.0 * j / hd)
    for p in positions:
        inv, cos, sin = gg.rope_rows(hd, THETA, p, 1)
        assert inv.dtype == cos.dtype == sin.dtype == np.float32 and cos.shape == sin.shape == (1, hd // 2)
        ulps = np.abs(inv.astype(np.float64) - want_inv) / np.spacing(want_inv.astype(np.float32)).astype(np.float64)
        print(f"hd {hd} pos {p}: inv worst {ulps.max():.2f} ulp")
        assert ulps.max() <= 2.0
        ang = float(p) * inv.astype(np.float64)
        ec, es = np.abs(cos[0] - np.cos(ang)).max(), np.abs(sin[0] - np.sin(ang)).max()
        print(f"hd {hd} pos {p}: cos off by {ec:.2e}, sin by {es:.2e}")
        assert ec <= 2.0 ** -23 and es <= 2.0 ** -23


@pytest.mark.parametrize("hd", (64, 128))
def test_rope_rows_one_call_or_one_by_one(gg, hd):
    """A span across the table length: the rows of one call are the rows asked for one at a time, bit for bit."""
    first, n = TABLE_LEN[hd] - 3, 7
    inv, cos, sin = gg.rope_rows(hd, THETA, first, n)
    for r in range(n):
        i1, c1, s1 = gg.rope_rows(hd, THETA, first + r, 1)
        assert np.array_equal(i1.view(np.uint32), inv.view(np.uint32))
        assert np.array_equal(c1[0].view(np.uint32), cos[r].view(np.uint32)) and np.array_equal(s1[0].view(np.uint32), sin[r].view(np.uint32))
    for p in ((1 << 20) + 3, (1 << 24) - 4):
        _, c4, s4 = gg.rope_rows(hd, THETA, p, 4)
        for r in range(4):
            _, c1, s1 = gg.rope_rows(hd, THETA, p + r, 1)
            assert np.array_equal(c1[0].view(np.uint32), c4[r].view(np.uint32)) and np.array_equal(s1[0].view(np.uint32), s4[r].view(np.uint32))


@pytest.mark.parametrize("hd", (64, 128))
def test_rope_rows_below_the_table_length_are_the_tables_formula(gg, hd):
    """Below the table length a row is the load-time formula: f32 product pos * inv, then f32 cos / sin (numpy's float32 product reproduces the angle; the cos / sin
    of the C library are held to 1 ulp of the f32 angle's float64 value, not to numpy's bits)."""
    for p in (0, 1, 4095, TABLE_LEN[hd] - 1):
        inv, cos, sin = gg.rope_rows(hd, THETA, p, 1)
        ang = (np.float32(p) * inv).astype(np.float64)      # the f32 product, as the tables form it
        assert np.abs(cos[0] - np.cos(ang)).max() <= 2.0 ** -23 and np.abs(sin[0] - np.sin(ang)).max() <= 2.0 ** -23
