"""The device-free part of the ring attention's test entries (vox_debug_stream_attn, vox_debug_stream_ring_init; tests/test_gpu_stream_attn.py runs them): both
symbols are exported and bound, the descriptor has the header's layout, and null and out-of-range arguments are refused with VOX_ERR_INVALID before the context is
bound -- with a context pointer that must never be dereferenced, on a machine without a device."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

NEW_SYMBOLS = ("vox_debug_stream_attn", "vox_debug_stream_ring_init")


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def test_new_symbols_are_bound(pkg):
    lib_mod = import_module(pkg.__name__ + "._lib")
    L = pkg.lib()
    for name in NEW_SYMBOLS:
        assert name in lib_mod.SIGNATURES, name
        assert getattr(L, name).argtypes is not None, name
    assert L.vox_abi_version() == 1      # new symbols are not signature changes


def test_descriptor_layout(gg):
    D = gg.StreamAttnDesc
    assert C.sizeof(D) == 12 * 4 + 2 * 8 and D.theta.offset == 44 and D.order.offset == 48 and D.enc_pos.offset == 56 and D.rope_per_member.offset == 40


def test_null_arguments_are_refused_without_a_device(pkg):
    L = pkg.lib()
    assert L.vox_debug_stream_attn(None, None, None, None, None, None) != 0 and b"null argument" in L.vox_last_error()
    assert L.vox_debug_stream_ring_init(None, 1, 1, 1, 64, 4, None, None, None) != 0 and b"null argument" in L.vox_last_error()


def test_bad_arguments_are_refused_before_the_context_is_bound(pkg, gg):
    L = pkg.lib(); dummy = C.c_void_p(1)
    order = np.array([1, 0], np.int32); pos = np.array([100, 17], np.int32); buf = np.zeros(16, np.float32)

    def call(ctx=dummy, q=buf, k=buf, v=buf, o=buf, **kw):
        base = dict(n_slots=2, n_members=2, rows=4, n_heads=3, head_dim=64, window=40, cap=48, layers=1, layer=0, rope_rows=0, rope_per_member=0, theta=1e6,
                    order=order.ctypes.data, enc_pos=pos.ctypes.data)
        base.update(kw)
        d = gg.StreamAttnDesc(**base)
        return L.vox_debug_stream_attn(ctx, C.byref(d), *(None if a is None else a.ctypes.data for a in (q, k, v, o)))

    far = np.array([100, 65533], np.int32); clash = np.array([100, 68], np.int32); twice = np.array([1, 1], np.int32); outside = np.array([1, 2], np.int32)
    cases = [(dict(ctx=None), "null argument"), (dict(q=None), "null argument"), (dict(k=None), "null argument"), (dict(v=None), "null argument"), (dict(o=None), "null argument"),
             (dict(order=None), "null argument"), (dict(enc_pos=None), "null argument"),
             (dict(rows=0), "rows 0"), (dict(rows=9), "rows 9"), (dict(n_slots=17, n_members=17), "n_slots 17"), (dict(n_slots=0), "n_slots 0"), (dict(n_members=1), "n_members 1"),
             (dict(n_members=65), "n_members 65"), (dict(n_heads=0), "n_heads 0"), (dict(head_dim=32), "head_dim 32"), (dict(head_dim=96), "head_dim 96"),
             (dict(window=-1), "window -1"), (dict(window=1024, cap=2000), "window 1024"), (dict(cap=44), "cap 44"), (dict(cap=16385), "cap 16385"),
             (dict(layers=0), "layers"), (dict(layers=9), "layers"), (dict(layer=1), "layer 1 of 1"), (dict(layer=-1), "layer -1"), (dict(theta=1.0), "theta"),
             (dict(rope_rows=2), "rope_rows 2"), (dict(rope_rows=24), "rope_rows 24"), (dict(rope_rows=8192), "rope_rows 8192"), (dict(rows=1, rope_rows=1), "rope_rows 1"),
             (dict(rope_per_member=1), "rope_per_member"), (dict(enc_pos=far.ctypes.data), "enc_pos[1] = 65533"), (dict(enc_pos=clash.ctypes.data, rope_rows=32), "cannot hold positions"),
             (dict(order=twice.ctypes.data), "served by one slot"), (dict(order=outside.ctypes.data), "order[1] = 2")]
    for kw, msg in cases:
        assert call(**kw) == 1, kw
        assert msg in L.vox_last_error().decode(), (kw, L.vox_last_error())
    ring = [(dict(head_dim=32), "head_dim 32"), (dict(layers=0), "layers"), (dict(n_heads=65), "heads"), (dict(cap=0), "cap 0"), (dict(rows=0), "rows 0"), (dict(rows=-3), "rows -3"),
            (dict(rows=10), "rows 10")]
    for kw, msg in ring:
        a = dict(layers=2, rows=5, n_heads=3, head_dim=64, cap=9); a.update(kw)
        assert L.vox_debug_stream_ring_init(dummy, a["layers"], a["rows"], a["n_heads"], a["head_dim"], a["cap"], buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == 1, kw
        assert msg in L.vox_last_error().decode(), (kw, L.vox_last_error())
    with pytest.raises(pkg.VoxError):      # the Python wrappers' own shape checks
        gg.stream_attn(None, np.zeros((7, 576), np.float32), np.zeros((2, 1, 3, 48, 64), np.float32), np.zeros((2, 1, 3, 48, 64), np.float32), order, pos, 4, 40, 1e6)
    with pytest.raises(pkg.VoxError):
        gg.stream_ring_init(None, np.zeros((2, 5, 100), np.float32), np.zeros((2, 3, 9, 64), np.float32), np.zeros((2, 3, 9, 64), np.float32))
