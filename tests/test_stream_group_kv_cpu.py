"""Host side of the bf16 K/V pool of paged stream groups (vox_stream_group_create_kv, vox_kv_round_bf16, vox_debug_attn_decode_paged_bf16; DESIGN.md section 8 "A bf16
K/V pool"): the rounding against a numpy restatement of its contract, the refusals that come before a context is bound, the exported symbols and the ABI version.
No GPU is touched: the rounding is host arithmetic, and every refused call is refused by argument checks."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vox_stream_group_create_kv", "vox_kv_round_bf16", "vox_debug_attn_decode_paged_bf16")


def rne_restated(u):
    """The contract in numpy, on uint32 bit patterns: NaN -> the upper half with the quiet bit; everything else (u + 0x7fff + ((u >> 16) & 1)) >> 16 in 64-bit arithmetic."""
    u = u.astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x40, r).astype(np.uint16)


def rounded(pkg, bits):
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    return pkg.gguf.kv_round_bf16(bits.view(np.float32))


def test_symbols_are_declared_and_bound_and_the_abi_stays_one(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES and f" {name}(" in hdr
    assert "#define VOX_KV_F32 0" in hdr and "#define VOX_KV_BF16 1" in hdr
    assert L.vox_abi_version() == 1
    # the paged call + (endless, kv_dtype) in front of `out`
    res, args = pkg._lib.SIGNATURES["vox_stream_group_create_kv"]
    pres, pargs = pkg._lib.SIGNATURES["vox_stream_group_create_paged"]
    assert res is pres and len(args) == len(pargs) + 2 and list(args[:9]) == list(pargs[:9]) and args[-1] is pargs[-1]
    assert "kv_dtype" in inspect.signature(pkg.Q4VoxtralModel.create_stream_group).parameters
    assert "kv_dtype" in inspect.signature(pkg.LiveStreamGroup.__init__).parameters
    assert "[16]" in hdr and "[17]" in hdr and "[18]" in hdr and "[19]" in hdr      # the four launch-counter slots behind the sixteen


def test_rounding_equals_the_restated_contract_on_random_bit_patterns(pkg):
    bits = np.random.default_rng(20).integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)
    got = rounded(pkg, bits); want = rne_restated(bits)
    assert got.dtype == np.uint16 and got.shape == bits.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    fin = np.isfinite(bits.view(np.float32))
    # a finite value moves by at most half a bf16 step: the widened result is the nearest of the two neighbours
    x = bits.view(np.float32)[fin].astype(np.float64); w = (got[fin].astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    lo = (bits[fin] & np.uint32(0xFFFF0000)).view(np.float32).astype(np.float64)
    hi_bits = (bits[fin] & np.uint32(0xFFFF0000)) + np.uint32(0x10000)
    hi = hi_bits.view(np.float32).astype(np.float64)
    ok = np.isfinite(hi)
    assert (np.abs(w - x)[ok] <= np.minimum(np.abs(lo - x), np.abs(hi - x))[ok]).all()


def test_rounding_edge_values(pkg):
    cases = {
        0x3F808000: 0x3F80,      # a tie above an even upper half: down, to even
        0x3F818000: 0x3F82,      # a tie above an odd upper half: up, to even
        0x3F808001: 0x3F81,      # just past the tie
        0x3F807FFF: 0x3F80,      # just short of it
        0xBF808000: 0xBF80, 0xBF818000: 0xBF82,      # the same ties, negative
        0x00000000: 0x0000, 0x80000000: 0x8000,      # +0, -0: the sign is kept
        0x00000001: 0x0000, 0x80000001: 0x8000,      # the smallest denormal rounds to a zero of its sign
        0x007FFFFF: 0x0080, 0x807FFFFF: 0x8080,      # the largest denormal rounds up into the smallest normal
        0x00010000: 0x0001, 0x00018000: 0x0002,      # denormals that bf16 holds, and a denormal tie
        0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,      # the largest finite rounds past it: inf
        0x7F7F7FFF: 0x7F7F,                          # ... the last value that stays finite
        0x7F800000: 0x7F80, 0xFF800000: 0xFF80,      # inf stays inf
    }
    bits = np.array(list(cases), np.uint32)
    got = rounded(pkg, bits)
    assert [int(x) for x in got] == list(cases.values()), [(hex(b), hex(int(g))) for b, g in zip(bits, got)]
    assert np.array_equal(got, rne_restated(bits))
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345,      # quiet
                     0x7F800001, 0xFF800001, 0x7FA00000, 0x7F80FFFF, 0x7FBFFFFF, 0xFFFFFFFF, 0x7FFFFFFF], np.uint32)      # signalling, and payloads whose rounding would carry
    got = rounded(pkg, nans)
    assert np.array_equal(got, rne_restated(nans))
    wide = (got.astype(np.uint32) << 16).view(np.float32)
    assert np.isnan(wide).all() and (got & 0x0040).all()      # still NaN, quiet
    assert np.array_equal(got >> 15, (nans >> 31).astype(np.uint16))      # the sign is kept
    assert rounded(pkg, np.zeros(0, np.uint32)).shape == (0,)


def test_bad_arguments_are_refused_before_any_device_use(pkg):
    L = pkg.lib(); INVALID = 1
    out = C.c_void_p(); t = np.zeros(8, np.float32)

    def refused(code):
        assert code == INVALID
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    # (model, t_embed, n_members, gains, rates, enc_capacity_rows, max_positions, page_rows, pool_pages, endless, kv_dtype, out); without a model a create can only be refused
    create = lambda *a: L.vox_stream_group_create_kv(None, t.ctypes.data, *a, C.byref(out))
    for bad in (2, -1, 7):
        assert "kv_dtype" in refused(create(4, None, None, 0, 256, 16, 0, 0, bad))
    assert "max_positions" in refused(create(4, None, None, 0, 256, 16, 0, 1, 1))      # endless given with max_positions
    assert "max_positions" in refused(create(4, None, None, 0, 256, 16, 0, 1, 0))      # ... whatever the dtype
    assert "endless" in refused(create(4, None, None, 0, 0, 16, 0, 2, 1))
    assert "page_rows" in refused(create(4, None, None, 0, 256, -1, 0, 0, 1))
    assert "page_rows" in refused(create(4, None, None, 0, 0, -16, 0, 1, 1))
    # with VOX_KV_F32 the refusals are the paged / endless calls' own
    assert "n_members" in refused(create(17, None, None, 0, 256, 16, 0, 0, 0)) and "n_members" in refused(create(17, None, None, 0, 256, 16, 0, 0, 1))
    assert "null" in refused(create(4, None, None, 0, 256, 16, 0, 0, 0)) and "null" in refused(create(4, None, None, 0, 0, 16, 0, 1, 1))
    assert out.value is None
    # the debug entry: the descriptor and the table length are checked before the context is looked at
    entry = L.vox_debug_attn_decode_paged_bf16
    assert "null" in refused(entry(None, None, 0, None, None, None, None))
    pos = np.array([300], np.int32); tab = np.zeros((1, 32), np.int32)
    d = pkg.gguf.AttnDecodeDesc(n_seq=1, n_heads=4, n_kv_heads=2, head_dim=128, window=255, page_rows=0, n_slices=1, pos=pos.ctypes.data)
    assert "paged" in refused(entry(None, C.byref(d), 0, None, None, None, None))
    d.page_rows = 16; d.pool_pages = 40; d.page_tab_stride = 32; d.score_rows = 256; d.page_tab = tab.ctypes.data
    for bad in (-1, 1025):
        assert "page_tab_len" in refused(entry(None, C.byref(d), bad, None, None, None, None))
    q = np.zeros((1, 512), np.float32); k = np.zeros((40, 2, 16, 128), np.uint16); o = np.zeros((1, 512), np.float32)
    args = (q.ctypes.data, k.ctypes.data, k.ctypes.data, o.ctypes.data)
    assert "null" in refused(entry(None, C.byref(d), 19, *args))      # every argument but the context: refused for the null context, after ...
    for short in (18, 17, 1):      # ... a ring table below window / page_rows + 4 = 19 entries, which is refused whatever else is given
        assert "page_tab_len" in refused(entry(None, C.byref(d), short, *args))
    for bad in (48, 8, 2048):
        d.page_rows = bad
        assert "page_rows" in refused(entry(None, C.byref(d), 0, *args))      # a bad page_rows
    d.page_rows = 16; d.window = -1
    assert "window" in refused(entry(None, C.byref(d), 19, *args))       # a ring table needs a sliding window


def test_python_refuses_an_unknown_dtype_and_max_positions_on_an_endless_group(pkg):
    class NoModel:      # the refusals come before the model is touched
        h = None
    for bad in ("f16", "fp8", 1, "BF16"):
        with pytest.raises(ValueError, match="kv_dtype"):
            pkg.LiveStreamGroup(NoModel(), np.zeros(8, np.float32), 2, kv_dtype=bad)
    with pytest.raises(ValueError, match="max_positions"):
        pkg.LiveStreamGroup(NoModel(), np.zeros(8, np.float32), 2, max_positions=256, endless=True, kv_dtype="bf16")


def test_cli_refuses_live_kv_without_live_group(pkg):
    import subprocess
    import sys
    cmd = [sys.executable, os.path.join(ROOT, "voxtral-mini-realtime-rs_amd", "cli.py"), "--gguf", "none.gguf", "--tokenizer", "none.json", "--audio", "x.wav", "--live"]
    for kv in ("bf16", "f32"):      # refused by the argument parser: nothing is opened
        p = subprocess.run(cmd + ["--live-kv", kv], capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "--live-kv applies with --live-group" in p.stderr, p.stderr[-2000:]
    p = subprocess.run(cmd + ["--live-group", "2", "--live-kv", "f16"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--live-kv" in p.stderr and "invalid choice" in p.stderr, p.stderr[-2000:]
