"""Host side of the endless paged stream group (vox_stream_group_create_endless, vox_debug_attn_decode_paged_ring; DESIGN.md section 8 "Endless paged groups"): the
exported symbols and their signatures, the refusals that need no device, the page arithmetic at positions near 2^24, the Python refusal of max_positions, the CLI's
acceptance of --live-group with --live-endless.  No GPU.  (The ring form of the page allocator itself is tools/page_pool_check.cpp's: a randomised run under the host
sanitizers.)"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vox_stream_group_create_endless", "vox_debug_attn_decode_paged_ring")


def test_symbols_are_declared_and_bound_and_the_abi_stays_one(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES and f" {name}(" in hdr
    assert L.vox_abi_version() == 1
    # (model, t_embed, n_members, gains, rates, enc_capacity_rows, page_rows, pool_pages, out): the paged call less max_positions
    res, args = pkg._lib.SIGNATURES["vox_stream_group_create_endless"]
    pres, pargs = pkg._lib.SIGNATURES["vox_stream_group_create_paged"]
    assert res is pres and len(args) == 9 and list(args) == list(pargs[:6]) + list(pargs[7:])
    decl = hdr[hdr.index("int32_t vox_stream_group_create_endless("):]
    decl = decl[:decl.index(";")]
    assert "max_positions" not in decl and decl.count(",") == 8 and "page_rows" in decl and "pool_pages" in decl and "rates" in decl
    import inspect
    assert "endless" in inspect.signature(pkg.Q4VoxtralModel.create_stream_group).parameters
    assert "endless" in inspect.signature(pkg.LiveStreamGroup.__init__).parameters


def test_the_launch_counters_have_two_slots_behind_13(pkg):
    out = (C.c_uint64 * 18)(*([7] * 18))
    assert pkg.lib().vox_debug_attn_launches(out, 18) == 0
    assert out[14] == 0 and out[15] == 0 and out[16] == 0 and out[17] == 0      # no ring-table launch in a process without a GPU; entries past [15] are 0
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    assert "[14]" in hdr and "[15]" in hdr


def test_bad_arguments_are_refused_before_any_device_use(pkg):
    L = pkg.lib(); INVALID = 1
    out = C.c_void_p(); t = np.zeros(8, np.float32)

    def refused(code):
        assert code == INVALID
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    # without a model there is no group: create can only be refused, and says why
    assert "page_rows" in refused(L.vox_stream_group_create_endless(None, t.ctypes.data, 4, None, None, 0, -1, 0, C.byref(out)))
    assert "null" in refused(L.vox_stream_group_create_endless(None, t.ctypes.data, 4, None, None, 0, 16, 0, C.byref(out)))
    assert "n_members" in refused(L.vox_stream_group_create_endless(None, t.ctypes.data, 17, None, None, 0, 0, 0, C.byref(out)))
    assert out.value is None
    # the debug entry: the descriptor and the table length are checked before the context is looked at
    assert "null" in refused(L.vox_debug_attn_decode_paged_ring(None, None, 19, None, None, None, None))
    d = pkg.gguf.AttnDecodeDesc(n_seq=1, n_heads=4, n_kv_heads=2, head_dim=128, window=255, page_rows=0)
    assert "paged" in refused(L.vox_debug_attn_decode_paged_ring(None, C.byref(d), 19, None, None, None, None))
    d.page_rows = 16
    for bad in (0, -3, 1025):
        assert "page_tab_len" in refused(L.vox_debug_attn_decode_paged_ring(None, C.byref(d), bad, None, None, None, None))


def test_python_refuses_max_positions_on_an_endless_group(pkg):
    class NoModel:      # the refusal comes before the model is touched
        h = None
    with pytest.raises(ValueError, match="max_positions"):
        pkg.LiveStreamGroup(NoModel(), np.zeros(8, np.float32), 2, max_positions=256, endless=True)
    with pytest.raises(ValueError, match="max_positions"):
        pkg.LiveStreamGroup(NoModel(), np.zeros(8, np.float32), 2, max_positions=16384, page_rows=64, endless=True)


@pytest.mark.parametrize("page_rows", [16, 64, 256, 1024])
def test_pages_for_near_the_position_limit(pkg, page_rows):
    """vox_stream_group_pages_for keeps its arithmetic up to 2^24: restated here without the function, position by position over the last pages and at the limit."""
    W = 8192; top = 1 << 24
    for P in list(range(top - 2 * page_rows - 3, top + 1)) + [top - W, top - W - 1, top - W + page_rows]:
        first = max(0, P - W) // page_rows; end = -(-P // page_rows)
        assert pkg.stream_group_pages_for(P, page_rows, W) == (first, end - first), P
        assert end - first <= W // page_rows + 2      # what a member holds between calls never exceeds the window's pages + 1 (+ 1 unaligned)


def _cli(*args):
    cli = os.path.join(ROOT, "voxtral-mini-realtime-rs_amd", "cli.py")
    return subprocess.run([sys.executable, cli, "-a", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json", *args], capture_output=True, text=True, timeout=120)


def test_cli_accepts_a_live_group_with_live_endless_at_argument_parsing():
    r = _cli("--live", "--live-group", "2", "--live-endless")
    assert "endless" not in r.stderr and "usage:" not in r.stderr, r.stderr      # past the parser: what fails now is the missing model file
    assert r.returncode != 2
    r = _cli("--live", "--live-group", "2", "--live-endless", "--live-page-rows", "64")
    assert "endless" not in r.stderr and "usage:" not in r.stderr and r.returncode != 2, r.stderr
    r = _cli("--live-group", "2", "--live-endless")      # still only with --live
    assert r.returncode == 2 and "--live" in r.stderr and r.stdout == ""


@pytest.mark.parametrize("sr", [16000, 48000, 44100, 8000])
def test_no_pass_of_the_feed_planner_runs_more_ticks_than_the_rope_rings_hold(pkg, sr):
    """An endless group's member has 64 rows in its decoder RoPE ring, one per tick of a pass (feed_pass_max_ticks: 65536 / 2560 + 2 = 27 at 4 encoder rows per
    position).  The planner itself -- feed_plan / feed_pass through vox_debug_stream_feed_passes -- never emits a pass with more ticks than that bound: pushes far
    larger than the 16 kHz ring, small and odd pieces between them, a finish, with and without the per-pass cap of a group's 16-bit staging."""
    bound = 65536 // 2560 + 2
    assert bound <= 64
    rng = np.random.default_rng(500 + sr)
    calls = [(int(40 * sr), False), (1, False), (int(rng.integers(1, 3 * sr)), False), (int(7.3 * sr), False)] + [(int(rng.integers(0, sr)), False) for _ in range(40)] + [(int(90 * sr), True)]
    for cap in (0, 65536):
        n = len(calls); ns = (C.c_size_t * n)(*[c[0] for c in calls]); fin = (C.c_int32 * n)(*[int(c[1]) for c in calls])
        rows = np.zeros((4096, 5), np.int64); k = C.c_int32(-1)
        assert pkg.lib().vox_debug_stream_feed_passes(sr, ns, fin, n, cap, rows.ctypes.data_as(C.POINTER(C.c_int64)), 4096, C.byref(k)) == 0
        ticks = rows[:k.value, 4]
        assert k.value > n and ticks.sum() > 800 and ticks.max() <= bound, (sr, cap, int(ticks.max()))
        if sr == 16000 and cap == 0:
            assert ticks.max() >= 25      # a large 16 kHz push fills the ring: the bound is close
