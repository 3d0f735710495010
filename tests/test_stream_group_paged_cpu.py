"""Host side of the paged stream group (vox_stream_group_create_paged, vox_stream_group_pool, vox_stream_group_pages_for, vox_debug_stream_group_pages): the exported
symbols, the page arithmetic against a brute-force restatement, the argument checks that need no device, the CLI's refusals.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGED_SYMBOLS = ("vox_stream_group_create_paged", "vox_stream_group_pool", "vox_stream_group_pages_for", "vox_debug_stream_group_pages")


def test_symbols_are_declared_and_bound_and_the_abi_stays_one(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(ROOT, "include", "voxtral_hip.h")).read()
    for name in PAGED_SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES and f" {name}(" in hdr
    assert L.vox_abi_version() == 1
    assert callable(pkg.stream_group_pages_for) and hasattr(pkg.LiveStreamGroup, "pool") and hasattr(pkg.LiveStreamGroup, "pages")


def _brute_force(page_rows, window, upto):
    """Row by row, no division of a position: the member at position P has written rows 0 .. P-1 and its next tick attends rows >= P - window (window -1: all).  rows[q]
    counts the rows of logical page q that are both written and still attended; the held pages are the ones with a row -> {P: (first page, pages)}."""
    rows = {}; out = {}; lo = 0
    for P in range(upto + 1):
        if P > 0:
            q = (P - 1) // page_rows; rows[q] = rows.get(q, 0) + 1      # row P-1 has been written
        while window >= 0 and lo < P - window:                    # row lo fell out of the window
            q = lo // page_rows; rows[q] -= 1
            if rows[q] == 0:
                del rows[q]
            lo += 1
        if rows:
            assert sorted(rows) == list(range(min(rows), max(rows) + 1))
            out[P] = (min(rows), len(rows))
        else:
            out[P] = (lo // page_rows, 0)      # nothing held: counted from the page of the next row
    return out


@pytest.mark.parametrize("page_rows", [16, 64, 256, 1024])
@pytest.mark.parametrize("window", [8192, 100, -1])
def test_pages_for_equals_the_brute_force_count(pkg, page_rows, window):
    L = pkg.lib(); f = C.c_int32(); n = C.c_int32()
    ref = _brute_force(page_rows, window, 20000)
    for positions in range(0, 20001):
        assert L.vox_stream_group_pages_for(positions, page_rows, window, C.byref(f), C.byref(n)) == 0
        assert (f.value, n.value) == ref[positions], (positions, page_rows, window)
    assert pkg.stream_group_pages_for(8392, page_rows, window) == ref[8392]      # the wrapper's tuple


def test_bad_arguments_are_refused_before_any_device_use(pkg):
    L = pkg.lib(); INVALID = 1
    f = C.c_int32(); n = C.c_int32(); out = C.c_void_p(); t = np.zeros(8, np.float32); v = (C.c_int64 * 4)()

    def refused(code):
        assert code == INVALID
        msg = (L.vox_last_error() or b"").decode()
        assert msg
        return msg

    for bad in (0, 8, 15, 48, 2048, -16):
        assert "page_rows" in refused(L.vox_stream_group_pages_for(100, bad, 8192, C.byref(f), C.byref(n)))
    assert "positions" in refused(L.vox_stream_group_pages_for(-1, 16, 8192, C.byref(f), C.byref(n)))
    assert "window" in refused(L.vox_stream_group_pages_for(100, 16, -2, C.byref(f), C.byref(n)))
    assert "null" in refused(L.vox_stream_group_pages_for(100, 16, 8192, None, C.byref(n)))
    assert "null" in refused(L.vox_stream_group_pages_for(100, 16, 8192, C.byref(f), None))
    # without a model there is no group: create can only be refused, and says why
    assert "page_rows" in refused(L.vox_stream_group_create_paged(None, t.ctypes.data, 4, None, None, 0, 0, -1, 0, C.byref(out)))
    assert "null" in refused(L.vox_stream_group_create_paged(None, t.ctypes.data, 4, None, None, 0, 0, 16, 0, C.byref(out)))
    assert "n_members" in refused(L.vox_stream_group_create_paged(None, t.ctypes.data, 17, None, None, 0, 0, 16, 0, C.byref(out)))
    assert out.value is None
    assert "null" in refused(L.vox_stream_group_pool(None, v, None))
    assert refused(L.vox_debug_stream_group_pages(None, 0, None, 0, C.byref(n)))


def _cli(*args):
    cli = os.path.join(ROOT, "voxtral-mini-realtime-rs_amd", "cli.py")
    return subprocess.run([sys.executable, cli, "-a", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json", *args], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("args, needle", [
    (("--live", "--live-page-rows", "16"), "--live-group"),
    (("--live", "--live-pool-pages", "64"), "--live-group"),
    (("--live-page-rows", "16"), "--live-group"),
    (("--live", "--live-group", "2", "--live-page-rows", "48"), "power of two"),
    (("--live", "--live-group", "2", "--live-pool-pages", "-1"), "--live-pool-pages"),
])
def test_cli_refuses_paging_misuse(args, needle):
    r = _cli(*args)
    assert r.returncode == 2 and needle in r.stderr and r.stdout == ""
