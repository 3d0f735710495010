"""The device-free parts of the burst groups (vox_stream_group_create_burst; DESIGN.md section 8, "Bursts in stream groups"): the new entries exist and are bound;
vox_stream_group_burst_rounds -- the rounds of a pass -- against a brute-force model that hands out one tick at a time; its refusals; the creation refusals that
are decided before the model or a device is touched.  No GPU, no model; every assertion is ==."""
import ctypes as C
import os
from importlib import import_module

import numpy as np
import pytest

NEW_SYMBOLS = ("vox_stream_group_create_burst", "vox_stream_group_burst_info", "vox_stream_group_burst_rounds", "vox_debug_stream_attn_group_burst")
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
    assert pkg.stream_group_burst_rounds is import_module(pkg.__name__ + ".gguf").stream_group_burst_rounds


def brute_rounds(due, burst):
    """The model: a round hands every member that still has a tick due one tick at a time, up to `burst` of them; the members that got none are not in the round."""
    left = list(due); rounds = []
    while any(left):
        row = []
        for z in range(len(left)):
            b = 0
            while left[z] > 0 and b < burst:
                left[z] -= 1; b += 1
            if b:
                row.append(b)
        rounds.append(tuple(row))
    return rounds


def test_rounds_against_the_brute_force_model(gg):
    rng = np.random.default_rng(20)
    seen_ragged = 0
    for _ in range(600):
        n = int(rng.integers(1, 17)); B = int(rng.integers(1, 17))
        due = sorted((int(v) for v in rng.integers(1, 27, size=n)), reverse=True)
        got = gg.stream_group_burst_rounds(due, B)
        assert got == brute_rounds(due, B), (due, B, got)
        assert len(got) == -(-due[0] // B)                                                     # ceil(max / B) rounds
        for z in range(n):
            assert sum(r[z] for r in got if len(r) > z) == due[z]                              # every member's b sums to its due
        for r in got:
            assert 1 <= len(r) <= n and all(1 <= b <= B for b in r)                            # every b <= B; the round's members are a prefix of the order
            assert all(a >= b for a, b in zip(r, r[1:]))                                       # descending
        for a, b in zip(got, got[1:]):
            assert len(b) <= len(a)                                                            # a later round serves a prefix of the round before
        seen_ragged += any(len(set(r)) > 1 for r in got)
    assert seen_ragged > 300


def test_fixed_cases(gg):
    assert gg.stream_group_burst_rounds((26, 3, 1, 1), 16) == [(16, 3, 1, 1), (10,)]
    assert gg.stream_group_burst_rounds((1, 1, 1), 16) == [(1, 1, 1)]
    assert gg.stream_group_burst_rounds((1, 1, 1), 1) == [(1, 1, 1)]
    assert gg.stream_group_burst_rounds((5, 3, 3, 1), 1) == [(1, 1, 1, 1), (1, 1, 1), (1, 1, 1), (1,), (1,)]      # B = 1: max due all-ones rounds, today's rounds
    assert gg.stream_group_burst_rounds((40, 7, 1), 16) == [(16, 7, 1), (16,), (8,)]
    assert gg.stream_group_burst_rounds((17,) * 16, 16) == [(16,) * 16, (1,) * 16]
    assert gg.stream_group_burst_rounds((26, 25, 2), 4)[-1] == (2, 1)


def test_the_raw_rows_are_zero_behind_the_round(pkg):
    L = pkg.lib(); due = (C.c_int32 * 3)(9, 4, 1); out = (C.c_int32 * (17 * 4))(*([-1] * 68)); n = C.c_int32(-1)
    assert L.vox_stream_group_burst_rounds(due, 3, 4, out, 4, C.byref(n)) == 0 and n.value == 3
    rows = np.array(out[:], np.int32).reshape(4, 17)
    assert rows[0].tolist() == [3, 4, 4, 1] + [0] * 13 and rows[1].tolist() == [1, 4] + [0] * 15 and rows[2].tolist() == [1, 1] + [0] * 15
    assert (rows[3] == -1).all()      # rows behind the last round are not written


def test_refusals(pkg, gg):
    L = pkg.lib(); out = (C.c_int32 * (17 * 8))(); n = C.c_int32(-7)

    def refused(due, n_due, burst, max_rounds, word):
        arr = (C.c_int32 * max(len(due), 1))(*due)
        out[0] = -5
        assert L.vox_stream_group_burst_rounds(arr, n_due, burst, out, max_rounds, C.byref(n)) != 0
        msg = L.vox_last_error()
        assert word.encode() in msg, msg
        assert n.value == -7 and out[0] == -5      # nothing written

    refused([], 0, 4, 8, "n 0")
    refused([1] * 17, 17, 4, 8, "n 17")
    refused([3, 5], 2, 4, 8, "descending")            # unsorted
    refused([3, 0], 2, 4, 8, "due[1] = 0")
    refused([3, 2], 2, 0, 8, "burst_ticks 0")
    refused([3, 2], 2, 17, 8, "burst_ticks 17")
    refused([9, 2], 2, 4, 2, "3 rounds")              # too few output rows
    assert L.vox_stream_group_burst_rounds(None, 1, 4, out, 8, C.byref(n)) != 0 and b"null argument" in L.vox_last_error()
    with pytest.raises(pkg.VoxError):
        gg.stream_group_burst_rounds((2, 3), 4)


def test_entries_refuse_null_arguments(pkg):
    L = pkg.lib()
    assert L.vox_stream_group_burst_info(None, None) != 0 and b"null argument" in L.vox_last_error()
    assert L.vox_debug_stream_attn_group_burst(None, None, None, None, None, None, None) != 0 and b"null argument" in L.vox_last_error()


def test_create_burst_refusals_without_a_device(pkg, gg):
    L = pkg.lib(); out = C.c_void_p(); t = (C.c_float * 8)()
    fake = (C.c_char * 64)()      # stands for a model: these refusals come before the model is looked at
    A = C.addressof(fake)
    #                      m  t  n  gains rates cap maxp paged page_rows pool endless kv burst
    for bad in (0, -1, 17):
        assert L.vox_stream_group_create_burst(A, t, 2, None, None, 0, 0, 0, 0, 0, 0, 0, bad, C.byref(out)) != 0
        msg = L.vox_last_error()
        assert f"burst_ticks {bad}".encode() in msg and b"1..16" in msg, msg
    assert L.vox_stream_group_create_burst(None, t, 2, None, None, 0, 0, 0, 0, 0, 0, 0, 4, C.byref(out)) != 0 and b"null argument" in L.vox_last_error()
    for args, word in (((0, 16, 0, 0, 0), b"slab group"), ((0, 0, 8, 0, 0), b"slab group"), ((0, 0, 0, 1, 0), b"slab group"), ((0, 0, 0, 0, 1), b"slab group"),
                       ((2, 0, 0, 0, 0), b"paged 2"), ((1, 0, 0, 2, 0), b"endless 2"), ((1, 0, 0, 0, 5), b"kv_dtype 5"), ((1, -16, 0, 0, 0), b"page_rows -16")):
        paged, page_rows, pool, endless, kv = args
        assert L.vox_stream_group_create_burst(A, t, 2, None, None, 0, 0, paged, page_rows, pool, endless, kv, 4, C.byref(out)) != 0
        assert word in L.vox_last_error(), (args, L.vox_last_error())
    assert L.vox_stream_group_create_burst(A, t, 2, None, None, 0, 512, 1, 0, 0, 1, 0, 4, C.byref(out)) != 0 and b"max_positions" in L.vox_last_error()
    assert L.vox_stream_group_create_burst(A, t, 0, None, None, 0, 0, 0, 0, 0, 0, 0, 4, C.byref(out)) != 0 and b"n_members 0" in L.vox_last_error()
    assert not out.value
    for bad in (0, 17, True, 2.0, "4"):
        with pytest.raises(pkg.VoxError) as e:
            gg.LiveStreamGroup(None, [0.0] * 8, 2, burst=bad)      # (no model: the refusal comes first)
        assert e.value.code == 1 and "burst" in str(e.value) and "1..16" in str(e.value)
