"""The live sessions' feed planner (feed_plan / feed_pass in vox_feed_plan.cpp: one implementation for a solo vox_stream and for every member of a vox_stream_group) through
its host-only view vox_debug_stream_feed_passes.  No GPU, no model; every assertion is == or <=.

A session takes calls (n samples at its rate, finish or not).  A call runs in PASSES, each bounded by the session's two rings: the input-rate ring (a power of two of at
least 2 fft_in + 32768 samples; none at 16 kHz) and the 65536-sample 16 kHz ring.  `_passes` below restates a pass independently: what is appended, what becomes 16 kHz
samples, the right pad, the ticks.  Held for every rate, over pushes of 0, 1, fft_in - 1, fft_in, fft_in + 1 samples, ~400 seeded random pieces, one push larger than
both rings, a finish after each, a finish with nothing pushed, and the large push again under a per-pass cap of 65536 input samples (a group's 16-bit staging slot):

  conservation   per call the appended input sums to n; after every call the cumulative 16 kHz samples are vox_stream_schedule_rate's samples_16k and the cumulative
                 ticks its ids; on finish the pad zeros sum to vox_pad_len(n16) - left - n16
  finality       before finish, the cumulative 16 kHz samples after any pass are <= max(0, (in_written // fft_in) * fft_out - delay): only complete blocks count
  input ring     in every pass, in_written after the append - max(0, c_next - 1) * fft_in <= the input ring's size, c_next = (n_written + delay) // fft_out taken before
                 the pass: block c_next - 1, whose tail the next 16 kHz sample reads, is never overwritten
  16 kHz ring    n_written after the pass - max(0, (16 pos - 3) * 160 - 200 - left) <= 65536, pos taken before the pass's ticks: the oldest sample the next tick reads stays
  progress       no pass is all zeros (the drivers' stall refusal is unreachable for valid input)

and the library's rows are the restatement's, row for row, for every rate and sequence."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from test_stream_rate_cpu import LEFT, RATES, _plan

RING16 = 1 << 16
ALL_RATES = RATES + (16000,)
SPP = 2560            # samples per decoder position (4 encoder rows x 4 frames x 160)
PREFIX_POS = 37       # a session starts behind the prefix: the next tick is decoder position 37


def _in_ring(sr):
    n = 1
    while n < 2 * _plan(sr)[0] + (1 << 15):
        n <<= 1
    return n


def _positions(n16):
    """decoder positions whose last frame reads nothing beyond n16 samples (unfinished form)"""
    return max(0, (LEFT + n16 - 40) // SPP)


def _padded(n16):
    total = LEFT + n16
    return total + (-total) % 1280 + 17 * 1280


def _passes(sr, calls, cap=None):
    """[(call, appended, samples into the 16 kHz ring, pad, ticks)] and, per row, the state the bounds are about:
    (finish, in_written after, c_next before, n_written after, pos before)"""
    rate = sr != 16000
    fi, fo, d = _plan(sr) if rate else (1, 1, 0)
    in_n = _in_ring(sr) if rate else 0
    pushed = n_written = in_written = 0; pos = PREFIX_POS
    rows, seen = [], []
    for ci, (n, finish) in enumerate(calls):
        total_in = pushed + n
        if not rate:
            goal = total_in
        elif finish:
            goal = math.ceil((16000 / sr) * total_in)
        else:
            goal = max(0, total_in // fi * fo - d)
        if finish:
            target = max(_padded(goal) // SPP - 1, pos); right = _padded(goal) - LEFT - goal
        else:
            target = max(_positions(goal), pos); right = 0
        pushed = total_in; done = 0
        while done < n + right or n_written < goal or pos < target:
            room = RING16 - (n_written - max(0, (16 * pos - 3) * 160 - 200 - LEFT))
            c_next = (n_written + d) // fo
            rest = max(0, n - done) if cap is None else min(max(0, n - done), cap)
            if rate:
                a = min(rest, in_n - max(0, in_written - max(0, c_next - 1) * fi))
                in_written += a; done += a
                have = goal if finish and done >= n else max(0, in_written // fi * fo - d)
                k = min(max(0, have - n_written), room)
            else:
                a = k = min(rest, room); in_written += a; done += a
            n_written += k; room -= k
            z = 0
            if n <= done < n + right and n_written >= goal:
                z = min(n + right - done, room); n_written += z; done += z
            ticks = max(0, min(target, _positions(n_written)) - pos)
            rows.append((ci, a, k, z, ticks)); seen.append((finish, in_written, c_next, n_written, pos))
            assert a or k or z or ticks, (sr, ci, n, finish)      # (the restatement itself would loop for ever)
            pos += ticks
    return rows, seen


def _library_passes(pkg, sr, calls, cap=None, max_rows=None):
    n = len(calls); ns = (C.c_size_t * max(n, 1))(*[c[0] for c in calls]); fin = (C.c_int32 * max(n, 1))(*[int(c[1]) for c in calls])
    max_rows = 4 * n + 64 if max_rows is None else max_rows
    rows = np.zeros((max(max_rows, 1), 5), np.int64); k = C.c_int32(-1)
    code = pkg.lib().vox_debug_stream_feed_passes(sr, ns, fin, n, cap or 0, rows.ctypes.data_as(C.POINTER(C.c_int64)), max_rows, C.byref(k))
    return code, [tuple(int(v) for v in r) for r in rows[:max(k.value, 0)]]


def _big(sr):
    """one push larger than both rings: at least 2 * 65536 samples at 16 kHz final after it (two blocks more than their worth: the delay), and more than the input ring"""
    fi, fo, _ = _plan(sr) if sr != 16000 else (1, 1, 0)
    return max(-(-2 * RING16 * fi // fo) + 2 * fi + 7, 2 * _in_ring(sr) + 3 if sr != 16000 else 0)


def _sequences(sr):
    fi = _plan(sr)[0] if sr != 16000 else 512
    rng = np.random.default_rng(7000 + sr)
    sizes = np.where(rng.random(400) < 0.9, rng.integers(0, 3 * fi + 1, 400), rng.integers(0, 3 * sr + 1, 400))
    return {"edges": ([(v, False) for v in (0, 1, fi - 1, fi, fi + 1)] + [(0, True)], None),
            "pieces": ([(int(v), False) for v in sizes] + [(0, True)], None),
            "big": ([(_big(sr), False), (0, True)], None),
            "nothing": ([(0, True)], None),
            "big_capped": ([(_big(sr), False), (fi + 1, True)], RING16),      # (the last call pushes and finishes at once, as a group entry may)
            "big_finishing": ([(1, False), (_big(sr), True)], None)}


@pytest.mark.parametrize("sr", ALL_RATES)
def test_every_pass_conserves_and_stays_inside_both_rings(pkg, sr):
    rate = sr != 16000
    fi, fo, d = _plan(sr) if rate else (1, 1, 0)
    in_n = _in_ring(sr)
    for name, (calls, cap) in _sequences(sr).items():
        code, rows = _library_passes(pkg, sr, calls, cap)
        assert code == 0, (sr, name, pkg.lib().vox_last_error())
        mine, seen = _passes(sr, calls, cap)
        assert rows == mine, (sr, name)      # the library's rows are the restatement's: the bounds below are about the library
        pushed = s16 = ticks = 0
        for ci, (n, finish) in enumerate(calls):
            mine_c = [r for r in rows if r[0] == ci]
            assert sum(r[1] for r in mine_c) == n, (sr, name, ci)
            pushed += n; s16 += sum(r[2] for r in mine_c); ticks += sum(r[4] for r in mine_c)
            _, ids, n16 = pkg.stream_schedule_rate(pushed, sr, finished=finish)
            assert (s16, ticks) == (n16, ids), (sr, name, ci, n)
            assert sum(r[3] for r in mine_c) == (pkg.PadConfig.voxtral().padded_len(n16) - LEFT - n16 if finish else 0), (sr, name, ci)
        for r, (finish, in_written, c_next, n_written, pos) in zip(rows, seen):
            assert r[1] or r[2] or r[3] or r[4], (sr, name, r)
            assert cap is None or r[1] <= cap
            if not finish:
                assert n_written <= max(0, in_written // fi * fo - d), (sr, name, r)
            if rate:
                assert in_written - max(0, c_next - 1) * fi <= in_n, (sr, name, r)
            assert n_written - max(0, (16 * pos - 3) * 160 - 200 - LEFT) <= RING16, (sr, name, r)
        if name in ("big", "big_capped"):      # the large push did wrap both rings, in more than one pass
            assert calls[0][0] > in_n and pkg.stream_schedule_rate(calls[0][0], sr)[2] >= 2 * RING16 and sum(1 for r in rows if r[0] == 0) > 2


def test_the_restated_rings_are_the_documented_ones():
    assert _in_ring(48000) == 1 << 16      # 2 * 513 + 32768 rounded up
    for sr in RATES:
        assert _in_ring(sr) >= 2 * _plan(sr)[0] + 32768 and _in_ring(sr) & (_in_ring(sr) - 1) == 0
    assert _padded(0) == LEFT + 17 * 1280 and _positions(40) == 38 and _positions(39) == 37


def test_symbol_and_refusals(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voxtral_hip.h")).read()
    assert hasattr(L, "vox_debug_stream_feed_passes") and "vox_debug_stream_feed_passes" in pkg._lib.SIGNATURES and " vox_debug_stream_feed_passes(" in hdr
    msg = lambda: (L.vox_last_error() or b"").decode()
    calls = [(100000, False), (0, True)]
    code, rows = _library_passes(pkg, 48000, calls)
    assert code == 0 and len(rows) >= 2
    assert _library_passes(pkg, 48000, calls, max_rows=len(rows))[0] == 0
    assert _library_passes(pkg, 48000, calls, max_rows=len(rows) - 1)[0] == 1 and "too small" in msg()
    assert _library_passes(pkg, 0, calls)[0] == 1 and "rate" in msg()
    assert _library_passes(pkg, 44101, calls)[0] == 5 and "44101" in msg()      # VOX_ERR_UNSUPPORTED: what the offline resampler refuses
    assert _library_passes(pkg, 48000, [(0, True), (5, False)])[0] == 1 and "finished" in msg()
    assert _library_passes(pkg, 48000, [(5, 2)])[0] == 1 and "finish" in msg()
    assert _library_passes(pkg, 48000, [((1 << 36) + 1, False)])[0] == 1
    k = C.c_int32()
    assert L.vox_debug_stream_feed_passes(48000, None, None, 1, 0, None, 0, C.byref(k)) == 1 and "null" in msg()
    assert L.vox_debug_stream_feed_passes(48000, None, None, 0, 0, None, 0, None) == 1 and "null" in msg()
    assert L.vox_debug_stream_feed_passes(48000, None, None, 0, 0, None, 0, C.byref(k)) == 0 and k.value == 0
