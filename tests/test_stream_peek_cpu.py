"""Host side of the live sessions' peek (vox_stream_peek, vox_stream_group_peek, vox_stream_peek_ids): the exported symbols and their argument checks, the id count
against the schedule, and the feed planner's peek mode (vox_debug_stream_feed_passes with finish[c] == 2) against the planner's own finish.  No GPU, no model; every
assertion is == or a stated range.

A peek is planned as a finish with no samples and must leave the session's feed what it was.  So, for any sequence of calls with peeks in it:
  * the rows of the calls that are not peeks are the rows of the same sequence without the peeks;
  * a peek's rows are the rows a finish at that point has;
  * a peek is ONE pass: a second pass would size its room from a position the session is then taken back from."""
import ctypes as C
import os

import numpy as np
import pytest

from test_stream_feed_cpu import _library_passes
from test_stream_rate_cpu import _plan

PEEK_RATES = (16000, 48000, 44100, 32000, 22050, 11025, 8000)


def _msg(pkg):
    return (pkg.lib().vox_last_error() or b"").decode()


def _peek_ids(pkg, n, sr, ids_out):
    k = C.c_int32(-7)
    code = pkg.lib().vox_stream_peek_ids(n, sr, ids_out, C.byref(k))
    return code, k.value


def test_symbols_and_refusals(pkg):
    L = pkg.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "voxtral_hip.h")).read()
    for name in ("vox_stream_peek", "vox_stream_group_peek", "vox_stream_peek_ids"):
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES and f" {name}(" in hdr, name
    n = C.c_int32(); ids = (C.c_int32 * 16)()
    assert L.vox_stream_peek(None, ids, 16, C.byref(n), None) == 1 and "null" in _msg(pkg)
    assert L.vox_stream_group_peek(None, None, 0, None) == 1 and "null" in _msg(pkg)
    assert L.vox_stream_peek_ids(100, 16000, 0, None) == 1 and "null" in _msg(pkg)
    assert _peek_ids(pkg, 100, 0, 0)[0] == 1 and "rate" in _msg(pkg)
    assert _peek_ids(pkg, 100, 44101, 0)[0] == 5 and "44101" in _msg(pkg)      # VOX_ERR_UNSUPPORTED: what the offline resampler refuses
    assert _peek_ids(pkg, 100, 16000, -1)[0] == 1
    # an empty utterance is (97280 + 17 * 1280) // 2560 = 46 positions, 46 - 38 = 8 ids: nobody was handed 9
    assert _peek_ids(pkg, 0, 16000, 8) == (0, 0) and _peek_ids(pkg, 0, 16000, 9)[0] == 1 and "handed out" in _msg(pkg)
    assert pkg.stream_peek_ids(0, 0) == 8 and pkg.stream_peek_ids(40, 1) == 8      # 40 samples pad to one token more: 47 positions, 9 ids, one of them out


def _lengths(sr):
    """0, every multiple of 1280 and 2560 +- 1 (the pad's token and the tick, at 16 kHz and at the rate), every block boundary +- 1, up to ~4 s"""
    fi = _plan(sr)[0] if sr != 16000 else 1280
    ns = {0, 1, 39, 40, 41}
    for k in range(1, 26):
        for step in (1280, 2560, 1280 * sr // 16000, 2560 * sr // 16000):
            ns.update({k * step - 1, k * step, k * step + 1, k * step + 40 * sr // 16000, k * step + 40 * sr // 16000 + 1})
    for k in range(1, 4 * sr // fi + 2):
        ns.update({k * fi - 1, k * fi, k * fi + 1})
    return sorted(ns)


@pytest.mark.parametrize("sr", PEEK_RATES)
def test_id_count_is_the_finished_schedule_minus_the_ids_handed_out(pkg, sr):
    seen = set()
    for n in _lengths(sr):
        out = pkg.stream_schedule_rate(n, sr, finished=False)[1]; fin = pkg.stream_schedule_rate(n, sr, finished=True)[1]
        code, k = _peek_ids(pkg, n, sr, out)
        assert code == 0 and k == fin - out, (sr, n, k, fin, out)
        assert 0 <= k <= 16, (sr, n, k)
        assert _peek_ids(pkg, n, sr, fin) == (0, 0) and _peek_ids(pkg, n, sr, fin + 1)[0] == 1
        seen.add(k)
    assert len(seen) >= 2 and min(seen) >= 8, (sr, sorted(seen))      # "the rest" is eight ids or more; the boundaries above do move it


def _without_peeks(calls):
    """the calls that are not peeks, and for every call its index among them (a peek: None)"""
    kept = []; index = []
    for n, f in calls:
        index.append(None if f == 2 else len(kept))
        if f != 2:
            kept.append((n, f))
    return kept, index


def _sequences(sr):
    fi = _plan(sr)[0] if sr != 16000 else 512
    rng = np.random.default_rng(9100 + sr)
    sizes = [int(v) for v in np.where(rng.random(60) < 0.8, rng.integers(0, 3 * fi + 1, 60), rng.integers(0, 2 * sr + 1, 60))]
    pieces = []
    for v in sizes:
        pieces += [(v, 0), (0, 2)]
    return {"issue": [(sr // 10, 0), (0, 2), (sr // 10, 0), (0, 2), (0, 1)],
            "nothing": [(0, 2), (0, 2), (0, 1)],
            "edges": [c for v in (0, 1, fi - 1, fi, fi + 1, 2560 * sr // 16000, 1) for c in ((v, 0), (0, 2))] + [(0, 1)],
            "pieces": pieces + [(0, 2), (7, 1)],
            "past_the_ring": [(5 * sr, 0), (0, 2), (0, 2), (3 * sr + 1, 0), (0, 2), (0, 1)]}      # pushes larger than the 65536-sample ring: the peek behind them still is one pass


@pytest.mark.parametrize("sr", PEEK_RATES)
def test_planner_peek_is_a_finish_that_leaves_the_session_alone(pkg, sr):
    for name, calls in _sequences(sr).items():
        code, rows = _library_passes(pkg, sr, calls, max_rows=8 * len(calls) + 64)
        assert code == 0, (sr, name, _msg(pkg))
        kept, index = _without_peeks(calls)
        code, plain = _library_passes(pkg, sr, kept, max_rows=8 * len(calls) + 64)
        assert code == 0
        # the calls that are not peeks: row for row what they are without the peeks
        assert [(index[r[0]],) + r[1:] for r in rows if calls[r[0]][1] != 2] == plain, (sr, name)
        n_peeks = 0
        for ci, (n, f) in enumerate(calls):
            if f != 2:
                continue
            n_peeks += 1
            mine = [r[1:] for r in rows if r[0] == ci]
            assert len(mine) == 1, (sr, name, ci, mine)      # ONE pass
            # a finish at this point, after the same calls without their peeks
            before = [c for c in calls[:ci] if c[1] != 2]
            code, fin = _library_passes(pkg, sr, before + [(0, 1)], max_rows=8 * len(calls) + 64)
            assert code == 0
            assert mine == [r[1:] for r in fin if r[0] == len(before)], (sr, name, ci)
            pushed = sum(c[0] for c in before)
            assert mine[0][0] == 0 and mine[0][3] == pkg.stream_peek_ids(pushed, pkg.stream_schedule_rate(pushed, sr)[1], sr), (sr, name, ci)
        assert n_peeks >= 2


def test_planner_peek_refusals(pkg):
    assert _library_passes(pkg, 48000, [(5, 2)])[0] == 1 and "peek" in _msg(pkg)      # a peek has no samples of its own
    assert _library_passes(pkg, 48000, [(5, 3)])[0] == 1 and "finish" in _msg(pkg)
    assert _library_passes(pkg, 16000, [(0, 1), (0, 2)])[0] == 1 and "finished" in _msg(pkg)      # finish's refusal
    code, rows = _library_passes(pkg, 16000, [(0, 2), (0, 0), (0, 1)])      # 0 / 1 behave as before behind a peek
    assert code == 0 and [r[0] for r in rows] == [0, 2] and rows[0][1:] == rows[1][1:]
