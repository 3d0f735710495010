"""Level records of the live sessions (vox_tick_level; DESIGN.md section 8, "Levels"), the parts that need no GPU: the entry points are exported and refuse bad
arguments before they touch a device, level_window agrees with the schedule, the float64 reference (tests/level_ref.py) has the values the definition gives on
hand-made windows, quiet_ticks / level_db / words(levels=) on hand-made records, and the CLI's refusals."""
import base64
import ctypes as C
import importlib
import json
import math

import numpy as np
import pytest

import level_ref as R

F32 = np.float32
SYMBOLS = ("vox_stream_set_levels", "vox_stream_levels", "vox_stream_quiet", "vox_stream_group_set_levels", "vox_stream_group_levels", "vox_stream_group_quiet",
           "vox_level_window", "vox_debug_stream_level")


def test_level_symbols_and_bad_arguments(pkg):
    """Exported, bound, and VOX_ERR_INVALID for null and bad arguments before any handle is read."""
    L = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES
    assert pkg.LEVEL_DTYPE.itemsize == 8 and [pkg.LEVEL_DTYPE.fields[n][1] for n in ("peak", "mean_square")] == [0, 4] and pkg.LEVEL_DTYPE == R.LEVEL_DTYPE
    out = np.full(2, -7, dtype=pkg.LEVEL_DTYPE); before = out.tobytes(); t = C.c_int32(-7); dummy = C.c_void_p(1)      # never dereferenced
    err = lambda: L.vox_last_error().decode()
    assert L.vox_stream_set_levels(None, 1) == 1 and "null stream" in err()
    assert L.vox_stream_set_levels(dummy, 2) == 1 and "0 or 1" in err()
    assert L.vox_stream_levels(None, 0, 1, out.ctypes.data) == 1 and "null stream" in err()
    assert L.vox_stream_quiet(None, 0.01, C.byref(t)) == 1 and "null stream" in err()
    assert L.vox_stream_group_set_levels(None, 0, 1) == 1 and "null group" in err()
    assert L.vox_stream_group_levels(None, 0, 0, 1, out.ctypes.data) == 1 and "null group" in err()
    assert L.vox_stream_group_quiet(None, 0, 0.01, C.byref(t)) == 1 and "null group" in err()
    a = C.c_int64(); b = C.c_int64()
    assert L.vox_level_window(0, None, C.byref(b)) == 1 and "null argument" in err()
    assert L.vox_level_window(-1, C.byref(a), C.byref(b)) == 1 and "record index" in err()
    ring = np.zeros(4096, F32); g = np.ones(1, F32); one = (C.c_int32 * 1)
    ok = dict(ctx=dummy, nm=1, rings=ring.ctypes.data, ring_n=4096, gains=g.ctypes.data, pos=one(37), frame=one(592), order=one(0), ns=1, ticks=1, bb=None, ll=2, out=out.ctypes.data)
    for change, msg in ((dict(ctx=None), "null argument"), (dict(rings=None), "null argument"), (dict(out=None), "null argument"), (dict(nm=17), "slots of"), (dict(ns=2), "slots of"),
                        (dict(ring_n=4095), "ring_n"), (dict(ring_n=2048), "ring_n"), (dict(ticks=0), "ticks"), (dict(ticks=17), "ticks"), (dict(ll=0), "list_len"),
                        (dict(order=one(1)), "order[0]"), (dict(bb=one(2)), "burst_b[0]"), (dict(pos=one(36)), "position"), (dict(frame=one(-1)), "frame"),
                        (dict(gains=np.full(1, np.inf, F32).ctypes.data), "gain")):
        a_ = dict(ok, **change)
        assert L.vox_debug_stream_level(*a_.values()) == 1 and msg in err(), (change, err())
    assert out.tobytes() == before and t.value == -7


@pytest.mark.parametrize("k", [0, 1, 2, 107, 16383])
def test_level_window_against_the_schedule(pkg, k):
    """Window k is the 2560 samples in front of sample 2560 k: it ends at or before the pushed-sample count at which id k is due, so every sample of it has been
    pushed when the id is handed out; it begins where window k - 1 ends; k = 0 lies in the left pad."""
    first, end = pkg.level_window(k)
    assert (first, end) == (2560 * (k - 1), 2560 * k) == R.window(k) and end - first == R.TICK
    assert end <= pkg.stream_id_due(k) and pkg.stream_id_due(k) - end == 40
    assert pkg.stream_schedule(end + 40)[1] == k + 1      # the id is handed out 40 samples behind its window
    if k:
        assert pkg.level_window(k - 1)[1] == first
    else:
        assert end == 0 and first < 0
    with pytest.raises(pkg.VoxError):
        pkg.level_window(-1)


def test_reference_pins():
    """The float64 reference on windows whose records the definition gives outright."""
    x = np.full(3 * R.TICK, 0.5, F32)
    pk, ms = R.levels(x, 1.0, 4)
    assert list(pk) == [0, 0.5, 0.5, 0.5] and list(ms) == [0, 0.25, 0.25, 0.25]      # record 0: all pad; a constant c: (c, c^2)
    pk, ms = R.levels(x, -2.0, 2)
    assert pk[1] == 1.0 and ms[1] == 1.0      # the gain's sign goes
    g = F32(0.37); v = F32(0.5) * g
    pk, ms = R.levels(x, float(g), 2)
    assert pk[1] == v and ms[1] == float(v) ** 2      # one f32 product, then float64
    for at, k in ((0, 1), (R.TICK - 1, 1), (R.TICK, 2), (2 * R.TICK - 1, 2)):      # a single spike at each edge of windows 1 and 2 lands in that window alone
        y = np.zeros(3 * R.TICK, F32); y[at] = -0.75
        pk, ms = R.levels(y, 1.0, 4)
        assert list(np.flatnonzero(pk)) == [k] and pk[k] == 0.75 and ms[k] == 0.5625 / R.TICK and list(np.flatnonzero(ms)) == [k]
    # a window straddling index 0 (not one of an utterance's own: the device sees them through the debug entry): the part below 0 is pad
    v = R.taken(x, 1.0, -1000, -1000 + R.TICK)
    assert (v[:1000] == 0).all() and (v[1000:] == 0.5).all() and R.level_of(v) == (F32(0.5), 0.25 * (R.TICK - 1000) / R.TICK)
    v = R.taken(x, 1.0, 3 * R.TICK - 10, 4 * R.TICK - 10)      # behind the end: a finish's zero pad
    assert (v[:10] == 0.5).all() and (v[10:] == 0).all()
    assert R.bound(0.0) == 2.0 ** -149 and R.bound(1.0) == 2.0 ** -19 + 2.0 ** -149


def _rec(peaks, ms=None):
    r = np.zeros(len(peaks), dtype=R.LEVEL_DTYPE); r["peak"] = peaks; r["mean_square"] = [p * p / 2 for p in peaks] if ms is None else ms
    return r


def test_quiet_ticks_and_level_db(pkg):
    thr = 10.0 ** (-50.0 / 20.0)      # 0.00316
    loud, quiet, nan = 0.3, 0.001, float("nan")
    assert pkg.quiet_ticks(_rec([]), -50.0) == 0
    assert pkg.quiet_ticks(_rec([quiet] * 5)) == 5                       # an all-quiet list
    assert pkg.quiet_ticks(_rec([quiet, quiet, loud])) == 0              # a loud last record
    assert pkg.quiet_ticks(_rec([loud, quiet, quiet, quiet])) == 3
    assert pkg.quiet_ticks(_rec([quiet, nan, quiet, quiet])) == 2        # a NaN record ends the run
    assert pkg.quiet_ticks(_rec([quiet, quiet, nan])) == 0
    assert pkg.quiet_ticks(_rec([0.0, 0.0])) == 2
    assert pkg.quiet_ticks(_rec([float(F32(thr))])) == 0 and pkg.quiet_ticks(_rec([float(np.nextafter(F32(thr), F32(0)))])) == 1      # strictly below
    assert pkg.quiet_ticks(_rec([0.05, 0.05]), -20.0) == 2 and pkg.quiet_ticks(_rec([0.05, 0.05]), -30.0) == 0
    for bad in (float("inf"), float("nan"), -2000.0):      # not a finite positive peak in f32
        with pytest.raises(ValueError):
            pkg.quiet_ticks(_rec([quiet]), bad)
    assert pkg.level_db(0) == -math.inf and pkg.level_db(0.0, power=True) == -math.inf
    assert pkg.level_db(1.0) == 0 and abs(pkg.level_db(0.1) + 20) < 1e-12 and abs(pkg.level_db(0.01, power=True) + 20) < 1e-12
    assert math.isnan(pkg.level_db(float("nan")))
    arr = pkg.level_db(np.array([0.0, 1.0, 10.0]))
    assert arr[0] == -math.inf and arr[1] == 0 and abs(arr[2] - 20) < 1e-12


def _tokenizer(pkg):      # as tests/test_stream_scores_cpu.py: vocab index -> bytes
    toks = [b" the", b" c", b"at", None, b" caf", b"\xc3", b"\xa9", b"\nnew", b"s", b"\tx"]
    vocab = [{"rank": i, "token_str": "<c>", "is_control": True} if b is None else {"rank": i, "token_bytes": base64.b64encode(b).decode(), "token_str": None}
             for i, b in enumerate(toks)]
    return pkg.VoxtralTokenizer.from_json(json.dumps({"config": {"pattern": "", "num_vocab_tokens": len(vocab), "default_vocab_size": 2048, "default_num_special_tokens": 1000,
                                                                 "version": "v7"}, "vocab": vocab}))


def test_words_carry_peak_db_and_rms_db(pkg):
    tok = _tokenizer(pkg)
    #      k: 0   1     2     3     4     5     6     7
    ids = [32, 1008, 1002, 1000, 33, 1001, 1002, 1007]      # "s" "at" | " the" | " c" "at" | "\nnew"
    sc = np.zeros(len(ids), dtype=pkg.SCORE_DTYPE); sc["id"] = ids
    lv = _rec([0.9, 0.5, 0.25, 0.0, 0.9, 0.1, float("nan"), 1.0], ms=[0.5, 0.04, 0.02, 0.0, 0.5, 0.01, float("nan"), 0.25])
    plain = pkg.words(ids, sc, tok)
    w = pkg.words(ids, sc, tok, levels=lv)
    assert [v["text"] for v in w] == ["sat", " the", " cat", "\nnew"]
    assert all("peak_db" not in v and "rms_db" not in v for v in plain)
    assert [{k: v for k, v in x.items() if k not in ("peak_db", "rms_db")} for x in w] == plain      # everything else is untouched
    f = lambda a: float(np.float64(F32(a)))
    assert abs(w[0]["peak_db"] - 20 * math.log10(0.5)) < 1e-12 and abs(w[0]["rms_db"] - 10 * math.log10((f(0.04) + f(0.02)) / 2)) < 1e-12      # the largest peak, the mean of the mean squares
    assert w[1]["peak_db"] == -math.inf and w[1]["rms_db"] == -math.inf      # a word recognised over digital silence says so
    assert math.isnan(w[2]["peak_db"]) and math.isnan(w[2]["rms_db"])       # an id without a record
    assert w[3]["peak_db"] == 0 and abs(w[3]["rms_db"] - 10 * math.log10(0.25)) < 1e-12


def test_cli_refuses_endpoint_and_levels_flags_before_a_model_is_loaded(pkg):
    """--live-endpoint-ms without --live or with a non-positive MS, and --live-levels without --live, are argument errors (exit status 2) with the flag's own message --
    an unknown flag exits with 2 as well, so the message is what shows that the flag exists; no file named here exists."""
    import contextlib, io
    cli = importlib.import_module(pkg.__name__ + ".cli")
    base = ["--audio", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json"]
    endpoint, levels = "--live-endpoint-ms MS (MS > 0) applies with --live", "--live-levels applies with --live"
    for extra, msg in ((["--live-endpoint-ms", "400"], endpoint), (["--live", "--live-endpoint-ms", "0"], endpoint), (["--live", "--live-endpoint-ms", "-160"], endpoint),
                       (["--live-levels"], levels), (["--live-endpoint-ms", "400", "--live-endpoint-db", "-40"], endpoint)):
        err = io.StringIO()
        with pytest.raises(SystemExit) as e, contextlib.redirect_stderr(err):
            cli.main(base + extra)
        assert e.value.code == 2 and msg in err.getvalue() and "unrecognized arguments" not in err.getvalue(), (extra, err.getvalue())


def test_cli_endpoint_trigger_fires_once_per_quiet_run(pkg):
    """The CLI's trigger on (ids handed out, quiet_ticks) pairs: once the run reaches MS, once per run, re-armed by a non-quiet record."""
    cli = importlib.import_module(pkg.__name__ + ".cli")
    e = cli.Endpoint(480, -50.0)
    seq = [(5, 0), (6, 1), (7, 2), (8, 3), (9, 4), (10, 5), (11, 0), (12, 1), (14, 3), (15, 4), (17, 1), (19, 3)]      # (ids, quiet): a run from id 5, one from 11, one from 16
    assert [e.due(i, q) for i, q in seq] == [False, False, False, True, False, False, False, False, True, False, False, True]
