"""Scores of the live sessions' ids (vox_token_score), the parts that need no GPU: the five entry points are exported and refuse bad arguments before they touch a
device, stream_id_due agrees with the schedule, words() groups ids into words on the tokenizer's bytes."""
import base64
import ctypes as C
import json

import numpy as np
import pytest

SYMBOLS = ("vox_score_rows", "vox_stream_set_scores", "vox_stream_scores", "vox_stream_group_set_scores", "vox_stream_group_scores")


def test_score_symbols_and_bad_arguments(pkg):
    """Exported, bound, and VOX_ERR_INVALID for null and bad arguments before any device is touched (the pattern of test_batch_tap_symbols_and_bad_arguments)."""
    L = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES
    assert C.sizeof(pkg._lib.TokenScore) == 16 and pkg.SCORE_DTYPE.itemsize == 16
    assert [pkg.SCORE_DTYPE.fields[n][1] for n in ("logprob", "margin", "runner_up", "id")] == [0, 4, 8, 12]
    x = np.zeros((2, 8), np.float32); out = np.full(2, -7, dtype=pkg.SCORE_DTYPE); before = out.copy(); ids = (C.c_int32 * 2)(0, 8)
    dummy = C.c_void_p(1)      # a context / session pointer that must never be dereferenced: every case fails on an argument checked before it is read
    cases = [((None, x.ctypes.data, 2, 8, None, out.ctypes.data, 0), "null argument"), ((dummy, None, 2, 8, None, out.ctypes.data, 0), "null argument"),
             ((dummy, x.ctypes.data, 2, 8, None, None, 0), "null argument"), ((dummy, x.ctypes.data, 0, 8, None, out.ctypes.data, 0), "bad shape"),
             ((dummy, x.ctypes.data, -1, 8, None, out.ctypes.data, 1), "bad shape"), ((dummy, x.ctypes.data, 2, 0, None, out.ctypes.data, 0), "bad shape"),
             ((dummy, x.ctypes.data, 2, -5, None, out.ctypes.data, 1), "bad shape"), ((dummy, x.ctypes.data, 2, 8, None, out.ctypes.data, 2), "mem_kind"),
             ((dummy, x.ctypes.data, 2, 8, None, out.ctypes.data, -1), "mem_kind"), ((dummy, x.ctypes.data, 2, 8, ids, out.ctypes.data, 0), "row 1: id 8")]
    for args, msg in cases:
        assert L.vox_score_rows(*args) == 1, args
        assert msg in L.vox_last_error().decode(), (args, L.vox_last_error())
    assert L.vox_stream_set_scores(None, 1) == 1 and "null stream" in L.vox_last_error().decode()
    assert L.vox_stream_set_scores(dummy, 2) == 1 and "0 or 1" in L.vox_last_error().decode()
    assert L.vox_stream_scores(None, 0, 1, out.ctypes.data) == 1 and "null stream" in L.vox_last_error().decode()
    assert L.vox_stream_group_set_scores(None, 0, 1) == 1 and "null group" in L.vox_last_error().decode()
    assert L.vox_stream_group_scores(None, 0, 0, 1, out.ctypes.data) == 1 and "null group" in L.vox_last_error().decode()
    assert out.tobytes() == before.tobytes()      # nothing was written


@pytest.mark.parametrize("k", [0, 1, 107])
def test_stream_id_due_agrees_with_the_schedule(pkg, k):
    """stream_id_due(k) is the smallest pushed sample count at which id k is handed out: the schedule says k + 1 ids there and k ids one sample earlier."""
    due = pkg.stream_id_due(k)
    assert due == 2560 * k + 40
    assert pkg.stream_schedule(due)[1] == k + 1 and pkg.stream_schedule(due - 1)[1] == k
    for sr in (48000, 44100, 8000):
        d = pkg.stream_id_due(k, sr)
        assert pkg.stream_schedule_rate(d, sr)[1] == k + 1 and pkg.stream_schedule_rate(d - 1, sr)[1] == k, (sr, d)
        assert d * 16000 >= due * sr      # a rate session cannot know the id before the 16 kHz samples it is made of exist
    with pytest.raises(ValueError):
        pkg.stream_id_due(-1)


def _tokenizer(pkg):
    """vocab index -> bytes: 0 " the", 1 " c", 2 "at", 3 control, 4 " caf", 5 / 6 the two bytes of U+00E9, 7 "\\nnew", 8 "s", 9 "\\tx"."""
    toks = [b" the", b" c", b"at", None, b" caf", b"\xc3", b"\xa9", b"\nnew", b"s", b"\tx"]
    vocab = [{"rank": i, "token_str": "<c>", "is_control": True} if b is None else {"rank": i, "token_bytes": base64.b64encode(b).decode(), "token_str": None}
             for i, b in enumerate(toks)]
    return pkg.VoxtralTokenizer.from_json(json.dumps({"config": {"pattern": "", "num_vocab_tokens": len(vocab), "default_vocab_size": 2048, "default_num_special_tokens": 1000,
                                                                 "version": "v7"}, "vocab": vocab}))


def test_words_groups_ids_on_the_tokenizers_bytes(pkg):
    tok = _tokenizer(pkg)
    #      k: 0   1     2     3     4     5     6     7     8     9     10    11    12
    ids = [32, 1008, 1002, 1000, 33, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1500]      # "s" "at" | " the" | " c" "at" | (control) | " caf" C3 A9 | "\nnew" | (past the vocabulary)
    sc = np.zeros(len(ids), dtype=pkg.SCORE_DTYPE)
    sc["logprob"] = -np.arange(1, len(ids) + 1, dtype=np.float32) / 8; sc["margin"] = np.float32([9, 5, 7, 3, 9, 4, 0.5, 0.125, 6, 2, 8, 1, 0.25]); sc["id"] = ids
    w = pkg.words(ids, sc, tok)
    assert [v["text"] for v in w] == ["sat", " the", " cat", " café", "\nnew"]      # the first text id opens a word; a character split over two ids stays in one
    assert "".join(v["text"] for v in w) == tok.decode(ids)
    assert [(v["first_id"], v["last_id"]) for v in w] == [(1, 2), (3, 3), (5, 6), (8, 10), (11, 11)]      # control ids (< 1000, a control entry, past the vocabulary) belong to no word
    lp = sc["logprob"].astype(np.float64)
    assert [v["logprob"] for v in w] == [lp[1] + lp[2], lp[3], lp[5] + lp[6], lp[8] + lp[9] + lp[10], lp[11]]
    assert [v["min_margin"] for v in w] == [5.0, 3.0, 0.5, 2.0, 1.0]
    assert [v["due_s"] for v in w] == [pkg.stream_id_due(v["last_id"]) / 16000.0 for v in w] and w[0]["due_s"] == (2560 * 2 + 40) / 16000.0
    w48 = pkg.words(ids, sc, tok, sample_rate=48000)
    assert [v["due_s"] for v in w48] == [pkg.stream_id_due(v["last_id"], 48000) / 48000.0 for v in w]
    assert pkg.words([32, 33, 1003], sc[:3], tok) == [] and pkg.words([], sc[:0], tok) == []
    assert [v["text"] for v in pkg.words([1009, 1008], sc[:2], tok)] == ["\txs"]      # a tab opens a word as a space does


def test_live_words_flag_is_refused_without_live(pkg):
    """--live-words without --live is an argument error (argparse: exit status 2), before anything is loaded."""
    import importlib
    cli = importlib.import_module(pkg.__name__ + ".cli")
    with pytest.raises(SystemExit) as e:
        cli.main(["--audio", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json", "--live-words", "w.jsonl"])
    assert e.value.code == 2
