"""Alternatives of the live sessions' ids (vox_token_alts), the parts that need no GPU: the seven entry points are exported and refuse bad arguments before they touch a
device, the record's layout is the header's, words() carries the records into its word entries and is unchanged without them, the CLI flag needs --live-words."""
import ctypes as C

import numpy as np
import pytest

from test_stream_scores_cpu import _tokenizer

SYMBOLS = ("vox_alternatives_rows", "vox_stream_set_alternatives", "vox_stream_alternatives", "vox_stream_peeked_alternatives", "vox_stream_group_set_alternatives",
           "vox_stream_group_alternatives", "vox_stream_group_peeked_alternatives")


def test_alternatives_symbols_and_layout(pkg):
    L = pkg.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES
    T = pkg._lib.TokenAlts
    assert C.sizeof(T) == 72 and pkg.ALTS_DTYPE.itemsize == 72 and C.sizeof(pkg._lib.Alt) == 8
    assert (T.entropy.offset, T.n.offset, T.alt.offset) == (0, 4, 8) and (pkg._lib.Alt.id.offset, pkg._lib.Alt.logprob.offset) == (0, 4)
    assert [pkg.ALTS_DTYPE.fields[n][1] for n in ("entropy", "n", "alt")] == [0, 4, 8]
    sub = pkg.ALTS_DTYPE.fields["alt"][0]
    assert sub.shape == (8,) and sub.base.itemsize == 8 and [sub.base.fields[n][1] for n in ("id", "logprob")] == [0, 4]
    r = np.zeros(1, dtype=pkg.ALTS_DTYPE); raw = r.view(np.uint8)
    for j in range(8):      # offsets 8 + 8 j / 12 + 8 j, checked on the bytes
        r["alt"][0][j] = (100 + j, np.float32(-j - 1))
        assert raw[8 + 8 * j: 12 + 8 * j].view(np.int32)[0] == 100 + j and raw[12 + 8 * j: 16 + 8 * j].view(np.float32)[0] == np.float32(-j - 1)
    assert L.vox_abi_version() == 1


def test_alternatives_bad_arguments(pkg):
    """VOX_ERR_INVALID with a telling message for null and bad arguments, before the dummy handle is read; the output buffers stay as they were."""
    L = pkg.lib()
    x = np.zeros((2, 8), np.float32); out = np.full(4, -7, dtype=pkg.ALTS_DTYPE).view(np.uint8); out[:] = 0xA5; before = out.copy(); n = C.c_int32(-3)
    dummy = C.c_void_p(1); xp, op = x.ctypes.data, out.ctypes.data
    cases = [((None, xp, 2, 8, 3, op, 0), "null argument"), ((dummy, None, 2, 8, 3, op, 0), "null argument"), ((dummy, xp, 2, 8, 3, None, 0), "null argument"),
             ((dummy, xp, 0, 8, 3, op, 0), "bad shape"), ((dummy, xp, -1, 8, 3, op, 1), "bad shape"), ((dummy, xp, 2, 0, 3, op, 0), "bad shape"),
             ((dummy, xp, 2, -5, 3, op, 1), "bad shape"), ((dummy, xp, 2, 8, 0, op, 0), "k 0 out of range (1..8)"), ((dummy, xp, 2, 8, 9, op, 0), "k 9 out of range (1..8)"),
             ((dummy, xp, 2, 8, -1, op, 1), "k -1 out of range"), ((dummy, xp, 2, 8, 3, op, 2), "mem_kind"), ((dummy, xp, 2, 8, 3, op, -1), "mem_kind")]
    for args, msg in cases:
        assert L.vox_alternatives_rows(*args) == 1, args
        assert msg in L.vox_last_error().decode(), (args, L.vox_last_error())
    err = lambda: L.vox_last_error().decode()
    assert L.vox_stream_set_alternatives(None, 3) == 1 and "null stream" in err()
    assert L.vox_stream_set_alternatives(dummy, -1) == 1 and "k -1 out of range (0..8)" in err()
    assert L.vox_stream_set_alternatives(dummy, 9) == 1 and "k 9 out of range (0..8)" in err()
    assert L.vox_stream_alternatives(None, 0, 1, op) == 1 and "null stream" in err()
    assert L.vox_stream_peeked_alternatives(None, op, 4, C.byref(n)) == 1 and "null stream" in err()
    assert L.vox_stream_group_set_alternatives(None, 0, 3) == 1 and "null group" in err()
    assert L.vox_stream_group_set_alternatives(dummy, 0, -1) == 1 and "k -1 out of range (0..8)" in err()      # (k is checked before the handle is read)
    assert L.vox_stream_group_set_alternatives(dummy, 0, 9) == 1 and "k 9 out of range (0..8)" in err()
    assert L.vox_stream_group_alternatives(None, 0, 0, 1, op) == 1 and "null group" in err()
    assert L.vox_stream_group_peeked_alternatives(None, 0, op, 4, C.byref(n)) == 1 and "null group" in err()
    assert out.tobytes() == before.tobytes() and n.value == -3      # nothing was written
    with pytest.raises(pkg.VoxError):
        pkg.alternatives_rows(type("Ctx", (), {"h": dummy})(), x, 0)


def test_words_with_alternatives(pkg):
    tok = _tokenizer(pkg)
    #      k: 0   1     2     3     4     5     6     7     8     9     10    11    12
    ids = [32, 1008, 1002, 1000, 33, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1500]      # the ids of test_words_groups_ids_on_the_tokenizers_bytes
    sc = np.zeros(len(ids), dtype=pkg.SCORE_DTYPE)
    sc["logprob"] = -np.arange(1, len(ids) + 1, dtype=np.float32) / 8; sc["margin"] = np.float32([9, 5, 7, 3, 9, 4, 0.5, 0.125, 6, 2, 8, 1, 0.25]); sc["id"] = ids
    al = np.zeros(len(ids), dtype=pkg.ALTS_DTYPE)
    al["entropy"] = np.float32([0, 0.5, 0.25, 1.5, 0, 0.75, 0.125, 9, 0.5, 2.5, 1.0, np.nan, 0]); al["n"] = 3; al["alt"]["id"] = -1; al["alt"]["logprob"] = np.nan
    for k, t in enumerate(ids):      # the id itself, then a control id, then an id past the vocabulary
        al["alt"][k][:3] = [(t, -0.125), (1003, -2.5), (1500 + k, -3.0)]
    al["n"][9] = 1      # the weakest id of " café" lists itself alone
    plain = pkg.words(ids, sc, tok)
    w = pkg.words(ids, sc, tok, alternatives=al)
    assert [{k: v for k, v in e.items() if k not in ("entropy", "weakest")} for e in w] == plain      # the fields of a call without records are untouched
    assert all(set(e) == {"text", "first_id", "last_id", "due_s", "logprob", "min_margin"} for e in plain)
    assert [e["entropy"] for e in w][:4] == [0.5, 1.5, 0.75, 2.5] and np.isnan(w[4]["entropy"])      # the largest over the word's own ids (k = 7, a control id, is no one's)
    assert [e["weakest"]["k"] for e in w] == [1, 3, 6, 9, 11]      # the smallest margin of each word
    assert [[a["id"] for a in e["weakest"]["alternatives"]] for e in w] == [[1008, 1003, 1501], [1000, 1003, 1503], [1002, 1003, 1506], [1005], [1007, 1003, 1511]]
    assert [a["text"] for a in w[0]["weakest"]["alternatives"]] == ["s", "", ""] and w[3]["weakest"]["alternatives"][0]["text"] == "�"      # lossy UTF-8; control / past the vocabulary: ""
    assert [a["logprob"] for a in w[1]["weakest"]["alternatives"]] == [-0.125, -2.5, -3.0]
    assert all(ids[e["weakest"]["k"]] == e["weakest"]["alternatives"][0]["id"] for e in w)
    off = np.zeros(len(ids), dtype=pkg.ALTS_DTYPE); off["entropy"] = np.nan; off["alt"]["id"] = -1      # records of a session with alternatives off
    wo = pkg.words(ids, sc, tok, alternatives=off)
    assert all(np.isnan(e["entropy"]) and e["weakest"]["alternatives"] == [] for e in wo)
    assert pkg.words([], sc[:0], tok, alternatives=al[:0]) == []


def test_live_alternatives_flag_needs_live_words(pkg):
    """--live-alternatives without --live-words, or outside 1..8, is an argument error (argparse: exit status 2), before anything is loaded."""
    import importlib
    cli = importlib.import_module(pkg.__name__ + ".cli")
    base = ["--audio", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json", "--live"]
    for extra in (["--live-alternatives", "3"], ["--live-alternatives", "0"], ["--live-words", "w.jsonl", "--live-alternatives", "9"], ["--live-words", "w.jsonl", "--live-alternatives", "0"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2
