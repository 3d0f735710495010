"""Records of the offline and batch paths (vox_records_rows, vox_transcribe_audio_scored, vox_transcribe_batch_scored), the parts that need no GPU: the three entry
points are declared, exported and bound, refuse every bad argument with VOX_ERR_INVALID and a message that names it before a device is touched, the CLI's --words /
--alternatives argument errors, and the word lines the CLI makes from records."""
import ctypes as C
import io
import json
import os
import re

import numpy as np
import pytest

from test_stream_scores_cpu import _tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("vox_records_rows", "vox_transcribe_audio_scored", "vox_transcribe_batch_scored")


def test_records_symbols_declared_exported_bound(pkg):
    L = pkg.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "voxtral_hip.h")).read(), flags=re.S)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(L, name) and name in pkg._lib.SIGNATURES
    assert [len(pkg._lib.SIGNATURES[n][1]) for n in SYMBOLS] == [8, 11, 13]
    assert L.vox_abi_version() == 1
    assert callable(pkg.records_rows) and hasattr(pkg.Q4VoxtralModel, "transcribe_audio_scored") and hasattr(pkg.Q4VoxtralModel, "transcribe_batch_scored")


def test_records_bad_arguments(pkg):
    """Every refusal comes before the dummy handle is read: VOX_ERR_INVALID (1), a message naming the argument, nothing written."""
    L = pkg.lib(); err = lambda: L.vox_last_error().decode()
    dummy = C.c_void_p(1)
    x = np.zeros((2, 8), np.float32); xp = x.ctypes.data
    sc = np.zeros(4, dtype=pkg.SCORE_DTYPE).view(np.uint8); al = np.zeros(4, dtype=pkg.ALTS_DTYPE).view(np.uint8); sc[:] = 0xA5; al[:] = 0xA5
    keep = (sc.copy(), al.copy()); sp, ap = sc.ctypes.data, al.ctypes.data
    # ---- vox_records_rows(ctx, logits, M, V, k, scores, alts, mem_kind)
    rows = [((None, xp, 2, 8, 0, sp, None, 0), "null context"), ((dummy, None, 2, 8, 0, sp, None, 0), "null logits"), ((dummy, xp, 0, 8, 0, sp, None, 0), "bad shape"),
            ((dummy, xp, 2, -1, 0, sp, None, 0), "bad shape"), ((dummy, xp, 2, 8, -1, sp, ap, 0), "k -1 out of range (0..8)"), ((dummy, xp, 2, 8, 9, sp, ap, 0), "k 9 out of range (0..8)"),
            ((dummy, xp, 2, 8, 0, sp, ap, 0), "alts given with k == 0"), ((dummy, xp, 2, 8, 3, sp, None, 0), "k 3 needs the alts array"),
            ((dummy, xp, 2, 8, 0, None, None, 0), "scores and alts are both null"), ((dummy, xp, 2, 8, 3, None, None, 0), "k 3 needs the alts array"),
            ((dummy, xp, 2, 8, 0, sp, None, 2), "mem_kind"), ((dummy, xp, 2, 8, 3, sp, ap, -1), "mem_kind")]
    for args, msg in rows:
        assert L.vox_records_rows(*args) == 1, args
        assert msg in err(), (args, err())
    # ---- vox_transcribe_audio_scored(m, samples, n, t_embed, out_ids, cap, n_ids, scores, alts, k, mem_kind)
    smp = np.zeros(1600, np.float32); te = np.zeros(32, np.float32); ids = np.full(8, -9, np.int32); n = C.c_int32(-3)
    s_, t_, i_ = smp.ctypes.data, te.ctypes.data, ids.ctypes.data
    audio = [((None, s_, 1600, t_, i_, 8, C.byref(n), sp, None, 0, 0), "null model"), ((dummy, s_, 1600, t_, i_, 8, None, sp, None, 0, 0), "null n_ids"),
             ((dummy, s_, 1600, t_, i_, 8, C.byref(n), sp, ap, -1, 0), "k -1 out of range (0..8)"), ((dummy, s_, 1600, t_, i_, 8, C.byref(n), sp, ap, 9, 0), "k 9 out of range (0..8)"),
             ((dummy, s_, 1600, t_, i_, 8, C.byref(n), sp, ap, 0, 0), "alts given with k == 0"), ((dummy, s_, 1600, t_, i_, 8, C.byref(n), sp, None, 2, 0), "k 2 needs the alts array"),
             ((dummy, s_, 1600, t_, i_, 8, C.byref(n), None, None, 0, 0), "scores and alts are both null"), ((dummy, s_, 0, t_, i_, 8, C.byref(n), sp, None, 0, 0), "empty audio"),
             ((dummy, s_, 1600, t_, i_, 8, C.byref(n), sp, None, 0, 7), "mem_kind")]
    for args, msg in audio:
        assert L.vox_transcribe_audio_scored(*args) == 1, args
        assert msg in err(), (args, err())
    # ---- vox_transcribe_batch_scored(m, n, samples, n_samples, norm_group, t_embed, out_ids, caps, n_ids, scores, alts, k, mem_kind)
    ptrs = (C.c_void_p * 1)(s_); lens = (C.c_size_t * 1)(1600); optrs = (C.c_void_p * 1)(i_); caps = (C.c_int32 * 1)(8); nids = (C.c_int32 * 1)(-3)
    sps = (C.c_void_p * 1)(sp); aps = (C.c_void_p * 1)(ap)
    B = lambda m=dummy, nn=1, caps_=caps, nids_=nids, s=sps, a=None, k=0, kind=0: (m, nn, ptrs, lens, None, t_, optrs, caps_, nids_, s, a, k, kind)
    batch = [(B(m=None), "null model"), (B(caps_=None), "null caps"), (B(nids_=None), "null n_ids"), (B(a=aps, k=-1), "k -1 out of range (0..8)"), (B(a=aps, k=9), "k 9 out of range (0..8)"),
             (B(a=aps, k=0), "alts given with k == 0"), (B(k=4), "k 4 needs the alts array"), (B(s=None), "scores and alts are both null"), (B(nn=0), "batch size 0 out of range"),
             (B(kind=3), "mem_kind"), (B(s=(C.c_void_p * 1)(None)), "null scores[0]"), (B(a=(C.c_void_p * 1)(None), k=2), "null alts[0]")]
    for args, msg in batch:
        assert L.vox_transcribe_batch_scored(*args) == 1, msg
        assert msg in err(), (msg, err())
    assert sc.tobytes() == keep[0].tobytes() and al.tobytes() == keep[1].tobytes() and n.value == -3 and nids[0] == -3 and (ids == -9).all()      # nothing was written
    with pytest.raises(pkg.VoxError, match="k 9 out of range"):
        pkg.records_rows(type("Ctx", (), {"h": dummy})(), x, 9)


def test_cli_words_argument_errors(pkg):
    """--alternatives without --words or outside 1..8, and --words with --live (the message points to --live-words): argument errors, exit status 2, before anything
    loads (the files named here do not exist)."""
    import importlib
    cli = importlib.import_module(pkg.__name__ + ".cli")
    base = ["--audio", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json"]
    for extra in (["--alternatives", "3"], ["--words", "w.jsonl", "--alternatives", "0"], ["--words", "w.jsonl", "--alternatives", "9"], ["--batch", "4", "--alternatives", "2"],
                  ["--words", "w.jsonl", "--live"], ["--words", "w.jsonl", "--alternatives", "3", "--live"], ["--words", "w.jsonl", "--gpus", "2"]):
        with pytest.raises(SystemExit) as e:
            cli.main(base + extra)
        assert e.value.code == 2, extra


def test_cli_words_live_message_points_to_live_words(pkg, capsys):
    import importlib
    cli = importlib.import_module(pkg.__name__ + ".cli")
    with pytest.raises(SystemExit):
        cli.main(["--audio", "x.wav", "--gguf", "m.gguf", "--tokenizer", "t.json", "--live", "--words", "w.jsonl"])
    assert "--live-words" in capsys.readouterr().err


def test_cli_word_lines_from_handmade_records(pkg):
    """unit_words / write_word_lines on hand-made records: no due_s (a live-session quantity), the file, the chunk index only for a chunk, first_id / last_id relative
    to the unit, the texts joined are the decoded transcript; with alternatives every line has entropy and weakest."""
    import importlib
    cli = importlib.import_module(pkg.__name__ + ".cli")
    tok = _tokenizer(pkg)
    ids = np.array([32, 1008, 1002, 1000, 33, 1001, 1002, 1003, 1004, 1005, 1006, 1007, 1500], np.int32)      # the ids of test_words_groups_ids_on_the_tokenizers_bytes
    sc = np.zeros(len(ids), dtype=pkg.SCORE_DTYPE)
    sc["logprob"] = -np.arange(1, len(ids) + 1, dtype=np.float32) / 8; sc["margin"] = np.float32([9, 5, 7, 3, 9, 4, 0.5, 0.125, 6, 2, 8, 1, 0.25]); sc["id"] = ids
    al = np.zeros(len(ids), dtype=pkg.ALTS_DTYPE); al["n"] = 2; al["entropy"] = 0.5; al["alt"]["id"] = -1; al["alt"]["logprob"] = np.nan
    for k, t in enumerate(ids):
        al["alt"][k][:2] = [(t, -0.125), (1003, -2.5)]
    ref = pkg.words(ids, sc, tok)
    plain = cli.unit_words(pkg, "a.wav", None, ids, sc, tok)
    assert len(plain) == len(ref) >= 3
    assert all(set(w) == {"text", "first_id", "last_id", "logprob", "min_margin", "file"} and w["file"] == "a.wav" for w in plain)
    assert [{k: v for k, v in r.items() if k != "due_s"} for r in ref] == [{k: v for k, v in w.items() if k != "file"} for w in plain]
    assert "".join(w["text"] for w in plain) == tok.decode([int(t) for t in ids if t >= 1000])
    chunk = cli.unit_words(pkg, "b.wav", 2, ids, sc, tok, al)
    assert all(w["chunk"] == 2 and w["file"] == "b.wav" and "due_s" not in w and "entropy" in w and w["weakest"]["alternatives"] for w in chunk)
    assert [w["first_id"] for w in chunk] == [w["first_id"] for w in plain] and max(w["last_id"] for w in chunk) < len(ids)
    out = io.StringIO(); cli.write_word_lines(out, plain + chunk)
    lines = [json.loads(l) for l in out.getvalue().splitlines()]
    assert lines == json.loads(json.dumps(plain + chunk)) and all("due_s" not in l for l in lines)
    assert cli.unit_words(pkg, "c.wav", None, ids[:0], sc[:0], tok) == []
