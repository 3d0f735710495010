"""voxtral-transcribe --live --live-levels / --live-endpoint-ms: every --live-words line carries peak_db and rms_db; the end-of-speech hint prints ONE tentative "  ~["
line per quiet run; stdout and the "  [" lines are those of the run without the flags."""
import base64
import contextlib
import importlib
import io
import json
import math
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _tekken(n=1200):
    vocab = [{"rank": i, "token_bytes": base64.b64encode(f" w{i}".encode()).decode(), "token_str": f" w{i}"} for i in range(n)]
    return {"config": {"pattern": "", "num_vocab_tokens": n, "default_vocab_size": 131072, "default_num_special_tokens": 1000, "version": "v7"}, "vocab": vocab}


def _write_wav(path, x, sr=16000):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def _lines(err, mark):
    return [l for l in err.split("\n") if l.startswith(mark)]


def test_live_levels_and_endpoint(pkg, tmp_path):
    S = pkg.synth
    cli = importlib.import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    x = S.synth_audio(6.0, seed=1234).copy(); x[24000:40000] = 0; x[64000:80000] = 0      # two silences of 1 s, at 1.5 s and at 4 s
    wav = str(tmp_path / "clip.wav"); _write_wav(wav, x)
    y = S.synth_audio(4.0, seed=77).copy(); y[16000:32000] = 0
    wav2 = str(tmp_path / "clip2.wav"); _write_wav(wav2, y)

    def run(audio, extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok] + [v for a in audio for v in ("--audio", a)] + ["--live"] + extra)
        return rc, buf.getvalue(), err.getvalue()

    words = lambda p: [json.loads(l) for l in open(p, encoding="utf-8").read().splitlines()]
    w0 = str(tmp_path / "w0.jsonl"); w1 = str(tmp_path / "w1.jsonl"); w2 = str(tmp_path / "w2.jsonl")
    rc0, out0, err0 = run([wav], ["--live-words", w0])
    rc1, out1, err1 = run([wav], ["--live-words", w1, "--live-levels"])
    assert rc0 == 0 and rc1 == 0 and out1 == out0 and out0.strip() and _lines(err1, "  [") == _lines(err0, "  [") and not _lines(err1, "  ~[")
    a, b = words(w0), words(w1)
    assert len(a) == len(b) >= 3 and all("peak_db" not in v for v in a)
    assert [{k: v for k, v in v.items() if k not in ("peak_db", "rms_db")} for v in b] == a
    level_ok = lambda v: (v["peak_db"] is None and v["rms_db"] is None) or v["rms_db"] <= v["peak_db"] <= 0.0      # null: digital silence; gained samples peak at 0.95, a mean square is at most the peak's square
    assert all(level_ok(v) for v in b) and "Infinity" not in open(w1).read() and "NaN" not in open(w1).read()      # strict JSON
    assert any(v["peak_db"] is not None and v["peak_db"] > -20 for v in b)

    # the hint: 480 ms of ticks below -50 dBFS -> one tentative line per silence, none elsewhere; everything else as without it
    rc2, out2, err2 = run([wav], ["--live-words", w2, "--live-endpoint-ms", "480"])
    assert rc2 == 0 and out2 == out0 and _lines(err2, "  [") == _lines(err0, "  [")
    assert words(w2) == b      # --live-endpoint-ms implies --live-levels
    ten = _lines(err2, "  ~[")
    assert len(ten) == 2, ten
    at = [float(l[4:].split(" s]")[0]) for l in ten]
    # silence from 1.5 s: the first window inside it is record 11's, [1.6, 1.76) s; id 13, the third of them, is handed out by the push that ends at 2.24 s (id k is due
    # 2.5 ms behind its window, so with the NEXT 160 ms push); the second silence begins on a window's edge, at 4.0 s
    assert math.isclose(at[0], 2.24, abs_tol=1e-6) and math.isclose(at[1], 4.64, abs_tol=1e-6), at
    rc3, out3, err3 = run([wav], ["--live-endpoint-ms", "480", "--live-endpoint-db", "-200"])      # nothing is that quiet but digital silence -- which these stretches are
    assert rc3 == 0 and len(_lines(err3, "  ~[")) == 2
    rc4, out4, err4 = run([wav], ["--live-endpoint-ms", "2000"])      # no silence lasts 2 s
    assert rc4 == 0 and out4 == out0 and not _lines(err4, "  ~[")

    # a group of two: one line per member's silence, and the words carry the levels
    wg = str(tmp_path / "wg.jsonl")
    rcg0, outg0, errg0 = run([wav, wav2], ["--live-group", "2"])
    rcg, outg, errg = run([wav, wav2], ["--live-group", "2", "--live-endpoint-ms", "480", "--live-words", wg])
    assert rcg0 == 0 and rcg == 0 and outg == outg0 and outg.count("\n") == 2 and _lines(errg, "  [") == _lines(errg0, "  [")
    ten = _lines(errg, "  ~[")
    assert len(ten) == 3 and sum(wav2 in l for l in ten) == 1, ten
    g = words(wg)
    assert {v["file"] for v in g} == {wav, wav2} and all("peak_db" in v and "rms_db" in v for v in g)
    assert all(level_ok(v) for v in g)
