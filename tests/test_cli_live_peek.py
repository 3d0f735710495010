"""voxtral-transcribe --live --live-peek: after every push a "  ~[" line on stderr with the text so far plus the tentative tail (vox_stream_peek); stdout, the "  ["
lines and the words file are those of the run without the flag."""
import base64
import contextlib
import io
import json
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


def test_live_peek_adds_tentative_lines_and_changes_nothing_else(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wav = str(tmp_path / "clip.wav"); _write_wav(wav, S.synth_audio(8.0, seed=1234))
    wav2 = str(tmp_path / "clip2.wav"); _write_wav(wav2, S.synth_audio(5.0, seed=77))
    rng = np.random.default_rng(3); n48 = 3 * 48000
    wav48 = str(tmp_path / "clip48.wav"); _write_wav(wav48, 0.3 * rng.standard_normal(n48) + 0.3 * np.sin(np.arange(n48) * 0.02), 48000)

    def run(audio, extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok] + [v for a in audio for v in ("--audio", a)] + extra)
        return rc, buf.getvalue(), err.getvalue()

    # one file, one session
    words0 = str(tmp_path / "w0.jsonl"); words1 = str(tmp_path / "w1.jsonl")
    live = ["--live", "--live-chunk-ms", "400"]
    rc0, out0, err0 = run([wav], live + ["--live-words", words0])
    rc1, out1, err1 = run([wav], live + ["--live-words", words1, "--live-peek"])
    assert rc0 == 0 and rc1 == 0 and out1 == out0 and out0.strip()
    assert _lines(err1, "  [") == _lines(err0, "  [") and not _lines(err0, "  ~[")
    assert open(words1).read() == open(words0).read()
    ten = _lines(err1, "  ~[")
    assert len(ten) == 20      # one per push: 8 s in 400 ms pieces
    assert ten[-1].split("] ", 1)[1].strip() == out0.strip()      # the last one, behind the last push, carries the final text
    shown = [l.split("] ", 1)[1].strip() for l in _lines(err1, "  [")]
    mid = ten[len(ten) // 2].split("] ", 1)[1].strip()
    assert any(mid.startswith(s) and len(mid) > len(s) for s in shown)      # the text so far plus a tail
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            cli.main(["--gguf", gguf, "--tokenizer", tok, "--audio", wav, "--live-peek"])      # applies with --live

    # the file's own rate
    rc0, out0, err0 = run([wav48], live + ["--live-native-rate"])
    rc1, out1, err1 = run([wav48], live + ["--live-native-rate", "--live-peek"])
    assert rc0 == 0 and rc1 == 0 and out1 == out0 and _lines(err1, "  [") == _lines(err0, "  [")
    ten = _lines(err1, "  ~[")
    assert len(ten) == 8 and ten[-1].split("] ", 1)[1].strip() == out0.strip()

    # a group of two
    rc0, out0, err0 = run([wav, wav2], live + ["--live-group", "2"])
    rc1, out1, err1 = run([wav, wav2], live + ["--live-group", "2", "--live-peek"])
    assert rc0 == 0 and rc1 == 0 and out1 == out0 and out0.count("\n") == 2 and _lines(err1, "  [") == _lines(err0, "  [")
    ten = _lines(err1, "  ~[")
    assert len(ten) == 19 + 12      # every call but a file's last, which finishes it
