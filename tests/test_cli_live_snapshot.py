"""voxtral-transcribe --live --live-suspend-every N: after every N pushes the session is snapshotted to host memory, its stream freed (its group member reset) and
a fresh one restored from the blob; stdout, the "  [" lines and the words file are those of the plain --live run, for one file and for --live-group 2."""
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


def test_live_suspend_every_changes_nothing(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wav = str(tmp_path / "clip.wav"); _write_wav(wav, S.synth_audio(8.0, seed=1234))
    wav2 = str(tmp_path / "clip2.wav"); _write_wav(wav2, S.synth_audio(5.0, seed=77))

    def run(audio, extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok] + [v for a in audio for v in ("--audio", a)] + extra)
        return rc, buf.getvalue(), err.getvalue()

    live = ["--live", "--live-chunk-ms", "400"]
    # one file, one session: 20 pushes, a suspension behind pushes 3, 6, .., 18
    words0 = str(tmp_path / "w0.jsonl"); words1 = str(tmp_path / "w1.jsonl")
    rc0, out0, err0 = run([wav], live + ["--live-words", words0])
    rc1, out1, err1 = run([wav], live + ["--live-words", words1, "--live-suspend-every", "3"])
    assert rc0 == 0 and rc1 == 0 and out1 == out0 and out0.strip()
    assert _lines(err1, "  [") == _lines(err0, "  [") and open(words1).read() == open(words0).read()
    assert len(_lines(err1, "  *[")) == 6 and not _lines(err0, "  *[")
    with pytest.raises(SystemExit):
        with contextlib.redirect_stderr(io.StringIO()):
            cli.main(["--gguf", gguf, "--tokenizer", tok, "--audio", wav, "--live-suspend-every", "3"])      # applies with --live
    # a group of two, slab and paged
    for extra in ([], ["--live-page-rows", "16"]):
        rc0, out0, err0 = run([wav, wav2], live + ["--live-group", "2"] + extra)
        rc1, out1, err1 = run([wav, wav2], live + ["--live-group", "2", "--live-suspend-every", "3"] + extra)
        assert rc0 == 0 and rc1 == 0 and out1 == out0 and out0.count("\n") == 2 and _lines(err1, "  [") == _lines(err0, "  [")
