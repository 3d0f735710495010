"""voxtral-transcribe --live --live-native-rate: a 48 kHz WAV pushed at its own rate into a live session created for that rate prints the line --live prints for it
(which resamples the whole file before its first push)."""
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


def _write_wav(path, x, sr):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_live_native_rate_prints_the_live_line(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    sr = 48000; n = 8 * sr
    rng = np.random.default_rng(48)
    x = 0.25 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * 0.02) * (1.0 + 0.5 * np.sin(np.arange(n) * 0.0004))
    wav = str(tmp_path / "clip48.wav"); _write_wav(wav, x, sr)
    args = ["--gguf", gguf, "--tokenizer", tok, "--audio", wav]

    def run(extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(args + extra)
        return rc, buf.getvalue(), err.getvalue()

    for ms in (100, 1000):
        rc0, out0, err0 = run(["--live", "--live-chunk-ms", str(ms)])
        assert rc0 == 0 and out0.count("\n") == 1 and out0.strip() and "live session at" not in err0
        rc, out, err = run(["--live", "--live-native-rate", "--live-chunk-ms", str(ms)])
        assert rc == 0 and out == out0, (ms, out, out0)
        assert "live session at 48000 Hz" in err
        partial = [l for l in err.split("\n") if l.startswith("  [")]
        assert len(partial) >= (5 if ms == 1000 else 30)      # text as ids arrive: an 8 s clip has 58 ids
        for l in partial:
            assert out0.strip().startswith(l.split("] ", 1)[1].strip())      # what was shown on the way is a prefix of the final line
