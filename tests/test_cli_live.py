"""voxtral-transcribe --live: a WAV fed through a live streaming session in --live-chunk-ms pieces prints the line of the un-chunked path."""
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


def _write_wav(path, x):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(x, -1, 1) * 32767).astype("<i2").tobytes())


def test_live_prints_the_unchunked_line(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wav = str(tmp_path / "clip.wav"); _write_wav(wav, S.synth_audio(16.0, seed=1234))
    args = ["--gguf", gguf, "--tokenizer", tok, "--audio", wav]

    def run(extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(args + extra)
        return rc, buf.getvalue(), err.getvalue()

    rc0, out0, err0 = run(["--max-mel-frames", "100000"])      # the whole file as one utterance
    assert rc0 == 0 and out0.count("\n") == 1 and out0.strip() and "chunk " not in err0
    for ms in (100, 1000):
        rc, out, err = run(["--live", "--live-chunk-ms", str(ms)])
        assert rc == 0 and out == out0, (ms, out, out0)
        partial = [l for l in err.split("\n") if l.startswith("  [")]
        assert len(partial) >= (10 if ms == 1000 else 60)      # text as ids arrive: a 16 s clip has 108 ids, the first after 40 samples
        assert out0.strip().startswith(partial[len(partial) // 2].split("] ", 1)[1].strip())      # what was shown on the way is a prefix of the final line
