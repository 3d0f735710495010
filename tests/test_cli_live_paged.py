"""voxtral-transcribe --live --live-group N --live-page-rows R --live-pool-pages P: the group is a paged one (vox_stream_group_create_paged); stdout and the "  ["
lines are those of the slab group's run, and the group did not fall back to one session per file."""
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


def test_live_group_gives_the_same_lines_on_a_paged_group(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wavs = []
    for i, (sec, seed) in enumerate(((8.0, 1234), (5.0, 77), (3.0, 78))):      # three files on two members: a member is reset and reused
        wavs.append(str(tmp_path / f"clip{i}.wav")); _write_wav(wavs[-1], S.synth_audio(sec, seed=seed))

    def run(extra):
        buf = io.StringIO(); err = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok] + [v for a in wavs for v in ("--audio", a)] + ["--live", "--live-chunk-ms", "400", "--live-group", "2"] + extra)
        return rc, buf.getvalue(), err.getvalue()

    rc0, out0, err0 = run([])
    rc1, out1, err1 = run(["--live-page-rows", "16", "--live-pool-pages", "64"])
    assert rc0 == 0 and rc1 == 0 and out0.count("\n") == 3 and out0.strip()
    assert "Error in the stream group" not in err0 and "Error in the stream group" not in err1      # neither run fell back to one session per file
    assert out1 == out0
    lines = lambda err: [l for l in err.split("\n") if l.startswith("  [")]
    assert lines(err1) == lines(err0) and lines(err0)
    rc2, out2, err2 = run(["--live-page-rows", "0"])      # either flag alone makes the group a paged one, 0 is the default page
    assert rc2 == 0 and out2 == out0 and "Error in the stream group" not in err2
