"""voxtral-transcribe --live --live-group N --live-delays D,D,...: the group is made with a t_embed per member (vox_stream_group_create_t_embeds).  With every delay
equal to --delay the stdout and the "  [" lines are those of the run without the flag and the words lines gain the member's delay and nothing else; with different
delays the group runs without falling back to one session per file and every words line carries the delay of the member that ran its file."""
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


def test_live_delays_on_a_group_of_two(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)      # (ids >= 1000 exist: the lines are not empty)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wavs = []
    for i, (sec, seed) in enumerate(((6.0, 1234), (4.0, 77), (3.0, 78))):      # three files on two members: member 1 is reset and reused
        wavs.append(str(tmp_path / f"clip{i}.wav")); _write_wav(wavs[-1], S.synth_audio(sec, seed=seed))

    def run(name, extra):
        buf = io.StringIO(); err = io.StringIO(); words = str(tmp_path / f"{name}.jsonl")
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(err):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok] + [v for a in wavs for v in ("--audio", a)] +
                          ["--live", "--live-chunk-ms", "400", "--live-group", "2", "--live-words", words] + extra)
        assert rc == 0 and "Error in the stream group" not in err.getvalue(), err.getvalue()      # the run did not fall back to one session per file
        return buf.getvalue(), [l for l in err.getvalue().split("\n") if l.startswith("  [")], [json.loads(l) for l in open(words)]

    out0, lines0, words0 = run("plain", [])
    out1, lines1, words1 = run("same", ["--live-delays", "6,6"])
    assert out0.count("\n") == 3 and out0.strip() and out1 == out0 and lines1 == lines0 and lines0
    assert words0 and all("delay" not in w for w in words0)
    assert [{k: v for k, v in w.items() if k != "delay"} for w in words1] == words0 and all(w["delay"] == 6 for w in words1)
    out2, lines2, words2 = run("one", ["--live-delays", "6"])      # a single value serves every member
    assert out2 == out0 and words2 == words1
    out3, lines3, words3 = run("mixed", ["--live-delays", "2,10"])
    assert out3.count("\n") == 3 and words3
    by_file = {}
    for w in words3:
        by_file.setdefault(w["file"], set()).add(w["delay"])
    assert by_file[wavs[0]] == {2} and by_file[wavs[1]] == {10}      # the first two files start on members 0 and 1
    assert all(len(v) == 1 and v <= {2, 10} for v in by_file.values())
