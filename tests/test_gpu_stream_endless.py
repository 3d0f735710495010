"""An endless session (vox_stream_create_endless) across its wrap, end to end on the tiny model: fed the samples of a bounded session (max_positions 16 384) up to
ring rows + 300 positions, it gives that session's ids, peeked ids and -- the tiny model never fuses attention + wo -- its f32 logits, bit for bit; its device
memory stops growing at the ring; after a reset it is a fresh session.  No tolerance anywhere.

The two sessions run in ONE child process (tests/stream_endless_worker.py, which documents the feeding): past the wrap the session launches the ring decode
attention, whose launch count (vox_debug_attn_launches [13]) the suite's other tests hold to 0 in their own process.  This module asserts on what the worker wrote.
A run of this length (2 x 8556 ticks and about 350 small pushes) is what reaching the wrap of an 8192-position window costs; the worker reports its seconds."""
import base64
import contextlib
import io
import json
import os
import subprocess
import sys
import wave

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
RING_SLOT, DECODE_SLOT, STREAM_RING_SLOT = 13, 3, 8
TAIL = 63


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("stream_endless") / "out.npz")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_endless_worker.py"), ROOT, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, f"the endless-session worker failed ({p.returncode}):\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}"
    with np.load(out) as z:
        r = {k: z[k] for k in z.files}
    print(f"bounded session {float(r['seconds_bounded']):.1f} s, endless session {float(r['seconds_endless']):.1f} s for {int(r['P'])} positions each")
    return r


def test_both_sessions_reached_past_the_wrap(run):
    ring, P = int(run["ring_rows"]), int(run["P"])
    assert ring == (8192 + 1 + TAIL + 63) // 64 * 64
    assert int(run["pos_b"]) == int(run["pos_e"]) >= P
    assert int(run["rows_b"]) == int(run["rows_e"]) == int(run["pos_e"]) - 37      # one tapped row per tick (the session starts at position 37)


def test_ids_are_the_bounded_sessions(run):
    assert len(run["ids_e"]) == len(run["ids_b"]) >= int(run["P"]) - 38
    assert np.array_equal(run["ids_e"], run["ids_b"]), np.flatnonzero(run["ids_e"] != run["ids_b"])[:8]


def test_logits_of_the_last_400_positions_are_bit_equal(run):
    a, b = run["lg_e"], run["lg_b"]
    assert a.shape == b.shape and a.shape[0] == 400 and np.isfinite(b).all()
    assert np.ptp(b, axis=0).max() > 0      # (the rows differ from one another: the comparison is not of 400 copies of one row)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"rows {np.unique(np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0])[:8]} of the last 400 differ"


def test_records_of_the_last_400_ids_are_equal(run):
    """Scores and alternatives (k = 3) were on in both sessions: the records behind the last 400 ids -- written into the endless session's grown lists -- byte for byte."""
    assert len(run["rec_b"]) == 400 * 16 and len(run["alt_b"]) == 400 * 72
    assert np.array_equal(run["rec_e"], run["rec_b"]) and np.array_equal(run["alt_e"], run["alt_b"])


def test_peeked_ids_are_equal(run):
    assert len(run["peek_b"]) >= 8 and np.array_equal(run["peek_e"], run["peek_b"])
    assert np.array_equal(run["e_peek0"], run["b_peek0"])


def test_past_the_wrap_the_ring_forms_ran(run):
    """The endless session's per-operator steps from position ring rows on launch the ring attention, dec_layers per tick (a peek's tail included), the bounded
    session none; both run the encoder's ring attention every tick."""
    ring, layers = int(run["ring_rows"]), int(run["dims"][0])
    ticks_past = int(run["pos_e"]) - ring
    assert int(run["counts_bounded"][RING_SLOT]) == 0
    n_ring = int(run["counts_endless"][RING_SLOT])
    assert n_ring >= layers * ticks_past and n_ring % layers == 0
    assert 0 < n_ring - layers * ticks_past <= layers * TAIL      # + the tail of the one peek past the wrap
    assert int(run["counts_endless"][DECODE_SLOT]) + n_ring == int(run["counts_bounded"][DECODE_SLOT])      # every other step: the flat per-head form, as the bounded session's
    assert int(run["counts_endless"][STREAM_RING_SLOT]) == int(run["counts_bounded"][STREAM_RING_SLOT]) > 0
    assert int(run["e_steps"][0]) == 0      # (the tiny model has no engine)


def test_memory_stops_growing_at_the_ring(run):
    """info[5] over the last 200 ticks is constant; from create to the end it grew by exactly the cache's rows 1024 -> ring rows and one doubling of the three
    position-indexed lists (ring rows -> 2 ring rows positions; 4 bytes a token, 16 a score record, 72 an alternatives record) -- so the cache never held more
    than ring rows rows -- and ends below the bounded session's, whose flat cache doubled to 16 384 rows."""
    ring = int(run["ring_rows"]); layers, kvh, hd, _ = (int(v) for v in run["dims"])
    pos, by = run["e_positions"], run["e_bytes"]
    last = by[pos >= pos[-1] - 200]
    assert len(last) >= 50 and (last == last[0]).all(), np.unique(last)
    row_bytes = 2 * layers * kvh * hd * 4
    assert int(by[-1]) - int(run["bytes_e0"]) == row_bytes * (ring - 1024) + (4 + 16 + 72) * ring
    assert int(by.max()) == int(by[-1])
    assert int(by[-1]) < int(run["bytes_b"]) - row_bytes * (16384 - ring) // 2


def test_reset_gives_a_fresh_session(run):
    assert len(run["fresh_ids"]) >= 30 and np.array_equal(run["reset_ids"], run["fresh_ids"])
    assert int(run["reset_info_positions"]) == int(run["fresh_info_positions"]) == 37 + len(run["fresh_ids"])


def test_a_ring_without_room_for_a_tail_is_refused(run):
    msg = str(run["refusal"])
    assert msg and str(8192 + 1 + TAIL) in msg and "dec_ring_rows" in msg, msg


# ---- the CLI flag: a short clip through --live --live-endless prints the line of --live
def _tekken(n=1200):
    vocab = [{"rank": i, "token_bytes": base64.b64encode(f" w{i}".encode()).decode(), "token_str": f" w{i}"} for i in range(n)]
    return {"config": {"pattern": "", "num_vocab_tokens": n, "default_vocab_size": 131072, "default_num_special_tokens": 1000, "version": "v7"}, "vocab": vocab}


def test_cli_live_endless_prints_the_live_line(pkg, tmp_path):
    S = pkg.synth
    cli = __import__("importlib").import_module(pkg.__name__ + ".cli")
    gguf = str(tmp_path / "m.gguf"); S.write_synthetic_gguf(gguf, S.tiny_dims(vocab=2048), seed=5)
    tok = str(tmp_path / "tekken.json"); json.dump(_tekken(1200), open(tok, "w"))
    wav = str(tmp_path / "clip.wav")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes((np.clip(S.synth_audio(8.0, seed=1234), -1, 1) * 32767).astype("<i2").tobytes())

    def run_cli(extra):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf), contextlib.redirect_stderr(io.StringIO()):
            rc = cli.main(["--gguf", gguf, "--tokenizer", tok, "--audio", wav, "--live", "--live-chunk-ms", "400"] + extra)
        return rc, buf.getvalue()

    rc0, out0 = run_cli([])
    rc1, out1 = run_cli(["--live-endless"])
    assert rc0 == 0 and rc1 == 0 and out0.strip() and out1 == out0, (out0, out1)
