"""The single-clip driver's plan and its decode graphs, on the tiny model (2 + 2 layers: the per-operator launches; the decode engine needs the
real geometry and is not involved).

Plan: S decoder positions give 0 ids below 38 and max(S - 38, 1) from there on; the first id comes out of the prefill, every further one out of a decode step, so a
graph-path call enqueues steps = max(S - 39, 0) steps.  Graph owner: the first graph-path call of a fresh model (or the first one after the graphs' key -- cache, audio
buffer, unroll, step form -- changed) runs one step eagerly, captures, and replays steps - 1; every later call replays all of them.

Tolerance: the rule of the neighbouring files -- ids equal to the CPU oracle's up to the first step whose oracle top-2 margin is below 10 x TOL x max|logit|, TOL = 2e-4."""
import numpy as np
import pytest

from model_fixtures import check_greedy_ids, fake_mel, tiny_gguf

pytestmark = pytest.mark.gpu
TOL = 2e-4
T_OF_S = {37: 592, 38: 608, 39: 624, 40: 640, 41: 656}      # mel frames -> decoder positions: two stride-2 convolutions, 4 rows per position
T_SHORT, S_SHORT = 800, 50          # 11 steps: with a 4-step graph 1 eager + 2 x 4 + 2 single
T_LONG, S_LONG = 4200, 262          # past the 256 rows the model's cache starts with: re-allocated


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle(orc):
    o = orc.Model(tiny_gguf()[0])
    yield o
    o.close()


@pytest.fixture(scope="module")
def t_embed(pkg):
    return pkg.TimeEmbedding(256).embed(6.0)


@pytest.fixture(scope="module")
def ref(oracle, t_embed):
    """(mel, oracle ids, oracle logits) per mel length, computed once."""
    memo = {}

    def get(T):
        if T not in memo:
            mel = fake_mel(T, seed=900 + T)
            rids, rlg = oracle.transcribe_streaming(mel, t_embed, want_logits=True)
            rids.setflags(write=False); rlg.setflags(write=False)
            memo[T] = (mel, rids, rlg)
        return memo[T]
    return get


@pytest.fixture
def fresh(pkg, ctx):
    made = []

    def load():
        made.append(pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx))
        return made[-1]
    yield load
    for m in made:
        m.close()


def _steps(S):
    return max(S - 39, 0)


def test_plan_edges(oracle, fresh, ref, t_embed):
    assert [oracle.enc_seq_len(T) // 4 for T in T_OF_S.values()] == [37, 38, 39, 40, 41]
    m = fresh()
    for (S, T), n in zip(T_OF_S.items(), (0, 1, 1, 2, 3)):
        mel, rids, rlg = ref(T)
        assert len(rids) == n, (S, len(rids))
        ids = m.transcribe_streaming(mel[None], t_embed)
        assert len(ids) == n and m.timings()["decode_tokens"] == n, (S, len(ids), m.timings())
        ids_l, lg = m.transcribe_streaming(mel[None], t_embed, return_logits=True)
        assert len(ids_l) == n and lg.shape == (n, 512) and m.timings()["decode_tokens"] == n, (S, len(ids_l), lg.shape)
        assert (np.argmax(lg, axis=1) == ids_l).all() and (ids_l == ids).all(), S
        if n:
            check_greedy_ids(ids, rids, rlg, TOL)


@pytest.mark.parametrize("unroll", [None, 4])
def test_replay_accounting(pkg, fresh, ref, t_embed, monkeypatch, unroll):
    mel, rids, rlg = ref(T_SHORT); steps = _steps(S_SHORT)
    assert len(rids) == S_SHORT - 38 and steps >= 9
    m = fresh()
    if unroll is None:
        base = None
    else:
        base = m.transcribe_streaming(mel[None], t_embed)      # the graphs of the default unroll exist: the knob must re-key them
        monkeypatch.setenv("VOX_DECODE_UNROLL", str(unroll)); pkg.lib()      # (lib() has the library re-read its knobs)
    first = m.transcribe_streaming(mel[None], t_embed); r1 = m.timings()["graph_replays"]
    second = m.transcribe_streaming(mel[None], t_embed); r2 = m.timings()["graph_replays"]
    if unroll is not None:
        monkeypatch.delenv("VOX_DECODE_UNROLL"); pkg.lib()
    print(f"unroll {unroll}: {steps} steps, replays {r1} then {r2}")
    assert (r1, r2) == (steps - 1, steps)
    assert (first == second).all() and (base is None or (base == first).all())
    check_greedy_ids(first, rids, rlg, TOL)


def test_graphs_are_rekeyed_when_the_cache_moves(oracle, fresh, ref, t_embed):
    assert oracle.enc_seq_len(T_SHORT) // 4 == S_SHORT <= 256 < S_LONG == oracle.enc_seq_len(T_LONG) // 4
    want = {}
    for T in (T_SHORT, T_LONG):
        want[T] = fresh().transcribe_streaming(ref(T)[0][None], t_embed)
        check_greedy_ids(want[T], ref(T)[1], ref(T)[2], TOL)
    m = fresh(); replays = []
    for T in (T_SHORT, T_LONG, T_SHORT):
        ids = m.transcribe_streaming(ref(T)[0][None], t_embed); replays.append(m.timings()["graph_replays"])
        assert len(ids) == len(want[T]) and (ids == want[T]).all(), (T, int((ids == want[T]).sum()))
    print(f"replays {replays}")
    # the re-allocation itself drops the graphs (ensure_decode_state); the larger cache stays, so going back to the short clip neither re-keys nor captures again.
    # (The key comparison of graphs_for is what test_replay_accounting[4] exercises: there only the unroll changes.)
    assert replays == [_steps(S_SHORT) - 1, _steps(S_LONG) - 1, _steps(S_SHORT)]


def test_samples_path_prefix_on_and_off(pkg, orc, oracle, fresh, t_embed):
    """transcribe_audio a few positions above 38 (the pad alone gives 47): prefix rows copied + a first step at position 37, against prefill + first step at 39."""
    x = pkg.synth.synth_audio(0.1, seed=17)
    xn = x.copy(); orc.lib().orc_peak_normalize(xn, xn.size, 0.95)
    mel = np.ascontiguousarray(orc.mel_compute_log(orc.pad_audio(xn)).T)
    S = oracle.enc_seq_len(mel.shape[1]) // 4
    assert 39 <= S <= 50, S
    rids, rlg = oracle.transcribe_streaming(mel, t_embed, want_logits=True)
    m = fresh()
    assert m.set_prefix_cache(True)
    on = m.transcribe_audio(x, t_embed); n_on = m.timings()["decode_tokens"]
    assert m.prefix_info()["built"]
    assert not m.set_prefix_cache(False)
    off = m.transcribe_audio(x, t_embed); n_off = m.timings()["decode_tokens"]
    assert len(on) == len(off) == S - 38 == n_on == n_off, (S, len(on), len(off), n_on, n_off)
    assert (on == off).all()
    check_greedy_ids(on, rids, rlg, TOL)
