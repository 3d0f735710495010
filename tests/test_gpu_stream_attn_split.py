"""The key-split decode attention in the live sessions (set_attn_split) on the tiny models, whose solo per-operator step runs from position 0.  (1) A paged group of
three members and a solo endless stream on the same audio with the flag never touched, set off, set on, and toggled off -> on -> off between calls: off is the untouched
container bit for bit, launch for launch; on, every decode step launches the split ([20]) and the merge ([21]) once per layer and no plain decode attention.  (2) An
endless stream 8300 ids long, past the wrap of its 8256-row ring, at 2:1 and at the full-size model's 4:1 heads (G = 4, 33 - 34 chunks, the 8192-key window): on
against a bounded session with the flag off (which tests/test_gpu_stream_endless.py holds the plain endless session to, and whose in-ring launches would count in slot
[13], which the suite holds to 0 in this process).  Ids: the off run's by check_greedy_ids at 2e-4 with at most 10 % of them behind a first near-tie, on clips whose
OFF logits have no near-tie (asserted from the off run alone); logits within 2e-4 of the largest.
NOT here: a full-size group at position 8300.  No call seeds a group's cache at a position but vox_stream_group_restore, whose blob for one full-size member at the
window is 2.1 GB of K / V, and 8300 full-size rounds are a minute: neither is a test of a few seconds.  The full-size geometry runs in (2) and, one launch at a time
against float64, in tests/test_gpu_attn_decode_split.py; full-size WEIGHTS with the flag on are not run by any test."""
import ctypes

import numpy as np
import pytest

from model_fixtures import check_greedy_ids, tiny_gguf
from stream_helpers import _gain, _stop, _t

pytestmark = pytest.mark.gpu
TOL, TICK = 2e-4, 2560
PLAIN = (3, 5, 11, 12, 13)


@pytest.fixture(scope="module")
def env(pkg):
    ctx = pkg.Context(0); held = {}

    def model(heads=4):
        if heads not in held:
            held[heads] = pkg.Q4ModelLoader.from_file(tiny_gguf(**({"dec_heads": heads} if heads != 4 else {}))[0]).load(ctx)
        return held[heads]
    yield pkg, model
    for m in held.values():
        m.close()
    ctx.close()


def slots(pkg):
    a = (ctypes.c_uint64 * 24)()
    assert pkg.lib().vox_debug_attn_launches(a, 24) == 0
    return np.array(a[:], np.int64)


def run(pkg, c, clips, step, mode):
    """The clips through container c (closed here) in pieces of `step` samples, the last piece finishing -> (ids, tapped logits) per clip, the launch slots' rise,
    their rise and the decode steps (a group: rounds) since the last change of the flag."""
    group = hasattr(c, "advance"); n_calls = -(-len(clips[0]) // step)
    steps = lambda: c.burst_info()["plain_rounds"] if group else c.info()["operator_steps"]
    try:
        if mode != "never":
            c.set_attn_split(mode == "on")
        for k in range(len(clips)):
            c.tap_arm(k, 256) if group else c.tap_arm(len(clips[0]) // TICK + 64)
        ids = [[] for _ in clips]; s0 = s1 = slots(pkg); n1 = 0
        for i in range(n_calls):
            if mode == "toggle" and i in (n_calls // 3, 2 * n_calls // 3):
                c.set_attn_split(i == n_calls // 3); s1 = slots(pkg); n1 = steps()
            feeds = {k: x[i * step:(i + 1) * step] for k, x in enumerate(clips) if i * step < len(x)}
            if group:
                for k, v in c.advance(feeds, finish=[k for k in feeds if (i + 1) * step >= len(clips[k])]).items():
                    ids[k].extend(v)
            else:
                ids[0].extend(c.push(feeds[0])); ids[0].extend(c.finish() if i == n_calls - 1 else [])
        assert c.attn_split() == (mode == "on")
        taps = [c.tap_fetch(k) if group else c.tap_fetch() for k in range(len(clips))]
        return [np.array(v, np.int32) for v in ids], taps, slots(pkg) - s0, slots(pkg) - s1, steps() - n1
    finally:
        c.close()


def near(on, off, what):
    """ids against the off run's, clip by clip: no near-tie in the off run; check_greedy_ids, at most 10 % left out; the logits rows up to there within TOL of the largest."""
    for k, (a, lg, r, rlg) in enumerate(zip(*on[:2], *off[:2])):
        assert _stop(rlg, TOL) == len(rlg) >= 20, f"{what}, clip {k}: the off run has a near-tie of its own at id {_stop(rlg, TOL)}: pick another clip"
        first = check_greedy_ids(a, r, rlg, TOL)
        d = float(np.abs(lg[:first] - rlg[:first]).max()) / float(np.abs(rlg).max())
        print(f"{what}, clip {k}: {first} of {len(r)} ids equal, logits within {d:.1e} of the largest")
        assert 10 * first >= 9 * len(r) and d <= TOL, (first, len(r), d)


@pytest.mark.parametrize("group", [True, False], ids=["paged_group", "solo_endless"])
def test_off_is_untouched_and_on_is_near(env, group):
    pkg, model = env; m = model(); t = _t(pkg, m); L = m.config.dec_layers
    clips = [pkg.synth.synth_audio(s, seed=910 + i) for i, s in enumerate((24.0, 9.0, 5.0) if group else (24.0,))]
    make = lambda: (m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], max_positions=256, page_rows=16, pool_pages=48) if group else
                    m.create_stream(t, gain=_gain(clips[0]), endless=True, dec_ring_rows=m.config.dec_window + 64))
    never, off, on, tog = (run(pkg, make(), clips, 6400, mode) for mode in ("never", "off", "on", "toggle"))
    assert np.array_equal(never[2], off[2]) and off[2][20] == off[2][21] == 0 and off[2][PLAIN,].sum() == off[4] * L, (never[2].tolist(), off[2].tolist())
    for a, x, b, y in zip(*never[:2], *off[:2]):
        assert np.array_equal(a, b) and np.array_equal(x, y), "a container with the flag set off differs from one that never had it set"
    assert on[2][20] == on[2][21] == on[4] * L > 0 and on[4] == off[4] and not on[2][PLAIN,].any(), (on[2].tolist(), on[4])      # dec_layers per round, nothing plain
    near(on, off, "on")
    assert 0 < tog[2][20] == tog[2][21] < on[2][20] and tog[3][20] == tog[3][21] == 0 and tog[3][PLAIN,].sum() == tog[4] * L > 0, (tog[2].tolist(), tog[3].tolist())
    near(tog, off, "off -> on -> off")


@pytest.mark.parametrize("heads", [4, 8])
def test_endless_stream_past_its_wrap(env, heads):
    pkg, model = env; m = model(heads); t = _t(pkg, m); L = m.config.dec_layers; rows = m.config.dec_window + 64
    x = [np.tile(pkg.synth.synth_audio(40.0, seed=4242), 34)[:TICK * 8299 + 40].copy()]
    off = run(pkg, m.create_stream(t, gain=0.37, max_positions=16384), x, 8250 * TICK, "never")
    on = run(pkg, m.create_stream(t, gain=0.37, endless=True, dec_ring_rows=rows), x, 8250 * TICK, "on")
    # every step of the run, the ~90 behind the wrap at position 8256 among them, launched the pair once per layer and neither the flat ([3]) nor the ring form ([13])
    assert len(on[0][0]) == on[4] >= 8300 and on[2][20] == on[2][21] == on[4] * L and not on[2][PLAIN,].any(), (on[2].tolist(), on[4])
    near(on, off, f"{heads} heads, past the wrap")
