"""The fused tick operators in a live session (set_tick_fused) on the tiny model: a fused stream against a plain stream on the same clip.  Ids: the plain stream's by the
group files' rule (stream_helpers._held) at 2e-4; the tapped logits rows up to the first differing id within 2e-4 of the row's largest logit.  Two cuts of the clip
(one behind a reset, which the flag survives) give two fused streams equal bits.  Launches: flag on, the four-row operator runs 4 x enc_layers times per tick and the
one-row GEMV that many times less than in the plain stream (the adapter's and the decode step's are left); flag off, the counts of a stream that never had the flag."""
import numpy as np
import pytest

from model_fixtures import check_greedy_ids, gemm_launches, gemm_launches_since, tiny_gguf
from stream_helpers import _gain, _held, _pieces, _t

pytestmark = pytest.mark.gpu
TOL, TICK = 2e-4, 2560


@pytest.fixture(scope="module")
def env(pkg):
    ctx = pkg.Context(0); m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    yield pkg, m, pkg.synth.synth_audio(24.0, seed=910)
    m.close(); ctx.close()


def run(pkg, m, x, step, mode, reset_first=False):          # -> ids, tapped logits, launches of the four-row operator, of the one-row GEMV, ticks
    st = m.create_stream(_t(pkg, m), gain=_gain(x), tick_fused=mode == "on")
    try:
        if mode == "off":
            st.set_tick_fused(False)
        if reset_first:
            st.push(x[:3 * TICK]); st.reset()
        assert st.tick_fused() == (mode == "on")
        st.tap_arm(len(x) // TICK + 64)
        r0, g0, k0 = pkg.rows4_launches(), gemm_launches(pkg), st.burst_info()["single_ticks"]
        ids = [i for a, b in _pieces(len(x), step) for i in st.push(x[a:b])] + list(st.finish())
        gemv = sum(v for k, v in gemm_launches_since(pkg, g0).items() if k.startswith("gemv_r"))
        return np.array(ids, np.int32), st.tap_fetch(), pkg.rows4_launches() - r0, gemv, st.burst_info()["single_ticks"] - k0
    finally:
        st.close()


def test_fused_stream_against_plain(env):
    pkg, m, x = env; per_tick = 4 * m.config.enc_layers
    never, off, on, cut = (run(pkg, m, x, step, mode, rst) for step, mode, rst in ((6400, "never", False), (6400, "off", False), (6400, "on", False), (3 * TICK + 17, "on", True)))
    assert never[2] == off[2] == 0 and never[3:] == off[3:] and np.array_equal(never[0], off[0]) and np.array_equal(never[1], off[1]), "flag off differs from a stream that never had it"
    assert on[4] == off[4] > 0 and on[2] == per_tick * on[4] and on[3] == off[3] - per_tick * on[4], (on[2:], off[2:])
    _held(on[0], off[0], off[1], "fused tick", TOL)
    first = check_greedy_ids(on[0], off[0], off[1], TOL)
    d = (np.abs(on[1][:first] - off[1][:first]).max(axis=1) / np.abs(off[1][:first]).max(axis=1)).max()
    assert d <= TOL, f"{first} of {len(off[0])} ids equal, logits within {d:.1e} of their row's largest"
    assert cut[2] == per_tick * cut[4] and np.array_equal(on[0], cut[0]) and np.array_equal(on[1], cut[1]), "a fused stream's bits depend on how the clip was cut"
