"""Worker of tests/test_gpu_stream_burst.py: an endless burst stream across the wrap of its decoder ring, through pytest in a process of its own (past the wrap the
session launches the ring decode attention; the launch counts of vox_debug_attn_launches are per process and the suite's other tests hold that slot to 0).

A burst stream (B = 16) is fed up to 3 positions in front of its wrap in calls of 1000 ticks -- the bursts cut at every growth of the decoder cache on the way -- and
snapshotted there.  A plain endless stream and the burst stream are both restored from that blob and pushed the same 22 ticks in one call: the burst stream runs them as
3 + 16 + 3 (no burst spans the wrap, where the encoder's RoPE source switches; 16 + 6 would be two bursts), and its ids are the plain stream's by stream_helpers._held."""
import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _held, _stop, _t

TOL = 2e-4
TICK = 2560
B = 16


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    yield m
    m.close()


def _n_for(pkg, positions):
    """The fewest samples after which `positions` decoder positions are determined (an unfinished 16 kHz stream)."""
    n = max(0, (positions - 38) * TICK)
    while pkg.stream_schedule(n)[0] < positions:
        n += 1
    assert pkg.stream_schedule(n)[0] == positions
    return n


def _bi(st):
    i = st.burst_info()
    return i["bursts"], i["burst_ticks"], i["single_ticks"]


def test_an_endless_burst_stream_is_cut_at_its_wrap(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m)
    ring = (m.config.dec_window + 1 + 63 + 63) // 64 * 64      # the smallest decoder ring this window takes: the default
    base = pkg.synth.synth_audio(40.0, seed=4242); gain = _gain(base)
    n0 = _n_for(pkg, ring - 3); n1 = _n_for(pkg, ring + 19)      # 22 ticks across the wrap: 3 before it, 19 from it on
    x = np.tile(base, n1 // len(base) + 1)[:n1].copy()
    se = m.create_stream(t, gain=gain, endless=True, dec_ring_rows=ring, burst=B)
    sp = m.create_stream(t, gain=gain, endless=True, dec_ring_rows=ring)
    try:
        for a in range(0, n0, 1000 * TICK):
            se.push(x[a:min(n0, a + 1000 * TICK)])
        info = se.burst_info()
        assert se.info()["positions"] == ring - 3 and info["bursts"] > 300 and info["burst_ticks"] + info["single_ticks"] == ring - 3 - 37
        blob = se.snapshot()
        sp.restore(blob); sp.tap_arm(32)
        rids = sp.push(x[n0:]); rlg = sp.tap_fetch()
        assert len(rids) == 22 and sp.info()["positions"] == ring + 19
        se.restore(blob)
        assert _bi(se) == (0, 0, 0)
        ids = se.push(x[n0:])
        assert _bi(se) == (3, 22, 0), _bi(se)      # 3 + 16 + 3: no burst spans the wrap (16 + 6 would be two bursts)
        assert se.info()["positions"] == ring + 19
    finally:
        se.close(); sp.close()
    stop = _stop(rlg, TOL)
    print(f"across the wrap at {ring}: {int((ids == rids).sum())} of 22 ids equal, the reference's first near-tie at {stop}")
    _held(ids, rids, rlg, "endless burst stream across its wrap", TOL)
