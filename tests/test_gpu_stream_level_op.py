"""The live sessions' level kernel on its own (vox_debug_stream_level: ONE launch of stream_level_kernel on hand-made sessions, no model), against the float64 reference
of tests/level_ref.py on the same f32 samples: peak bit for bit, mean_square within the derived bound (2^-19 relative; + 2^-149 where squares underflow), exactly 0 on
zeros.  Rings of 65 536 random samples with a stretch of exact zeros and a stretch of subnormal-scale values; gains 1, 0.37 and -2; windows inside each stretch, across
the ring's wrap and across index 0; 1, 3 and 16 slots in a permuted order; the burst forms against the chain of single-tick launches, bit for bit."""

import numpy as np
import pytest

import level_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
RING = 65536; LEFT = 97280; P0 = 37; LIST = 64
ZEROS = (20000, 26000); TINY = (30000, 36000)
GAINS = (1.0, 0.37, -2.0)
# STRM_FRAME values and what the window 160 f - LEFT .. + 2560 is: all pad | straddles index 0 | random | exact zeros | subnormal-scale | wraps the ring | random | two
# rings further on (the index is masked, not the pointer advanced)
FRAMES = (592, 600, 650, 736, 800, 1008, 912, 608 + 2 * RING // 160 + 44)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def rings():
    """16 rings: 0.5 N(0, 1) with a loud sample here and there, exact zeros in ZEROS, values of 1e-39 .. 1e-41 (subnormal in f32, their squares 0) in TINY."""
    out = np.zeros((16, RING), F32)
    for i in range(16):
        rng = np.random.default_rng([77, i])
        x = (0.5 * rng.standard_normal(RING)).astype(F32); x[rng.integers(0, RING, 40)] *= F32(9)
        x[ZEROS[0]:ZEROS[1]] = 0
        with np.errstate(under="ignore"):
            x[TINY[0]:TINY[1]] = (rng.standard_normal(TINY[1] - TINY[0]) * 10.0 ** rng.uniform(-41, -39, TINY[1] - TINY[0])).astype(F32)
        out[i] = x
    assert (out[:, TINY[0]:TINY[1]] != 0).mean() > 0.9 and np.abs(out[:, TINY[0]:TINY[1]]).max() < 1.2e-38
    return out


def _launch(pkg, ctx, rings, gains, pos, frame, order, ticks=1, burst_b=None):
    nm = len(rings); out = np.zeros((nm, LIST), dtype=pkg.LEVEL_DTYPE)
    i32 = lambda v: np.ascontiguousarray(v, dtype=np.int32)
    r = np.ascontiguousarray(rings, dtype=F32); g = np.ascontiguousarray(gains, dtype=F32); p = i32(pos); f = i32(frame); o = i32(order); b = None if burst_b is None else i32(burst_b)
    pkg._lib.check(pkg.lib().vox_debug_stream_level(ctx.h, nm, r.ctypes.data, RING, g.ctypes.data, p.ctypes.data, f.ctypes.data, o.ctypes.data, len(o), ticks,
                                               None if b is None else b.ctypes.data, LIST, out.ctypes.data))
    return out


def _ref(ring, gain, frame, t=0):
    """The reference record of the window 160 frame - LEFT + 2560 t of a ring: sample i lives at ring[i mod RING], below 0 it is pad."""
    w0 = 160 * frame - LEFT + R.TICK * t
    idx = np.arange(w0, w0 + R.TICK)
    with np.errstate(under="ignore"):
        v = np.where(idx >= 0, ring[idx % RING] * F32(gain), F32(0)).astype(F32)
    return R.level_of(v)


def _nan_elsewhere(out, written):
    mask = np.ones(out.shape, bool)
    for m, k in written:
        mask[m, k] = False
    assert np.isnan(out["peak"][mask]).all() and np.isnan(out["mean_square"][mask]).all()


@pytest.mark.parametrize("n_slots", [1, 3, 16])
def test_plain_form_against_the_reference(pkg, ctx, rings, n_slots):
    """One launch of n slots over 16 sessions, three times with the windows and gains rotated, so every kind of window meets every gain: each slot's member gets the
    reference's record at index STRM_POS - 37, every other record of every list stays (NaN, NaN)."""
    order = list(np.random.default_rng(n_slots).permutation(16)[:n_slots])
    worst = 0.0
    for rot in range(3):
        gains = [GAINS[(i + rot) % 3] for i in range(16)]; frame = [FRAMES[(i + 3 * rot) % len(FRAMES)] for i in range(16)]; pos = [P0 + (5 * i + rot) % LIST for i in range(16)]
        out = _launch(pkg, ctx, rings, gains, pos, frame, order)
        _nan_elsewhere(out, [(m, pos[m] - P0) for m in order])
        rec = np.array([out[m, pos[m] - P0] for m in order]); ref = [_ref(rings[m], gains[m], frame[m]) for m in order]
        worst = max(worst, R.check(rec, np.array([r[0] for r in ref], F32), np.array([r[1] for r in ref]), f"{n_slots} slots, rotation {rot}"))
        for m, (pk, ms) in zip(order, ref):      # what each kind of window must give, spelled out
            got = out[m, pos[m] - P0]
            if frame[m] == 592:
                assert got["peak"] == 0 and got["mean_square"] == 0      # all pad: record 0's window
            if frame[m] == 736:
                assert got["peak"] == 0 and got["mean_square"] == 0 and pk == 0      # exact zeros
            if frame[m] == 800:
                assert 0 < got["peak"] < 1.2e-38 * 2 and pk > 0      # subnormal-scale: the peak is kept, not flushed
    print(f"{n_slots} slots: largest |mean_square - ref| / bound = {worst:.3f}")


def test_window_edges_one_sample_at_a_time(pkg, ctx):
    """A ring of zeros with ONE sample set: it is seen by exactly the window that holds it -- at both edges of a window, at the ring's last and first sample of a
    wrapping window, and at index 0 of a straddling one; a sample just outside is not."""
    cases = [(650, 0, True), (650, R.TICK - 1, True), (650, -1, False), (650, R.TICK, False), (1008, RING - 64000 - 1, True), (1008, RING - 64000, True), (600, 1280, True), (600, 1279, False)]
    for frame, off, inside in cases:
        w0 = 160 * frame - LEFT; ring = np.zeros((1, RING), F32); ring[0, (w0 + off) % RING] = -0.75
        got = _launch(pkg, ctx, ring, [1.0], [P0 + 1], [frame], [0])[0, 1]
        want = (F32(0.75), F32(0.5625) / F32(R.TICK)) if inside else (F32(0), F32(0))
        assert (got["peak"], got["mean_square"]) == want, (frame, off, got)


@pytest.mark.parametrize("burst", [(2,), (16,), (16, 3, 1)])
def test_burst_forms_equal_the_chain_of_single_tick_launches(pkg, ctx, rings, burst):
    """A burst launch (grid: ticks x slots) writes, for every slot and tick, the bits the single-tick launch writes when STRM_POS has moved by t and STRM_FRAME by 16 t;
    a ragged descriptor's slots stop at their own b.  One slot: the solo burst form (no descriptor); three: a burst round's.  The records are the reference's too."""
    n = len(burst); order = {(2,): [0], (16,): [1], (16, 3, 1): [2, 0, 1]}[burst]; gains = list(GAINS); pos = [P0 + 3, P0 + 20, P0]; frame = [600 - 16, 1008 - 32, 592]      # windows that cross index 0 and the wrap inside the burst
    sub = rings[:3]
    out = _launch(pkg, ctx, sub, gains, pos, frame, order, ticks=burst[0], burst_b=None if n == 1 else burst)
    written = []
    for z, m in enumerate(order):
        for t in range(burst[z]):
            one = _launch(pkg, ctx, sub, gains, [p + t for p in pos], [f + 16 * t for f in frame], [m])
            k = pos[m] - P0 + t; written.append((m, k))
            assert out[m, k].tobytes() == one[m, k].tobytes(), (z, m, t, out[m, k], one[m, k])
            pk, ms = _ref(sub[m], gains[m], frame[m], t)
            R.check(one[m, k:k + 1], np.array([pk], F32), np.array([ms]), f"slot {z} tick {t}")
    _nan_elsewhere(out, written)      # a slot's ticks beyond its b, and the sessions outside the order, wrote nothing
