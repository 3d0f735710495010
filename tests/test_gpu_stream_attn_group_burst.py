"""The RAGGED burst form of the live sessions' encoder ring attention (stream_attn_burst_kernel<HD, StreamAttnGroupParams> behind launch_stream_attn_group_burst,
csrc/vox_kernels.hip: a burst group's round -- slot z has its own 4 b_z rows, packed behind the slots before it) through vox_debug_stream_attn_group_burst.

The reference is the tick kernel itself: ONE ragged launch against the chain of vox_debug_stream_attn calls with rows = 4 -- call t serves the slots with more than
t ticks, enc_pos moving by 4, the rings fed back.  The comparison is equality of every word of out and of both rings (the tick kernel's own values are held against
float64 by tests/test_gpu_stream_attn.py).  Both head sizes; rows_per_slot (64, 12, 4), (4, 64), (8, 8) and a single slot (20); `order` a non-identity subset of 4
members, the members not served keep every ring word; one member below its window (position 100), one past it (5000), one whose burst rows wrap the ring
(3 cap - 2), in layer 1 of 2; cap = window + 64 + 1, the smallest legal value; the flat RoPE table and a RoPE ring of 64 rows per member (far positions).  Refusals
(rows of 0, 6 and 68, cap = window + max rows, a RoPE ring shorter than the rows) launch nothing; every passing call moves the burst launch counter by one and no
slot of vox_debug_attn_launches."""
from importlib import import_module

import numpy as np
import pytest

from model_fixtures import attn_launches, launches_since

pytestmark = pytest.mark.gpu
THETA = 1e6
WINDOW = 750
CAP = WINDOW + 64 + 1
GEOS = ((64, 3), (128, 2))      # (head_dim, n_heads)
POS = (100, 1234, 3 * CAP - 2, 5000)      # member 0 below its window, 1 never served, 2 wraps the ring inside the burst, 3 past its window
FAR = (70000, 1234, 3 * CAP - 2 + 815 * 1200, (1 << 24) - 70)      # the ring-per-member form: positions the flat table does not hold
SLOTS = {(64, 12, 4): (3, 0, 2), (4, 64): (0, 2), (8, 8): (3, 2), (20,): (2,)}      # rows_per_slot -> order
DONE = set()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


_INPUTS = {}


def _inputs(geo):
    """(qkv rows for 80 = 64 + 12 + 4 rows, kring, vring): seeded, built once per head size, read-only."""
    if geo not in _INPUTS:
        hd, H = geo; rng = np.random.default_rng(1000 + hd)
        qkv = rng.standard_normal((80, 3 * H * hd)).astype(np.float32)
        kring = rng.standard_normal((len(POS), 2, H, CAP, hd)).astype(np.float32); vring = rng.standard_normal(kring.shape).astype(np.float32)
        for a in (qkv, kring, vring):
            a.setflags(write=False)
        _INPUTS[geo] = (qkv, kring, vring)
    return _INPUTS[geo]


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _ragged(pkg, gg, ctx, qkv, kring, vring, order, pos, rps, **kw):
    before, b0 = attn_launches(pkg), gg.stream_attn_burst_launches()
    got = gg.stream_attn_group_burst(ctx, qkv, kring, vring, order, pos, rps, WINDOW, THETA, layer=1, **kw)
    assert gg.stream_attn_burst_launches() - b0 == 1 and launches_since(pkg, before) == {}, (gg.stream_attn_burst_launches() - b0, launches_since(pkg, before))
    return got


def _chain(pkg, gg, ctx, qkv, kring, vring, order, pos, rps, **kw):
    """The chain of tick launches: call t serves the slots with more than t ticks (4 rows each at enc_pos + 4 t), the rings fed back."""
    row0 = np.concatenate([[0], np.cumsum(rps)[:-1]]); out = np.full((int(sum(rps)), qkv.shape[1] // 3), np.nan, np.float32)
    ck, cv = kring, vring; calls = 0
    before = attn_launches(pkg)
    for t in range(max(rps) // 4):
        zs = [z for z in range(len(rps)) if rps[z] > 4 * t]
        rows = np.concatenate([np.arange(row0[z] + 4 * t, row0[z] + 4 * t + 4) for z in zs])
        o, ck, cv = gg.stream_attn(ctx, qkv[rows], ck, cv, [order[z] for z in zs], tuple(p + 4 * t for p in pos), 4, WINDOW, THETA, layer=1, **kw)
        out[rows] = o; calls += 1
    assert launches_since(pkg, before) == {"stream_ring": calls}
    return out, ck, cv


CASES = [(g, r, "flat") for g in GEOS for r in SLOTS] + [(g, r, "ring64pm") for g in GEOS for r in ((64, 12, 4), (4, 64))]      # the RoPE-ring form: the shapes with a 64-row slot


@pytest.mark.parametrize("geo,rps,form", CASES, ids=[f"hd{g[0]}-{'-'.join(map(str, r))}-{f}" for g, r, f in CASES])
def test_one_ragged_launch_is_the_chain_of_ticks_bit_for_bit(pkg, gg, ctx, geo, rps, form):
    qkv_all, kring, vring = _inputs(geo)
    order = SLOTS[rps]; n_rows = sum(rps); qkv = qkv_all[:n_rows]
    pos, kw = (POS, {}) if form == "flat" else (FAR, dict(rope_rows=64, rope_per_member=True))
    out, k1, v1 = _ragged(pkg, gg, ctx, qkv, kring, vring, order, pos, rps, **kw)
    assert out.shape == (n_rows, geo[0] * geo[1]) and np.isfinite(out).all()
    cout, ck, cv = _chain(pkg, gg, ctx, qkv, kring, vring, order, pos, rps, **kw)
    for name, a, w in (("out", out, cout), ("kring", k1, ck), ("vring", v1, cv)):
        d = np.argwhere(_words(a) != _words(w))
        assert not len(d), f"{len(d)} words of {name} differ from the chain of ticks; first: {d[:4].tolist()}"
    served = set(order)
    for mb in range(len(POS)):      # a member not in the round keeps every ring word; a served one received its rows, in layer 1 alone
        for ring, was in ((k1, kring), (v1, vring)):
            if mb not in served:
                assert np.array_equal(_words(ring[mb]), _words(was[mb])), f"member {mb} is not served and its ring changed"
            else:
                assert np.array_equal(_words(ring[mb, 0]), _words(was[mb, 0])) and not np.array_equal(_words(ring[mb, 1]), _words(was[mb, 1]))
    z = len(rps) - 1; mb = order[z]; rows = (pos[mb] + np.arange(rps[z])) % CAP      # the appended V rows of the last slot are its input rows
    QD = geo[0] * geo[1]; r0 = n_rows - rps[z]
    assert np.array_equal(_words(v1[mb, 1][:, rows].transpose(1, 0, 2).reshape(rps[z], QD)), _words(qkv[r0:, 2 * QD:]))
    DONE.add((geo[0], rps, form))


def test_refusals_launch_nothing(pkg, gg, ctx):
    geo = GEOS[0]; qkv_all, kring, vring = _inputs(geo); W = qkv_all.shape[1]

    def refused(word, rps, order=(3, 0), kring=kring, **kw):
        before, b0 = attn_launches(pkg), gg.stream_attn_burst_launches()
        with pytest.raises(pkg.VoxError) as e:
            gg.stream_attn_group_burst(ctx, np.zeros((sum(max(r, 0) for r in rps), W), np.float32), kring, kring, order, POS, rps, WINDOW, THETA, **kw)
        assert e.value.code == 1 and word in str(e.value), e.value
        assert launches_since(pkg, before) == {} and gg.stream_attn_burst_launches() == b0

    refused("rows_per_slot[1] = 0", (8, 0))
    refused("rows_per_slot[1] = 6", (8, 6))
    refused("rows 68", (68, 4))
    refused(f"cap {WINDOW + 64}", (64, 4), kring=np.zeros((4, 1, 3, WINDOW + 64, 64), np.float32))      # cap == window + max rows
    refused("rope_rows 8", (12, 4), rope_rows=8, rope_per_member=True)                                   # a RoPE ring shorter than the 12 rows
    refused("served by one slot", (8, 8), order=(2, 2))
    L = pkg.lib()
    assert L.vox_debug_stream_attn_group_burst(ctx.h, None, None, None, None, None, None) != 0 and b"null argument" in L.vox_last_error()
    _ragged(pkg, gg, ctx, qkv_all[:12], kring, vring, (3, 0), POS, (8, 4))      # a valid launch then passes
    DONE.add("refusals")


def test_every_case_ran():
    want = {(g[0], r, f) for g, r, f in CASES} | {"refusals"}
    assert want <= DONE, sorted(map(str, want - DONE))
