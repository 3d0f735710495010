"""Worker of tests/test_gpu_stream_group_enc_kv.py (a process of its own: one kind below runs a bf16 K/V pool, whose decode attention counts in
vox_debug_attn_launches [16] .. [19], which other tests of the suite hold to 0 in theirs).  Not collected by the suite (no test_ prefix).

Stream groups with a bf16 ENCODER ring (vox_stream_group_create_enc_kv, VOX_KV_BF16; DESIGN.md section 8, "A bf16 encoder ring") end to end on the tiny model: three
members (8 s, 5 s, 3 s) fed 160 ms per call, as a slab, a paged, an endless paged, a bf16-pool and a burst group.

Against the f32-ring group of the same kind and calls, the ids follow the group files' rule (stream_helpers._held) and the logits stay within 4x the gap MEASURED on
an MI355X -- the largest |delta logit| / max(1, max |logit|) over the rows up to each member's first differing id (profiles/stream_group_enc_kv_bf16.txt):

    slab, paged, endless 5.848356e-04      bf16 pool 6.221732e-04      burst (B = 4) 5.833125e-04      (no id differs over the 58 + 40 + 27 ids of the three members)

The reference of that bound is always the f32-ring group, never the bf16 group's own output.  On the bf16 group alone, bit for bit: one call against the 160 ms calls
(member 0 fed alone, so that every round has one member in both runs: the row count of a round selects its GEMM kernels), a peek in the middle,
snapshot -> reset -> restore of member 1.  info()'s bytes drop by exactly half the f32 ring; and the new creator with VOX_KV_F32 is the group of vox_stream_group_create_t_embeds, bit for bit and launch for launch."""
import ctypes as C

import numpy as np
import pytest

from model_fixtures import gemm_launches, tiny_gguf
from stream_helpers import _gain, _held, _t

pytestmark = pytest.mark.gpu
PAGED = dict(page_rows=16, pool_pages=48)
KINDS = {"slab": dict(max_positions=256), "paged": dict(max_positions=256, **PAGED), "endless": dict(endless=True, **PAGED),
         "bf16pool": dict(max_positions=256, kv_dtype="bf16", **PAGED), "burst": dict(max_positions=256, burst=4)}
MEASURED = 6.221732e-04      # on an MI355X: the largest gap over the five kinds (the docstring lists each)
TOL = 4 * MEASURED
TICK = 2560         # 160 ms
CAP = 832           # enc_capacity_rows of every group here: the burst group's default, legal for all (the capacity changes addresses only)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def model(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf(seed=7)[0]).load(ctx)
    yield m
    m.close()


def _counts(pkg):
    a = (C.c_uint64 * 20)()
    assert pkg.lib().vox_debug_attn_launches(a, 20) == 0
    return [int(x) for x in a] + sorted(gemm_launches(pkg).items())


def run(pkg, m, kind, enc_kv, cut=TICK, peek_at=None, suspend_at=None, fed=(0, 1, 2)):
    """The members `fed` of a group of three of `kind` with the ring dtype enc_kv (None: vox_stream_group_create_t_embeds), `cut` samples per call -> ids, logits rows, bytes"""
    clips = [pkg.synth.synth_audio(s, seed=930 + i) for i, s in enumerate((8.0, 5.0, 3.0))]; gains = [_gain(x) for x in clips]
    g = m.create_stream_group(None, 3, gains=gains, t_embeds=np.tile(_t(pkg, m), (3, 1)), enc_capacity_rows=CAP, **KINDS[kind], **({"enc_kv_dtype": enc_kv} if enc_kv else {}))
    try:
        assert g.enc_kv() == (enc_kv or "f32")
        inf = g.info(0); ids = [[] for _ in clips]; taps = [[] for _ in clips]
        for k in range(3):
            g.tap_arm(k, 256)
        for c in range(-(-max(len(x) for x in clips) // cut)):
            feeds = {k: x[c * cut:(c + 1) * cut] for k, x in enumerate(clips) if k in fed and c * cut < len(x)}
            for k, v in g.advance(feeds, finish=[k for k in feeds if (c + 1) * cut >= len(clips[k])]).items():
                ids[k].extend(v)
            if c == peek_at:
                assert all(len(v) for v in g.peek([0, 1]).values())
            if c == suspend_at:
                blob = g.snapshot(1); taps[1].append(g.tap_fetch(1))
                g.reset(1, gain=0.5); g.restore(1, blob); g.tap_arm(1, 256)
        for k in range(3):
            taps[k].append(g.tap_fetch(k))
    finally:
        g.close()
    return dict(ids=[np.array(v, np.int32) for v in ids], taps=[np.concatenate(t) for t in taps], bytes=inf["bytes"])


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a["ids"], b["ids"])) and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a["taps"], b["taps"]))


_RUNS = {}      # (kind, dtype) -> the plain run of 160 ms calls: computed once, read-only


def plain(pkg, m, kind, enc_kv):
    if (kind, enc_kv) not in _RUNS:
        _RUNS[(kind, enc_kv)] = run(pkg, m, kind, enc_kv)
    return _RUNS[(kind, enc_kv)]


@pytest.mark.parametrize("kind", KINDS)
def test_bf16_ring_group_against_the_f32_ring_group(pkg, model, kind):
    ref, got = plain(pkg, model, kind, "f32"), plain(pkg, model, kind, "bf16")
    gap = 0.0; firsts = []
    for a, la, b, lb in zip(got["ids"], got["taps"], ref["ids"], ref["taps"]):
        assert len(a) == len(b) == la.shape[0] == lb.shape[0] > 0
        d = np.flatnonzero(a != b); n = int(d[0]) + 1 if len(d) else len(a); firsts.append(int(d[0]) if len(d) else None)
        gap = max(gap, float(np.abs(la[:n].astype(np.float64) - lb[:n]).max() / max(1.0, float(np.abs(lb[:n]).max()))))
    print(f"MEASURED {kind} {gap:.6e} first differing ids {firsts} of {[len(v) for v in ref['ids']]}")
    assert gap <= TOL, (gap, TOL)
    assert not same(got, ref)      # (the ring did change what is computed)
    for k in range(3):
        _held(got["ids"][k], ref["ids"][k], ref["taps"][k], f"{kind} member {k}", TOL)
    c = model.config      # the rings halve, nothing else changes: a member's share of the group's bytes drops by half its f32 rings, K and V
    assert ref["bytes"] - got["bytes"] == c.enc_layers * c.enc_heads * CAP * c.enc_head_dim * 4, (ref["bytes"], got["bytes"])


@pytest.mark.parametrize("kind", ("slab", "paged"))
def test_ids_and_logits_do_not_depend_on_the_cut(pkg, model, kind):
    a, b = run(pkg, model, kind, "bf16", cut=1 << 20, fed=(0,)), run(pkg, model, kind, "bf16", fed=(0,))
    assert len(a["ids"][0]) >= 40 and same(a, b)


@pytest.mark.parametrize("kind", ("slab", "burst"))
def test_a_peek_leaves_every_later_id_and_logit(pkg, model, kind):
    assert same(run(pkg, model, kind, "bf16", peek_at=9), plain(pkg, model, kind, "bf16"))


@pytest.mark.parametrize("kind", ("slab", "endless"))
def test_snapshot_reset_restore_continues_bit_for_bit(pkg, model, kind):
    assert same(run(pkg, model, kind, "bf16", suspend_at=12), plain(pkg, model, kind, "bf16"))


def test_f32_by_the_new_creator_is_the_existing_group(pkg, model):
    c0 = _counts(pkg); a = run(pkg, model, "paged", None); c1 = _counts(pkg); b = run(pkg, model, "paged", "f32"); c2 = _counts(pkg)
    assert same(a, b) and a["bytes"] == b["bytes"]
    d = lambda x, y: [(q[0], q[1] - p[1]) if isinstance(p, tuple) else q - p for p, q in zip(x, y)]
    assert d(c0, c1) == d(c1, c2) and any(v for v in d(c0, c1) if not isinstance(v, tuple))
