"""Worker of tests/test_gpu_stream_group_burst.py: its tests run through pytest in a process of their own (worker_tests.run_worker) -- an endless group launches the
paged attention on ring page tables and a bf16 group the bf16 decode forms, whose slots of vox_debug_attn_launches other tests of the suite hold to 0 in their own
process.  Not collected by the suite (no test_ prefix).

Burst groups (vox_stream_group_create_burst, DESIGN.md section 8 "Bursts in stream groups") of every kind under ONE sequence of calls with backlogs -- 20, 5 and 1
ticks due in the first call, then a second of audio (6 or 7 ticks) per member and call:
 * the slab burst group, the paged one and the endless one agree bit for bit: ids, tapped logits, score and alternatives records, burst_info; the paged and the
   endless one also in pool() after every call.  Every round has the same rows in the three, so the same kernels run; the decoder caches differ in addresses only;
 * the bf16 pool is held by the rule of tests/stream_group_kv_worker.py against the f32 paged BURST group: the largest |delta logit| / max(1, max |logit|) up to
   each member's first differing id within TOL = 4 x the value measured there for this model (3.2278e-04), and the ids by stream_helpers._held at that TOL."""
import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _gain, _held, _t

pytestmark = pytest.mark.gpu
TICK = 2560
B = 16
TOL_BF16 = 4 * 3.2278e-04      # tests/stream_group_kv_worker.py: MEASURED["head"], the factor and the reasons given there
KINDS = {"slab": dict(max_positions=256), "paged": dict(max_positions=256, page_rows=16, pool_pages=32), "endless": dict(page_rows=16, pool_pages=32, endless=True),
         "bf16": dict(max_positions=256, page_rows=16, pool_pages=32, kv_dtype="bf16")}


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
    n = max(0, (positions - 38) * TICK)
    while pkg.stream_schedule(n)[0] < positions:
        n += 1
    return n


def _same(a, b, what):
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), f"{what} differ"


_RUNS = {}


def _run(pkg, m, kind):
    """The three members (24 s, 9 s, 5 s: the clips of tests/stream_group_kv_worker.py) on a burst group of `kind`: computed once per kind, read-only."""
    if kind in _RUNS:
        return _RUNS[kind]
    t = _t(pkg, m); clips = [pkg.synth.synth_audio(s, seed=910 + i) for i, s in enumerate((24.0, 9.0, 5.0))]
    g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], burst=B, **KINDS[kind])
    out = {"ids": [[] for _ in range(3)], "pools": []}
    try:
        for k in range(3):
            g.tap_arm(k, 256)
        g.set_scores(0, True); g.set_alternatives(1, 3)
        at = [_n_for(pkg, 37 + d) for d in (20, 5, 1)]
        feeds = {k: clips[k][:at[k]] for k in range(3)}; fin = []
        while feeds:
            for k, v in g.advance(feeds, finish=fin).items():
                out["ids"][k].extend(v)
            if kind != "slab":
                p = dict(g.pool()); p.pop("kv_dtype", None); out["pools"].append((p, [g.pages(k) for k in range(3)]))
            feeds = {}; fin = []
            for k in range(3):
                if at[k] < len(clips[k]):
                    feeds[k] = clips[k][at[k]:at[k] + 16000]; at[k] += 16000
                    if at[k] >= len(clips[k]):
                        fin.append(k)
        out["ids"] = [np.array(v, np.int32) for v in out["ids"]]
        out["taps"] = [g.tap_fetch(k) for k in range(3)]
        out["scores"] = g.scores(0).copy(); out["alts"] = g.alternatives(1).copy()
        out["info"] = g.burst_info(); out["positions"] = [g.info(k)["positions"] for k in range(3)]
    finally:
        g.close()
    _RUNS[kind] = out
    return out


def test_slab_paged_and_endless_burst_groups_agree_bit_for_bit(pkg, ctx, tiny):
    s, p, e = (_run(pkg, tiny, k) for k in ("slab", "paged", "endless"))
    print(f"burst_info {p['info']}, positions {p['positions']}")
    assert p["info"]["burst"] == B and p["info"]["burst_rounds"] >= 20 and p["info"]["burst_member_ticks"] >= 150 and max(p["positions"]) < 256
    for name, other in (("slab", s), ("endless", e)):
        assert other["info"] == p["info"] and other["positions"] == p["positions"]
        for k in range(3):
            _same(other["ids"][k], p["ids"][k], f"{name} / paged: member {k} ids"); _same(other["taps"][k], p["taps"][k], f"{name} / paged: member {k} logits")
            assert len(p["ids"][k]) == p["taps"][k].shape[0] >= 30
        _same(other["scores"], p["scores"], f"{name} / paged: scores"); _same(other["alts"], p["alts"], f"{name} / paged: alternatives")
    assert e["pools"] == p["pools"] and len(p["pools"]) >= 20


def test_bf16_burst_group_against_the_f32_paged_burst_group(pkg, ctx, tiny):
    ref, got = _run(pkg, tiny, "paged"), _run(pkg, tiny, "bf16")
    assert got["info"] == ref["info"] and got["pools"] == ref["pools"]      # the schedule and the allocator do not know the dtype
    worst = 0.0
    for k in range(3):
        a, la, b, lb = got["ids"][k], got["taps"][k], ref["ids"][k], ref["taps"][k]
        assert len(a) == len(b) == la.shape[0] == lb.shape[0] > 0
        diff = np.flatnonzero(a != b); n = int(diff[0]) + 1 if len(diff) else len(a)      # the row behind the first differing id saw the same ids: it still compares
        worst = max(worst, float(np.abs(la[:n].astype(np.float64) - lb[:n]).max() / max(1.0, float(np.abs(lb[:n]).max()))))
    print(f"bf16 burst group: largest logit gap {worst:.6e} (bar {TOL_BF16:.6e})")
    assert worst <= TOL_BF16
    assert any(not np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got["taps"], ref["taps"]))      # (the rows did move)
    for k in range(3):
        _held(got["ids"][k], ref["ids"][k], ref["taps"][k], f"bf16 member {k}", TOL_BF16)
