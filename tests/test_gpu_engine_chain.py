"""The decode engine's q|k|v -> attention -> wo -> h1 chain (vox_engine.hip) against the per-operator launches, on the full-size synthetic decoder (the engine exists
only for that geometry): ONE engine launch per case on a synthetic cache (N(0, 1) K / V rows written through KVCache::update, as in the position-700 test), at the
positions where the attention changes path: 0 and 1 (no old key / one), 95, 96, 97 and 191, 192, 193 (the register-key boundaries of the two 96-key passes) and 400
(the 192-key round loop).  Two sums of the chain have a fixed order that is the engine's own: the twelve key groups' attention partials (summed once per CU by the
wave that arrives last at the attention's second barrier) and wo's 32 partial planes (eight per lane group, then the four groups).

Bound: the parent's worst case over these nine positions, measured with this file against the parent's library, was 3.63e-6 of the largest |logit| (position 97;
3.46e-6 for the step over the written K / V rows, position 400; this synthetic model's largest |logit| is about 5, which is why the figure is above the 1.5e-6 of the
engine harness's model).  The test allows twice that, PARENT_WORST * 2 = 7.26e-6 -- the margin is for the changed f32 order of the two sums.  The new build measured
3.47e-6 (position 97) and 3.44e-6 (position 192).

The K / V rows a launch writes cannot be read back through the API, so they are checked by what they do: a SECOND step, on the per-operator path in both cases, runs
once on the cache whose row P the engine wrote and once on the cache whose row P the per-operator path wrote; its logits depend on the two caches' rows P only, and
must agree to the same bound (tools/micro/engine_bench compares the rows themselves).  Two runs of the same launch give bit-identical logits, and a short clip decoded
with the argmax folded into the launch (engine flags 65536, the default) gives the tokens of the two-launch form (VOX_ENGINE_ARGMAX_IN=0)."""
import os

import numpy as np
import pytest

from model_fixtures import attn_launches, cache_dir, launches_since

pytestmark = pytest.mark.gpu
PARENT_WORST = 3.63e-6
BOUND = 2 * PARENT_WORST
POSITIONS = [0, 1, 95, 96, 97, 191, 192, 193, 400]
L, KV, HD, D = 26, 8, 128, 3072


@pytest.fixture(scope="module")
def full(pkg):
    S = pkg.synth
    path = os.path.join(cache_dir(), "full_q4_seed42.gguf")
    if not os.path.exists(path):
        S.write_synthetic_gguf(path + f".tmp{os.getpid()}", S.ModelDims(), seed=42); os.replace(path + f".tmp{os.getpid()}", path)
    ctx = pkg.Context(0)
    m = pkg.Q4ModelLoader.from_file(path).load(ctx)
    yield m, pkg.TimeEmbedding(D).embed(6.0)
    m.close(); ctx.close()


def _filled(dec, P):
    c = dec.create_cache_preallocated(512)
    if P > 0:
        for l in range(L):
            rng = np.random.default_rng([2026, l])
            k = rng.standard_normal((KV, P, HD)).astype(np.float32); v = rng.standard_normal((KV, P, HD)).astype(np.float32)
            c.update(l, 0, k, v)
    assert c.seq_len() == P
    return c


@pytest.mark.parametrize("P", POSITIONS)
def test_engine_chain_one_launch_vs_per_operator_path(pkg, full, P):
    m, t = full
    if not m.set_decode_engine(True):
        pytest.skip("decode engine not available on this device (needs 256 CUs)")
    dec = m.decoder()
    x1 = (0.3 * np.random.default_rng([77, P]).standard_normal((1, 1, D))).astype(np.float32)
    x2 = (0.3 * np.random.default_rng([78, P]).standard_normal((1, 1, D))).astype(np.float32)
    ce = _filled(dec, P); co = _filled(dec, P)
    try:
        before = attn_launches(pkg)
        le = dec.lm_head(dec.forward_hidden_with_cache(x1, t, ce))[0, 0]          # the logits of the launch itself
        assert launches_since(pkg, before) == {"engine": 1}
        ce.truncate(P)
        le2 = dec.lm_head(dec.forward_hidden_with_cache(x1, t, ce))[0, 0]         # the same launch again (row P rewritten)
        assert not m.set_decode_engine(False)
        lo = dec.lm_head(dec.forward_hidden_with_cache(x1, t, co))[0, 0]
        assert ce.seq_len() == P + 1 and co.seq_len() == P + 1
        s_e = dec.lm_head(dec.forward_hidden_with_cache(x2, t, ce))[0, 0]         # second step, per-operator path: row P as the engine wrote it ...
        s_o = dec.lm_head(dec.forward_hidden_with_cache(x2, t, co))[0, 0]         # ... and as the per-operator path wrote it
    finally:
        m.set_decode_engine(True); ce.close(); co.close()
    top = float(np.abs(lo).max()); err = float(np.abs(le - lo).max()) / top
    top2 = float(np.abs(s_o).max()); err_kv = float(np.abs(s_e - s_o).max()) / top2
    print(f"engine chain, position {P}: logits {err:.3e} of the largest ({top:.2f}); next step over the written K / V rows {err_kv:.3e}; "
          f"run-to-run {'bit-identical' if np.array_equal(le, le2) else 'DIFFERENT'}; argmax {int(le.argmax())} / {int(lo.argmax())}")
    assert np.array_equal(le, le2)
    assert err <= BOUND
    assert err_kv <= BOUND
    assert int(le.argmax()) == int(lo.argmax())


def test_engine_chain_argmax_in_launch_gives_the_two_launch_tokens(pkg, full, monkeypatch):
    m, t = full
    if not m.set_decode_engine(True):
        pytest.skip("decode engine not available on this device (needs 256 CUs)")
    x = pkg.synth.synth_audio(2.0, seed=97)
    ids = m.transcribe_audio(x, t)                        # flags 65536: every launch forms its own input from the previous launch's argmax partials
    assert len(ids) >= 3
    monkeypatch.setenv("VOX_ENGINE_ARGMAX_IN", "0")
    two = m.transcribe_audio(x, t)                        # engine launch + argmax / embedding launch per step
    monkeypatch.delenv("VOX_ENGINE_ARGMAX_IN")
    print(f"engine chain: {len(ids)} ids, argmax in the launch == two-launch form: {np.array_equal(ids, two)}")
    assert np.array_equal(ids, two)
