"""The multi-row decoder forward (decoder_prefill_dev) in every form it can take, on the tiny synthetic models, through the piecewise
forward_hidden_with_cache: the general f32-rows form on both sides of the 17..48-row window, the XF / K-slice-planes form at its first, product and last
row counts and away from position 0, each under every cross-check knob, and the dense f32 model (no layer eligible).

Per case: (1) the hidden states against the CPU oracle, (2) one more single-row forward on the same cache against the oracle -- the only place a wrong or
missing K / V row of the fused RoPE / cache-write finish (or of a skipped kv_store) shows -- and (3) the linear and attention launches of the multi-row call by
kernel form against EXPECT.  EXPECT was recorded from the commit BEFORE the prefill was split into a planner and a runner (profiles/r07_prefill_forms_launches.txt
is that run's output); it is a record of what was launched then, not a restatement of the planner.

Tolerance: TOL of tests/test_gpu_model.py (hidden states max|d| <= 2e-4 * max|ref|)."""
import numpy as np
import pytest

from model_fixtures import attn_launches, gemm_launches, gemm_launches_since, launches_since, rel_err, tiny_f32_pair, tiny_gguf
from test_gpu_model import TOL

pytestmark = pytest.mark.gpu

CASES = {
    # the general form's last row count, served by the <= 16-row skinny kernel: one row more and the layer changes shape
    "m16": (16, 0),
    # the XF form's first row count: two 16-row m-tiles, the second holding ONE row (tile-tail masking of every finishing kernel and of the XF writers)
    "m17": (17, 0),
    # the product's 38-token prefix: three m-tiles, the last with six rows
    "m38": (38, 0),
    # the XF form's last row count: three full m-tiles, the plane buffer's row bound
    "m48": (48, 0),
    # one row past the window: back on the general form, now on the tiled GEMMs
    "m49": (49, 0),
    # 38 rows after a 5-row forward on the same cache: the short-sequence attention (XF tiles out) only runs from position 0, so wo goes through xf_rows + planes,
    # and the RoPE / cache-write finish runs at a non-zero position offset (5 is no multiple of anything the kernels tile by)
    "m38_off5": (38, 5),
}
KNOBS = {"none": None, "no_fused_fin": "VOX_PREFILL_NO_FUSED_FIN", "no_sumk": "VOX_PREFILL_NO_SUMK", "no_norm_xf": "VOX_PREFILL_NO_NORM_XF",
         "no_skinny_mt": "VOX_NO_SKINNY_MT"}

# (case, knob set) -> launches of the multi-row call by kernel form (model_fixtures.GEMM_FORMS and the attention forms), recorded at the parent commit
EXPECT = {
    ('m16', 'none'): {'skinny': 8, 'prefill_small': 2},
    ('m16', 'no_fused_fin'): {'skinny': 8, 'prefill_small': 2},
    ('m16', 'no_sumk'): {'skinny': 8, 'prefill_small': 2},
    ('m16', 'no_norm_xf'): {'skinny': 8, 'prefill_small': 2},
    ('m16', 'no_skinny_mt'): {'skinny': 8, 'prefill_small': 2},
    ('m17', 'none'): {'splitk_finish': 1, 'wide': 8, 'prefill_small': 2},
    ('m17', 'no_fused_fin'): {'skinny_mt2': 4, 'xf_rows': 2, 'splitk_finish': 5, 'wide': 4, 'prefill_small': 2},
    ('m17', 'no_sumk'): {'skinny_mt2': 8, 'xf_rows': 4, 'splitk_finish': 8, 'prefill_small': 2},
    ('m17', 'no_norm_xf'): {'skinny_mt2': 8, 'xf_rows': 8, 'splitk_finish': 8, 'prefill_small': 2},
    ('m17', 'no_skinny_mt'): {'tile_11': 8, 'prefill_small': 2},
    ('m38', 'none'): {'splitk_finish': 1, 'wide': 8, 'prefill_small': 2},
    ('m38', 'no_fused_fin'): {'skinny_mt2': 4, 'xf_rows': 2, 'splitk_finish': 5, 'wide': 4, 'prefill_small': 2},
    ('m38', 'no_sumk'): {'skinny_mt2': 8, 'xf_rows': 4, 'splitk_finish': 8, 'prefill_small': 2},
    ('m38', 'no_norm_xf'): {'skinny_mt2': 8, 'xf_rows': 8, 'splitk_finish': 8, 'prefill_small': 2},
    ('m38', 'no_skinny_mt'): {'tile_11': 8, 'prefill_small': 2},
    ('m48', 'none'): {'splitk_finish': 1, 'wide': 8, 'prefill_small': 2},
    ('m48', 'no_fused_fin'): {'skinny_mt2': 4, 'xf_rows': 2, 'splitk_finish': 5, 'wide': 4, 'prefill_small': 2},
    ('m48', 'no_sumk'): {'skinny_mt2': 8, 'xf_rows': 4, 'splitk_finish': 8, 'prefill_small': 2},
    ('m48', 'no_norm_xf'): {'skinny_mt2': 8, 'xf_rows': 8, 'splitk_finish': 8, 'prefill_small': 2},
    ('m48', 'no_skinny_mt'): {'tile_11': 8, 'prefill_small': 2},
    ('m49', 'none'): {'tile_21_tb': 8, 'prefill_mfma': 2},
    ('m49', 'no_fused_fin'): {'tile_21_tb': 8, 'prefill_mfma': 2},
    ('m49', 'no_sumk'): {'tile_21_tb': 8, 'prefill_mfma': 2},
    ('m49', 'no_norm_xf'): {'tile_21_tb': 8, 'prefill_mfma': 2},
    ('m49', 'no_skinny_mt'): {'tile_21_tb': 8, 'prefill_mfma': 2},
    ('m38_off5', 'none'): {'xf_rows': 2, 'splitk_finish': 1, 'wide': 8, 'prefill_mfma': 2},
    ('m38_off5', 'no_fused_fin'): {'skinny_mt2': 4, 'xf_rows': 4, 'splitk_finish': 5, 'wide': 4, 'prefill_mfma': 2},
    ('m38_off5', 'no_sumk'): {'skinny_mt2': 8, 'xf_rows': 4, 'splitk_finish': 8, 'prefill_mfma': 2},
    ('m38_off5', 'no_norm_xf'): {'skinny_mt2': 8, 'xf_rows': 8, 'splitk_finish': 8, 'prefill_mfma': 2},
    ('m38_off5', 'no_skinny_mt'): {'tile_11': 8, 'prefill_mfma': 2},
    ('m38_f32', 'none'): {'tile_11': 8, 'prefill_small': 2},
}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _t_embed(pkg):
    return pkg.TimeEmbedding(256).embed(6.0)


def _set_t_embed(pkg, m):
    """One single-row forward: a model's first forward with a time embedding also computes the Ada scales (two single-row linears per layer), which would count
    into whichever case happened to run first."""
    dec = m.decoder(); c = dec.create_cache_preallocated(8)
    dec.forward_hidden_with_cache(np.zeros((1, 1, 256), np.float32), _t_embed(pkg), c); c.close()


@pytest.fixture(scope="module")
def tiny(pkg, orc, ctx):
    path, _ = tiny_gguf()
    m = pkg.Q4ModelLoader.from_file(path).load(ctx)
    o = orc.Model(path)
    _set_t_embed(pkg, m)
    yield m, o
    m.close(); o.close()


@pytest.fixture(scope="module")
def tiny_f32(pkg, orc, ctx):
    st, gg, _ = tiny_f32_pair()
    m = pkg.VoxtralModelLoader.from_file(st).load(ctx)
    o = orc.Model(gg)
    _set_t_embed(pkg, m)
    yield m, o
    m.close(); o.close()


@pytest.fixture(scope="module")
def refs():
    return {}      # (model kind, M, off) -> (x, t, oracle rows of the multi-row call, oracle row of the step after it): computed once, shared by the knob sets


def _reference(pkg, refs, kind, o, M, off):
    if (kind, M, off) not in refs:
        x = (0.5 * np.random.default_rng([3, M, off]).standard_normal((off + M + 1, 256))).astype(np.float32)
        t = _t_embed(pkg)
        oc = o.cache(64)
        try:
            if off:
                o.forward_hidden_with_cache(x[:off], t, oc)
            ref = o.forward_hidden_with_cache(x[off:off + M], t, oc)
            ref1 = o.forward_hidden_with_cache(x[off + M:], t, oc)
        finally:
            o.cache_free(oc)
        for a in (x, ref, ref1):
            a.setflags(write=False)
        refs[(kind, M, off)] = (x, t, ref, ref1)
    return refs[(kind, M, off)]


def _check(pkg, refs, kind, pair, M, off, key):
    m, o = pair
    x, t, ref, ref1 = _reference(pkg, refs, kind, o, M, off)
    dec = m.decoder(); c = dec.create_cache_preallocated(64)
    try:
        if off:
            dec.forward_hidden_with_cache(x[None, :off], t, c)
        g0, a0 = gemm_launches(pkg), attn_launches(pkg)
        h = dec.forward_hidden_with_cache(x[None, off:off + M], t, c)[0]
        got = {**gemm_launches_since(pkg, g0), **launches_since(pkg, a0)}
        assert c.seq_len() == off + M
        h1 = dec.forward_hidden_with_cache(x[None, off + M:], t, c)[0]
    finally:
        c.close()
    e, e1 = rel_err(h, ref), rel_err(h1, ref1)
    print(f"PREFILL_FORMS {key!r}: {got!r},      # hidden {e:.2e}, next row {e1:.2e}")
    assert e < TOL, e
    assert e1 < TOL, e1                  # the K / V rows the multi-row call left in the cache
    assert got == EXPECT[key], (got, EXPECT[key])


@pytest.mark.parametrize("knob", list(KNOBS))
@pytest.mark.parametrize("case", list(CASES))
def test_prefill_forms_q4(pkg, tiny, refs, monkeypatch, case, knob):
    M, off = CASES[case]
    if KNOBS[knob]:
        monkeypatch.setenv(KNOBS[knob], "1")
    try:
        _check(pkg, refs, "q4", tiny, M, off, (case, knob))
    finally:
        if KNOBS[knob]:
            monkeypatch.delenv(KNOBS[knob])


def test_prefill_forms_f32_model(pkg, tiny_f32, refs):
    """Dense f32 weights at the product's 38 rows: no operator is XF-capable, so every layer takes the general form inside the 17..48-row window."""
    _check(pkg, refs, "f32", tiny_f32, 38, 0, ("m38_f32", "none"))
