"""CPU checks of the window-edge probes (no GPU): the inputs the GPU tests past the decoder's 8192-position window use must make an off-by-one in
the window's first key visible, far above the tolerance those tests apply.  The oracle's window is moved by one (orc_model_set_dec_window /
orc_attention's window argument) to stand for a kernel that starts its window one key early or late.  Also the oracle's cache truncate."""
import numpy as np
import pytest

from model_fixtures import DEC_WINDOW, EDGE_ATTN_CASES, edge_attention_inputs, fill_edge_caches, tiny_gguf, window_edge_rows

TOL_OPS = 2e-5       # tests/test_gpu_ops.py: attention core, of the largest |ref|
TOL = 2e-4           # tests/test_gpu_model.py: hidden states and logits, of the largest |ref|


@pytest.mark.parametrize("M,kv,off,win", EDGE_ATTN_CASES)
def test_attention_edge_inputs_expose_a_window_off_by_one(orc, M, kv, off, win):
    L = orc.lib()
    for H, KV in ((4, 1), (4, 2)):
        q, k, v = edge_attention_inputs(M, kv, H, KV, off, win)
        outs = []
        for w in (win, win - 1, win + 1):
            r = np.zeros((M, H * 128), np.float32)
            L.orc_attention(q, k, v, M, kv, H, KV, 128, off, 1, w, r)
            outs.append(r)
        scale = np.abs(outs[0]).max()
        assert np.abs(outs[1] - outs[0]).max() > 100 * TOL_OPS * scale          # the window starts one key late: key p - window dropped
        if off + M - 1 > win:      # some query has a key p - window - 1 to wrongly include
            assert np.abs(outs[2] - outs[0]).max() > 100 * TOL_OPS * scale


def test_oracle_cache_truncate(orc):
    path, dims = tiny_gguf()
    o = orc.Model(path); c = o.cache(16)
    try:
        k = np.ones((dims.dec_kv_heads, 5, 128), np.float32)
        o.cache_update(c, 0, 0, k, k)
        assert orc.lib().orc_cache_len(c) == 5
        with pytest.raises(ValueError):
            o.cache_truncate(c, 6)
        o.cache_truncate(c, 2); assert orc.lib().orc_cache_len(c) == 2
        o.cache_truncate(c, 0); assert orc.lib().orc_cache_len(c) == 0
        with pytest.raises(ValueError):
            o.cache_truncate(c, -1)
    finally:
        o.cache_free(c); o.close()


def test_tiny_decoder_edge_cache_exposes_a_window_off_by_one(pkg, orc):
    """The tiny model (2 layers, 2 KV heads) on a 16384-row cache filled by fill_edge_caches: one decode step at positions where the window has
    moved, oracle at window 8192 against the oracle at 8191 and 8193 -- hidden state and logits must differ by 20x the GPU tests' 2e-4 or more (measured: >= 60x)."""
    path, dims = tiny_gguf()
    o = orc.Model(path); oc = o.cache(16384)
    t = pkg.TimeEmbedding(dims.dec_dim).embed(6.0)
    probes = [8192, 8193, 8194, 8353, 12345, 16383]
    try:
        filled = 0
        for p in probes:
            fill_edge_caches([lambda l, a, k, v: o.cache_update(oc, l, a, k, v)], dims.dec_layers, dims.dec_kv_heads, 128, filled, p, window_edge_rows(probes))
            filled = p
            x = (0.5 * np.random.default_rng([5, p]).standard_normal((1, dims.dec_dim))).astype(np.float32)
            res = []
            for w in (DEC_WINDOW, DEC_WINDOW - 1, DEC_WINDOW + 1):
                o.set_dec_window(w); o.cache_truncate(oc, p)
                h = o.forward_hidden_with_cache(x, t, oc)
                res.append((h, o.lm_head(h)))
            o.set_dec_window(DEC_WINDOW)
            hs, ls = np.abs(res[0][0]).max(), np.abs(res[0][1]).max()
            for i, (h, lg) in enumerate(res[1:]):
                if i == 1 and p <= DEC_WINDOW:
                    continue       # nothing before key 0 to include
                assert np.abs(h - res[0][0]).max() > 20 * TOL * hs, (p, i)
                assert np.abs(lg - res[0][1]).max() > 20 * TOL * ls, (p, i)
    finally:
        o.set_dec_window(DEC_WINDOW); o.cache_free(oc); o.close()
