"""Pins the float64 reference of the linear-operator tests (tests/linear_ref.py) to the CPU oracle (f32 sequential sums, orc_gelu / orc_silu) and to the reference
project's own per-component vectors (tests/golden/ref_python_components.npz), so tests/test_gpu_linear.py measures the kernels against those numbers and not
against a reference of its own making."""
import os

import numpy as np
import pytest

from linear_ref import EPI_GELU, EPI_SWIGLU, LinearRef, carry_bound, gelu64, linear_ref64, silu64
from model_fixtures import component_weight, rel_err

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_python_components.npz")
ENC = "mm_streams_embeddings.embedding_module.whisper_encoder."


def _vec(fn, a):
    return np.array([fn(float(v)) for v in np.ravel(a)], dtype=np.float32).reshape(np.shape(a))


@pytest.mark.parametrize("m,k,n", [(1, 128, 530), (5, 3072, 530), (17, 160, 1062), (38, 1280, 1062), (65, 32, 96), (3, 3104, 130)])
def test_linear_ref64_vs_oracle_q4_matmul(pkg, orc, m, k, n):
    """x W^T + bias against the oracle's f32 sequential-k sums: the oracle's own error is <= k 2^-24 of sum |x||w| (<= mag), the float64 product's is negligible."""
    rng = np.random.default_rng(m + k + n)
    raw = pkg.synth.synth_q4_blocks(rng, n * k, 0.04)
    x = (rng.standard_normal((1, m, k)) * (1 + np.arange(k) / k)).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    ref, pre, rowmax, mag = linear_ref64(raw, n, k, x, bias)
    assert ref is pre and ref.shape == mag.shape == (m, n) and rowmax.shape == (m,)
    exp = orc.q4_matmul(raw, n, k, x, bias=bias).reshape(m, n)
    assert (np.abs(exp - ref) <= k * 2.0 ** -24 * mag + 2.0 ** -23 * np.abs(ref)).all()
    assert (rowmax == np.abs(ref).max(axis=1)).all()
    # mag bounds every sum of |x||w| term by term: |w| <= 8 |d| inside a block
    W = orc.q4_dequantize(raw, n * k).reshape(n, k).astype(np.float64)
    assert (np.abs(x[0].astype(np.float64)) @ np.abs(W).T <= mag * (1 + 1e-12)).all()


def test_linear_ref64_epilogues_vs_oracle_scalars(pkg, orc):
    """GELU and SiLU in float64 against orc_gelu / orc_silu (f32), and the interleaved gate / up pairing of the SwiGLU epilogue."""
    v = np.concatenate([np.linspace(-12, 12, 4001), [0.0, -0.0, 1e-20, -1e-20, 30.0, -30.0]]).astype(np.float32)
    L = orc.lib()
    assert np.abs(_vec(L.orc_gelu, v) - gelu64(v)).max() < 2e-6 and np.abs(_vec(L.orc_silu, v) - silu64(v)).max() < 2e-6
    assert gelu64(0.0) == 0.0 and silu64(0.0) == 0.0
    rng = np.random.default_rng(3); n, k, m = 10, 64, 3
    raw = pkg.synth.synth_q4_blocks(rng, n * k, 0.5); x = rng.standard_normal((m, k)).astype(np.float32)
    ref, pre, _, _ = linear_ref64(raw, n, k, x, None, EPI_SWIGLU)
    acc = orc.q4_matmul(raw, n, k, x[None]).reshape(m, n)
    assert ref.shape == (m, n // 2)
    assert np.abs(ref - _vec(L.orc_silu, acc[:, 0::2]) * acc[:, 1::2]).max() < 1e-5 * np.abs(ref).max()
    refg, _, _, _ = linear_ref64(raw, n, k, x, np.arange(n, dtype=np.float32), EPI_GELU)
    assert np.abs(refg - _vec(L.orc_gelu, (acc + np.arange(n, dtype=np.float32)))).max() < 1e-5 * np.abs(refg).max()
    # the carried bounds: none -> the bound itself; GELU / SwiGLU scale it by the derivative's maximum
    b = np.full(pre.shape, 1e-3)
    assert (carry_bound(pre, b, 0) == b).all()
    assert (carry_bound(pre, b, EPI_GELU) >= 1.13e-3).all() and carry_bound(pre, b, EPI_SWIGLU).shape == ref.shape
    d = 1e-3 * rng.standard_normal(pre.shape)
    moved = silu64((pre + d)[:, 0::2]) * (pre + d)[:, 1::2]
    assert (np.abs(moved - ref) <= carry_bound(pre, np.abs(d), EPI_SWIGLU) + 1.2 * np.abs(d[:, 0::2] * d[:, 1::2])).all()
    assert (np.abs(gelu64(pre + d) - gelu64(pre)) <= carry_bound(pre, np.abs(d), EPI_GELU)).all()


def test_linear_ref64_reproduces_reference_python_component_vectors():
    """The reference's own SwiGLU and Ada-modulation vectors (scripts/reference_forward.py on synthetic weights of the real shapes; what models/layers/swiglu.rs and
    rms_norm.rs load) from the dense weights component_weight gives: w2 (silu(w1 x) * w3 x) as one interleaved w1 | w3 operand with the SwiGLU epilogue, and
    w2 gelu(w0 t).  Tolerance 2e-4 of the largest value, as every comparison with those f32 PyTorch vectors."""
    g = np.load(G)
    w1, w2, w3 = (component_weight(ENC + f"transformer.layers.0.feed_forward.w{i}.weight") for i in (1, 2, 3))
    w13 = np.empty((2 * w1.shape[0], w1.shape[1]), np.float32); w13[0::2] = w1; w13[1::2] = w3
    h, _, _, mag = linear_ref64(w13, w13.shape[0], w13.shape[1], g["swiglu_input"][0], None, EPI_SWIGLU)
    assert h.shape == (10, 5120) and mag.shape == (10, 10240)
    out, _, _, _ = linear_ref64(w2, w2.shape[0], w2.shape[1], h.astype(np.float32))
    assert rel_err(out, g["swiglu_output"][0]) < 2e-4
    w0, wa2 = component_weight("layers.0.ada_rms_norm_t_cond.0.weight"), component_weight("layers.0.ada_rms_norm_t_cond.2.weight")
    ref0 = LinearRef(w0, *w0.shape)
    hid, _, _, _ = ref0(g["ada_rms_norm_t_embed"], None, EPI_GELU)
    scale, _, _, _ = linear_ref64(wa2, wa2.shape[0], wa2.shape[1], hid.astype(np.float32))
    assert rel_err(scale, g["ada_rms_norm_scale"][0]) < 2e-4
    assert rel_err(g["ada_rms_norm_input"][0] * (1.0 + scale), g["ada_rms_norm_output"][0]) < 2e-4


# ---- the XF-step pieces of linear_ref (tests/test_gpu_xf_ops.py)
def test_xf_planes_round_trip_and_the_layout_comments_slots():
    """xf_pack / xf_unpack restate xf_store4: a one-hot row sits at the slot the layout comment names -- lane 16 g + row of uint4 [q][j], K-slot order
    {4g, 4g+2, 16+4g, 16+4g+2, 4g+1, 4g+3, 16+4g+1, 16+4g+3} -- every slot is taken exactly once, and hi + lo gives the row back to 2^-17 |x| (bf16-exact values: exactly)."""
    import linear_ref as R
    K = 256
    order = [0, 2, 16, 18, 1, 3, 17, 19]
    for row, k in ((0, 0), (3, 2), (15, 255), (7, 128 + 32 * 2 + 4 * 3 + 16 + 1), (9, 37)):
        x = np.zeros((16, K), np.float32); x[row, k] = 1.5
        p = R.xf_pack(x)
        q, j, e = k // 128, (k // 32) % 4, k % 32
        g = (e % 16) // 4
        slot = order.index(e - 4 * g)
        want = (((q * 4 + j) * 64 + 16 * g + row) * 8) + slot
        assert np.flatnonzero(p).tolist() == [want] and p[want] == 0x3FC0, (row, k)
    idx = R.xf_index(np.arange(16)[:, None], np.arange(K)[None, :])
    assert sorted(idx.ravel().tolist()) == list(range(K * 16))
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((11, K)) * 10.0 ** rng.integers(-3, 4, (11, 1))).astype(np.float32)
    val, hi, lo = R.xf_unpack(R.xf_pack(x), K)
    assert (np.abs(val[:11] - x) <= R.XF_SPLIT * np.abs(x)).all() and not val[11:].any() and (lo[:11] != 0).any()
    xb = R.bf16_f32(R.bf16_rne(x))
    assert (R.xf_unpack(R.xf_pack(xb), K)[0][:11] == xb).all()
    assert R.bf16_rne(np.array([1.0, 1.00390625, 1.01171875, -2.5], np.float32)).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC020]      # ties to even, both ways


def test_xf_step_reference_pieces(pkg, orc):
    """The folded norm's factor, interleaved-pair RoPE (against the oracle's rope on f32), the bounds' shapes, and the chunked LinearRef against the whole one."""
    import linear_ref as R
    rng = np.random.default_rng(9)
    part = rng.random((7, 16)).astype(np.float32)
    r = R.rstd64(part, 256, 1e-5)
    assert r.shape == (16,) and np.allclose(r, 1.0 / np.sqrt(part.astype(np.float64).sum(0) / 256 + 1e-5), rtol=1e-15)
    pre = rng.standard_normal((3, 8)); c = np.cos(rng.random((3, 4))); s = np.sin(rng.random((3, 4)))
    out = R.rope64(pre, c, s)
    for i in range(4):
        assert np.allclose(out[:, 2 * i], pre[:, 2 * i] * c[:, i] - pre[:, 2 * i + 1] * s[:, i]) and np.allclose(out[:, 2 * i + 1], pre[:, 2 * i + 1] * c[:, i] + pre[:, 2 * i] * s[:, i])
    b = R.carry_bound(pre, np.full((3, 8), 1e-3), R.EPI_ROPE, cos=c, sin=s)
    assert b.shape == (3, 8) and (b >= 1e-3 * (np.abs(c) + np.abs(s)).repeat(2, axis=1) * 0.999).all()
    # a perturbation of `pre` inside the bound moves the result by no more than the carried bound
    d = 1e-3 * rng.uniform(-1, 1, (3, 8))
    assert (np.abs(R.rope64(pre + d, c, s) - out) <= b).all()
    assert (R.norm_bound(pre, np.full((3, 8), 1e-3), np.array([2.0, 3.0, 4.0]), 5) >= 1e-3 * np.array([2.0, 3.0, 4.0])[:, None]).all()
    N, K = 96, 128
    raw = pkg.synth.synth_q4_blocks(rng, N * K, 0.04)
    x = rng.standard_normal((5, K)).astype(np.float32)
    whole, chunked = R.LinearRef(raw, N, K)(x), R.LinearRef(raw, N, K, chunk_rows=40)(x)
    assert np.array_equal(whole[1], chunked[1]) and np.array_equal(whole[3], chunked[3])
