"""Q8_0 tensor handles (vox_q8_tensor_from_bytes) through vox_linear_forward_ex against float64 (linear_ref.LinearRef on the dequantised matrix, which is exact:
f16 x int8 fits f32).  M <= 4 with K <= 8192 runs q8_rows_kernel (int8 matrix core), everything else q8_gemm_kernel (bf16 hi + lo), csrc/vox_q8.hip.

Error bar, both kernels, every element: |out - ref| <= carry_bound(2^-16 mag + [bias] 2^-23 |pre|), mag = |x| . |W|^T -- the componentwise bar test_gpu_linear.py and
test_gpu_rows4_op.py hold the Q4 kernels of these two arithmetic classes to.  Derived, not measured: the bf16 split leaves 2^-17 |x| per element and the f32 chain
over K / 32 <= 257 blocks at most 257 x 2^-24 of mag; the integer kernel rounds a block's activations to 2^-26 of the block maximum and sums exactly.  With a bias
the sum acc + bias is rounded once more, one f32 ulp of |pre|, which mag (no bias in it) does not cover.
Measured on an MI355X (profiles/q8_linear.txt): worst |err| / mag over this table 7.8e-07 (rows kernel, 2^-20.3) and 5.9e-06 (GEMM, 2^-17.4); 2^-16 = 1.5e-05.
No constant differs from the Q4 tables', so none is set from a measurement.

The weight bytes are written raw: q uniform in -128..127 with q = -128 forced into every block, scales positive, negative, +0, -0, small and the largest finite f16
(65504: every product stays finite in f32); every fourth weight row holds one scale class in all its blocks, so a lost class loses a whole column."""
import numpy as np
import pytest

from linear_ref import EPI_GELU, EPI_NONE, EPI_SWIGLU, ULP32, LinearRef, activations, carry_bound

pytestmark = pytest.mark.gpu
SHAPES = [(M, K, N) for M in (1, 3, 4, 5, 16, 17, 65) for N in (16, 80) for K in (32, 96, 1280)] + [(1, 8224, 16), (1, 8224, 80)]
FORMS = [(EPI_NONE, False), (EPI_NONE, True), (EPI_GELU, False), (EPI_GELU, True), (EPI_SWIGLU, False)]
WORST = {"rows": 0.0, "gemm": 0.0}          # worst |err| / mag without bias and epilogue, printed with every case (pytest -s)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def q8_blocks(rng, N, K):
    """Raw Q8_0 blocks [N][K / 32][34] (see the module docstring) and the dequantised matrix f32(d) * q, float32 [N][K]."""
    nb = K // 32
    q = rng.integers(-128, 128, (N, nb, 32)).astype(np.int8); q[:, :, rng.integers(0, 32)] = -128
    cls = rng.integers(0, 5, (N, nb)); cls[1::4] = (np.array([5, 1, 2, 0, 4, 3])[np.arange(len(cls[1::4])) % 6])[:, None]      # the largest scale in uniform rows only
    u = 0.5 + rng.random((N, nb))
    d = np.select([cls == 0, cls == 1, cls == 4], [0.01 * u, -0.01 * u, 2.0 ** -13 * u], 0.0).astype(np.float16)
    bits = d.view(np.uint16).copy(); bits[cls == 3] = 0x8000; bits[cls == 5] = 0x7BFF
    raw = np.empty((N, nb, 34), np.uint8)
    raw[:, :, :2] = bits.view(np.uint8).reshape(N, nb, 2); raw[:, :, 2:] = q.view(np.uint8)
    return raw.reshape(-1), (bits.view(np.float16).astype(np.float32)[:, :, None] * q.astype(np.float32)).reshape(N, K)


@pytest.mark.parametrize("act", ["scales", "outlier"])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_q8_linear(pkg, orc, ctx, M, K, N, act):
    rng = np.random.default_rng([M, K, N, len(act)])
    raw, W = q8_blocks(rng, N, K)
    t = pkg.q8_tensor_from_bytes(raw, [N, K], ctx); ref_w = LinearRef(W, N, K)
    assert t.shape() == [N, K] and t.num_blocks() == N * K // 32
    x, zrow = activations(rng, act, M, K)
    kern = "rows" if M <= 4 and K <= 8192 else "gemm"
    for epi, with_bias in FORMS:
        bias = rng.standard_normal(N).astype(np.float32) if with_bias else None
        out = pkg.linear_forward(t, x[None], bias, epi)[0].astype(np.float64)
        ref, pre, _, mag = ref_w(x, bias, epi)
        assert out.shape == ref.shape and np.isfinite(out).all()
        err = np.abs(out - ref)
        bound = carry_bound(pre, 2.0 ** -16 * mag + (ULP32 * np.abs(pre) if with_bias else 0.0), epi)
        if epi == EPI_NONE and not with_bias:
            WORST[kern] = max(WORST[kern], float((err / np.maximum(mag, 1e-300))[mag > 0].max(initial=0.0)))
        ratio = err / np.maximum(bound, 1e-300)
        print(f"q8 {kern} {M}x{K}x{N} {act} epi {epi} bias {with_bias}: worst |err| {ratio.max():.3f} of its bound; worst |err| / mag so far {WORST}")
        assert not (err > bound).any(), f"epi {epi} bias {with_bias}: {int((err > bound).sum())} elements past the bound, worst {ratio.max():.2f} x at {np.unravel_index(np.argmax(ratio), err.shape)}"
        if zrow is not None and not with_bias:
            assert (out[zrow] == 0.0).all(), "an all-zero activation row must give exactly zero"
    t.close()


@pytest.mark.parametrize("K,N", [(96, 16), (1280, 80)])
def test_q8_rows_bits(pkg, orc, ctx, K, N):
    """q8_rows_kernel: row r of a four-row call has the bits of the one-row call on that row, two runs have equal bits; dequantize returns f32(d) * q exactly."""
    rng = np.random.default_rng([K, N])
    raw, W = q8_blocks(rng, N, K)
    t = pkg.q8_tensor_from_bytes(raw, [N, K], ctx)
    assert (np.ascontiguousarray(t.dequantize()).view(np.uint32) == W.view(np.uint32)).all()
    x, _ = activations(rng, "scales", 4, K)
    b = rng.standard_normal(N).astype(np.float32)
    for epi, bias in ((EPI_NONE, b), (EPI_SWIGLU, None)):
        four = pkg.linear_forward(t, x[None], bias, epi)[0]
        assert (pkg.linear_forward(t, x[None], bias, epi)[0].view(np.uint32) == four.view(np.uint32)).all()
        for r in range(4):
            assert (pkg.linear_forward(t, x[None, r:r + 1], bias, epi)[0, 0].view(np.uint32) == four[r].view(np.uint32)).all(), r
    t.close()


def test_q4_path_untouched_and_refusals(pkg, orc, ctx):
    """A Q4_0 handle gives the same bits through vox_linear_forward_ex and vox_q4_matmul, as before; what vox_q8_tensor_from_bytes does not take is a VoxError."""
    rng = np.random.default_rng(4)
    t = pkg.Q4Tensor.from_q4_bytes(pkg.synth.synth_q4_blocks(rng, 80 * 1280, 0.04), [80, 1280], ctx)
    x = rng.standard_normal((1, 3, 1280)).astype(np.float32)
    assert (pkg.linear_forward(t, x).view(np.uint32) == pkg.q4_matmul(x, t).view(np.uint32)).all()
    t.close()
    raw = np.zeros(16 * 2 * 34, np.uint8)
    for shape, n in (([16, 48], 16 * 48 // 32 * 34), ([8, 64], 8 * 2 * 34), ([16, 64], 16 * 2 * 34 - 34)):
        with pytest.raises(pkg.VoxError) as e:
            pkg.q8_tensor_from_bytes(raw[:n], shape, ctx)
        assert e.value.code == 1


def test_model_loader_refuses_q8_file(pkg, orc, ctx, tmp_path):
    """vox_q4_model_load_gguf on the tiny model with one matrix stored as Q8_0: VOX_ERR_INVALID naming the tensor, nothing loaded."""
    from model_fixtures import tiny_gguf
    S = pkg.synth; path, _ = tiny_gguf()
    name = "layers.0.attention.wo.weight"; tensors = []
    for nm, (shape, dt, data) in S.read_gguf_tensors(path).items():
        if nm == name:
            dt, data = S.GGML_Q8_0, pkg.quantize_q8_0(S.dequantize_q4_0(np.asarray(data), int(np.prod(shape))))
        tensors.append((nm, shape, dt, np.asarray(data)))
    p = str(tmp_path / "q8.gguf"); S.write_gguf(p, tensors)
    for loader in (pkg.Q4ModelLoader.from_bytes(open(p, "rb").read()), pkg.Q4ModelLoader.from_file(p)):
        with pytest.raises(pkg.VoxError, match=name.replace(".", r"\.") + ".*Q8_0 models are not loaded yet") as e:
            loader.load(ctx)
        assert e.value.code == 1
