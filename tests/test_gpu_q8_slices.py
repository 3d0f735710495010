"""The Q8_0 K-slice operator (csrc/vox_q8_slices.hip: q8_slice_kernel + q8_slice_finish_kernel) through vox_q8_rows_forward (pkg.q8_rows_forward) against float64:
linear_ref.LinearRef on the dequantised matrix (exact: f16 x int8 fits f32); with the fused norm the reference is the float64 RMSNorm, then the float64 product; the
residual is added to the reference.  Bound, every element: carry_bound(pre, 2^-16 mag + ulps, epi), mag = |pro(x)| . |W|^T -- the bar of test_gpu_q8_linear.py and
test_gpu_rows4_op.py, derived there (the integer kernel rounds a block's activations to 2^-26 of the block maximum and sums exactly; the f32 chain over blocks, slices
and rstd stays far below 2^-16 mag).  ulps: with a bias one f32 ulp of |pre| (the sum acc + bias is rounded once more); with a residual one f32 ulp of |pre + resid|,
the value that last rounding produces -- |pre| alone does not cover it where a weight row of zero scales leaves pre = bias next to a larger residual.
Shapes: K = 32 (one block and a pad block), 96 (an odd block count, one step per wave); the slice edges of Q8S_COLS = 3072: K = 3072 (exactly one slice), 3104 (one
block in the second slice: seven waves without steps), 6176 (two slices and an odd block), 9216 (three full slices, the decoder's w2); N = 8240 = 515 tiles at K = 32,
three more than the 512 workgroups the grid rule allows a slice.  Measured on an MI355X: worst |err| / mag 5.7e-7 without the norm, 9.0e-7 with it (2^-16 = 1.5e-5);
no constant is set from them.  The weight bytes: test_gpu_q8_linear.py's q8_blocks (q = -128 in every block, scales +, -, +-0, 2^-13, 65504)."""
import ctypes as C

import numpy as np
import pytest

from linear_ref import EPI_GELU, EPI_NONE, EPI_SWIGLU, ULP32, LinearRef, activations, carry_bound

pytestmark = pytest.mark.gpu
STORE, RESID, SWIGLU, GELU, EPS = 0, 1, 2, 3, 1e-5
REF_EPI = {STORE: EPI_NONE, RESID: EPI_NONE, SWIGLU: EPI_SWIGLU, GELU: EPI_GELU}
CASES = [(M, K, N, pro, epi, bias) for K in (32, 96) for N in (16, 48) for M in (1, 3, 4) for pro in (0, 1) for epi in (STORE, RESID, SWIGLU, GELU) for bias in (False, True)]
CASES += [(4, K, 16) + f for K in (3072, 3104, 6176, 9216) for f in ((1, RESID, True), (0, SWIGLU, False))] + [(4, 32, 8240, 1, RESID, True)]
WORST = {}          # pro -> worst |err| / mag of the plain store form, printed with every case (pytest -s)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture
def q8t(pkg, ctx):
    """Makes Q8_0 tensors and closes them behind the test, also behind a failed one (a tensor freed after its context takes the process down)."""
    made = []
    yield lambda raw, N, K: made.append(pkg.q8_tensor_from_bytes(raw, [N, K], ctx)) or made[-1]
    for t in made:
        t.close()


def q8_blocks(rng, N, K):
    """Raw Q8_0 blocks [N][K / 32][34] and the dequantised matrix f32(d) * q, float32 [N][K] (a copy of tests/test_gpu_q8_linear.py's writer)."""
    nb = K // 32
    q = rng.integers(-128, 128, (N, nb, 32)).astype(np.int8); q[:, :, rng.integers(0, 32)] = -128
    cls = rng.integers(0, 5, (N, nb)); cls[1::4] = (np.array([5, 1, 2, 0, 4, 3])[np.arange(len(cls[1::4])) % 6])[:, None]      # the largest scale in uniform rows only
    u = 0.5 + rng.random((N, nb))
    d = np.select([cls == 0, cls == 1, cls == 4], [0.01 * u, -0.01 * u, 2.0 ** -13 * u], 0.0).astype(np.float16)
    bits = d.view(np.uint16).copy(); bits[cls == 3] = 0x8000; bits[cls == 5] = 0x7BFF
    raw = np.empty((N, nb, 34), np.uint8)
    raw[:, :, :2] = bits.view(np.uint8).reshape(N, nb, 2); raw[:, :, 2:] = q.view(np.uint8)
    return raw.reshape(-1), (bits.view(np.float16).astype(np.float32)[:, :, None] * q.astype(np.float32)).reshape(N, K)


def operands(rng, M, K, N, pro, epi, bias, act="scales"):
    x, zrow = activations(rng, act, M, K)
    b = rng.standard_normal(N).astype(np.float32) if bias else None
    gamma = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32) if pro else None
    resid = rng.standard_normal((M, N)).astype(np.float32) if epi == RESID else None
    return x, zrow, b, gamma, resid


@pytest.mark.parametrize("act", ["scales", "outlier"])
@pytest.mark.parametrize("M,K,N,pro,epi,bias", CASES)
def test_q8_slices_case(pkg, orc, q8t, M, K, N, pro, epi, bias, act):
    rng = np.random.default_rng([M, K, N, pro, epi, int(bias), len(act)])
    raw, W = q8_blocks(rng, N, K)
    t = q8t(raw, N, K); ref_w = LinearRef(W, N, K)
    x, zrow, b, gamma, resid = operands(rng, M, K, N, pro, epi, bias, act)
    before = pkg.q8_rows_launches()
    out32 = pkg.q8_rows_forward(t, x, b, gamma, EPS, epi, resid); out = out32.astype(np.float64)
    assert pkg.q8_rows_launches() == before + 1
    xn = x.astype(np.float64)
    if pro:
        xn = xn / np.sqrt((xn * xn).mean(axis=1, keepdims=True) + EPS) * gamma.astype(np.float64)[None, :]
    ref, pre, _, mag = ref_w(xn, b, REF_EPI[epi])
    ulps = (ULP32 * np.abs(pre) if bias else 0.0) + (ULP32 * np.abs(pre + resid) if epi == RESID else 0.0)
    ref = ref + resid.astype(np.float64) if epi == RESID else ref
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = np.abs(out - ref)
    bound = carry_bound(pre, 2.0 ** -16 * mag + ulps, REF_EPI[epi])
    if epi == STORE and not bias:          # the product's own error: no bias or residual rounding in it
        WORST[pro] = max(WORST.get(pro, 0.0), float((err / np.maximum(mag, 1e-300))[mag > 0].max(initial=0.0)))
    ratio = err / np.maximum(bound, 1e-300)
    print(f"q8 slices pro {pro} epi {epi} bias {bias} {M}x{K}x{N} {act}: worst |err| {ratio.max():.3f} of its bound; worst |err| / mag so far {WORST}")
    assert not (err > bound).any(), f"{int((err > bound).sum())} elements past the bound, worst {ratio.max():.2f} x at {np.unravel_index(np.argmax(ratio), err.shape)}"
    if zrow is not None:          # an all-zero row: exactly epi(bias) (+ resid)
        if b is None:
            assert (out32[zrow] == (resid[zrow] if epi == RESID else 0.0)).all()
        elif epi in (STORE, RESID):
            assert (out32[zrow] == (b + resid[zrow] if epi == RESID else b)).all()
        else:          # GELU / SwiGLU of the bias: the bits of the same operator on one zero row (its distance from float64 is held by the bound above: mag = 0 there)
            one = pkg.q8_rows_forward(t, np.zeros((1, K), np.float32), b, gamma, EPS, epi)[0]
            assert (out32[zrow].view(np.uint32) == one.view(np.uint32)).all()


@pytest.mark.parametrize("pro,epi,bias", [(1, RESID, True), (0, SWIGLU, False)])
def test_q8_slices_bits(pkg, orc, q8t, pro, epi, bias):
    """K = 6176, N = 48: row r of the four-row call has the bits of the one-row call on that row; two runs have equal bits."""
    K, N = 6176, 48; rng = np.random.default_rng([K, N, pro, epi])
    raw, _ = q8_blocks(rng, N, K); t = q8t(raw, N, K)
    x, _, b, gamma, resid = operands(rng, 4, K, N, pro, epi, bias)
    four = pkg.q8_rows_forward(t, x, b, gamma, EPS, epi, resid)
    assert (pkg.q8_rows_forward(t, x, b, gamma, EPS, epi, resid).view(np.uint32) == four.view(np.uint32)).all()
    for r in range(4):
        one = pkg.q8_rows_forward(t, x[r:r + 1], b, gamma, EPS, epi, None if resid is None else resid[r:r + 1])
        assert (one[0].view(np.uint32) == four[r].view(np.uint32)).all(), r


@pytest.mark.parametrize("M,K,count", [(1, 8224, 1), (4, 8224, 1), (5, 8224, 0), (1, 1280, 0)])
def test_q8_slices_routing(pkg, orc, q8t, M, K, count):
    """linear_forward on a Q8 handle runs the K-slice operator for M <= 4 with K > 8192, and for nothing else."""
    rng = np.random.default_rng([M, K]); raw, _ = q8_blocks(rng, 16, K); t = q8t(raw, 16, K)
    before = pkg.q8_rows_launches()
    pkg.linear_forward(t, rng.standard_normal((1, M, K)).astype(np.float32))
    assert pkg.q8_rows_launches() == before + count


@pytest.mark.parametrize("what", ["q4", "M5", "resid", "gamma"])
def test_q8_slices_refusals(pkg, orc, ctx, q8t, what):          # a VoxError with code 1, no launch counted
    rng = np.random.default_rng(7); raw, _ = q8_blocks(rng, 16, 64)
    t = pkg.Q4Tensor.from_q4_bytes(pkg.synth.synth_q4_blocks(rng, 16 * 64, 0.04), [16, 64], ctx) if what == "q4" else q8t(raw, 16, 64)
    x = np.ones((5 if what == "M5" else 2, 64), np.float32); out = np.empty((5, 16), np.float32); before = pkg.q8_rows_launches()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with pytest.raises(pkg.VoxError) as e:
        if what in ("q4", "M5"):
            pkg.q8_rows_forward(t, x)
        else:          # the residual epilogue without resid; the norm without gamma
            pkg._lib.check(pkg.lib().vox_q8_rows_forward(ctx.h, t.h, None, None, EPS, p(x), 2, p(out), int(what == "gamma"), int(what == "resid"), None, 0))
    code, after = e.value.code, pkg.q8_rows_launches()
    t.close()
    assert code == 1 and after == before
