"""The float64 reference of one linear operator (Q4_0 or dense weights, bias, GELU / SwiGLU epilogue) and the error bars that go with it
(tests/test_gpu_linear.py).  Independent of the HIP kernels and of the oracle's summation order: the weights are the oracle's dequantised values
(orc.q4_dequantize, pinned bit-exact elsewhere) widened to float64, the product is one BLAS call, the epilogue is evaluated in float64.
tests/test_linear_ref.py ties it to the oracle and to the reference project's own component vectors."""
import math

import numpy as np

import oracle_lib as orc

EPI_NONE, EPI_GELU, EPI_SWIGLU = 0, 1, 2
ULP32 = 2.0 ** -23          # one f32 ulp of v is at most ULP32 * |v|

_erf = np.frompyfunc(math.erf, 1, 1)


def gelu64(v):
    """x/2 (1 + erf(x / sqrt 2)): the form of gelu_f and orc_gelu."""
    v = np.asarray(v, dtype=np.float64)
    return 0.5 * v * (1.0 + np.asarray(_erf(v / math.sqrt(2.0)), dtype=np.float64))


def silu64(v):
    v = np.asarray(v, dtype=np.float64)
    with np.errstate(over="ignore"):          # exp(-v) = inf for v < -709: v / inf = -0, the limit
        return v / (1.0 + np.exp(-v))


def q4_scales(raw, n_blocks):
    """The f16 block scales d of raw 18-byte Q4_0 blocks, as float64 [n_blocks]."""
    b = np.ascontiguousarray(np.asarray(raw, dtype=np.uint8).reshape(n_blocks, 18)[:, :2])
    return b.view(np.float16).reshape(n_blocks).astype(np.float64)


class LinearRef:
    """One weight matrix [N][K] held in float64: `w` = raw Q4_0 bytes (uint8, 18 per 32 elements) or a dense float32 [N][K] array."""

    def __init__(self, w, N, K):
        w = np.asarray(w)
        self.N, self.K = int(N), int(K)
        if w.dtype == np.uint8:
            assert w.size == N * K // 32 * 18 and K % 32 == 0
            self.W = orc.q4_dequantize(w, N * K).reshape(N, K).astype(np.float64)
            self.absd8 = 8.0 * np.abs(q4_scales(w, N * K // 32)).reshape(N, K // 32)      # the largest |weight| a block can hold
        else:
            assert w.shape == (N, K) and w.dtype == np.float32
            self.W = w.astype(np.float64)
            self.absd8 = None

    def __call__(self, x, bias=None, epilogue=EPI_NONE):
        """x [..., K] -> (ref, pre, rowmax, mag), rows flattened: ref [M][N or N/2] the operator's float64 result; pre [M][N] = x W^T + bias, the values before the
        epilogue; rowmax [M] = max_j |pre_ij|; mag [M][N] = sum_b 8 |d_jb| sum_{k in b} |x_ik| (dense: sum_k |x_ik| |w_jk|), the size of the terms a sum is made of."""
        x = np.asarray(x, dtype=np.float64).reshape(-1, self.K)
        pre = x @ self.W.T
        if bias is not None:
            pre = pre + np.asarray(bias, dtype=np.float64)[None, :]
        ax = np.abs(x)
        mag = ax.reshape(x.shape[0], self.K // 32, 32).sum(-1) @ self.absd8.T if self.absd8 is not None else ax @ np.abs(self.W).T
        return apply_epilogue(pre, epilogue), pre, np.abs(pre).max(axis=1), mag


def apply_epilogue(pre, epilogue):
    if epilogue == EPI_GELU:
        return gelu64(pre)
    if epilogue == EPI_SWIGLU:
        assert pre.shape[1] % 2 == 0
        return silu64(pre[:, 0::2]) * pre[:, 1::2]          # interleaved rows: 2j gate, 2j + 1 up
    assert epilogue == EPI_NONE
    return pre


def linear_ref64(raw_or_dense, N, K, x, bias=None, epilogue=EPI_NONE):
    return LinearRef(raw_or_dense, N, K)(x, bias, epilogue)


def carry_bound(pre, bound, epilogue):
    """The bound on |out - ref| after the epilogue, given the elementwise bound `bound` [M][N] on the error of `pre`: GELU's derivative is at most 1.13 in magnitude,
    SiLU's at most 1.1, so |d(silu(g) u)| <= 1.1 |u| |dg| + |silu(g)| |du| (float64 g, u); plus 4 ulp of the result for erff / expf.  No epilogue: `bound` itself."""
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), pre.shape)
    if epilogue == EPI_GELU:
        return 1.13 * bound + 4 * ULP32 * np.abs(gelu64(pre))
    if epilogue == EPI_SWIGLU:
        g, u = pre[:, 0::2], pre[:, 1::2]
        return 1.1 * np.abs(u) * bound[:, 0::2] + np.abs(silu64(g)) * bound[:, 1::2] + 4 * ULP32 * np.abs(silu64(g) * u)
    return bound
