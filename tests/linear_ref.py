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

    def __init__(self, w, N, K, chunk_rows=0):
        """chunk_rows > 0 (Q4 only): no float64 copy of the whole weight -- the raw blocks are kept and dequantised chunk_rows weight rows at a time
        (f32, exact; then float64), for the large weights of the XF-step table."""
        w = np.asarray(w)
        self.N, self.K = int(N), int(K)
        self.raw, self.chunk_rows = None, int(chunk_rows)
        if w.dtype == np.uint8:
            assert w.size == N * K // 32 * 18 and K % 32 == 0
            if chunk_rows:
                self.raw, self.W = w.reshape(N, K // 32 * 18), None
            else:
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
        if self.W is None:
            pre = np.empty((x.shape[0], self.N))
            for n0 in range(0, self.N, self.chunk_rows):
                n1 = min(n0 + self.chunk_rows, self.N)
                pre[:, n0:n1] = x @ orc.q4_dequantize(np.ascontiguousarray(self.raw[n0:n1]).reshape(-1), (n1 - n0) * self.K).reshape(n1 - n0, self.K).astype(np.float64).T
        else:
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


def carry_bound(pre, bound, epilogue, cos=None, sin=None):
    """The bound on |out - ref| after the epilogue, given the elementwise bound `bound` [M][N] on the error of `pre`: GELU's derivative is at most 1.13 in magnitude,
    SiLU's at most 1.1, so |d(silu(g) u)| <= 1.1 |u| |dg| + |silu(g)| |du| (float64 g, u); plus 4 ulp of the result for erff / expf.  No epilogue: `bound` itself.
    EPI_ROPE (cos, sin [M][N / 2], exact table values): |c| b_v + |s| b_other + 4 ulp of |a c| + |b s| (two products, one sum, each rounded before anything cancels)."""
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), pre.shape)
    if epilogue == EPI_ROPE:
        out = np.empty(pre.shape)
        c, s = np.abs(cos), np.abs(sin)
        out[:, 0::2] = c * bound[:, 0::2] + s * bound[:, 1::2]; out[:, 1::2] = c * bound[:, 1::2] + s * bound[:, 0::2]
        a, b = np.abs(pre[:, 0::2]), np.abs(pre[:, 1::2])
        out[:, 0::2] += 4 * ULP32 * (a * c + b * s); out[:, 1::2] += 4 * ULP32 * (b * c + a * s)      # of |a c| + |b s|: the products are rounded before they cancel
        return out
    if epilogue == EPI_GELU:
        return 1.13 * bound + 4 * ULP32 * np.abs(gelu64(pre))
    if epilogue == EPI_SWIGLU:
        g, u = pre[:, 0::2], pre[:, 1::2]
        return 1.1 * np.abs(u) * bound[:, 0::2] + np.abs(silu64(g)) * bound[:, 1::2] + 4 * ULP32 * np.abs(silu64(g) * u)
    return bound


# ---- activation kinds of the operator tables (tests/test_gpu_linear.py, tests/test_gpu_xf_ops.py)
def row_scales(rows):
    """10^-3 .. 10^3 across the rows of every 16-row group, the phase moved from group to group; fewer than 16 rows: the whole range across them."""
    i = np.arange(rows)
    if rows <= 16:
        return 10.0 ** (-3 + 6 * i / max(rows - 1, 1))
    return 10.0 ** (-3 + 6 * ((i + 5 * (i // 16)) % 16) / 15)


def activations(rng, act, rows, K):
    """[rows][K] f32 and the index of the all-zero row (or None)."""
    z = None
    g = rng.standard_normal((rows, K))
    if act == "ramp":
        x = g * (1 + np.arange(K) / K)
    elif act == "scales":
        x = g * (1 + np.arange(K) / K) * row_scales(rows)[:, None]
        x[rng.random((rows, K)) < 0.03] = 0.0
        x[rng.random((rows, K)) < 0.03] = -0.0
        if rows >= 2:
            z = rows // 2; x[z] = 0.0
    elif act in ("offset3", "offset30"):
        x = g + (3.0 if act == "offset3" else 30.0)
    elif act == "abs":
        x = np.abs(g)
    elif act == "outlier":
        x = g; x[:, 5::97] = 200.0 * (1 + 0.1 * np.abs(g[:, 5::97]))          # 1 column in 97 at 200 sigma, constant sign
    else:
        raise AssertionError(act)
    return x.astype(np.float32), z


# ---- the batched XF decode step (tests/test_gpu_xf_ops.py): XF planes, the folded norm, RoPE, the XF output, and their error bars
EPI_ROPE = 3                 # carry_bound: interleaved-pair RoPE (cos=, sin= per pair)
XF_SPLIT = 2.0 ** -17        # |x - (hi + lo)| <= 2^-17 |x| (split_pair)


def xf_index(row, k):
    """The 16-bit slot of element k of row `row` (0..15) in the hi plane of an XF tile (xf_store4's index arithmetic): the plane is uint4 [K/128 (q)][4 (j)][64 lanes],
    lane = 16 g + row holds the elements of block 4q + j in the K-slot order {4g, 4g+2, 16+4g, 16+4g+2, 4g+1, 4g+3, 16+4g+1, 16+4g+3}; the lo plane follows the hi
    plane, K * 16 slots later."""
    k = np.asarray(k)
    q, j, e = k >> 7, (k >> 5) & 3, k & 31
    half, g, t = e >> 4, (e & 15) >> 2, e & 3
    return ((q * 4 + j) * 64 + g * 16 + row) * 8 + 2 * half + (t >> 1) + 4 * (t & 1)


def bf16_rne(x):
    """float32 -> bf16 bits, round to nearest even (v_cvt_pk_bf16_f32); finite inputs."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def xf_pack(x):
    """f32 rows [M <= 16][K] -> one XF tile, uint16 [K * 32]: hi = bf16(x), lo = bf16(x - hi); rows >= M zero."""
    x = np.asarray(x, dtype=np.float32); M, K = x.shape
    assert M <= 16 and K % 128 == 0
    out = np.zeros(K * 32, np.uint16)
    hi = bf16_rne(x); lo = bf16_rne(x - bf16_f32(hi))
    idx = xf_index(np.arange(M)[:, None], np.arange(K)[None, :])
    out[idx] = hi; out[K * 16 + idx] = lo
    return out


def xf_unpack(planes, K, fill=None):
    """One XF tile (uint16 [K * 32]) -> (values float64 [16][K] = hi + lo, hi bits [16][K], lo bits [16][K])."""
    planes = np.asarray(planes, dtype=np.uint16)
    assert planes.size == K * 32
    idx = xf_index(np.arange(16)[:, None], np.arange(K)[None, :])
    hi, lo = planes[idx], planes[K * 16 + idx]
    return bf16_f32(hi).astype(np.float64) + bf16_f32(lo).astype(np.float64), hi, lo


def rstd64(ssq_part, K, eps):
    """The folded RMSNorm's row factors: ssq_part [n_part][16] partial sums of squares -> 1 / sqrt(sum / K + eps), float64 [16]."""
    s = np.asarray(ssq_part, dtype=np.float64).reshape(-1, 16).sum(axis=0)
    return 1.0 / np.sqrt(s / K + float(eps))


def norm_bound(ref, bound, rstd, n_part):
    """`bound` on x W^T carried through the multiplication by rstd: the kernel sums n_part f32 partials (each addition 2^-24 of a sum of non-negative terms), divides,
    adds eps, takes sqrtf and the reciprocal (correctly rounded here or to 1 ulp: 8 roundings at most) and multiplies: |ref| (n_part + 8) 2^-24 on top."""
    return np.asarray(bound) * np.asarray(rstd)[:, None] + np.abs(ref) * (n_part + 8) * 2.0 ** -24


def rope64(pre, cos, sin):
    """Interleaved-pair RoPE: pre [M][2P], cos / sin [M][P] (the f32 table values, taken exactly) -> (2i, 2i + 1) = (a c - b s, b c + a s)."""
    a, b = pre[:, 0::2], pre[:, 1::2]
    out = np.empty_like(pre)
    out[:, 0::2] = a * cos - b * sin; out[:, 1::2] = b * cos + a * sin
    return out


def xf_bound(a, bound):
    """A value read back from XF planes (hi + lo): `bound` on the f32 value a plus the split's 2^-17 |a|."""
    return np.asarray(bound) + XF_SPLIT * np.abs(a)
