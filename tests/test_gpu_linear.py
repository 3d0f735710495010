"""Every linear kernel behind vox_linear_forward_ex (q4_linear_dev -> launch_q4_gemv / launch_q4_gemm_epi, csrc/vox_kernels.hip) against a float64 reference
(tests/linear_ref.py, pinned on the CPU by tests/test_linear_ref.py): the dispatcher's row-count and workgroup-count edges, every fused epilogue of every kernel
form at ragged N, the block formats of real GGUF files, and activations with row scales, offsets and outlier channels.

Every case asserts WHICH kernel ran (vox_debug_gemm_launches), so a moved threshold cannot silently take a kernel out of the table; the last test of the module
fails if a form the operator entry can reach was never the asserted kernel of a passing case.

Error bars (derived, not measured; `pre` = x W^T + bias in float64, before the epilogue):
  * ordinary and row-scaled activations: per row i, |out_ij - ref_ij| <= 2e-5 max_j |pre_ij| -- the suite's f32-class bar, row by row instead of over the whole output;
  * offset and outlier activations, and the hostile block formats: componentwise |out_ij - ref_ij| <= 2^-16 mag_ij, mag_ij = sum_b 8 |d_jb| sum_{k in b} |x_ik|
    (dense: sum_k |x_ik| |w_jk|).  The kernels document the bf16 hi + lo activation split as |err| <= 2^-17 |x| (split_bf16x8), the weights are exact integers times
    an f16 scale, the accumulation is f32: 2^-16 leaves a factor 2 for the f32 sums.  The global 2e-5 max|ref| bar would be the wrong one here: with mu = 30 the useful
    product is a small difference of two large sums in the 128 + q kernels;
  * after an epilogue the bar is carried through it (linear_ref.carry_bound): |d gelu| <= 1.13 |d|, |d(silu(g) u)| <= 1.1 |u| |dg| + |silu(g)| |du|, + 4 ulp;
  * an all-zero activation row gives exactly zero (with a bias: epilogue(bias) to 1 ulp).
The worst error of every kernel form under both norms is printed by the last test (pytest -s) and recorded in DESIGN.md.

That the table can fail was checked once on an MI355X with six temporary value-only mutations (no address, guard or loop bound touched), each caught:
gate / up swapped in q4_skinny_kernel's SwiGLU -> epi-skinny e2; bias added after GELU in q4_gemm_k32_kernel -> epi-k32 e1b; the f16 scale's sign dropped in
q4_gemm_big_kernel -> the big SwiGLU rows (negated gate scales) and blocks-big (the synthetic generator's positive scales alone do not see it); the lo plane left out
of q4_skinny_mt_kernel's correction MFMA -> all 13 skinny_mt rows; a row's -136 sum(x) correction taken from its neighbour in the big kernel -> all 15 big rows;
M <= 48 -> M <= 47 in the dispatcher -> the six 48-row cases, by the launch-count assertion alone (the 16 x 64 tile kernel that ran instead is correct)."""
import zlib
from collections import namedtuple

import numpy as np
import pytest

from linear_ref import EPI_GELU, EPI_NONE, EPI_SWIGLU, LinearRef, activations, apply_epilogue, carry_bound
from model_fixtures import GEMM_FORMS, gemm_launches, gemm_launches_since

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ---- the kernel forms a case is expected to launch (vox_debug_gemm_launches names), helper launches included
def GV(r):
    return {f"gemv_r{r}": 1}


DGV, SK, K32, BIG, D2 = {"dense_gemv": 1}, {"skinny": 1}, {"k32": 1}, {"big": 1}, {"dense2": 1}
MT1 = {"xf_rows": 1, "skinny_mt": 1}                            # 17..48 rows, odd N: rows -> XF tiles, then the one-dimensional kernel
MT2 = {"xf_rows": 1, "skinny_mt2": 1, "splitk_finish": 1}       # 17..48 rows, even N: XF tiles, split-K planes, finishing sum + epilogue
T11, T12, T21B, T22B = {"tile_11": 1}, {"tile_12": 1}, {"tile_21_tb": 1}, {"tile_22_tb": 1}
HELPERS = ("xf_rows", "splitk_finish")
# what the operator entry cannot reach: the 32-row tile forms without the tile-ordered copy serve only the WFMT_BF16 weights of a bf16 checkpoint, which no operator
# entry creates.  COVERED_ELSEWHERE: the wide batched-decode GEMM and the big kernel's RoPE epilogue take XF planes / RoPE tables, which this entry does not pass --
# tests/test_gpu_xf_ops.py holds both to float64 through vox_debug_xf_op and asserts their forms in its own closing test
UNREACHABLE = {"tile_21", "tile_22"}
COVERED_ELSEWHERE = {"wide", "big_rope"}
NO_MT, NO_SK = {"VOX_NO_SKINNY_MT": "1"}, {"VOX_NO_SKINNY": "1"}

Case = namedtuple("Case", "fam M K N fmt epi bias act knobs B")
CASES = {}


def add(tag, fam, M, K, N, fmt="q4", epi=EPI_NONE, bias=False, act="ramp", knobs=None, B=1):
    cid = f"{tag}-{'+'.join(k for k in fam if k not in HELPERS)}-{B}x{M}x{K}x{N}-{fmt}-e{epi}{'b' if bias else ''}-{act}"
    assert cid not in CASES, cid
    CASES[cid] = Case(dict(fam), M, K, N, fmt, epi, bias, act, dict(knobs or {}), B)


def ceil_div(a, b):
    return -(-a // b)


# ---- the dispatcher's own thresholds (launch_q4_gemm_epi / gemm_launch_f): the shapes below are computed from them
BIG_MIN_WG = 200          # workgroups of 64 x 256 from which q4_gemm_big_kernel takes over (N % 256 == 0 only)
NT2_MIN_WG = 256          # 16-row tile forms: two n-tiles per wave from this many 16 x 128 workgroups
TB_NT2_MIN_WG = 128       # tile-ordered 32-row forms: two n-tiles per wave from this many 32 x 128 workgroups


def q4_rows_family(M, N, K):
    """Which Q4 kernel the row count picks (K % 128 == 0, N % 256 != 0 or too few workgroups for the big kernel, no knob) -- the M edges 4 | 5, 16 | 17, 48 | 49."""
    if M <= 4:
        raise AssertionError("GEMV rows: the rows-per-wave form depends on K and N, name it in the table")
    if M <= 16:
        return SK
    if M <= 48:
        return MT2 if N % 2 == 0 else MT1
    return T22B if ceil_div(N, 128) * ceil_div(M, 32) >= TB_NT2_MIN_WG else T21B


ROW_EDGES = [1, 2, 3, 4, 5, 15, 16, 17, 32, 33, 47, 48, 49, 63, 64, 65]

# 1. row-count edges: K = 3072 and 128, a ragged N and a model N.  GEMV rows per wave (q4_gemv_default_R): K = 3072 -> two rows fill the passes exactly (even N),
#    K = 128 -> one row per wave
for K_, gv in ((3072, GV(2)), (128, GV(1))):
    for N_ in (528 + 2, 1280):
        for M_ in ROW_EDGES:
            add("rows", gv if M_ <= 4 else q4_rows_family(M_, N_, K_), M_, K_, N_)
add("rows", MT2, 6, 3072, 530, B=3)              # B * M = 18 crosses 16 | 17
add("rows", SK, 4, 128, 530, B=4)                # B * M = 16
add("rows", GV(1), 2, 128, 530, B=2)             # B * M = 4
add("rows", MT1, 17, 128, 531)                   # odd N: no room for interleaved pairs in the planes' finishing kernel -> the one-dimensional form
add("rows", MT1, 48, 3072, 531)
add("rows", GV(1), 3, 3072, 531)                 # odd N: two rows per wave do not divide N -> one
add("rows", GV(4), 4, 512, 1060)                 # K = 512: four rows per wave fill one pass exactly
add("rows", GV(1), 3, 512, 1062)                 # ... unless N % 4 != 0: one row per wave
add("rows", MT1, 33, 128, 8209)                  # >= 512 column tiles: two n-tiles per wave in the one-dimensional 17..48-row kernel

# 2. the tile forms, each once just below and once just above its threshold, partial last row tile and partial last column tile (N % 256 != 0 keeps the big kernel away)
M_ = 65                                          # three 32-row tiles, the last with one row
n_lo, n_hi = 128 * (ceil_div(TB_NT2_MIN_WG, 3) - 1) - 126, 128 * (ceil_div(TB_NT2_MIN_WG, 3) - 1) + 2      # 42 / 43 column workgroups of 128
assert ceil_div(n_lo, 128) * 3 == 126 < TB_NT2_MIN_WG <= ceil_div(n_hi, 128) * 3 == 129 and n_lo % 64 and n_hi % 128 and n_lo % 2 == 0
add("tile", T21B, M_, 256, n_lo); add("tile", T22B, M_, 256, n_hi)
M_ = 38                                          # behind VOX_NO_SKINNY_MT: three 16-row tiles, the last with six rows
n_lo, n_hi = 128 * (ceil_div(NT2_MIN_WG, 3) - 1) - 2, 128 * (ceil_div(NT2_MIN_WG, 3) - 1) + 2            # 85 / 86 column workgroups
assert ceil_div(n_lo, 128) * 3 == 255 < NT2_MIN_WG <= ceil_div(n_hi, 128) * 3 == 258
add("tile", T11, M_, 128, n_lo, knobs=NO_MT); add("tile", T12, M_, 128, n_hi, knobs=NO_MT)
add("tile", T11, 11, 1280, 1062, knobs=NO_SK)   # <= 16 rows behind VOX_NO_SKINNY
add("tile", T11, 17, 3072, 530, knobs=NO_MT); add("tile", T11, 48, 3072, 530, knobs=NO_MT)

# 3. K % 128 != 0: the K-32 kernel at every row count above the GEMV's (such a weight has no tile-ordered copy and skips the skinny kernels)
for K_ in (32, 96, 160, 3104):
    for M_ in (5, 16, 17, 64, 65):
        add("k32", K32, M_, K_, 530)

# 4. the big kernel: taken without a knob at the first M with >= 200 workgroups of 64 x 256, a tile form one workgroup row below; N % 256 != 0 falls back
for N_, K_ in ((6144, 1280), (1280, 2048)):
    rows_wg = ceil_div(BIG_MIN_WG, N_ // 256)
    m_big, m_below = 64 * (rows_wg - 1) + 1, 64 * (rows_wg - 1)
    assert (N_ // 256) * ceil_div(m_big, 64) >= BIG_MIN_WG > (N_ // 256) * ceil_div(m_below, 64) and m_big % 64
    add("big", BIG, m_big, K_, N_); add("big", T22B, m_below, K_, N_)
add("big", T22B, 64 * (ceil_div(BIG_MIN_WG, 5) - 1) + 1, 2048, 1280 + 48)
add("big", BIG, 64 * ceil_div(BIG_MIN_WG, 24) + 37, 128, 6144)

# 5. the model's shapes at full N: decoder GEMVs, encoder / adapter (K, N)
MODEL_SHAPES = [(3072, 6144), (4096, 3072), (3072, 18432), (9216, 3072), (3072, 32), (32, 3072),
                (1280, 6144), (2048, 1280), (1280, 10240), (5120, 1280), (5120, 3072), (3072, 3072)]
MODEL_GEMV_R = {3072: 2, 4096: 1, 9216: 1, 32: 1, 1280: 1, 2048: 1, 5120: 2}      # q4_gemv_default_R: the R that fills every pass exactly, else one row per wave
for K_, N_ in MODEL_SHAPES:
    for M_ in (1, 3, 16, 38):
        add("model", GV(MODEL_GEMV_R[K_]) if M_ <= 4 else K32 if K_ % 128 else q4_rows_family(M_, N_, K_), M_, K_, N_)

# 6. one base shape per kernel form (ragged N, N / 2 odd and no multiple of any column tile where the form allows it): epilogues, block formats, activations
BASE = {          # name: (family, M, K, N, fmt, knobs)
    "gemv_r1": (GV(1), 3, 2048, 1062, "q4", None), "gemv_r2": (GV(2), 4, 3072, 1062, "q4", None),
    "gemv_r4": (GV(4), 4, 512, 1060, "q4", None),           # four rows per wave need N % 4 == 0: N / 2 = 530 is even, still no multiple of 16
    "skinny": (SK, 11, 1280, 1062, "q4", None), "skinny_mt": (MT1, 38, 1280, 1063, "q4", None), "skinny_mt2": (MT2, 38, 1280, 1062, "q4", None),
    "tile_11": (T11, 38, 1280, 1062, "q4", NO_MT), "tile_12": (T12, 38, 128, 10882, "q4", NO_MT),
    "tile_21_tb": (T21B, 65, 1280, 1062, "q4", None), "tile_22_tb": (T22B, 65, 256, 5378, "q4", None),
    "k32": (K32, 17, 160, 1062, "q4", None),
    "big": (BIG, 64 * ceil_div(BIG_MIN_WG, 24) + 1, 256, 6144, "q4", None),      # N % 256 == 0 is the kernel's condition: the ragged edge is M
    "dense_gemv": (DGV, 3, 1280, 1062, "dense", None), "dense2": (D2, 11, 1280, 1062, "dense", None),
}
for name, (fam, M_, K_, N_, fmt_, kn) in BASE.items():
    for epi_, bias_ in ((EPI_NONE, True), (EPI_GELU, False), (EPI_GELU, True), (EPI_SWIGLU, False)):
        f = fam
        if epi_ == EPI_SWIGLU:
            if name == "skinny_mt":
                continue                  # SwiGLU needs an even N, and an even N takes the split-K form: the one-dimensional kernel's SwiGLU has no operator entry
            if name == "gemv_r1":
                f = GV(2)                 # a gate / up pair needs an even number of rows per wave: the GEMV's SwiGLU runs two rows per wave at this shape
        add("epi-" + name, f, M_, K_, N_, fmt_, epi_, bias_, knobs=kn)
    if fmt_ == "q4":
        add("blocks-" + name, fam, M_, K_, N_, "q4h", knobs=kn)
        add("blocks-" + name, fam, M_, K_, N_, "q4h", EPI_GELU, True, knobs=kn)
    for act_ in ("scales", "offset3", "offset30", "abs", "outlier"):
        add("act-" + name, fam, M_, K_, N_, fmt_, act=act_, knobs=kn)
add("epi-gemv_r2", GV(2), 3, 512, 1062, epi=EPI_SWIGLU)            # N % 4 != 0 at K = 512: pairs on two rows per wave
add("act-skinny_mt2", MT2, 48, 3072, 530, act="scales", bias=True)      # three full 16-row groups, zero row with bias
add("act-tile_21_tb", T21B, 65, 1280, 1062, epi=EPI_GELU, bias=True, act="scales")
add("act-big", BIG, 64 * ceil_div(BIG_MIN_WG, 24) + 1, 256, 6144, epi=EPI_SWIGLU, act="scales")

# 7. the dense twins (Q4Tensor.from_f32): rows 1..4 dense_gemv_kernel, rows >= 5 dense2_gemm_kernel (K % 128 != 0: its partial-last-step form); ragged even N
for K_ in (32, 1280, 5120, 10240):
    for M_ in ROW_EDGES:
        add("dense", DGV if M_ <= 4 else D2, M_, K_, 530, "dense")
for K_ in (32, 5120, 10240):          # (K = 1280: the epilogue rows of BASE)
    for fam_, M_ in ((DGV, 3), (D2, 11)):
        add("dense", fam_, M_, K_, 1062, "dense", EPI_GELU, True)
        add("dense", fam_, M_, K_, 1062, "dense", EPI_SWIGLU)
add("dense", D2, 6, 1280, 530, "dense", B=3)
add("dense", D2, 65, 96, 531, "dense", bias=True)                   # odd N is the GEMV's limit only
add("dense", D2, 7, 160, 1062, "dense", EPI_SWIGLU)
add("dense", D2, 64 * 4 + 3, 256, 128 * 100 + 2, "dense", EPI_GELU, True)      # >= 400 workgroups of 64 x 128: two n-tiles per wave

OFFSET_ACTS = ("offset3", "offset30", "abs", "outlier")


def hostile_q4_blocks(rng, n_elems, row_blocks=None):
    """Raw Q4_0 blocks with what real GGUF files hold and the synthetic generator (nibbles 1..15, positive scales) does not: nibbles uniform in 0..15 with a forced
    share of all-0 and all-15 blocks (a llama.cpp-style quantiser, d = max / -8, produces nibble 0 and negative d), and f16 scales from
    {ordinary positive, ordinary negative, +0, -0, the f16 subnormals 0x0001 and 0x03FF, small normal, large ~2^10} -- finite only.  row_blocks (= K / 32): every
    fourth weight row holds ONE scale class in all its blocks, so that a kernel which flushes a subnormal scale, or drops a sign, loses a whole output column."""
    nb = n_elems // 32
    out = np.empty((nb, 18), dtype=np.uint8)
    out[:, 2:] = rng.integers(0, 256, (nb, 16), dtype=np.uint8)
    kind = rng.integers(0, 16, nb)
    out[kind == 0, 2:] = 0x00; out[kind == 1, 2:] = 0xFF
    cls = rng.integers(0, 8, nb)
    if row_blocks:
        rows = nb // row_blocks
        c2 = cls.reshape(rows, row_blocks)
        c2[1::4] = (np.arange(len(c2[1::4])) % 8)[:, None]
    u = 0.5 + rng.random(nb)
    d = np.select([cls == 0, cls == 1, cls == 6, cls == 7], [0.01 * u, -0.01 * u, 2.0 ** -14 * (u + 0.5), 1024.0 * u], 0.0).astype(np.float16)
    bits = d.view(np.uint16).copy()
    bits[cls == 2] = 0x0000; bits[cls == 3] = 0x8000; bits[cls == 4] = 0x0001; bits[cls == 5] = 0x03FF
    assert np.isfinite(bits.view(np.float16)).all()
    out[:, 0:2] = bits.view(np.uint8).reshape(nb, 2)
    return out.reshape(-1)


def _scale_up_rows(raw, N, K, factor=3.0):
    """Interleaved gate / up rows that a swapped pair cannot survive: the f16 scales of the up rows (odd) times 3, the gate rows' (even) negated."""
    b = raw.reshape(N, K // 32, 18)
    d = np.ascontiguousarray(b[:, :, :2]).view(np.float16).reshape(N, K // 32).astype(np.float32)
    d[1::2] *= factor; d[0::2] *= -1.0
    b[:, :, :2] = d.astype(np.float16).view(np.uint8).reshape(N, K // 32, 2)
    return b.reshape(-1)


_WEIGHTS = {}          # one entry: the last (fmt, N, K, swiglu) -> (LinearRef, device tensor); the model-shape cases reuse it across their row counts


def weights(pkg, ctx, fmt, N, K, swiglu):
    key = (fmt, N, K, swiglu)
    if key in _WEIGHTS:
        return _WEIGHTS[key]
    for _, t in _WEIGHTS.values():
        t.close()
    _WEIGHTS.clear()
    rng = np.random.default_rng([zlib.crc32(repr(key).encode()), 1])
    if fmt == "dense":
        w = (0.03 * rng.standard_normal((N, K))).astype(np.float32)
        if swiglu:
            w[1::2] *= 3.0; w[0::2] += np.float32(0.01)
            t = pkg.Q4Tensor.from_f32(np.ascontiguousarray(w[0::2]), ctx, other=np.ascontiguousarray(w[1::2]))
        else:
            t = pkg.Q4Tensor.from_f32(w, ctx)
        ref = LinearRef(w, N, K)
    else:
        raw = hostile_q4_blocks(rng, N * K, K // 32) if fmt == "q4h" else pkg.synth.synth_q4_blocks(rng, N * K, 0.04)
        if swiglu:
            raw = _scale_up_rows(raw, N, K)
        t = pkg.Q4Tensor.from_q4_bytes(raw, [N, K], ctx)
        ref = LinearRef(raw, N, K)
    assert t.shape() == [N, K]
    _WEIGHTS[key] = (ref, t)
    return ref, t


WORST = {}             # kernel form -> {"ordinary" / "hostile" / an offset activation: [worst |err| / its row's max, worst |err| / mag]}, cases without an epilogue
PASSED, ASSERTED = set(), set()


def run_case(pkg, ctx, c, monkeypatch):
    for k, v in c.knobs.items():
        monkeypatch.setenv(k, v)
    rows = c.B * c.M
    ref_w, t = weights(pkg, ctx, c.fmt, c.N, c.K, c.epi == EPI_SWIGLU)
    rng = np.random.default_rng([zlib.crc32(repr(tuple(c)).encode()), 2])
    x, zrow = activations(rng, c.act, rows, c.K)
    bias = rng.standard_normal(c.N).astype(np.float32) if c.bias else None
    before = gemm_launches(pkg)
    out = pkg.linear_forward(t, x.reshape(c.B, c.M, c.K), bias, c.epi)
    ran = gemm_launches_since(pkg, before)
    No = c.N // 2 if c.epi == EPI_SWIGLU else c.N
    assert out.shape == (c.B, c.M, No) and np.isfinite(out).all()
    assert ran == c.fam, f"expected {c.fam}, the dispatcher ran {ran}"
    out = out.reshape(rows, No).astype(np.float64)
    ref, pre, rowmax, mag = ref_w(x, bias, c.epi)
    err = np.abs(out - ref)
    pre_err_row = (err.max(axis=1) / np.maximum(rowmax, 1e-300)).max() if c.epi == EPI_NONE else float("nan")
    pre_err_mag = (err / np.maximum(mag, 1e-300))[mag > 0].max() if c.epi == EPI_NONE else float("nan")
    form = next(k for k in c.fam if k not in HELPERS)
    print(f"{form}: {c.B}x{c.M} rows, K {c.K}, N {c.N}, {c.fmt}, epilogue {c.epi}, bias {c.bias}, {c.act}: worst |err| {pre_err_row:.2e} of its row's max, {pre_err_mag:.2e} of mag")
    if c.epi == EPI_NONE:
        w = WORST.setdefault(form, {}).setdefault(c.act if c.act in OFFSET_ACTS else "hostile" if c.fmt == "q4h" else "ordinary", [0.0, 0.0])
        w[0] = max(w[0], pre_err_row); w[1] = max(w[1], pre_err_mag)
    per_row = carry_bound(pre, 2e-5 * rowmax[:, None], c.epi)
    per_elem = carry_bound(pre, 2.0 ** -16 * mag, c.epi)
    if c.act in OFFSET_ACTS:
        bad = err > per_elem
        assert not bad.any(), f"{int(bad.sum())} elements past 2^-16 mag, worst {(err / np.maximum(per_elem, 1e-300)).max():.2f} x the bound at {np.unravel_index(np.argmax(err / np.maximum(per_elem, 1e-300)), err.shape)}"
    else:
        bad = err > per_row
        assert not bad.any(), f"{int(bad.sum())} elements past 2e-5 of their row's max, worst {(err / np.maximum(per_row, 1e-300)).max():.2f} x the bound at {np.unravel_index(np.argmax(err / np.maximum(per_row, 1e-300)), err.shape)}"
        if c.fmt == "q4h" and bias is None and c.epi == EPI_NONE:
            # mixed scale classes: the row's max belongs to the 2^10 blocks, so a lost subnormal column only shows componentwise.  (Without bias and epilogue only:
            # next to a bias of order 1 the f32 rounding of acc + bias alone is 2^-24, far above 2^-16 of a subnormal column's mag.)
            bad = err > per_elem
            assert not bad.any(), f"{int(bad.sum())} elements past 2^-16 mag, worst {(err / np.maximum(per_elem, 1e-300)).max():.2f} x the bound"
    if zrow is not None:
        if bias is None:
            assert (out[zrow] == 0.0).all(), "an all-zero activation row must give exactly zero"
        else:
            # epilogue(bias) as the library evaluates it: the same operator on a single all-zero row (another kernel form, the same gelu_f).  Not the float64 value:
            # the reference's GELU form x/2 (1 + erf(x / sqrt 2)) cancels in the negative tail, so no f32 evaluation of it is within 1 ulp of the float64 result
            # (measured here: 72 ulp over N(0, 1) biases); against float64 the zero row is held to that form's own rounding,
            # |b| 2^-22 (erff to 4 ulp of a value below 1, the sum 1 + erf, the argument's rounding) + 2 ulp of the result.
            want = pkg.linear_forward(t, np.zeros((1, 1, c.K), np.float32), bias, c.epi).reshape(No).astype(np.float64)
            ulps = np.abs(out[zrow] - want) / np.spacing(np.abs(want).astype(np.float32))
            w64 = apply_epilogue(bias.astype(np.float64)[None, :], c.epi)[0]
            print(f"zero row with bias, epilogue {c.epi}: {ulps.max():.1f} ulp from the library's epilogue(bias), "
                  f"{(np.abs(out[zrow] - w64) / np.spacing(np.abs(w64).astype(np.float32))).max():.1f} ulp from the float64 value")
            assert (ulps <= 1.0).all(), "an all-zero activation row must give epilogue(bias) to 1 ulp"
            if c.epi == EPI_NONE:
                assert (out[zrow] == bias).all()
            assert (np.abs(out[zrow] - w64) <= 2.0 ** -22 * np.abs(bias) + 2 * np.spacing(np.abs(w64).astype(np.float32))).all()
    ASSERTED.update(c.fam)


@pytest.mark.parametrize("cid", list(CASES))
def test_linear_case(pkg, orc, ctx, monkeypatch, cid):
    """One row of the table above: the expected kernel form ran (and nothing else), the output meets the module's error bars."""
    run_case(pkg, ctx, CASES[cid], monkeypatch)
    PASSED.add(cid)


def test_hostile_blocks_dequantize_bit_exact(pkg, orc, ctx):
    """The repack and the tile-ordered copy keep every block of hostile_q4_blocks bit for bit (negative, zero, subnormal and large scales, nibbles 0 and 15)."""
    rng = np.random.default_rng(11)
    for n, k in ((16, 32), (130, 1280), (3, 3072), (64, 96)):
        raw = hostile_q4_blocks(rng, n * k, k // 32)
        d = np.ascontiguousarray(raw.reshape(-1, 18)[:, :2]).view(np.uint16).reshape(-1)
        q = raw.reshape(-1, 18)[:, 2:]
        if n * k >= 4096:
            assert {0x0000, 0x8000, 0x0001, 0x03FF} <= set(d.tolist()) and (q == 0).all(axis=1).any() and (q == 0xFF).all(axis=1).any()
        t = pkg.Q4Tensor.from_q4_bytes(raw, [n, k], ctx)
        a, b = np.ascontiguousarray(t.dequantize().reshape(-1)), orc.q4_dequantize(raw, n * k)
        assert (a.view(np.uint32) == b.view(np.uint32)).all()
        t.close()


def test_linear_limits_are_clean_errors(pkg, orc, ctx):
    """What the operators do not support ends in a VoxError before anything is launched, and the context stays usable: the dense GEMV's K <= 10240 and even N
    (rows <= 4; the same tensors at 5 rows run on dense2_gemm_kernel), SwiGLU with an odd N or with a bias, a K mismatch."""
    rng = np.random.default_rng(5)

    def refused(fn):
        before = gemm_launches(pkg)
        with pytest.raises(pkg.VoxError):
            fn()
        assert gemm_launches_since(pkg, before) == {}

    def works(t, ref, rows, K, fam, bias=None, epi=EPI_NONE):
        x = rng.standard_normal((1, rows, K)).astype(np.float32)
        before = gemm_launches(pkg)
        out = pkg.linear_forward(t, x, bias, epi)
        assert gemm_launches_since(pkg, before) == fam
        r, pre, rowmax, _ = ref(x, bias, epi)
        assert (np.abs(out[0] - r) <= carry_bound(pre, 2e-5 * rowmax[:, None], epi)).all()

    for N, K in ((530, 10272), (531, 128)):
        w = (0.03 * rng.standard_normal((N, K))).astype(np.float32)
        t = pkg.Q4Tensor.from_f32(w, ctx); ref = LinearRef(w, N, K)
        for rows in (1, 4):
            refused(lambda: pkg.linear_forward(t, np.ones((1, rows, K), np.float32)))
        works(t, ref, 5, K, D2)
        refused(lambda: pkg.linear_forward(t, np.ones((1, 2, K + 32), np.float32)))
        if N % 2:
            refused(lambda: pkg.linear_forward(t, np.ones((1, 5, K), np.float32), None, EPI_SWIGLU))
        t.close()
    N, K = 531, 256
    raw = pkg.synth.synth_q4_blocks(rng, N * K, 0.04); t = pkg.Q4Tensor.from_q4_bytes(raw, [N, K], ctx); ref = LinearRef(raw, N, K)
    for rows in (1, 5, 17, 65):
        refused(lambda: pkg.linear_forward(t, np.ones((1, rows, K), np.float32), None, EPI_SWIGLU))
        refused(lambda: pkg.linear_forward(t, np.ones((1, rows, K - 32), np.float32)))
        refused(lambda: pkg.q4_matmul(np.ones((1, rows, K + 32), np.float32), t))
    works(t, ref, 5, K, SK)
    t.close()
    N = 530
    raw = pkg.synth.synth_q4_blocks(rng, N * K, 0.04); t = pkg.Q4Tensor.from_q4_bytes(raw, [N, K], ctx); ref = LinearRef(raw, N, K)
    b = rng.standard_normal(N).astype(np.float32)
    for rows in (2, 9, 38, 70):
        refused(lambda: pkg.linear_forward(t, np.ones((1, rows, K), np.float32), b, EPI_SWIGLU))
        refused(lambda: pkg.linear_forward(t, np.ones((1, rows, K), np.float32), b[:-1]))
    refused(lambda: pkg.linear_forward(t, np.ones((1, 2, K), np.float32), None, 3))
    works(t, ref, 38, K, MT2, b, EPI_GELU)
    works(t, ref, 2, K, GV(2), None, EPI_SWIGLU)
    t.close()


def test_every_reachable_form_was_asserted():
    """Every row of the table ran and passed, and every kernel form of vox_debug_gemm_launches that the operator entry can reach was the asserted form of a passing
    case (UNREACHABLE and COVERED_ELSEWHERE name the rest, with the reason).  Prints the worst error of every form under both norms."""
    for form in sorted(WORST):
        for kind, (r, m) in sorted(WORST[form].items()):
            print(f"worst error, {form:12s} {kind:8s}: {r:.2e} of the row's max, {m:.2e} of mag (2^-16 = {2.0 ** -16:.2e})")
    for k in _WEIGHTS.values():
        k[1].close()
    _WEIGHTS.clear()
    assert set(CASES) == PASSED, f"{len(set(CASES) - PASSED)} rows of the table did not pass: {sorted(set(CASES) - PASSED)[:8]}"
    missing = set(GEMM_FORMS) - UNREACHABLE - COVERED_ELSEWHERE - ASSERTED
    assert not missing, f"no passing case asserted {sorted(missing)}"
