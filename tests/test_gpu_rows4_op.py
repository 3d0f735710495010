"""The fused tick's four-row operator (csrc/vox_rows4.hip), one launch at a time through vox_debug_rows4_op (pkg.rows4_forward) against float64 (tests/linear_ref.py;
with the fused norm the reference is the float64 RMSNorm, then the float64 product).  Error bars: tests/test_gpu_linear.py's own, carried through the epilogue by
linear_ref.carry_bound -- per row 2e-5 max_j |pre_ij| for ordinary and row-scaled activations, componentwise 2^-16 mag_ij for offset and outlier activations (the
residual is added to the reference behind them).  An all-zero row gives exact zeros (+ the residual); with a bias, epi(bias): bit for bit for store / residual, for
SwiGLU within 1 ulp of the same operator on a single zero row and within carry_bound's 4 ulp of the float64 value.  Every case counts exactly one launch.
Shapes, all crossed with the twelve pro x epi x bias forms: M in {1, 3, 4}; N in {16, 48}; K in {32, 96, 160} (one block; an odd number of blocks: a K step with an
empty second block; three steps, one per wave), 256 (the tiny model's FFN width), 608 (19 blocks, 10 steps, two per wave: the in-wave loop and its prefetch, the pad
block in a two-step wave, waves 5..7 empty) and 1280 (the encoder width: three steps per wave, wave 6 has two, wave 7 none).  Twice K = 5120, the FFN width: ten
steps per wave, LDS past the default 64 KiB.  N = 8240 = 515 tiles, three more than the grid's 512 workgroups.  No Q4 tensor with K % 32 != 0 can be made (refused
where the tensor is made), so the operator's own K % 32 check cannot be reached from here: the K = 48 case shows that refusal."""
import numpy as np
import pytest

from linear_ref import EPI_NONE, EPI_SWIGLU, ULP32, LinearRef, activations, carry_bound

pytestmark = pytest.mark.gpu
STORE, RESID, SWIGLU, EPS, OFFSET_ACTS = 0, 1, 2, 1e-5, ("offset30", "outlier")
FORMS = [(pro, epi, bias) for pro in (0, 1) for epi in (STORE, RESID, SWIGLU) for bias in (False, True)]
CASES = [(M, K, N) + f + ("ramp", False) for K in (32, 96, 160, 256, 608, 1280) for N in (16, 48) for M in (1, 3, 4) for f in FORMS]
CASES += [(4, 5120, 48, 0, RESID, True, "ramp", False), (3, 5120, 16, 1, SWIGLU, False, "ramp", False)] + [(4, 96, 8240) + f + ("ramp", False) for f in FORMS]
CASES += [(4, 160, 48, pro, epi, bias, "scales", False) for pro, epi, bias in ((0, STORE, False), (1, STORE, True), (0, RESID, True), (1, RESID, False), (1, SWIGLU, True), (0, SWIGLU, False))] + [(3, 160, 48, pro, epi, True, act, False) for act in OFFSET_ACTS for pro, epi in ((0, STORE), (1, SWIGLU))]
CASES += [(4, 96, 48, 1, RESID, True, "ramp", True)]          # a block of all-0xF nibbles under a negative f16 scale, in every weight row
WORST = {}          # (pro, epi) -> worst |err| of the row's max, of mag: printed with every case (pytest -s; DESIGN.md records them)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("M,K,N,pro,epi,bias,act,hostile", CASES, ids=lambda v: v if isinstance(v, str) else str(int(v)))
def test_rows4_case(pkg, orc, ctx, M, K, N, pro, epi, bias, act, hostile):
    rng = np.random.default_rng([M, K, N, pro, epi, int(bias), len(act), int(hostile)])
    raw = pkg.synth.synth_q4_blocks(rng, N * K, 0.04).reshape(N, K // 32, 18).copy()
    if hostile:
        raw[:, K // 64, 2:] = 0xFF; raw[:, K // 64, :2] = np.array([-0.02], np.float16).view(np.uint8)
    raw = raw.reshape(-1); t = pkg.Q4Tensor.from_q4_bytes(raw, [N, K], ctx); ref_w = LinearRef(raw, N, K)
    x, zrow = activations(rng, act, M, K)
    b = rng.standard_normal(N).astype(np.float32) if bias else None; gamma = (1.0 + 0.2 * rng.standard_normal(K)).astype(np.float32) if pro else None
    resid = rng.standard_normal((M, N)).astype(np.float32) if epi == RESID else None
    before = pkg.rows4_launches()
    out = pkg.rows4_forward(t, x, b, gamma, EPS, epi, resid).astype(np.float64)
    assert pkg.rows4_launches() == before + 1
    xn = x.astype(np.float64); ref_epi = EPI_SWIGLU if epi == SWIGLU else EPI_NONE
    if pro:
        xn = xn / np.sqrt((xn * xn).mean(axis=1, keepdims=True) + EPS) * gamma.astype(np.float64)[None, :]
    ref, pre, rowmax, mag = ref_w(xn, b, ref_epi)
    ref = ref + resid.astype(np.float64) if epi == RESID else ref
    assert out.shape == ref.shape and np.isfinite(out).all()
    err = np.abs(out - ref)
    bound = carry_bound(pre, 2.0 ** -16 * mag if act in OFFSET_ACTS else 2e-5 * rowmax[:, None], ref_epi)
    if epi != SWIGLU:
        w = WORST.setdefault((pro, epi), [0.0, 0.0])
        w[0] = max(w[0], float((err.max(axis=1) / np.maximum(rowmax, 1e-300)).max())); w[1] = max(w[1], float((err / np.maximum(mag, 1e-300))[mag > 0].max(initial=0.0)))
    ratio = err / np.maximum(bound, 1e-300)
    print(f"rows4 pro {pro} epi {epi} bias {bias} {M}x{K}x{N} {act}: worst |err| {ratio.max():.3f} of its bound; so far (row's max, mag) {WORST.get((pro, epi))}")
    assert not (err > bound).any(), f"{int((err > bound).sum())} elements past the bound, worst {ratio.max():.2f} x at {np.unravel_index(np.argmax(ratio), err.shape)}"
    if zrow is not None:
        if b is None:
            assert (out[zrow] == (resid[zrow] if epi == RESID else 0.0)).all(), "an all-zero activation row must give exactly zero (+ the residual)"
        elif epi == SWIGLU:
            one = pkg.rows4_forward(t, np.zeros((1, K), np.float32), b, gamma, EPS, epi).astype(np.float64)[0]
            assert (np.abs(out[zrow] - one) <= np.spacing(np.abs(one).astype(np.float32))).all() and (np.abs(out[zrow] - ref[zrow]) <= 4 * ULP32 * np.abs(ref[zrow])).all()
        else:
            assert (out[zrow] == (b + resid[zrow] if epi == RESID else b)).all(), "an all-zero activation row must give epi(bias)"
    t.close()


@pytest.mark.parametrize("what", ["M5", "K48", "dense"])
def test_rows4_refusals(pkg, orc, ctx, what):          # what the operator does not serve is a clean VoxError and counts no launch
    rng = np.random.default_rng(3); before = pkg.rows4_launches()
    if what == "K48":          # no whole number of Q4 blocks: refused where the tensor is made, so no such tensor ever reaches the operator
        with pytest.raises(pkg.VoxError):
            pkg.Q4Tensor.from_q4_bytes(pkg.synth.synth_q4_blocks(rng, 16 * 64, 0.04)[:16 * 48 // 32 * 18], [16, 48], ctx)
    else:
        t = pkg.Q4Tensor.from_f32((0.03 * rng.standard_normal((16, 64))).astype(np.float32), ctx) if what == "dense" else pkg.Q4Tensor.from_q4_bytes(pkg.synth.synth_q4_blocks(rng, 16 * 64, 0.04), [16, 64], ctx)
        with pytest.raises(pkg.VoxError):
            pkg.rows4_forward(t, np.ones((5 if what == "M5" else 2, 64), np.float32))
    assert pkg.rows4_launches() == before
