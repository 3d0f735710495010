"""The per-row Ada multiply of a stream group with a delay per member, one launch at a time (vox_debug_resid_xf: launch_q4_gemm's EPI_RESID_XF on the XF tile of the
rows -- the decode round's wo operator): row m of a per-row launch whose row -> set map is `order` equals row m of a per-column launch given scale set order[m], bit
for bit -- the f32 rows, the row's slots of the XF planes (hi and lo) and its sums of squares.

Cases: M in {1, 3, 16}; `order` a non-identity permutation of all sets and a strict subset of 16 sets (a burst's late decode round serves a prefix of the pass's order);
scale sets that differ in every column; and the smallest (K, N) that reach each form launch_q4_skinny picks for EPI_RESID_XF at 1..16 XF rows (n-tiles per wave is 1;
split-K over ks = 8 waves when N / 16 < 256 and K / 128 >= 16, else 4, 2 or 1; the straight-line forms run when K / 128 / ks is 4 or 9, the loop otherwise):
  (128, 128)   the loop, one K step, one wave;
  (512, 256)   the loop -- the tiny model's own wo (dec_heads 4 x 128 -> dec_dim 256);
  (4096, 128)  ks = 8, 4 steps per wave: the straight-line form the real model's wo runs (K = 4096);
  (9216, 128)  ks = 8, 9 steps per wave: the other straight-line form (the real model's w2 shape class).
The 17..48-row kernel (q4_skinny_mt_kernel) and the wide step never see a group's round: a group has at most 16 rows and runs the one-group chain."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128), (512, 256), (4096, 128), (9216, 128)]
N_SETS = 16
ORDERS = {1: [("subset", [7], 16)],
          3: [("perm", [2, 0, 1], 3), ("subset", [9, 2, 14], 16)],
          16: [("perm", [(5 * m + 3) % 16 for m in range(16)], 16)]}


class Desc(C.Structure):
    _fields_ = [("M", C.c_int32), ("n_sets", C.c_int32), ("set", C.c_int32), ("reserved", C.c_int32)]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: f"K{s[0]}_N{s[1]}")
def op(request, pkg, ctx):
    """One weight, its inputs for 16 rows and 16 scale sets per shape: made once, read-only."""
    K, N = request.param
    rng = np.random.default_rng(1000 + K + N)
    t = pkg.Q4Tensor.from_q4_bytes(pkg.synth.synth_q4_blocks(rng, N * K, 0.04), [N, K], ctx)
    x = rng.standard_normal((16, K)).astype(np.float32); resid = rng.standard_normal((16, N)).astype(np.float32)
    xf_w = (1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32)
    scales = (1.0 + 0.2 * rng.standard_normal((N_SETS, N))).astype(np.float32)
    for a in range(N_SETS):      # the sets differ in EVERY column
        for b in range(a):
            assert (scales[a] != scales[b]).all()
    for a in (x, resid, xf_w, scales):
        a.setflags(write=False)
    yield pkg, ctx, t, K, N, x, resid, xf_w, scales
    t.close()


def _run(op, M, n_sets, order=None, which=0):
    pkg, ctx, t, K, N, x, resid, xf_w, scales = op
    d = Desc(M, n_sets, which, 0)
    out = np.full((M, N), np.nan, np.float32); xf = np.zeros(2 * (N // 128) * 256 * 8, np.uint16); ssq = np.full((N // 16, 16), np.nan, np.float32)
    xs = np.ascontiguousarray(x[:M]); rs = np.ascontiguousarray(resid[:M]); sc = np.ascontiguousarray(scales[:n_sets])
    o = None if order is None else np.ascontiguousarray(order, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    code = pkg.lib().vox_debug_resid_xf(ctx.h, t.h, C.byref(d), p(xs), p(rs), p(xf_w), p(sc), None if o is None else p(o), p(out), p(xf), p(ssq))
    assert code == 0, (pkg.lib().vox_last_error() or b"").decode()
    # row m's slots of the planes: [hi | lo][K step and block][lane group][row][8 values]
    return out, xf.reshape(2, N // 32, 4, 16, 8), ssq


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


@pytest.mark.parametrize("M", [1, 3, 16])
def test_a_per_row_launch_is_the_per_column_launches_row_by_row(op, M):
    N = op[4]
    for name, order, n_sets in ORDERS[M]:
        assert len(order) == M and len(set(order)) == M and order != list(range(M))
        out, xf, ssq = _run(op, M, n_sets, order=order)
        assert np.isfinite(out).all() and np.isfinite(ssq).all()
        cols = {s: _run(op, M, n_sets, which=s) for s in sorted(set(order))}
        for m, s in enumerate(order):
            cout, cxf, cssq = cols[s]
            assert np.array_equal(_bits(out[m]), _bits(cout[m])), (name, m, "out")
            assert np.array_equal(xf[:, :, :, m, :], cxf[:, :, :, m, :]), (name, m, "XF planes")
            assert np.array_equal(_bits(ssq[:, m]), _bits(cssq[:, m])), (name, m, "sums of squares")
            assert xf[:, :, :, m, :].any()
        assert not xf[:, :, :, M:, :].any() and not _bits(ssq[:, M:]).any()      # rows >= M: nothing written
        # not vacuous: the set decides the planes -- a row under another row's set differs
        if M > 1:
            other = cols[order[1]][1]
            assert not np.array_equal(xf[:, :, :, 0, :], other[:, :, :, 0, :])


def test_refusals_touch_nothing(op):
    pkg, ctx, t, K, N, x, resid, xf_w, scales = op
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros((3, N), np.float32); xf = np.zeros(2 * (N // 128) * 256 * 8, np.uint16); ssq = np.zeros((N // 16, 16), np.float32)
    xs = np.ascontiguousarray(x[:3]); rs = np.ascontiguousarray(resid[:3]); sc = np.ascontiguousarray(scales[:3])
    for M, n_sets, order in ((3, 3, [0, 1, 3]), (3, 3, [0, -1, 2]), (17, 3, None), (3, 0, None)):
        d = Desc(M, n_sets, 0, 0); o = None if order is None else np.asarray(order, np.int32)
        code = pkg.lib().vox_debug_resid_xf(ctx.h, t.h, C.byref(d), p(xs), p(rs), p(xf_w), p(sc), None if o is None else p(o), p(out), p(xf), p(ssq))
        assert code == 1, (M, n_sets, order)      # VOX_ERR_INVALID: an order entry outside the sets never reaches the kernel
    assert not out.any() and not xf.any() and not ssq.any()
