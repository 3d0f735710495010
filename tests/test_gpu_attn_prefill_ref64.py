"""The MFMA prefill attention at head_dim 64 (attn_prefill_mfma_kernel<64, false>, through vox_attention) against a float64 softmax written here, on chains of one to ten key
tiles with offsets, windows that start inside a tile and queries for which whole tiles are masked; and the property any re-partition of its key loop has to keep: a query
row's bits do not depend on the launch geometry (M, which rows share its workgroup, where its block's first tile lies).  Bar: |out - ref| <= 2e-5 max|ref|, the one
tests/test_gpu_ops.py holds the kernel to."""
from importlib import import_module

import numpy as np
import pytest

from model_fixtures import attn_launches, launches_since

pytestmark = pytest.mark.gpu

HD = 64
BAR = 2e-5
# (M, kv_len, offset, window)
CASES = [
    (1, 1, 0, -1),            # one key
    (17, 17, 0, -1),          # one tile; ragged wave
    (64, 128, 64, -1),        # exactly two tiles
    (70, 200, 130, -1),       # four tiles; a 6-row second query block
    (130, 190, 60, 64),       # window start not on a tile edge; whole tiles outside the window for late queries
    (40, 300, 260, 16),       # most tiles hold no visible key for a query: running max stays -inf across them
    (100, 586, 486, -1),      # ten tiles: the single clip's longest chain
]
GQA = [(2, 2), (2, 1)]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _inputs(kv, H, KV, seed):
    """q for every key position (a launch takes the rows of its own positions), k, v."""
    rng = np.random.default_rng(seed)
    q = (rng.standard_normal((kv, H * HD)) * 1.5).astype(np.float32)
    k = (rng.standard_normal((kv, KV * HD)) * 1.5).astype(np.float32)
    v = rng.standard_normal((kv, KV * HD)).astype(np.float32)
    return q, k, v


def _ref64(q, k, v, H, KV, off, win):
    """softmax(q k^T / sqrt(hd) + mask) v in float64: query m at position off + m sees keys j <= off + m with off + m - j <= win (win < 0: no window)."""
    M, kv = q.shape[0], k.shape[0]
    pos = off + np.arange(M)[:, None]; j = np.arange(kv)[None, :]
    vis = j <= pos
    if win >= 0:
        vis &= (pos - j) <= win
    out = np.zeros((M, H * HD))
    for h in range(H):
        g = h // (H // KV)
        s = q[:, h * HD:(h + 1) * HD].astype(np.float64) @ k[:, g * HD:(g + 1) * HD].astype(np.float64).T / np.sqrt(HD)
        s = np.where(vis, s, -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        out[:, h * HD:(h + 1) * HD] = (p / p.sum(axis=1, keepdims=True)) @ v[:, g * HD:(g + 1) * HD].astype(np.float64)
    return out


@pytest.mark.parametrize("H,KV", GQA)
@pytest.mark.parametrize("M,kv,off,win", CASES)
def test_prefill_attention_vs_float64(pkg, ctx, M, kv, off, win, H, KV):
    attention = import_module(pkg.__name__ + ".gguf").attention
    qall, k, v = _inputs(kv, H, KV, 1000 * M + kv + KV)
    q = np.ascontiguousarray(qall[off:off + M])
    ref = _ref64(q, k, v, H, KV, off, win)
    before = attn_launches(pkg)
    out = attention(ctx, q, k, v, H, KV, offset=off, window=win)
    assert launches_since(pkg, before) == {"prefill_mfma": 1}
    assert np.isfinite(out).all()
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"prefill attention M {M} kv {kv} offset {off} window {win} heads {H}:{KV}: {err:.2e} of the largest")
    assert err <= BAR, err


@pytest.mark.parametrize("first", [64, 40])
@pytest.mark.parametrize("H,KV", GQA)
def test_rows_do_not_depend_on_the_launch_geometry(pkg, ctx, H, KV, first):
    """Rows first .. 129 of the windowed case launched alone (same K / V) equal the full launch's rows bit for bit.  first = 64: the full launch's last two query blocks on
    their own (another grid).  first = 40: the rows are cut into other query blocks and waves than in the full launch, and the first block starts at another key tile
    (j_lo 36 against 0 and 60), so tiles that are wholly masked for a row come and go around it."""
    attention = import_module(pkg.__name__ + ".gguf").attention
    M, kv, off, win = CASES[4]
    qall, k, v = _inputs(kv, H, KV, 1000 * M + kv + KV)
    full = attention(ctx, np.ascontiguousarray(qall[off:off + M]), k, v, H, KV, offset=off, window=win)
    part = attention(ctx, np.ascontiguousarray(qall[off + first:off + M]), k, v, H, KV, offset=off + first, window=win)
    assert part.shape == (M - first, H * HD)
    assert np.array_equal(part.view(np.uint32), full[first:].view(np.uint32)), np.abs(part - full[first:]).max()
