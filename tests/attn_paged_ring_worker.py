"""Worker of tests/test_gpu_attn_decode_paged_ring.py: its tests run through pytest in a process of their own (worker_tests.run_worker) -- they launch the paged attention on ring
page tables, whose launch counts (vox_debug_attn_launches [14] [15]) the suite's other tests hold to 0 in their own process.  Not collected by the suite (no test_ prefix).

The paged decode attention on a RING page table (AttnParams::page_tab_len, attn_stage_pages' ring index), one launch at a time through
vox_debug_attn_decode_paged_ring: logical page q of a sequence is entry q % L of its table row.  The reference is the flat-table paged launch of the same build on the
same keys in the same physical pages -- the paged kernels' arithmetic depends on the key's index inside the window alone, so the claim is np.array_equal on the f32
output viewed as uint32, no tolerance.  A position past what a flat table can express (its stride ends at 1024 pages) is compared with the flat launch at the position
of the same row-in-page whose window is as full: the same keys, the same page structure, other logical page numbers.

Both forms (per-head: 4 heads on 2 KV heads; GQA: 8 on 2), pages of 16 rows, a window of 255 (256 keys: up to 17 pages), L in {19, 32} -- 19 the least the entry
admits, and no power of two.  Every table entry outside a window's pages is -1 and every pool page no window names is NaN: a stray read shows.  Each launch moves its
own counter slot ([14] per-head, [15] GQA) by exactly one and leaves the flat forms' slots [11] [12] alone."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HD, P, W, KV = 128, 16, 255, 2
SLOTS = {"head": (4, 14, 11), "gqa": (8, 15, 12)}      # query heads, the ring form's counter slot, the flat form's


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _counts(pkg):
    a = (C.c_uint64 * 16)()
    assert pkg.lib().vox_debug_attn_launches(a, 16) == 0
    return [int(x) for x in a]


def positions(L):
    """The staged span (logical pages (p - 255) // 16 .. p // 16) starts at entry 0, ends at entry L - 1, straddles the wrap at p = 16 L k + {0, 1, 15, 16, 17} for
    k = 1, 3, sits at the run's start (no wrap yet, a window not yet full) and at the last position of a session."""
    ps = [40, 255, 256, 300]
    ps += [16 * L * 2 + 255, 16 * L * 2 + 255 + 7]                          # first page at entry 0
    ps += [16 * L * 2 + 16 * (L - 1), 16 * L * 4 + 16 * (L - 1) + 15]      # last page at entry L - 1
    ps += [16 * L * k + r for k in (1, 3) for r in (0, 1, 15, 16, 17)]     # straddling the wrap
    ps += [(1 << 24) - 1]
    for p in ps[4:8]:
        q0, q1 = (p - W) // P, p // P
        assert q0 % L == 0 or q1 % L == L - 1
    for p in ps[8:18]:
        assert ((p - W) // P) % L > (p // P) % L      # the span wraps
    return ps


def flat_twin(p):
    """A position a flat table of 64 entries expresses, with p's row-in-page and as full a window: the same keys in the same page structure."""
    return p if p < 64 * P else 20 * P + p % P


def build(L, H, seed):
    rng = np.random.default_rng([seed, L, H])
    ps = positions(L); n = len(ps)
    pool_pages = 17 * n + 5
    free = list(rng.permutation(pool_pages))
    k = np.full((pool_pages, KV, P, HD), np.nan, np.float32); v = k.copy()
    ring = np.full((n, L), -1, np.int32); flat = np.full((n, 64), -1, np.int32); fpos = []
    for s, p in enumerate(ps):
        f = flat_twin(p); fpos.append(f)
        q0, q1 = max(0, p - W) // P, p // P; f0 = max(0, f - W) // P
        assert q1 - q0 == f // P - f0 and (p - max(0, p - W)) == (f - max(0, f - W)) and p % P == f % P
        for q in range(q0, q1 + 1):
            page = int(free.pop())
            k[page] = rng.standard_normal((KV, P, HD)).astype(np.float32); v[page] = rng.standard_normal((KV, P, HD)).astype(np.float32)
            assert ring[s, q % L] == -1      # L entries hold a window's pages without collision
            ring[s, q % L] = page; flat[s, q - q0 + f0] = page
    q = (1.5 * rng.standard_normal((n, H * HD))).astype(np.float32)
    return ps, fpos, q, k, v, ring, flat


@pytest.mark.parametrize("L", [19, 32])
@pytest.mark.parametrize("kind", ["head", "gqa"])
def test_ring_table_equals_flat_table_bit_for_bit(pkg, ctx, kind, L):
    gg = pkg.gguf; H, slot, flat_slot = SLOTS[kind]
    ps, fpos, q, k, v, ring, flat = build(L, H, 20)
    order = np.arange(len(ps), dtype=np.int32)[::-1].copy()      # sequence s reads table row kv_row[s] = n - 1 - s, not its own number (the tables are stored reversed)
    c0 = _counts(pkg)
    ref = gg.attn_decode(ctx, q, k, v, fpos, H, KV, window=W, kv_row=order, page_tab=flat[order], score_rows=W + 1)
    c1 = _counts(pkg)
    out = gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, kv_row=order, page_tab=ring[order], score_rows=W + 1, page_tab_len=L)
    c2 = _counts(pkg)
    assert [b - a for a, b in zip(c0, c1)] == [int(i == flat_slot) for i in range(16)]      # the flat launch: its own slot, once
    assert [b - a for a, b in zip(c1, c2)] == [int(i == slot) for i in range(16)]           # the ring launch: the new slot, once; [11] [12] do not move
    assert np.isfinite(out).all() and np.isfinite(ref).all()
    assert out.shape == ref.shape == (len(ps), H * HD)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), [ps[i] for i in sorted(set(np.argwhere(out != ref)[:, 0].tolist()))]
    assert len({out[i].tobytes() for i in range(len(ps))}) == len(ps)      # every sequence read its own keys


def test_a_wider_stride_than_the_ring_is_read_by_the_ring_length(pkg, ctx):
    """page_tab_len < page_tab_stride: the entries past the ring's length are never read (they hold pages of NaN rows here)."""
    gg = pkg.gguf; H = 4; L = 19
    ps, fpos, q, k, v, ring, flat = build(L, H, 21)
    spare = min(set(range(k.shape[0])) - set(ring[ring >= 0].tolist()))      # a page no window names: NaN rows
    assert np.isnan(k[spare]).all()
    wide = np.concatenate([ring, np.full((len(ps), 13), spare, np.int32)], axis=1)
    a = gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, page_tab=ring, score_rows=W + 1, page_tab_len=L)
    b = gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, page_tab=wide, score_rows=W + 1, page_tab_len=L)
    assert np.isfinite(a).all() and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_refusals_launch_nothing(pkg, ctx):
    gg = pkg.gguf; H = 4
    ps, fpos, q, k, v, ring, flat = build(19, H, 22)

    def refused(fn, word):
        before = _counts(pkg)
        with pytest.raises(pkg.VoxError) as e:
            fn()
        assert e.value.code == 1 and word in str(e.value), e.value
        assert _counts(pkg) == before

    # a ring shorter than the window's pages + 2 (255 in pages of 16: 17 pages, so 19 entries)
    refused(lambda: gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, page_tab=ring[:, :18], score_rows=W + 1, page_tab_len=18), "page_tab_len")
    refused(lambda: gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, page_tab=ring, score_rows=W + 1, page_tab_len=20), "page_tab_stride")
    bad = list(ps); bad[0] = 1 << 24
    refused(lambda: gg.attn_decode(ctx, q, k, v, bad, H, KV, window=W, page_tab=ring, score_rows=W + 1, page_tab_len=19), "2^24")
    refused(lambda: gg.attn_decode(ctx, q, k, v, ps, H, KV, window=-1, page_tab=ring, score_rows=W + 1, page_tab_len=19), "window")
    gone = ring.copy(); gone[3, (ps[3] // P) % 19] = -1      # a page of a window, released
    refused(lambda: gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, page_tab=gone, score_rows=W + 1, page_tab_len=19), "outside the pool")
    out = gg.attn_decode(ctx, q, k, v, ps, H, KV, window=W, page_tab=ring, score_rows=W + 1, page_tab_len=19)      # the context is still usable
    assert np.isfinite(out).all()
