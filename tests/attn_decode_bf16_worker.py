"""Worker of tests/test_gpu_attn_decode_bf16.py: its tests run through pytest in a process of their own (worker_tests.run_worker) -- the reference launches on ring
page tables count in vox_debug_attn_launches [14] [15], and the bf16 launches in [16] .. [19], which other tests of the suite hold to 0 in their own process.  Not
collected by the suite (no test_ prefix).

The paged decode attention on a bf16 pool (AttnParams::kv_bf16; vox_debug_attn_decode_paged_bf16), one launch at a time.  K and V are random f32 values rounded by
vox_kv_round_bf16; the bf16 launch reads the 16-bit pool, the reference launch (vox_debug_attn_decode, or _paged_ring on a ring table) reads the SAME pages holding the
widened f32 values.  The bf16 kernels load 16 bytes of K and 8 of V where the f32 kernels load two / one float4 and widen in registers; everything behind the load --
the 160 prefetched keys, the scan order, the reduction trees, the P.V order -- is the same code, so the claim is np.array_equal on the output bits, no tolerance.
Beside it the float64 reference on the widened values at the bar of tests/test_gpu_attn_decode.py (attn_decode_ref.BAR per row), and the launch counters: exactly
the bf16 slot moves ([16] per-head, [17] GQA, [18] [19] on a ring table), never [11] [12] [14] [15].

head_dim 128, pages of 16 rows, three sequences on scattered physical pages, 4 heads on 2 KV heads (per-head form) and 8 on 2 (GQA form).  Every row of a named page
outside its sequence's window, every page no window names and every table entry outside a window's pages is hostile (NaN rows; entry -1): a stray read shows."""
import ctypes as C

import numpy as np
import pytest

import attn_decode_ref as R

pytestmark = pytest.mark.gpu
HD, P, KV = 128, 16, 2
N_SLOTS = 20
SLOTS = {"head": (4, {"flat": (16, 11), "ring": (18, 14)}), "gqa": (8, {"flat": (17, 12), "ring": (19, 15)})}      # query heads; (bf16 slot, f32 reference's slot) by table kind
RING_L = 255 // P + 4      # 19: the least ring table a window of 255 admits
# name -> (window, positions of the three sequences, ring table length or None)
CASES = {
    "one_key": (255, (0, 1, 17), None),                             # a single key; a few keys
    "prefetch_end_160_161": (255, (159, 160, 161), None),           # 160, 161, 162 keys: the end of the prefetched block, the loop's first key
    "partial_pass_225": (255, (224, 223, 225), None),               # 225 keys: 160 + 64 + 1 -- a partial 64-key pass (per-head), 32-key passes (GQA)
    "moved_window_of_100": (100, (205, 300, 333), None),            # j_lo = 105, 200, 233: not page-aligned, the window has moved
    "window_straddles_three_pages": (20, (33, 81, 129), None),      # 21 keys over three pages of 16
    "full_window_flat": (255, (255, 256, 1000), None),              # 256 keys on 16 / 17 pages
    "ring_table_wrapped": (255, (16 * RING_L * 3 + 5, 20000, (1 << 24) - 1), RING_L),      # the staged span wraps; above 16 384; the last position of a session
    "ring_table_short_windows": (255, (40, 300, 16 * RING_L + 16), RING_L),               # a window not yet full; no wrap; first page at entry ... RING_L - 1
}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _counts(pkg):
    a = (C.c_uint64 * N_SLOTS)()
    assert pkg.lib().vox_debug_attn_launches(a, N_SLOTS) == 0
    return [int(x) for x in a]


def widen(bits):
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


_BUILT = {}


def build(pkg, name, H):
    """q, the bf16 pools, the f32 pools of the widened values, the table, and per sequence the window's widened K / V [KV][n][128] -- built once per (case, H), read-only."""
    if (name, H) in _BUILT:
        return _BUILT[(name, H)]
    W, ps, L = CASES[name]
    rng = np.random.default_rng([sum(map(ord, name)), H])
    spans = [(max(0, p - W) // P, p // P) for p in ps]
    n_pages = sum(q1 - q0 + 1 for q0, q1 in spans) + 4      # four pages no window names
    free = [int(x) for x in rng.permutation(n_pages)]
    nan16 = np.uint16(0x7FC0)
    kb = np.full((n_pages, KV, P, HD), nan16, np.uint16); vb = kb.copy()
    stride = L if L else max(q1 for _, q1 in spans) + 3
    tab = np.full((len(ps), stride), -1, np.int32)
    keys = []
    for s, (p, (q0, q1)) in enumerate(zip(ps, spans)):
        j_lo = max(0, p - W); n = p - j_lo + 1
        k = pkg.gguf.kv_round_bf16(rng.standard_normal((KV, n, HD)).astype(np.float32)); v = pkg.gguf.kv_round_bf16(rng.standard_normal((KV, n, HD)).astype(np.float32))
        v[:, 0] = pkg.gguf.kv_round_bf16(100 * widen(v[:, 0])); v[:, -1] = pkg.gguf.kv_round_bf16(100 * widen(v[:, -1]))      # the window's edge rows weigh: a dropped one shows
        for q in range(q0, q1 + 1):
            page = free.pop(); e = q % L if L else q
            assert tab[s, e] == -1
            tab[s, e] = page
            j0, j1 = max(j_lo, q * P), min(p, q * P + P - 1)      # the window's rows on this page
            kb[page, :, j0 - q * P:j1 - q * P + 1] = k[:, j0 - j_lo:j1 - j_lo + 1]; vb[page, :, j0 - q * P:j1 - q * P + 1] = v[:, j0 - j_lo:j1 - j_lo + 1]
        keys.append((widen(k), widen(v)))
    q = (1.5 * rng.standard_normal((len(ps), H * HD))).astype(np.float32)
    kf, vf = widen(kb), widen(vb)
    assert np.array_equal(pkg.gguf.kv_round_bf16(kf[~np.isnan(kf)]), kb[~np.isnan(kf)])      # widening and rounding again is the identity on bf16 values
    ref = np.zeros((len(ps), H * HD)); G = H // KV
    for s, (kw, vw) in enumerate(keys):
        for h in range(H):
            sc = kw[h // G].astype(np.float64) @ q[s, h * HD:(h + 1) * HD].astype(np.float64) / np.sqrt(float(HD))
            pr = np.exp(sc - sc.max())
            ref[s, h * HD:(h + 1) * HD] = (pr @ vw[h // G].astype(np.float64)) / pr.sum()
    out = (W, ps, L, q, kb, vb, kf, vf, tab, ref)
    for a in out[3:]:
        a.setflags(write=False)
    _BUILT[(name, H)] = out
    return out


@pytest.mark.parametrize("out_xf", [False, True], ids=["rows", "xf"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("kind", ["head", "gqa"])
def test_bf16_attention_is_the_f32_attention_on_the_widened_values(pkg, ctx, kind, name, out_xf):
    gg = pkg.gguf; H, slots = SLOTS[kind]
    W, ps, L, q, kb, vb, kf, vf, tab, ref = build(pkg, name, H)
    slot, f32_slot = slots["ring" if L else "flat"]
    kw = dict(window=W, page_tab=tab, score_rows=W + 1, out_xf=out_xf)
    c0 = _counts(pkg)
    want = gg.attn_decode(ctx, q, kf, vf, ps, H, KV, page_tab_len=L, **kw)
    c1 = _counts(pkg)
    got = gg.attn_decode(ctx, q, kb, vb, ps, H, KV, page_tab_len=L, bf16=True, **kw)
    c2 = _counts(pkg)
    assert [b - a for a, b in zip(c0, c1)] == [int(i == f32_slot) for i in range(N_SLOTS)]      # the reference launch: the f32 form's slot, once
    assert [b - a for a, b in zip(c1, c2)] == [int(i == slot) for i in range(N_SLOTS)]          # the bf16 launch: the new slot, once, and nothing else
    assert got.shape == want.shape and got.dtype == want.dtype
    if out_xf:
        assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()      # the raw planes of the wo GEMM
        hi, lo = R.xf_decode(got, len(ps), H * HD)
        val = widen(hi).astype(np.float64) + widen(lo).astype(np.float64)             # hi + lo: the row to 2^-17 of each value
    else:
        assert np.isfinite(got).all()
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:4].tolist()
        assert len({got[i].tobytes() for i in range(len(ps))}) == len(ps)             # every sequence read its own keys
        val = got
    e = R.row_err(val, ref, H)
    print(f"{kind} {name} {'xf' if out_xf else 'rows'}: worst row {e.max():.2e} of its max (bar {R.BAR:.0e})")
    assert (e <= R.BAR).all(), np.argwhere(e > R.BAR)[:6].tolist()


def test_refusals_launch_nothing(pkg, ctx):
    gg = pkg.gguf; H = 4
    W, ps, L, q, kb, vb, kf, vf, tab, ref = build(pkg, "ring_table_wrapped", H)

    def refused(fn, word):
        before = _counts(pkg)
        with pytest.raises(pkg.VoxError) as e:
            fn()
        assert e.value.code == 1 and word in str(e.value), e.value
        assert _counts(pkg) == before

    kw = dict(window=W, score_rows=W + 1, bf16=True)
    refused(lambda: gg.attn_decode(ctx, q, kb, vb, ps, H, KV, page_tab=tab[:, :18], page_tab_len=18, **kw), "page_tab_len")
    refused(lambda: gg.attn_decode(ctx, q, kb, vb, ps, H, KV, page_tab=tab, page_tab_len=L + 1, **kw), "page_tab_stride")
    gone = tab.copy(); gone[1, (ps[1] // P) % L] = -1      # a page of a window, released
    refused(lambda: gg.attn_decode(ctx, q, kb, vb, ps, H, KV, page_tab=gone, page_tab_len=L, **kw), "outside the pool")
    refused(lambda: gg.attn_decode(ctx, q, kb, vb, ps, H, KV, page_tab=tab, page_tab_len=None, **kw), "outside")      # a flat table cannot express these positions
    out = gg.attn_decode(ctx, q, kb, vb, ps, H, KV, page_tab=tab, page_tab_len=L, **kw)      # the context is still usable
    assert np.isfinite(out).all()
