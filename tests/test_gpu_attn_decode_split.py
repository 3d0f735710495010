"""The key-split decode attention (attn_decode_split_kernel + attn_decode_merge_kernel) through vox_debug_attn_decode_split, against the float64 reference and the
cases of tests/attn_decode_ref.py: positions on, before and behind a 256-row chunk edge, mostly empty grids, j_lo mid-chunk, the real window's 33 - 34 chunks, pages
smaller and larger than a chunk, `peaked` for the merge's rescale.  Every call: 2e-5 of each row's maximum, exactly one split ([20]) and one merge ([21]) launch."""
import ctypes

import numpy as np
import pytest

import attn_decode_ref as R

pytestmark = pytest.mark.gpu
GEOS2 = ((4, 1), (4, 2))
CASES = ([R.seam_case(kd, g) for g in R.ALL_GEOS for kd in R.KINDS] + [R.small_window_case(kd, g, w) for g in GEOS2 for kd in R.KINDS for w in R.SMALL_WINDOWS] +
         [R.real_window_case(kd, g, 16384) for g in GEOS2 for kd in R.KINDS] + [R.kv_row_case("normal", g) for g in R.ALL_GEOS])
LAYOUT_CASES = [R.small_window_case("normal", (4, 1), 200), R.small_window_case("peaked", (4, 2), 65), R.kv_row_case("normal", (2, 2)), R.real_window_case("uniform", (4, 1), 16384)]


@pytest.fixture(scope="module")
def env(pkg):
    from importlib import import_module
    c = pkg.Context(0)
    yield pkg, import_module(pkg.__name__ + ".gguf"), c
    c.close()


def slots(pkg):
    a = (ctypes.c_uint64 * 24)()
    assert pkg.lib().vox_debug_attn_launches(a, 24) == 0
    return np.array(a[:], np.int64)


def split(env, c, q, k, v, layout="flat", P=64, bf16=False, **kw):
    """One call on the case's rows as flat slices, a ring (capacity no multiple of the chunk), pages of P rows, or pages behind a ring table."""
    pkg, gg, ctx = env
    before = slots(pkg)
    if layout == "ring":
        cap = c.window + 1 + 99
        rk = np.full((c.n_slices, c.KV, cap, R.HD), np.nan, np.float32); rv = rk.copy()
        for i in range(len(c.pos)):
            j = np.arange(*np.cumsum(R.window_of(c, i))); s = R.slice_of(c, i)
            rk[s][:, j % cap] = k[s][:, j]; rv[s][:, j % cap] = v[s][:, j]
        out = gg.attn_decode_split(ctx, q, rk, rv, c.pos, c.H, c.KV, window=c.window, kv_row=c.kv_row, ring=True, **kw)
    elif layout != "flat":
        pk, pv, tab = R.to_paged(c, k, v, P); L = 0
        if layout == "paged_ring":      # logical page g at entry g % L, L shorter than the flat row
            L = c.window // P + 6; flat_tab = tab; tab = np.full((c.n_slices, L), -1, np.int32)
            for s, g in zip(*np.nonzero(flat_tab >= 0)):
                tab[s, g % L] = flat_tab[s, g]
        if bf16:
            pk, pv = gg.kv_round_bf16(pk), gg.kv_round_bf16(pv)
        out = gg.attn_decode_split(ctx, q, pk, pv, c.pos, c.H, c.KV, window=c.window, kv_row=c.kv_row, page_tab=tab, score_rows=R.score_rows_of(c), page_tab_len=L, bf16=bf16, **kw)
    else:
        out = gg.attn_decode_split(ctx, q, k, v, c.pos, c.H, c.KV, window=c.window, kv_row=c.kv_row, **kw)
    ran = slots(pkg) - before
    assert ran[20] == 1 and ran[21] == 1 and ran.sum() == 2, f"expected one split and one merge launch, the slots moved by {ran.tolist()}"
    return out


def held(c, out, ref):
    e = R.row_err(out, ref, c.H)
    i, h = np.unravel_index(int(np.argmax(e)), e.shape)
    print(f"{R.case_id(c)}: worst row {e.max():.2e} of its max (sequence {i} at position {c.pos[i]}, {R.window_of(c, i)[1]} keys, head {h})")
    assert (e <= R.BAR).all(), f"{int((e > R.BAR).sum())} rows past 2e-5 of their max, worst {e.max() / R.BAR:.1f} x the bar at sequence {i} (position {c.pos[i]}), head {h}"


def same_bits(a, b, what):
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} values differ"


@pytest.mark.parametrize("c", CASES, ids=R.case_id)
def test_split_meets_the_bar(env, c):
    held(c, split(env, c, *R.cached(c)[:3]), R.cached(c)[3])


@pytest.mark.parametrize("c", LAYOUT_CASES, ids=R.case_id)
def test_every_layout_gives_the_flat_bits(env, c):
    q, k, v, ref = R.cached(c)
    P = 256 if c.rows > 1024 else 64
    flat = split(env, c, q, k, v)
    held(c, flat, ref)
    for layout in ("ring", "paged", "paged_ring"):
        same_bits(split(env, c, q, k, v, layout, P), flat, layout)


@pytest.mark.parametrize("geo", GEOS2)
@pytest.mark.parametrize("P", [16, 64, 1024])
def test_page_edges(env, P, geo):
    for c in R.page_edge_cases(geo, P):
        q, k, v, ref = R.cached(c)
        paged = split(env, c, q, k, v, "paged", P)
        held(c, paged, ref)
        same_bits(paged, split(env, c, q, k, v), R.case_id(c))


@pytest.mark.parametrize("layout", ["paged", "paged_ring"])
def test_bf16_pool_equals_its_widened_values(env, layout):
    gg = env[1]
    for c in (R.small_window_case("normal", (4, 1), 200), R.small_window_case("peaked", (4, 2), 160)):
        q, k, v, _ = R.cached(c)
        wide = lambda x: (gg.kv_round_bf16(x).astype(np.uint32) << np.uint32(16)).view(np.float32)
        out = split(env, c, q, k, v, layout, bf16=True)
        assert np.isfinite(out).all()
        same_bits(out, split(env, c, q, wide(k), wide(v), layout), R.case_id(c))


@pytest.mark.parametrize("layout", ["flat", "ring", "paged"])
def test_xf_planes_are_the_split_of_the_f32_rows(env, layout):
    c = R.small_window_case("normal", (8, 2), 200) if layout == "ring" else R.seam_case("normal", (8, 2))      # 37 sequences: three 16-row groups
    q, k, v, _ = R.cached(c)
    hi, lo = R.xf_decode(split(env, c, q, k, v, layout, out_xf=True), len(c.pos), c.H * R.HD)
    want_hi, want_lo = R.bf16_split(split(env, c, q, k, v, layout))
    assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo)


def test_refusals_launch_nothing(env):
    pkg, gg, ctx = env
    c = R.make_case("refuse", "normal", 4, 1, 40, 128, (100, 17))
    q, k, v = R.build_inputs(c)
    pk, pv, tab = R.to_paged(c, k, v, 16)
    bad = tab.copy(); bad[0, 100 >> 4] = pk.shape[0]
    paged = dict(window=40, page_tab=tab, score_rows=41)
    for word, fn in (("head_dim", lambda: gg.attn_decode_split(ctx, q, k, v, c.pos, 4, 1, window=40, head_dim=64)),
                     ("outside the cache", lambda: gg.attn_decode_split(ctx, q, k, v, (128, 17), 4, 1, window=40)),
                     ("kv_row", lambda: gg.attn_decode_split(ctx, q, k, v, c.pos, 4, 1, window=40, kv_row=(0, 2))),
                     ("window", lambda: gg.attn_decode_split(ctx, q, k, v, c.pos, 4, 1, window=128, ring=True)),
                     ("outside the pool", lambda: gg.attn_decode_split(ctx, q, pk, pv, c.pos, 4, 1, **dict(paged, page_tab=bad))),
                     ("score_rows", lambda: gg.attn_decode_split(ctx, q, pk, pv, c.pos, 4, 1, **dict(paged, score_rows=40))),
                     ("kv_dtype", lambda: gg.attn_decode_split(ctx, q, k.view(np.uint16)[..., ::2], v.view(np.uint16)[..., ::2], c.pos, 4, 1, window=40, bf16=True)),
                     ("prefer_gqa", lambda: gg.attn_decode_split(ctx, q, k, v, c.pos, 4, 1, window=40, prefer_gqa=1)),
                     ("1, 2 or 4", lambda: gg.attn_decode_split(ctx, np.tile(q, 2), k, v, c.pos, 8, 1, window=40))):
        before = slots(pkg)
        with pytest.raises(pkg.VoxError) as e:
            fn()
        assert e.value.code == 1 and word in str(e.value), (word, e.value)
        assert not (slots(pkg) - before).any()
    held(c, split(env, c, q, k, v, "paged", 16), R.reference(c, q, k, v))      # the context is still usable
