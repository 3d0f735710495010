"""The session blob's K / V kernel on its own (snapshot_kv_kernel through vox_debug_snapshot_kv: exactly one launch per call) against numpy indexing.

Everything is compared as bits (uint32 views): the kernel does no arithmetic, so the packed blob IS the named rows, an unpack writes exactly the named rows and every
other word of a NaN-filled cache keeps its own NaN payload.  The caches hold a distinct integer-valued float in every word, so a row taken from the wrong layer,
head, slot or page shows.  The four layouts: flat planes with a layer stride, a ring (row % cap, cap 100: no power of two), a page table, a ring page table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _numbered(shape, base):
    """a distinct integer-valued f32 in every word (all below 2^24)"""
    n = int(np.prod(shape))
    assert base + n < (1 << 24)
    return (np.arange(n, dtype=np.float32) + np.float32(base)).reshape(shape)


def _nan_fill(shape, seed):
    """NaNs with distinct payloads: a word the kernel must not touch is recognisable"""
    rng = np.random.default_rng(seed)
    return (np.uint32(0x7fc00000) | rng.integers(1, 1 << 20, size=shape, dtype=np.uint32)).view(np.float32)


class Flat:
    name = "flat"

    def __init__(self, layers, heads, hd, rows, slack=0):
        self.layers, self.heads, self.hd, self.rows = layers, heads, hd, rows
        self.stride = heads * rows * hd + slack      # a layer stride larger than the layer's rows
        self.shape = (layers, self.stride)

    def index(self, l, h, r):
        """float offset of row r of (l, h) inside the layer"""
        return (h * self.rows + self.slot(r)) * self.hd

    def slot(self, r):
        return r

    def args(self):
        return dict(layout=self.name, rows=self.rows)


class Ring(Flat):
    name = "ring"

    def slot(self, r):
        return r % self.rows


class Paged:
    name = "paged"

    def __init__(self, layers, heads, hd, page_rows, pool_pages, tab):
        self.layers, self.heads, self.hd, self.page_rows, self.tab = layers, heads, hd, page_rows, np.asarray(tab, np.int32)
        self.shape = (layers, pool_pages, heads, page_rows, hd)

    def entry(self, r):
        return r // self.page_rows

    def index(self, l, h, r):
        page = int(self.tab[self.entry(r)])
        return ((page * self.heads + h) * self.page_rows + r % self.page_rows) * self.hd

    def args(self):
        return dict(layout=self.name, page_tab=self.tab, page_rows=self.page_rows)


class PagedRing(Paged):
    name = "paged_ring"

    def entry(self, r):
        return (r // self.page_rows) % len(self.tab)


def _gather(lay, ck, cv, lo, hi):
    """numpy's blob [2, layers, heads, hi - lo, hd] of the cache"""
    out = np.zeros((2, lay.layers, lay.heads, hi - lo, lay.hd), np.float32)
    fk = ck.reshape(lay.layers, -1); fv = cv.reshape(lay.layers, -1)
    for l in range(lay.layers):
        for h in range(lay.heads):
            for r in range(lo, hi):
                o = lay.index(l, h, r)
                out[0, l, h, r - lo] = fk[l, o:o + lay.hd]; out[1, l, h, r - lo] = fv[l, o:o + lay.hd]
    return out


def _scatter(lay, ck, cv, blob, lo, hi):
    """numpy's unpack into copies of the caches"""
    ck, cv = ck.copy(), cv.copy()
    fk = ck.reshape(lay.layers, -1); fv = cv.reshape(lay.layers, -1)
    for l in range(lay.layers):
        for h in range(lay.heads):
            for r in range(lo, hi):
                o = lay.index(l, h, r)
                fk[l, o:o + lay.hd] = blob[0, l, h, r - lo]; fv[l, o:o + lay.hd] = blob[1, l, h, r - lo]
    return ck, cv


def _pack(pkg, ctx, lay, ck, cv, lo, hi):
    return pkg.gguf.snapshot_kv(ctx, ck, cv, lo, hi, lay.heads, lay.hd, **lay.args())


def _unpack(pkg, ctx, lay, ck, cv, blob, lo, hi):
    return pkg.gguf.snapshot_kv(ctx, ck, cv, lo, hi, lay.heads, lay.hd, blob=blob, **lay.args())


def _layouts(layers, hd):
    """the four layouts, each with the row range(s) the issue names: (layout, [(lo, hi)])"""
    heads = 2
    perm = np.random.default_rng(5).permutation(40)
    return [
        (Flat(layers, heads, hd, 50, slack=72), [(0, 50), (7, 30), (49, 50)]),                                  # a layer stride larger than its rows; 23 rows: no multiple of 4
        (Ring(layers, heads, hd, 100), [(950, 1010), (37, 38), (0, 100), (1 << 23, (1 << 23) + 99)]),           # crosses the wrap; a single row; the whole ring; far out
        (Paged(layers, heads, hd, 16, 40, perm[:20]), [(0, 37), (13, 131), (160, 320), (31, 33)]),              # page boundaries mid-range, 118 rows: no multiple of 4
        (PagedRing(layers, heads, hd, 16, 40, perm[20:27]), [(200, 290), (0, 112), (1 << 23, (1 << 23) + 45)]),      # 7 entries: rows 200..290 cross the table's wrap (pages 12..18 -> entries 5, 6, 0, ..)
    ]


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("layers", [1, 3])
def test_pack_and_unpack_against_numpy(pkg, ctx, hd, layers):
    for lay, ranges in _layouts(layers, hd):
        ck = _numbered(lay.shape, 1000); cv = _numbered(lay.shape, 5_000_000)
        for lo, hi in ranges:
            label = (lay.name, hd, layers, lo, hi)
            want = _gather(lay, ck, cv, lo, hi)
            got = _pack(pkg, ctx, lay, ck, cv, lo, hi)
            assert np.array_equal(_bits(got), _bits(want)), label
            # the same blob into a NaN-filled cache of EVERY layout that can hold the range: exactly the named rows are written
            for other, _ in _layouts(layers, hd):
                if isinstance(other, Ring) and hi - lo > other.rows or type(other) is Flat and hi > other.rows:
                    continue
                if type(other) is Paged and (hi - 1) // 16 >= len(other.tab) or type(other) is PagedRing and (hi - 1) // 16 - lo // 16 + 1 > len(other.tab):
                    continue
                nk = _nan_fill(other.shape, 1); nv = _nan_fill(other.shape, 2)
                wk, wv = _scatter(other, nk, nv, want, lo, hi)
                gk, gv = _unpack(pkg, ctx, other, nk, nv, got, lo, hi)
                assert np.array_equal(_bits(gk), _bits(wk)) and np.array_equal(_bits(gv), _bits(wv)), (label, "into", other.name)
                assert int((_bits(gk) != _bits(nk)).sum()) == want[0].size, (label, "into", other.name)      # (no NaN equals a numbered word: every named word changed, no other)


def test_ring_to_paged_to_ring_round_trip(pkg, ctx):
    hd, layers, lo, hi = 128, 3, 950, 1010
    ring = Ring(layers, 2, hd, 100)
    pages = PagedRing(layers, 2, hd, 16, 12, np.random.default_rng(9).permutation(12)[:7])
    ck = _numbered(ring.shape, 10); cv = _numbered(ring.shape, 3_000_000)
    first = _pack(pkg, ctx, ring, ck, cv, lo, hi)
    pk, pv = _unpack(pkg, ctx, pages, _nan_fill(pages.shape, 3), _nan_fill(pages.shape, 4), first, lo, hi)
    second = _pack(pkg, ctx, pages, pk, pv, lo, hi)
    rk, rv = _unpack(pkg, ctx, Ring(layers, 2, hd, 77), _nan_fill((layers, 2 * 77 * hd), 5), _nan_fill((layers, 2 * 77 * hd), 6), second, lo, hi)
    third = _pack(pkg, ctx, Ring(layers, 2, hd, 77), rk, rv, lo, hi)
    assert np.array_equal(_bits(second), _bits(first)) and np.array_equal(_bits(third), _bits(first))


def test_an_empty_range_launches_nothing(pkg, ctx):
    import ctypes as C
    lay = Ring(2, 2, 64, 100)
    ck = _nan_fill(lay.shape, 7); cv = _nan_fill(lay.shape, 8)
    d = pkg.gguf.SnapshotKvDesc(layers=2, n_heads=2, head_dim=64, lo=41, hi=41, layout=1, rows=100, layer_stride=lay.shape[1])
    k0, v0 = ck.copy(), cv.copy(); blob = _nan_fill((4,), 9); b0 = blob.copy()
    for restore in (0, 1):
        assert pkg.lib().vox_debug_snapshot_kv(ctx.h, C.byref(d), ck.ctypes.data, cv.ctypes.data, blob.ctypes.data, restore) == 0
        assert np.array_equal(_bits(ck), _bits(k0)) and np.array_equal(_bits(cv), _bits(v0)) and np.array_equal(_bits(blob), _bits(b0))      # the caller's arrays were not even copied


def test_refusals_reach_no_launch(pkg, ctx):
    """Every refusal comes before the context is bound: the caller's arrays keep their bits (a launch would have copied them back)."""
    hd = 64
    ring = Ring(1, 2, hd, 100); pages = Paged(1, 2, hd, 16, 8, [3, 1, 9, 2]); rpages = PagedRing(1, 2, hd, 16, 8, [3, 1, -1, 2])
    cases = [
        (pages, 0, 40, {}, "table entry 2 of the range is 9, outside the pool's 8 pages"),      # a table entry outside the pool
        (rpages, 100, 120, {}, "table entry 6 of the range is -1, outside the pool's 8 pages"),
        (ring, 30, 20, {}, "hi 20 < lo 30"),
        (ring, 0, 10, dict(hd=32), "head_dim 32"),
        (ring, 900, 1001, {}, "a ring of 100 rows is shorter than the 101 rows"),             # a ring shorter than hi - lo
        (rpages, 0, 70, {}, "touch 5 pages, the ring table has 4 entries"),
        (pages, 60, 70, {}, "lies in page 4 of a table of 4 entries"),
        (Flat(1, 2, hd, 50), 40, 51, {}, "outside the cache's 50 rows"),
    ]
    for lay, lo, hi, kw, text in cases:
        ck = _nan_fill(lay.shape, 11); cv = _nan_fill(lay.shape, 12)
        with pytest.raises(pkg.VoxError, match="vox error 1") as e:
            pkg.gguf.snapshot_kv(ctx, ck, cv, lo, hi, lay.heads, kw.get("hd", lay.hd), **lay.args())
        assert text in str(e.value), (text, str(e.value))
    # pages 0, 1 of the bad table are fine: only the entries the range touches are looked at
    ck = _numbered(pages.shape, 0); cv = _numbered(pages.shape, 100000)
    assert np.array_equal(_pack(pkg, ctx, pages, ck, cv, 0, 32), _gather(pages, ck, cv, 0, 32))
