"""Float64 reference, deterministic inputs and the case table of the decode attention kernels (one query row per sequence; tests/test_gpu_attn_decode.py runs the
kernels, tests/test_attn_decode_ref.py pins this file on the CPU).

A case is LOGICAL: head counts, window, rows per cache slice, one position per sequence, optionally the slice each sequence reads.  Its inputs are q [n_seq][H * 128] and
K / V [n_slices][KV][rows][128]; a slab launch takes them as they are, to_paged() scatters the same rows over a pool behind a page table, so every kernel form of a case
is held to one reference, computed once (cached()).

Input kinds (every kind: rows behind a sequence's position are NaN in K and V -- stale memory may hold anything; rows in front of its window have random K and V = 1e6 (peaked: 1e24),
so a key admitted there shows at any softmax weight; slices no sequence reads are NaN throughout):
  normal   q ~ N(0, 1.5^2), K, V ~ N(0, 1); the V rows of the window's first and last key are scaled by EDGE_V_SCALE.
  uniform  q = 0: every visible key weighs exactly 1 / n.  V row j holds bit b of its logical index j in column b (b = 0..13) as +-0.5, the whole row times a
           seeded sign, the other columns 0.  Every column is then a balanced +-0.5 sequence whatever the window (plain bits would make column 13 constant in a window
           past row 8192: the output 1, a dropped key invisible in it, and the oracle's one-chain float32 sum of 8193 equal terms off by 9e-5 on its own), the row's
           largest output is a few 0.5 / sqrt(n), and a dropped or doubled key moves EVERY column by ~0.5 / n -- far above the bar even at n = 8193, where N(0, 1)
           data would hide one interior key among 8193.
  peaked   normal, but ONE key per KV head has K aligned with the first query head of its group, score 35 (the rest: N(0, 1.5^2)): exp underflow and the maximum
           subtraction.  The key sits on a loop seam: window index 159, 160, n - 1 or 0, cycling with the sequence (n - 1 where the window is shorter).
"""
import zlib
from collections import namedtuple

import numpy as np

from model_fixtures import EDGE_V_SCALE

HD = 128
BAR = 2e-5            # per row (one sequence, one head): |out - ref| <= BAR * max|ref of that row|
KINDS = ("normal", "uniform", "peaked")
PEAK_AT = (159, 160, -1, 0)      # window index of the peaked key, by sequence % 4 (-1: the last key)
PEAK_SCORE = 35.0
FRONT_V = {"normal": 1e6, "uniform": 1e6, "peaked": 1e24}      # V of the rows in front of the window (peaked: next to a key of weight ~1 an admitted row weighs ~e^-33)

Case = namedtuple("Case", "name kind H KV window rows pos kv_row n_slices")


def make_case(name, kind, H, KV, window, rows, pos, kv_row=None, n_slices=None):
    pos = tuple(int(p) for p in pos)
    assert kind in KINDS and H % KV == 0 and all(0 <= p < rows for p in pos)
    kv_row = None if kv_row is None else tuple(int(r) for r in kv_row)
    n_slices = len(pos) if n_slices is None else n_slices
    assert (kv_row is None and n_slices >= len(pos)) or (kv_row is not None and len(set(kv_row)) == len(pos) and max(kv_row) < n_slices)
    return Case(name, kind, H, KV, window, rows, pos, kv_row, n_slices)


def case_id(c):
    return f"{c.name}-{c.kind}-{c.H}x{c.KV}"


def window_of(c, i):
    """(first visible row j_lo, key count n) of sequence i."""
    p = c.pos[i]
    j_lo = max(0, p - c.window) if c.window >= 0 else 0
    return j_lo, p - j_lo + 1


def slice_of(c, i):
    return c.kv_row[i] if c.kv_row is not None else i


def peak_index(c, i):
    n = window_of(c, i)[1]
    t = PEAK_AT[i % 4]
    return n - 1 if t < 0 or t >= n else t


def build_inputs(c):
    """q [n_seq][H*128], K, V [n_slices][KV][rows][128], float32: a function of the case alone."""
    seed = zlib.crc32(repr(tuple(c)).encode())
    n_seq, G = len(c.pos), c.H // c.KV
    q = np.zeros((n_seq, c.H * HD), np.float32)
    k = np.full((c.n_slices, c.KV, c.rows, HD), np.nan, np.float32); v = np.full_like(k, np.nan)
    for i, p in enumerate(c.pos):
        rng = np.random.default_rng([seed, i])
        s = slice_of(c, i); j_lo, n = window_of(c, i)
        if c.kind != "uniform":
            q[i] = 1.5 * rng.standard_normal(c.H * HD, dtype=np.float32)
        k[s, :, :p + 1] = rng.standard_normal((c.KV, p + 1, HD), dtype=np.float32)
        v[s, :, :j_lo] = FRONT_V[c.kind]
        if c.kind == "uniform":
            j = np.arange(j_lo, p + 1)
            v[s, :, j_lo:p + 1] = 0.0
            sgn = rng.integers(0, 2, len(j)).astype(np.float32) * 2 - 1
            v[s, :, j_lo:p + 1, :14] = ((((j[:, None] >> np.arange(14)[None, :]) & 1).astype(np.float32) - 0.5) * sgn[:, None])[None]
        else:
            v[s, :, j_lo:p + 1] = rng.standard_normal((c.KV, n, HD), dtype=np.float32)
        if c.kind == "normal":
            for e in {j_lo, p}:
                v[s, :, e] *= np.float32(EDGE_V_SCALE)
        if c.kind == "peaked":
            t = j_lo + peak_index(c, i)
            for g in range(c.KV):
                qh = q[i, g * G * HD:(g * G + 1) * HD].astype(np.float64)
                k[s, g, t] = (qh * (PEAK_SCORE * np.sqrt(HD) / (qh @ qh))).astype(np.float32)
    return q, k, v


def visible(c, i, mutate=None):
    """Logical rows sequence i attends.  mutate (the CPU pin's stand-ins for a wrong kernel): "first" / "last" drop that key, "early" admits row j_lo - 1,
    ("drop", t) drops window index t."""
    j_lo, n = window_of(c, i)
    idx = np.arange(j_lo, j_lo + n)
    if mutate == "first":
        idx = idx[1:]
    elif mutate == "last":
        idx = idx[:-1]
    elif mutate == "early":
        idx = np.arange(j_lo - 1, j_lo + n) if j_lo > 0 else idx
    elif mutate is not None:
        idx = np.delete(idx, mutate[1])
    return idx


def reference(c, q, k, v, mutate=None, only=None):
    """float64 [n_seq][H*128]: scores over the visible keys, scaled by 1 / sqrt(128), softmax with the maximum subtracted, weighted sum of V.  Reads the
    logical rows alone (a sequence without a visible key -- a mutation of a one-key window -- keeps NaN)."""
    G = c.H // c.KV
    out = np.full((len(c.pos), c.H * HD), np.nan)
    for i in (range(len(c.pos)) if only is None else only):
        idx = visible(c, i, mutate); s = slice_of(c, i)
        if not len(idx):
            continue
        for h in range(c.H):
            kk = k[s, h // G, idx].astype(np.float64); vv = v[s, h // G, idx].astype(np.float64)
            sc = kk @ q[i, h * HD:(h + 1) * HD].astype(np.float64) / np.sqrt(float(HD))
            pr = np.exp(sc - sc.max())
            out[i, h * HD:(h + 1) * HD] = (pr @ vv) / pr.sum()
    return out


def _sum8_f32(t):
    """float32 sum over axis 0 as 8 interleaved chains (key i in chain i % 8), each added in key order (cumsum accumulates sequentially), then the 8 in order."""
    n = t.shape[0]
    pad = np.zeros(((-n) % 8,) + t.shape[1:], np.float32)
    parts = np.cumsum(np.concatenate([t, pad]).reshape((-1, 8) + t.shape[1:]), axis=0, dtype=np.float32)[-1]
    return np.cumsum(parts, axis=0, dtype=np.float32)[-1]


def reference_f32(c, q, k, v):
    """The same operation with every value and every sum in float32: the 128-term score dot product as one sequential chain, the softmax sum and P.V as 8 interleaved
    sequential chains -- the shape both kernels give P.V (8 key groups, each in key order), and no better than theirs.  ONE chain over all keys is not the yardstick:
    with the first key's V scaled by 100 the running sum is as large as the result from the first add on, and 8192 further roundings of 2^-25 of it leave ~3e-6 of
    the column (1 sigma), up to 7e-6 over the rows of the 8193-key cases."""
    G = c.H // c.KV
    out = np.zeros((len(c.pos), c.H * HD), np.float32)
    for i in range(len(c.pos)):
        idx = visible(c, i); s = slice_of(c, i)
        for h in range(c.H):
            kk = k[s, h // G, idx]; vv = v[s, h // G, idx]
            sc = np.cumsum(kk * q[i, h * HD:(h + 1) * HD][None, :], axis=1, dtype=np.float32)[:, -1] * np.float32(1.0 / np.sqrt(np.float32(HD)))
            pr = np.exp(sc - sc.max())
            out[i, h * HD:(h + 1) * HD] = _sum8_f32(pr[:, None] * vv) / _sum8_f32(pr)
    return out


def row_max(ref, H):
    """max|ref| of every row (sequence, head): [n_seq][H]."""
    return np.abs(ref.reshape(ref.shape[0], H, HD)).max(axis=2)


def row_err(out, ref, H):
    """Worst |out - ref| of every row as a multiple of its row's max|ref|: [n_seq][H]; a NaN or inf in out gives inf."""
    e = np.abs(out.astype(np.float64) - ref).reshape(ref.shape[0], H, HD).max(axis=2) / np.maximum(row_max(ref, H), 1e-300)
    return np.where(np.isfinite(e), e, np.inf)


_CACHE = {}


def cached(c):
    """(q, k, v, ref) of a case: built once per process, shared by every form that runs it, and read-only."""
    if c not in _CACHE:
        if len(_CACHE) >= 4:      # the big cases hold ~200 MB each: keep the few most recent (the table is ordered by case)
            _CACHE.pop(next(iter(_CACHE)))
        q, k, v = build_inputs(c); ref = reference(c, q, k, v)
        for a in (q, k, v, ref):
            a.setflags(write=False)
        _CACHE[c] = (q, k, v, ref)
    return _CACHE[c]


def score_rows_of(c):
    """LDS score rows per query head of a paged launch, by the product's rule (group_round): min(rows, window + 1)."""
    return min(c.rows, c.window + 1) if c.window >= 0 else c.rows


def to_paged(c, k, v, page_rows, spare=3):
    """The case's rows behind a page table: pool K / V [pages][KV][page_rows][128] and table [n_slices][rows / page_rows] int32.  Physical pages are a seeded
    permutation; only the logical pages that hold a row of a sequence's window are named (copied WHOLE: their rows outside the window keep the hostile values), every
    other entry is -1, and `spare` pool pages no entry names are NaN like the rest of the pool's unnamed rows."""
    assert c.rows % page_rows == 0
    sh = page_rows.bit_length() - 1
    named = []
    for i in range(len(c.pos)):
        j_lo, _ = window_of(c, i)
        named += [(slice_of(c, i), pg) for pg in range(j_lo >> sh, (c.pos[i] >> sh) + 1)]
    n_pool = len(named) + spare
    phys = np.random.default_rng([zlib.crc32(repr(tuple(c)).encode()), page_rows, 77]).permutation(n_pool)
    pk = np.full((n_pool, c.KV, page_rows, HD), np.nan, np.float32); pv = np.full_like(pk, np.nan)
    tab = np.full((c.n_slices, c.rows // page_rows), -1, np.int32)
    for (s, pg), ph in zip(named, phys):
        tab[s, pg] = ph
        pk[ph] = k[s, :, pg * page_rows:(pg + 1) * page_rows]; pv[ph] = v[s, :, pg * page_rows:(pg + 1) * page_rows]
    return pk, pv, tab


# ---- the XF planes (xf_store4, csrc/vox_kernels.hip): bf16 hi + lo of a 16-row group in the MFMA A-operand order the wo GEMM loads
def bf16_rne(x):
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def bf16_split(x):
    """(hi, lo) bf16 bits of float32 x: hi = rne(x), lo = rne(x - hi) (split_pair)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - (hi.astype(np.uint32) << np.uint32(16)).view(np.float32))


def xf_decode(planes, n_seq, K):
    """planes uint16 [groups][2][K / 128 * 2048] -> (hi, lo) uint16 [n_seq][K]: element k of row r of a group lies at uint16 index
    ((q * 4 + j) * 64 + g * 16 + r) * 8 + 2 * half + 4 * (t & 1) + (t >> 1), q = k >> 7, j = (k >> 5) & 3, e = k & 31, half = e >> 4, g = (e & 15) >> 2, t = e & 3."""
    kk = np.arange(K)
    qq, jj, e = kk >> 7, (kk >> 5) & 3, kk & 31
    half, g, t = e >> 4, (e & 15) >> 2, e & 3
    col = ((qq * 4 + jj) * 64 + g * 16) * 8 + 2 * half + 4 * (t & 1) + (t >> 1)
    s = np.arange(n_seq)
    at = col[None, :] + 8 * (s % 16)[:, None]
    return planes[(s // 16)[:, None], 0, at], planes[(s // 16)[:, None], 1, at]


# ---- the table.  Head geometries: the GQA forms take 4 query heads per KV head; the per-head kernels serve every ratio
GQA_GEOS = ((4, 1), (8, 2))
HEAD_GEOS = ((4, 2), (4, 1), (2, 2))
ALL_GEOS = ((4, 1), (8, 2), (4, 2), (2, 2))
SEAM_KEYS = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 159, 160, 161, 167, 168, 169, 191, 192, 193, 223, 224, 225, 255, 256, 257, 287, 288, 289, 511, 512, 513,
             1023, 1024)
SEAM_POS = tuple(n - 1 for n in SEAM_KEYS)                       # 37 sequences: crosses the 16-row XF group twice
SEAM40_POS = SEAM_POS + (99, 299, 699)                           # 40: n_heads * n_seq is a multiple of 8 G (the XCD re-map of the per-head kernels runs), 37 is not
SMALL_WINDOWS = (20, 65, 159, 160, 200)
REAL_WINDOW = 8192
REAL_GEOS = ((4, 1), (8, 2), (4, 2))                             # the 16 384-row caches (64 MB of K per KV head and four sequences): the per-head forms at 4:1 and 2:1, the paged GQA form at both 4:1 shapes
KV_ROW_ORDER = (6, 2, 7, 0, 3)                                   # 5 sequences reading 5 of 8 slices, scrambled
KV_ROW_POS = (700, 40, 1023, 160, 333)


def small_window_pos(w):
    return (w - 1, w, w + 1, w + 159, w + 160, 1023)


def real_window_pos(rows):
    return (8191, 8192, 8193, rows - 1)


def seam_case(kind, geo, n40=False):
    return make_case("seam40" if n40 else "seam", kind, geo[0], geo[1], -1, 1024, SEAM40_POS if n40 else SEAM_POS)


def small_window_case(kind, geo, w):
    return make_case(f"win{w}", kind, geo[0], geo[1], w, 1024, small_window_pos(w))


def real_window_case(kind, geo, rows):
    return make_case("real16384" if rows == 16384 else "realgqa", kind, geo[0], geo[1], REAL_WINDOW, rows, real_window_pos(rows))


def kv_row_case(kind, geo):
    return make_case("kvrow", kind, geo[0], geo[1], 300, 1024, KV_ROW_POS, KV_ROW_ORDER, 8)


def page_edge_cases(geo, P):
    """pos and j_lo each at a page's last row, first row and mid-page: phase a of pos and b of j_lo need window = (a - b) mod P (+ P: the window spans a page
    boundary); the six distinct windows, each one launch with the positions that realise its (a, b) pairs and one whose window has not moved."""
    ph = {"last": P - 1, "first": 0, "mid": P // 2}
    by_w = {}
    for a in ph.values():
        for b in ph.values():
            by_w.setdefault((a - b) % P + P, set()).add(3 * P + a)
    out = []
    for w, ps in sorted(by_w.items()):
        pos = tuple(sorted(ps)) + (P // 2 + 3,)
        for p in pos[:-1]:
            assert (p % P) in ph.values() and ((p - w) % P) in ph.values() and p - w > 0
        out.append(make_case(f"page{P}w{w}", "normal", geo[0], geo[1], w, 4 * P, pos))
    assert len(out) == 6
    return out


def logical_cases(gqa_rows):
    """Every logical case of the GPU table (tests/test_gpu_attn_decode.py), once.  gqa_rows: the most rows per KV head the slab GQA form serves (the real-window case
    of that form takes a cache of exactly that many rows)."""
    out = [seam_case(kd, g) for g in ALL_GEOS for kd in KINDS] + [seam_case(kd, g, True) for g in HEAD_GEOS for kd in KINDS]
    out += [small_window_case(kd, g, w) for g in ALL_GEOS for kd in KINDS for w in SMALL_WINDOWS]
    out += [real_window_case(kd, g, 16384) for g in REAL_GEOS for kd in KINDS] + [real_window_case(kd, g, gqa_rows) for g in GQA_GEOS for kd in KINDS]
    out += [kv_row_case("normal", g) for g in ALL_GEOS]
    out += [c for g in ((4, 1), (4, 2)) for P in (16, 64, 1024) for c in page_edge_cases(g, P)]
    assert len({case_id(c) for c in out}) == len(out)
    return out
