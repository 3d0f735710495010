"""The burst form of the live sessions' encoder ring attention (stream_attn_burst_kernel<64> / <128> behind launch_stream_attn_burst, csrc/vox_kernels.hip: up to 64
rows per session -- b ticks of 4 -- in one launch, one workgroup per head and tile of 4 query rows) through vox_debug_stream_attn_burst, one launch at a time.  The
inputs, the float64 reference and the bars are tests/stream_attn_ref.py, the tick kernel's own (make_case takes any `rows` with cap > window + rows).

Held per case, after exactly ONE burst launch (vox_debug_stream_attn_burst_launches moves by one, no slot of vox_debug_attn_launches moves):
  out         per (row, head) |out - ref| <= BAR (2e-5) of that row and head's max|ref|, every value finite;
  appended K  componentwise within K_BAR (2^-22) (|xr| + |xi|);
  appended V  the input's bits;
  the rest    every other ring word its bits from before the launch, NaN payloads included.
The table: head_dim 64 with 3 heads and 128 with 2; 5, 8, 12 and 64 rows (a last tile of 1 row, whole tiles, 16 tiles); the window-1023 seam as 16 members of one launch
with cap = window + rows + 1 (a first tick with j0 = 0, key counts around 16, 64, 256 and 1024, the window's first move inside a tile and between tiles, rows that
straddle the ring's wrap); window 5 in a ring of 14 with 8 rows and in a ring of 70 with 64 rows (queries whose whole window lies inside the burst: no ring key at all);
the real window 750 at cap 832 with 64 rows straddling the ring's wrap, layer 1 of 3, 3 of 5 members served in the order 2, 0, 1; RoPE rows from the flat table, from
one ring of 128 rows and from rings of exactly `rows` rows (8 and 64).
The contract, bit for bit: for b in 2, 3 and 16 one burst launch of 4 b rows against b chained vox_debug_stream_attn launches of 4 rows (enc_pos moving by 4, the
rings fed back) agrees in every word of out, kring and vring.  Refusals (rows 65, cap = window + rows, head_dim 32) count no launch.  The last test fails if either head
size was never the asserted launch of a passing case.
"""
from importlib import import_module

import numpy as np
import pytest

import stream_attn_ref as S
from model_fixtures import attn_launches, launches_since

pytestmark = pytest.mark.gpu

BIG = 1 << 24
# window 1023, 16 members: first positions of the burst; the key counts of its rows are min(p, 1023) + 1
SEAM_POS = {
    5: (0, 11, 12, 59, 60, 251, 252, 1018, 1019, 1020, 1022, 1023, 1024, 2 * 1029 - 3, 3000, 7),          # 1019 .. 1023: the window's first move at each row of the 5 (tiles of 4 + 1)
    8: S.SEAM_POS[8],
    12: (0, 4, 52, 53, 244, 245, 740, 1011, 1012, 1015, 1016, 1019, 1023, 2 * 1036 - 6, 3000, 7),         # 1012 .. 1023: the first move in every tile
    64: (0, 1, 192, 193, 700, 959, 960, 961, 990, 1000, 1022, 1023, 1024, 2 * 1088 - 32, 5000, 7),        # 960 .. 1023: the first move inside the burst; 2144: the rows straddle the wrap
}


def seam_case(kind, geo, rows):
    return S.make_case(f"seam{rows}", kind, geo, rows, 1023, 1023 + rows + 1, tuple(reversed(range(16))), SEAM_POS[rows])


def real_case(kind, geo, rows=64, cap=832, **kw):
    """The real window at the burst streams' default capacity, layer 1 of 3, 3 of 5 members in the order 2, 0, 1: member 0 has not filled its window (j0 = 0), member
    1's window straddles the ring's wrap, member 2's burst rows straddle it (cap - rows / 2 ..)."""
    return S.make_case(f"real{cap}x{rows}", kind, geo, rows, 750, cap, (2, 0, 1), (300, 5000, 3 * cap - rows // 2, 77, 1234), layers=3, layer=1, **kw)


def table():
    out = []
    for geo in S.GEOS:
        out += [seam_case("normal", geo, rows) for rows in (5, 8, 12, 64)] + [seam_case(kd, geo, 64) for kd in ("uniform", "peaked")] + [seam_case("peaked", geo, 5)]
        out += [real_case(kd, geo) for kd in S.KINDS]
        out += [S.tiny_case(kd, geo) for kd in ("normal", "uniform")]                                                  # window 5, ring of 14, 8 rows
        out += [S.make_case("tiny70", kd, geo, 64, 5, 70, (2, 0, 1), (0, 10, 2 * 70 - 30)) for kd in ("normal", "uniform")]
        out += [S.make_case("ring128", "normal", geo, 12, 750, 832, (2, 0, 1), (65530, 1000003, BIG - 40), rope_rows=128),      # across the table length, far out (ring rows 122 .. 5, 67 .. 78, 88 .. 99)
                S.make_case("exact8", "peaked", geo, 8, 750, 760, (0,), (BIG - 9,), rope_rows=8),
                S.make_case("exact64", "normal", geo, 64, 750, 832, (1, 0), (70000, 65500), rope_rows=64, per_member=True)]
    assert len({S.case_id(c) for c in out}) == len(out)
    return out


CASES = table()
CASE_IDS = [S.case_id(c) for c in CASES]
PASSED, ASSERTED, WORST = set(), set(), {}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def launch(pkg, gg, ctx, c, inp):
    """ONE burst launch of the case on `inp`: the burst counter moves by one, no slot of the attention counters moves.  Returns (out, kring, vring)."""
    before, b0 = attn_launches(pkg), gg.stream_attn_burst_launches()
    got = gg.stream_attn_burst(ctx, inp.qkv, inp.kring, inp.vring, c.order, c.enc_pos, c.rows, c.window, S.THETA, layer=c.layer, rope_rows=c.rope_rows, rope_per_member=c.per_member)
    assert gg.stream_attn_burst_launches() - b0 == 1 and launches_since(pkg, before) == {}, (gg.stream_attn_burst_launches() - b0, launches_since(pkg, before))
    return got


def held(c, out, ref):
    assert out.shape == ref.shape and np.isfinite(out).all(), f"{(~np.isfinite(out)).sum()} output values are not finite"
    e = S.row_err(out, ref, c.H)
    w = float(e.max()); r, h = np.unravel_index(int(np.argmax(e)), e.shape); z, m = divmod(int(r), c.rows)
    print(f"{S.case_id(c)}: worst row {w:.2e} of its max (slot {z} = member {c.order[z]}, row {m}, {S.window_of(c, c.order[z], m)[1]} keys, head {h})")
    WORST[(c.hd, c.kind)] = max(WORST.get((c.hd, c.kind), 0.0), w)
    bad = np.argwhere(e > S.BAR)
    assert not len(bad), (f"{len(bad)} rows past 2e-5 of their max, worst {w / S.BAR:.1f} x the bar at slot {z} (member {c.order[z]} at {c.enc_pos[c.order[z]]}), row {m}, "
                          f"{S.window_of(c, c.order[z], m)[1]} keys from {S.window_of(c, c.order[z], m)[0]}, head {h}; first (row, head): {bad[:6].tolist()}")


def run_case(pkg, gg, ctx, c):
    _, inp, (ref, kapp, kmag) = S.cached(c, gg.rope_rows)
    out, kring, vring = launch(pkg, gg, ctx, c, inp)
    held(c, out, ref)
    S.check_rings(c, inp, kapp, kmag, kring, vring)
    ASSERTED.add(c.hd)
    return out, kring, vring


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_burst_case(pkg, gg, ctx, c):
    """One row of the table: one burst launch; the output, the appended K and V rows and every other ring word are held."""
    run_case(pkg, gg, ctx, c)
    PASSED.add(S.case_id(c))


@pytest.mark.parametrize("kind", ("normal", "peaked"))
@pytest.mark.parametrize("b", (2, 3, 16))
@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_one_burst_is_the_chain_of_ticks_bit_for_bit(pkg, gg, ctx, geo, b, kind):
    """The contract: one burst launch of 4 b rows against b chained launches of the tick kernel with 4 rows each, enc_pos moving by 4 and the rings fed back -- every
    word of out, kring and vring.  3 of 5 members in the order 2, 0, 1 in layer 1 of 3: an unfilled window, a window across the wrap, rows across the wrap."""
    M = 4 * b
    c = real_case(kind, geo, rows=M)
    _, inp, (ref, kapp, kmag) = S.cached(c, gg.rope_rows)
    out, kring, vring = launch(pkg, gg, ctx, c, inp)
    held(c, out, ref); S.check_rings(c, inp, kapp, kmag, kring, vring)      # (the burst is right, not only equal)
    ck, cv = inp.kring, inp.vring
    cout = np.empty_like(out)
    before = attn_launches(pkg)
    for t in range(b):
        rows = np.concatenate([np.arange(z * M + 4 * t, z * M + 4 * t + 4) for z in range(len(c.order))])
        o, ck, cv = gg.stream_attn(ctx, inp.qkv[rows], ck, cv, c.order, tuple(p + 4 * t for p in c.enc_pos), 4, c.window, S.THETA, layer=c.layer)
        cout[rows] = o
    assert launches_since(pkg, before) == {"stream_ring": b}
    for name, a, w in (("out", out, cout), ("kring", kring, ck), ("vring", vring, cv)):
        d = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(w).view(np.uint32))
        assert not len(d), f"{len(d)} words of {name} differ from the chain of {b} ticks; first: {d[:4].tolist()}"
    ASSERTED.add(c.hd); PASSED.add(f"chain-{geo[0]}-{b}-{kind}")


def test_refusals_launch_nothing(pkg, gg, ctx):
    """rows 65, cap = window + rows and head_dim 32 end in a VoxError before any launch: neither the burst counter nor an attention slot moves.  A valid launch then passes."""
    c = S.make_case("refuse", "normal", S.GEOS[0], 12, 40, 64, (1, 0), (100, 17))
    _, inp, _ = S.cached(c, gg.rope_rows)
    W = inp.qkv.shape[1]

    def refused(word, qkv=inp.qkv, kring=inp.kring, rows=12, **kw):
        before, b0 = attn_launches(pkg), gg.stream_attn_burst_launches()
        with pytest.raises(pkg.VoxError) as e:
            gg.stream_attn_burst(ctx, qkv, kring, kring, c.order, c.enc_pos, rows, 40, S.THETA, **kw)
        assert e.value.code == 1 and word in str(e.value), e.value
        assert launches_since(pkg, before) == {} and gg.stream_attn_burst_launches() == b0

    refused("rows 65", qkv=np.zeros((130, W), np.float32), rows=65, kring=np.zeros((2, 1, 3, 128, 64), np.float32))
    refused("rows 0", qkv=np.zeros((0, W), np.float32), rows=0)
    refused("cap 52", kring=np.zeros((2, 1, 3, 52, 64), np.float32))                      # cap == window + rows
    refused("head_dim 32", qkv=np.zeros((24, 3 * 3 * 32), np.float32), kring=np.zeros((2, 1, 3, 64, 32), np.float32))
    refused("rope_rows 8", rope_rows=8)                                                   # a RoPE ring shorter than the 12 rows
    run_case(pkg, gg, ctx, c)
    PASSED.add("refusals")


def test_both_head_sizes_were_asserted():
    """Every row of the table and every chain ran and passed, and each head size was the asserted launch of a passing case."""
    for (hd, kind), w in sorted(WORST.items()):
        print(f"worst error, hd {hd:3d} {kind:8s}: {w:.2e} of the row's max (bar {S.BAR:.0e})")
    want = set(CASE_IDS) | {f"chain-{g[0]}-{b}-{kd}" for g in S.GEOS for b in (2, 3, 16) for kd in ("normal", "peaked")} | {"refusals"}
    assert want <= PASSED, f"{len(want - PASSED)} rows of the table did not pass: {sorted(want - PASSED)[:8]}"
    assert ASSERTED == {64, 128}, f"no passing case asserted head_dim {sorted({64, 128} - ASSERTED)}"
