"""The live sessions' encoder ring attention (stream_attn_kernel<64> / <128> behind launch_stream_attn, csrc/vox_kernels.hip: RoPE on q and k, the K / V append into
each session's ring and the windowed softmax in one launch, enc_layers times in every tick of every vox_stream and stream group) against a float64 reference, one
launch at a time through vox_debug_stream_attn; and launch_stream_ring_init, which seeds the rings, through vox_debug_stream_ring_init.  The reference, the inputs and
the case table are tests/stream_attn_ref.py, pinned on the CPU by tests/test_stream_attn_ref.py.

Held per case, after exactly ONE `stream_ring` launch (vox_debug_attn_launches [8]):
  out         per (row, head) |out - ref| <= 2e-5 max|ref of that row and head| -- the suite's f32-class bar, row by row (stream_attn_ref.BAR); every value finite;
  appended K  componentwise |k - ref| <= 2^-22 (|xr| + |xi|): the rotation is two products and one sum, each rounded once, contracted or not;
  appended V  the input's bits;
  the rest    every other ring word -- the other rows, the other layers, the members no slot serves -- its bits from before the launch, NaN payloads included.
The table (stream_attn_ref.table): head_dim 64 with 3 heads and 128 with 2; the key counts 1, 2, 15 .. 17, 63 .. 65, 255 .. 257, 751, 1023, 1024 as 16 members of
one launch under window 1023, with 1, 4 and 8 rows per tick (a first tick, j0 = 0, the window's first move at every row of a tick, tick rows and windows that straddle
the ring's wrap, cap = window + rows + 1); the real window 750 at cap 755 / 760 / 768 in layer 1 of 3 with 3 of 5 members served in the order 2, 0, 1; window 5 in a
ring of 14; one slot; RoPE rows from the flat table, from one ring of 32 rows and from a ring per member, at ticks across the table length (65 534 .. 65 537, where the
rows switch to the double-precision angle), at 1 000 003 and at 2^24 - 9; RoPE rings of exactly `rows` rows.  Properties, bit for bit: the ring capacity and the layer
change addresses only; a member's rows do not depend on the slots around it or on its slot; the three RoPE modes agree; and a chain of 40 ticks fed back through the
entry is the float64 windowed causal attention over its 160 rows.  The last test fails if either head size was never the asserted launch of a passing case.

That the table can fail was checked once on an MI355X with five temporary mutations of stream_attn_kernel, each changing a value or reading FEWER rows, no address,
bound or loop widened.  Of the 72 tests (56 table cases, 8 property tests, the refusal test, 6 ring-seeding tests, the closing test):
  * j0 = qpos - window + 1 (the window starts one key late) -> 64 fail: every table case but seam1-peaked at both head sizes (with one row per tick only two members
    stand past the window there, and their peaks are not the first key: a dropped key of weight e^-35 cannot show), all four properties, the refusal test's closing
    launch; the six ring-seeding tests pass, as they must;
  * the V loop ending at nk - 1 -> 66 fail: every table case in every kind (the query's own V row), every property, the closing launch;
  * wave 3's partial left out of `sum` -> 57 fail: every case with more than 192 keys in some row (that wave's first score); tiny (6 keys), the 21-key chain and the
    41-key closing launch of the refusal test pass, as they must;
  * the sign of sn flipped on k only -> 66 fail: every table case, the uniform kind included (q = 0 hides it from the output, the appended K's bound does not), every
    property, the chain, the closing launch;
  * order[blockIdx.z] replaced by blockIdx.z in the RoPE-ring index -> 13 fail: the member-ring cases far-*-ring32pm and exact4-*-ring4pm (NaN or another member's
    row), test_rope_modes_agree; every flat-table and one-ring case passes, exact8 (one ring, one slot) included, as they must.
Each mutation also fails test_both_head_sizes_were_asserted.
"""
from importlib import import_module

import numpy as np
import pytest

import stream_attn_ref as S
from model_fixtures import attn_launches, launches_since

pytestmark = pytest.mark.gpu

CASES = S.table()
CASE_IDS = [S.case_id(c) for c in CASES]
WORST = {}            # (hd, kind, RoPE mode) -> worst row error as a multiple of the row's max|ref|
WORST_K = {}          # hd -> worst appended-K error as a multiple of its bound
PASSED, ASSERTED = set(), set()


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def launch(pkg, gg, ctx, c, inp):
    """ONE launch of the case on `inp`; asserts that exactly one stream_ring launch ran.  Returns (out, kring, vring)."""
    before = attn_launches(pkg)
    got = gg.stream_attn(ctx, inp.qkv, inp.kring, inp.vring, c.order, c.enc_pos, c.rows, c.window, S.THETA, layer=c.layer, rope_rows=c.rope_rows, rope_per_member=c.per_member)
    ran = launches_since(pkg, before)
    assert ran == {"stream_ring": 1}, f"expected one stream_ring launch, the entry ran {ran}"
    return got


def held(c, out, ref):
    """The output's bar, per (row, head); records the worst error of (hd, kind, RoPE mode)."""
    assert out.shape == ref.shape and np.isfinite(out).all(), f"{(~np.isfinite(out)).sum()} output values are not finite"
    e = S.row_err(out, ref, c.H)
    w = float(e.max()); r, h = np.unravel_index(int(np.argmax(e)), e.shape); z, m = divmod(int(r), c.rows)
    print(f"{S.case_id(c)}: worst row {w:.2e} of its max (slot {z} = member {c.order[z]}, row {m}, {S.window_of(c, c.order[z], m)[1]} keys, head {h})")
    key = (c.hd, c.kind, S.rope_mode(c)); WORST[key] = max(WORST.get(key, 0.0), w)
    bad = np.argwhere(e > S.BAR)
    assert not len(bad), (f"{len(bad)} rows past 2e-5 of their max, worst {w / S.BAR:.1f} x the bar at slot {z} (member {c.order[z]} at {c.enc_pos[c.order[z]]}), row {m}, "
                          f"{S.window_of(c, c.order[z], m)[1]} keys from {S.window_of(c, c.order[z], m)[0]}, head {h}; first (row, head): {bad[:6].tolist()}")


def run_case(pkg, gg, ctx, c):
    _, inp, (ref, kapp, kmag) = S.cached(c, gg.rope_rows)
    out, kring, vring = launch(pkg, gg, ctx, c, inp)
    held(c, out, ref)
    wk = S.check_rings(c, inp, kapp, kmag, kring, vring)
    WORST_K[c.hd] = max(WORST_K.get(c.hd, 0.0), wk)
    ASSERTED.add(c.hd)
    return out, kring, vring


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("c", CASES, ids=CASE_IDS)
def test_stream_attn_case(pkg, gg, ctx, c):
    """One row of the table: one stream_ring launch; the output, the appended K and V rows and every other ring word are held."""
    run_case(pkg, gg, ctx, c)
    PASSED.add(S.case_id(c))


@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_ring_capacity_changes_addresses_only(pkg, gg, ctx, geo):
    """The same logical keys in rings of 758, 760, 768 and 2012 rows: the same output bits and the same appended rows (the kernel walks the window by key index)."""
    base = None
    for cap in S.CAPS:
        c = S.cap_case(geo, cap)
        out, kring, vring = run_case(pkg, gg, ctx, c)
        rows = [(S.ring_rows(c, kring, z), S.ring_rows(c, vring, z)) for z in range(len(c.order))]
        if base is None:
            base = (out, rows)
        else:
            assert same_bits(out, base[0]), f"cap {cap}: {np.argwhere(out != base[0])[:4].tolist()}"
            assert all(same_bits(a[0], b[0]) and same_bits(a[1], b[1]) for a, b in zip(rows, base[1]))
    PASSED.add(f"caps-{geo[0]}")


@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_a_member_does_not_depend_on_its_slot_or_the_other_slots(pkg, gg, ctx, geo):
    """Members of the 16-slot seam launch again, alone (slot 0 of one) and as the second of two slots: their rows and their appended ring rows have the bits of the
    16-slot launch."""
    c16 = S.seam_case("normal", geo, 4)
    _, inp, _ = S.cached(c16, gg.rope_rows)
    out16, k16, v16 = run_case(pkg, gg, ctx, c16)
    M, QD = c16.rows, c16.H * c16.hd
    for order in ((11,), (0,), (3, 15), (15, 3)):
        c = c16._replace(name="alone", order=order)
        qkv = np.concatenate([inp.qkv[c16.order.index(mb) * M:(c16.order.index(mb) + 1) * M] for mb in order])
        out, kring, vring = launch(pkg, gg, ctx, c, S.Inputs(qkv, inp.kring, inp.vring))
        for z, mb in enumerate(order):
            z16 = c16.order.index(mb)
            assert same_bits(out[z * M:(z + 1) * M], out16[z16 * M:(z16 + 1) * M]), (order, mb)
            assert same_bits(S.ring_rows(c, kring, z), S.ring_rows(c16, k16, z16)) and same_bits(S.ring_rows(c, vring, z), S.ring_rows(c16, v16, z16))
        w = S.appended(c)
        assert np.array_equal(kring.view(np.uint32)[~w], inp.kring.view(np.uint32)[~w]) and np.array_equal(vring.view(np.uint32)[~w], inp.vring.view(np.uint32)[~w])
        assert out.shape == (len(order) * M, QD)
    PASSED.add(f"slots-{geo[0]}")


@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_rope_modes_agree(pkg, gg, ctx, geo):
    """The flat table, one RoPE ring and a ring per member at positions all three serve: the same output and ring bits (the rows are one function's)."""
    flat, ring, per_member = S.mode_cases(geo)
    base = run_case(pkg, gg, ctx, flat)
    for c in (ring, per_member):
        got = run_case(pkg, gg, ctx, c)
        assert all(same_bits(a, b) for a, b in zip(got, base)), S.case_id(c)
    PASSED.add(f"modes-{geo[0]}")


@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_chain_of_ticks_is_windowed_causal_attention(pkg, gg, ctx, geo):
    """40 ticks of 4 rows from position 0, window 20 in a ring of 32, the rings fed back through the entry: every row against the float64 windowed causal attention
    over the whole 160-row sequence.  The test rotates no ring row: the kernel reads what it appended, across five wraps."""
    hd, H = geo; M, W, CAP, T = 4, 20, 32, 40; QD = H * hd; N = M * T
    rng = np.random.default_rng([hd, 4020])
    qkv = np.concatenate([1.5 * rng.standard_normal((N, QD)), rng.standard_normal((N, 2 * QD))], axis=1).astype(np.float32)
    _, cos, sin = gg.rope_rows(hd, S.THETA, 0, N)
    q, k, v = (qkv[:, i * QD:(i + 1) * QD].reshape(N, H, hd).astype(np.float64) for i in range(3))
    qr = S.rotate(q, cos[:, None, :].astype(np.float64), sin[:, None, :].astype(np.float64)); kr = S.rotate(k, cos[:, None, :].astype(np.float64), sin[:, None, :].astype(np.float64))
    pos = np.arange(N); mask = (pos[None, :] <= pos[:, None]) & (pos[:, None] - pos[None, :] <= W)
    ref = np.empty((N, QD))
    for h in range(H):
        s = np.where(mask, qr[:, h] @ kr[:, h].T / np.sqrt(float(hd)), -np.inf)
        p = np.exp(s - s.max(axis=1, keepdims=True))
        ref[:, h * hd:(h + 1) * hd] = (p @ v[:, h]) / p.sum(axis=1, keepdims=True)
    kring = S.nan_words((1, 1, H, CAP, hd), 5); vring = S.nan_words(kring.shape, 9)
    out = np.empty((N, QD), np.float32)
    before = attn_launches(pkg)
    for t in range(T):
        out[t * M:(t + 1) * M], kring, vring = gg.stream_attn(ctx, qkv[t * M:(t + 1) * M], kring, vring, (0,), (t * M,), M, W, S.THETA)
    assert launches_since(pkg, before) == {"stream_ring": T}
    c = S.make_case("chain", "normal", geo, M, W, CAP, (0,), (0,))
    held(c._replace(rows=N), out, ref)      # (rows = N: one slot of 160 rows for the report)
    last = (N - CAP + np.arange(CAP)) % CAP      # the ring's last 32 positions: rotated k within its bound, raw v
    kmag = np.repeat(np.abs(k[N - CAP:, :, 0::2]) + np.abs(k[N - CAP:, :, 1::2]), 2, axis=-1)
    assert (np.abs(kring[0, 0][:, last].transpose(1, 0, 2) - kr[N - CAP:]) <= S.K_BAR * kmag).all()
    assert same_bits(vring[0, 0][:, last].transpose(1, 0, 2), qkv[N - CAP:, 2 * QD:].reshape(CAP, H, hd))
    PASSED.add(f"chain-{hd}")


def test_refusals_launch_nothing(pkg, gg, ctx):
    """What launch_stream_attn would refuse -- rows 0 or 9, 17 slots, window + 1 > 1024, cap <= window + rows, head_dim 32, a RoPE ring shorter than the rows or
    no power of two -- and what would leave the uploaded buffers ends in a VoxError before any launch; slot [8] stays where it was.  A valid launch then passes."""
    c = S.make_case("refuse", "normal", S.GEOS[0], 4, 40, 48, (1, 0), (100, 17))
    _, inp, _ = S.cached(c, gg.rope_rows)

    def refused(word, qkv=inp.qkv, kring=inp.kring, order=c.order, enc_pos=c.enc_pos, rows=4, window=40, **kw):
        before = attn_launches(pkg)
        with pytest.raises(pkg.VoxError) as e:
            gg.stream_attn(ctx, qkv, kring, kring, order, enc_pos, rows, window, S.THETA, **kw)
        assert e.value.code == 1 and word in str(e.value), e.value
        assert launches_since(pkg, before) == {}

    W = inp.qkv.shape[1]
    refused("rows 0", qkv=np.zeros((0, W), np.float32), rows=0)
    refused("rows 9", qkv=np.zeros((18, W), np.float32), rows=9, kring=np.zeros((2, 1, 3, 64, 64), np.float32))
    refused("n_slots 17", qkv=np.zeros((17, W), np.float32), rows=1, order=tuple(range(17)), enc_pos=tuple(range(17)), kring=np.zeros((17, 1, 3, 48, 64), np.float32))
    refused("window 1024", window=1024, kring=np.zeros((2, 1, 3, 1100, 64), np.float32))
    refused("cap 44", kring=np.zeros((2, 1, 3, 44, 64), np.float32))                      # cap == window + rows
    refused("head_dim 32", qkv=np.zeros((8, 3 * 3 * 32), np.float32), kring=np.zeros((2, 1, 3, 48, 32), np.float32))
    refused("rope_rows 2", rope_rows=2)                                                   # shorter than the 4 rows
    refused("rope_rows 24", rope_rows=24)                                                 # no power of two
    refused("rope_rows 1", qkv=np.zeros((2, W), np.float32), rows=1, rope_rows=1)         # mask 0 would mean "a flat table"
    refused("rope_per_member", rope_per_member=True)
    refused("cannot hold positions", enc_pos=(100, 68), rope_rows=32)                     # positions 100 and 68 share a row of one ring of 32
    refused("order[1] = 2", order=(1, 2))
    refused("a member is served by one slot", order=(1, 1))
    refused("enc_pos[0]", enc_pos=(65533, 17))                                            # the flat table ends at 65 536
    refused("enc_pos[1]", enc_pos=(100, (1 << 24) - 3), rope_rows=32, rope_per_member=True)
    refused("enc_pos[1]", enc_pos=(100, -1))
    refused("layer 1 of 1", layer=1)
    run_case(pkg, gg, ctx, c)                                                             # the context is still usable
    PASSED.add("refusals")


@pytest.mark.parametrize("hd", (64, 128))
@pytest.mark.parametrize("rows", (1, 5, 9))
def test_ring_init_seeds_rows_and_touches_nothing_else(pkg, gg, ctx, rows, hd):
    """launch_stream_ring_init: rows 0 .. rows - 1 of every layer and head are the transposed token-major input, bit for bit (rows 1, 5 and cap = 9; 2 layers, 3
    heads); every other ring word keeps its bits.  rows 0 and rows > cap are refused."""
    L, H, CAP = 2, 3, 9
    rng = np.random.default_rng([hd, rows, 31])
    kv = rng.standard_normal((L, rows, 2 * H * hd)).astype(np.float32)
    kv.view(np.uint32)[0, 0, :4] = (0x7fc01234, 0xffc00001, 0x80000000, 0x00000001)      # NaN payloads, -0.0 and a denormal travel as bits
    k0 = S.nan_words((L, H, CAP, hd), 3); v0 = S.nan_words(k0.shape, 1001)
    before = attn_launches(pkg)
    kring, vring = gg.stream_ring_init(ctx, kv, k0, v0)
    assert launches_since(pkg, before) == {}      # (not an attention launch)
    want_k = kv[:, :, :H * hd].reshape(L, rows, H, hd).transpose(0, 2, 1, 3); want_v = kv[:, :, H * hd:].reshape(L, rows, H, hd).transpose(0, 2, 1, 3)
    assert same_bits(kring[:, :, :rows], want_k) and same_bits(vring[:, :, :rows], want_v)
    assert same_bits(kring[:, :, rows:], k0[:, :, rows:]) and same_bits(vring[:, :, rows:], v0[:, :, rows:])
    for bad in (np.zeros((L, 0, 2 * H * hd), np.float32), np.zeros((L, CAP + 1, 2 * H * hd), np.float32)):
        with pytest.raises(pkg.VoxError) as e:
            gg.stream_ring_init(ctx, bad, k0, v0)
        assert e.value.code == 1 and f"rows {bad.shape[1]}" in str(e.value)


def test_both_head_sizes_were_asserted():
    """Every row of the table and every property ran and passed, and each head size was the asserted launch of a passing case.  Prints the worst row error per head
    size, input kind and RoPE mode (recorded in DESIGN.md)."""
    for (hd, kind, mode), w in sorted(WORST.items()):
        print(f"worst error, hd {hd:3d} {kind:8s} {mode:12s}: {w:.2e} of the row's max (bar {S.BAR:.0e})")
    for hd, w in sorted(WORST_K.items()):
        print(f"worst appended K, hd {hd:3d}: {w:.2f} of its bound 2^-22 (|xr| + |xi|)")
    want = set(CASE_IDS) | {f"{p}-{g[0]}" for p in ("caps", "slots", "modes", "chain") for g in S.GEOS} | {"refusals"}
    assert want <= PASSED, f"{len(want - PASSED)} rows of the table did not pass: {sorted(want - PASSED)[:8]}"
    assert ASSERTED == {64, 128}, f"no passing case asserted head_dim {sorted({64, 128} - ASSERTED)}"
    assert {k[:2] for k in WORST} == {(hd, kd) for hd in (64, 128) for kd in S.KINDS} and {k[2] for k in WORST} == {"flat", "one ring", "member rings"}
