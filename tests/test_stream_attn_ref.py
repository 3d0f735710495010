"""Pins tests/stream_attn_ref.py on the CPU, so that tests/test_gpu_stream_attn.py can fail: the float64 reference of the live sessions' ring attention agrees with a
dense masked softmax written independently (rotation as a complex product, one score matrix under a boolean mask); it leaves the bar by more than 100x when it is
made wrong the way a kernel could be; and a float32 restatement of the kernel's arithmetic stays inside the bar at the largest key counts.  No device: the RoPE rows
come from vox_debug_rope_rows, which is host arithmetic.

Which mutation must move what, from the inputs alone:
  early      a window that starts one key early admits the row in front of it: V = 1e6 (1e24) in front of row 0's window, the previous row's first key (V x 100)
             otherwise.  Row 0 of every member whose window has moved leaves the bar by 100x, in every kind.
  late       (per case: one row's first key may weigh e^-5 of its neighbours by chance) drops the first key: V x 100 (normal), 0.5 / n of a column against a row of a few 0.5 / sqrt(n) (uniform).  Peaked rows give that key a weight of
             e^-35 unless it is the peak itself (slot % 4 == 3): peaked cases are asserted where they have four slots.
  drop_last  drops the query's own key: as `late`, per case.
  rope+-1, swap   move every appended K component by about its own size, in every kind; the output moves wherever a query has ring keys and q != 0 (the tick's
             own keys turn with the query: their scores do not change; uniform's q = 0 sees no rotation at all; a peaked row keeps its peak -- most pairs of a
             head turn by far less than a radian per position, the aligned key stays e^20 above the rest and the output stays that key's V row: normal alone).
  by_slot    member rings indexed by the slot: with a permuted order the row read is another member's, or NaN.
"""
from importlib import import_module

import numpy as np
import pytest

import stream_attn_ref as S

FAR = 100 * S.BAR
G64, G128 = S.GEOS
PIN = ([S.seam_case(kd, g, 1) for g in S.GEOS for kd in S.KINDS] + [S.seam_case("normal", g, 4) for g in S.GEOS] + [S.seam_case("uniform", G64, 8), S.seam_case("peaked", G128, 4)] +
       [S.real_case(kd, G64, 760) for kd in S.KINDS] + [S.real_case("normal", G128, 755)] + [S.tiny_case(kd, g) for g in S.GEOS for kd in S.KINDS] +
       [S.far_case("normal", G64, False), S.far_case("peaked", G128, True), S.far_case("uniform", G64, True)] + S.exact_ring_cases("normal", G64) + S.mode_cases(G128))
PIN_IDS = [S.case_id(c) for c in PIN]


@pytest.fixture(scope="module")
def rows_fn(pkg):
    return import_module(pkg.__name__ + ".gguf").rope_rows


def moved(c):
    """Members whose first query's window has moved (j0 > 0) / that read ring keys at all."""
    return [mb for mb in c.order if c.enc_pos[mb] > c.window], [mb for mb in c.order if c.enc_pos[mb] > 0]


def test_table_is_what_the_issue_asks_for():
    t = S.table()
    assert {(c.hd, c.H) for c in t} == {(64, 3), (128, 2)} and {c.rows for c in t} >= {1, 4, 8}
    for geo in S.GEOS:
        nk = {S.window_of(c, mb, m)[1] for c in t if (c.hd, c.H) == geo for mb in c.order for m in range(c.rows)}
        assert nk >= {1, 2, 15, 16, 17, 63, 64, 65, 255, 256, 257, 751, 1023, 1024}, sorted(nk)
        assert any(n % (256 // geo[0]) for n in nk)
    for c in t:
        assert len({c.enc_pos[mb] for mb in c.order}) == len(c.order)                      # the members of one launch stand at different positions
        assert c.cap > c.window + c.rows and c.window + 1 <= 1024 and max(c.enc_pos) + c.rows <= (1 << 24 if c.rope_rows else S.TABLE_LEN)
    assert any(c.cap == c.window + c.rows + 1 for c in t) and {c.cap for c in t} >= {14, 755, 760, 768}
    assert any(c.layers == 3 and c.layer == 1 for c in t) and any(len(c.enc_pos) > len(c.order) for c in t)
    assert {len(c.order) for c in t} >= {1, 3, 16} and any(c.order == (2, 0, 1) for c in t) and any(c.order == tuple(reversed(range(16))) for c in t)
    # the tick's rows straddling the ring's wrap, a window straddling it, the window's first move inside a tick, a first tick
    assert any((c.enc_pos[mb] % c.cap) + c.rows > c.cap for c in t for mb in c.order)
    assert any(c.enc_pos[mb] > c.window and c.enc_pos[mb] % c.cap < c.window for c in t for mb in c.order)
    assert any(c.enc_pos[mb] <= c.window < c.enc_pos[mb] + c.rows - 1 for c in t for mb in c.order) and any(c.enc_pos[mb] == 0 for c in t for mb in c.order)
    far = {c.enc_pos[mb] for c in t if c.rope_rows for mb in c.order}
    assert far >= {65534, 1000003, (1 << 24) - 9} and any(c.rope_rows == c.rows for c in t) and any(c.per_member for c in t) and any(c.rope_rows and not c.per_member for c in t)


@pytest.mark.parametrize("c", PIN, ids=PIN_IDS)
def test_reference_agrees_with_a_dense_masked_softmax(rows_fn, c):
    rope, inp, (ref, _, _) = S.cached(c, rows_fn)
    assert np.isfinite(ref).all()
    e = S.row_err(S.reference_dense(c, inp, rope), ref, c.H)
    assert e.max() <= 1e-11, e.max()


@pytest.mark.parametrize("c", PIN, ids=PIN_IDS)
def test_hostile_inputs(rows_fn, c):
    """NaN wherever nothing live is, V = 1e6 in front of the first query's window (the row in front of it included), appended rows NaN before the launch."""
    _, inp, _ = S.cached(c, rows_fn)
    w = S.appended(c)
    assert np.isnan(inp.kring[w]).all() and np.isnan(inp.vring[w]).all()
    for mb in range(len(c.enc_pos)):
        for l in range(c.layers):
            if mb not in c.order or l != c.layer:
                assert np.isnan(inp.kring[mb, l]).all() and np.isnan(inp.vring[mb, l]).all()
    for mb in c.order:
        ep = c.enc_pos[mb]; j0 = max(0, ep - c.window)
        live = np.arange(max(0, ep - c.cap + c.rows), ep)
        assert np.isfinite(inp.kring[mb, c.layer][:, live % c.cap]).all()
        dead = np.setdiff1d(np.arange(c.cap), live % c.cap)
        assert np.isnan(inp.kring[mb, c.layer][:, dead]).all() and np.isnan(inp.vring[mb, c.layer][:, dead]).all()
        if j0 > 0:
            assert (inp.vring[mb, c.layer][:, (j0 - 1) % c.cap] == np.float32(S.FRONT_V[c.kind])).all() and (j0 - 1) % c.cap not in (ep + np.arange(c.rows)) % c.cap
    assert len(np.unique(inp.kring.view(np.uint32)[~np.isfinite(inp.kring)])) > 1      # NaN payloads differ


@pytest.mark.parametrize("c", PIN, ids=PIN_IDS)
def test_a_wrong_reference_leaves_the_bar_by_100x(rows_fn, c):
    rope, inp, (ref, kapp, kmag) = S.cached(c, rows_fn)
    has_moved, has_ring = moved(c)
    M = c.rows

    def err(mut):
        out, k2, _ = S.reference(c, inp, rope, mutate=mut)
        with np.errstate(invalid="ignore"):
            kerr = np.abs(k2 - kapp) / np.maximum(S.K_BAR * kmag, 1e-300)
        return S.row_err(out, ref, c.H), float(np.where(np.isfinite(kerr), kerr, np.inf).max())

    if has_moved:
        e, _ = err("early")
        assert e.max() > FAR
        rows = [z * M for z, mb in enumerate(c.order) if mb in has_moved]      # row 0 of every moved member admits a V = 1e6 row
        assert (e[rows] > FAR).all(), e[rows].min()
    if c.kind != "peaked" or len(c.order) >= 4:
        for mut in ("late", "drop_last"):
            e, _ = err(mut)
            assert e.max() > FAR, (mut, e.max())
    for mut in ("rope+1", "rope-1", "swap"):
        e, ke = err(mut)
        assert ke > 100, (mut, ke)                      # appended K: 100x its own bar
        if has_ring and c.kind == "normal":
            assert e.max() > FAR, (mut, e.max())
    if c.per_member and c.order != tuple(range(len(c.order))):
        e, ke = err("by_slot")
        assert e.max() > FAR and ke > 100


@pytest.mark.parametrize("kind", S.KINDS)
@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_f32_restatement_stays_inside_the_bar(rows_fn, geo, kind):
    """The kernel's arithmetic in float32 (sequential dot, f32 exp, sums strided by 256, V sums in 256 / hd groups) at 1 .. 1024 keys: the bar leaves room for it."""
    worst = 0.0
    for rows in (1, 4):
        c = S.seam_case(kind, geo, rows)
        rope, inp, (ref, _, _) = S.cached(c, rows_fn)
        e = S.row_err(S.reference_f32(c, inp, rope), ref, c.H)
        worst = max(worst, float(e.max()))
    print(f"f32 restatement, hd {geo[0]} {kind}: worst row {worst:.2e} of its max (bar {S.BAR:.0e})")
    assert worst <= S.BAR
