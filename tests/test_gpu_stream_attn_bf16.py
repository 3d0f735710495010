"""The encoder ring attention on a bf16 ring (stream_attn_kernel<.., uint16_t> and both forms of stream_attn_burst_kernel<.., uint16_t>, csrc/vox_kernels.hip) through
vox_debug_stream_attn_elem, one launch at a time.  Inputs and the bar are tests/stream_attn_ref.py's; the f32 rings it builds are rounded by vox_kv_round_bf16.

One geometry per head size serves every form: window 20, 3 of 4 members in the order 2, 0, 1 -- member 0 has not filled its window (position 7), member 1 stands at
window + 1, member 2 two rows in front of its ring's second wrap -- in a ring of the smallest legal capacity, window + rows + 1, so member 2's window straddles the
wrap; once with the flat RoPE table and once with a RoPE ring per member.  Forms: the tick launch (4 rows), bursts of b = 2 and b = 16, and a ragged round of
b = 3, 1, 2.

Held per case:
  out        against float64 windowed causal attention over the ring AS READ BACK and widened (it holds the launch's own rounded rows), q rotated in float64: the f32
             kernel's bar, stream_attn_ref.BAR per (row, head) -- the arithmetic on the widened values is the f32 kernel's;
  appended   the rows the launch owns equal vox_kv_round_bf16 of the rows the f32 kernel appends for the same (widened) inputs, bit for bit;
  the rest   every other 16-bit ring word is untouched.
Bit for bit between the forms: a burst, and every slot of a ragged round, leaves the `out` and ring words of the chain of its tick launches; two ring capacities
give the same `out`."""
from importlib import import_module

import numpy as np
import pytest

import stream_attn_ref as S

pytestmark = pytest.mark.gpu
WINDOW = 20
FORMS = {"tick": ("tick", (4, 4, 4)), "burst2": ("burst", (8, 8, 8)), "burst16": ("burst", (64, 64, 64)), "ragged": ("ragged", (12, 4, 8))}
MODES = {"flat": {}, "ring64pm": dict(rope_rows=64, per_member=True)}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def widen(u16):
    return (np.ascontiguousarray(u16).astype(np.uint32) << 16).view(np.float32)


def make(gg, geo, rows_z, mode, cap=None):
    """(case, its inputs, its 16-bit rings, the rotated float64 q per slot); rows = the largest slot's, every slot's first rows_z[z] rows are used.  cap None: the
    smallest legal one, whose second wrap member 2 straddles (the positions do not depend on `cap`)"""
    M = max(rows_z); least = WINDOW + M + 1
    c = S.make_case(f"bf16-{M}", "normal", geo, M, WINDOW, cap or least, (2, 0, 1), (7, WINDOW + 1, 2 * least - 2, 50), layers=2, layer=1, **MODES[mode])
    rope, inp, _ = S.cached(c, gg.rope_rows)
    qr = [S.rotated_tick(c, inp, rope, z)[0][:rows_z[z]] for z in range(3)]
    return c, inp, gg.kv_round_bf16(inp.kring), gg.kv_round_bf16(inp.vring), qr


def slot_rows(c, inp, rows_z, t0=0, n=None):
    """qkv rows t0 .. t0 + n - 1 of every slot that has them, slot after slot (n None: all of the slot's)"""
    return np.concatenate([inp.qkv[z * c.rows + t0:z * c.rows + (rows_z[z] if n is None else t0 + n)] for z in range(3) if rows_z[z] > t0])


def launch(gg, ctx, c, qkv, k, v, form, rows_z, dtype="bf16", order=None, enc_pos=None):
    rows = rows_z if form == "ragged" else rows_z[0]
    return gg.stream_attn_elem(ctx, qkv, k, v, order or c.order, enc_pos or c.enc_pos, rows, c.window, S.THETA, form=form, enc_kv_dtype=dtype, layer=c.layer,
                               rope_rows=c.rope_rows, rope_per_member=c.per_member)


def owned(c, rows_z):
    mask = np.zeros((len(c.enc_pos), c.layers, c.H, c.cap, c.hd), bool)
    for z, mb in enumerate(c.order):
        mask[mb, c.layer][:, (c.enc_pos[mb] + np.arange(rows_z[z])) % c.cap] = True
    return mask


def chain(gg, ctx, c, inp, k, v, rows_z):
    """the tick launches of every slot, 4 rows at a time with the rings fed back -> (out in the ragged layout, kring, vring)"""
    start = np.concatenate([[0], np.cumsum(rows_z)]); out = np.empty((start[-1], c.H * c.hd), np.float32)
    for t in range(0, max(rows_z), 4):
        zs = [z for z in range(3) if rows_z[z] > t]
        o, k, v = launch(gg, ctx, c, slot_rows(c, inp, rows_z, t, 4), k, v, "tick", (4,), order=tuple(c.order[z] for z in zs), enc_pos=tuple(p + t for p in c.enc_pos))
        for i, z in enumerate(zs):
            out[start[z] + t:start[z] + t + 4] = o[4 * i:4 * i + 4]
    return out, k, v


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_bf16_ring_launch_against_float64(gg, ctx, geo, form, mode):
    form_name, rows_z = FORMS[form]
    c, inp, k16, v16, qr = make(gg, geo, rows_z, mode)
    out, k, v = launch(gg, ctx, c, slot_rows(c, inp, rows_z), k16, v16, form_name, rows_z)
    assert k.dtype == np.uint16 and out.shape == (sum(rows_z), c.H * c.hd) and np.isfinite(out).all()
    kw, vw = widen(k).astype(np.float64), widen(v).astype(np.float64)
    ref = np.empty(out.shape); r = 0
    for z, mb in enumerate(c.order):
        for m in range(rows_z[z]):
            j0, n = S.window_of(c, mb, m); at = (j0 + np.arange(n)) % c.cap
            for h in range(c.H):
                sc = kw[mb, c.layer, h, at] @ qr[z][m, h] / np.sqrt(float(c.hd)); pr = np.exp(sc - sc.max())
                ref[r, h * c.hd:(h + 1) * c.hd] = (pr @ vw[mb, c.layer, h, at]) / pr.sum()
            r += 1
    e = S.row_err(out, ref, c.H)
    print(f"{form}-hd{c.hd}-{mode}: worst row {e.max():.2e} of its max (bar {S.BAR:.0e})")
    assert (e <= S.BAR).all(), (float(e.max()), np.argwhere(e > S.BAR)[:4].tolist())
    # the appended rows: the f32 kernel's, rounded by the one function; everything else untouched
    _, kf, vf = launch(gg, ctx, c, slot_rows(c, inp, rows_z), widen(k16), widen(v16), form_name, rows_z, dtype="f32")
    w = owned(c, rows_z)
    assert w.sum() == sum(rows_z) * c.H * c.hd
    assert np.array_equal(k[w], gg.kv_round_bf16(kf)[w]) and np.array_equal(v[w], gg.kv_round_bf16(vf)[w])
    assert np.array_equal(k[~w], k16[~w]) and np.array_equal(v[~w], v16[~w])
    if form_name != "tick":      # the form against the chain of its tick launches
        cout, ck, cv = chain(gg, ctx, c, inp, k16, v16, rows_z)
        assert np.array_equal(out.view(np.uint32), cout.view(np.uint32)), np.argwhere(out != cout)[:4].tolist()
        assert np.array_equal(k, ck) and np.array_equal(v, cv)


@pytest.mark.parametrize("form", ("tick", "burst16"))
@pytest.mark.parametrize("geo", S.GEOS, ids=("hd64", "hd128"))
def test_ring_capacity_changes_addresses_only(gg, ctx, geo, form):
    form_name, rows_z = FORMS[form]
    outs = []
    for cap in (None, 128):      # the same logical keys (stream_attn_ref generates them by position) in the smallest ring and in one of 128 rows
        c, inp, k16, v16, _ = make(gg, geo, rows_z, "flat", cap=cap)
        outs.append(launch(gg, ctx, c, inp.qkv, k16, v16, form_name, rows_z)[0])
    assert np.isfinite(outs[0]).all() and np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_an_unknown_dtype_or_form_is_refused(pkg, ctx):
    """(form, dtype) outside 0..2 x {VOX_KV_F32, VOX_KV_BF16} ends in VOX_ERR_INVALID before anything else is looked at"""
    for form, dtype in ((0, 2), (3, 1), (0, -1)):
        assert pkg.lib().vox_debug_stream_attn_elem(ctx.h, None, form, dtype, None, None, None, None, None) == 1
