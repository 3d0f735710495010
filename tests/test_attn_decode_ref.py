"""CPU pin of tests/attn_decode_ref.py: the float64 reference of the decode attention table agrees with the oracle, float32 rounding stays far inside the bar the GPU
table asserts, and the inputs CAN fail -- a reference that drops the window's first or last key, or admits the key in front of it, leaves the bar by a wide margin in
every case of the table, and in the uniform kind so does the loss of ANY single key.  Conditions on the inputs, not measurements of a kernel: a case that misses one
gets other inputs, the bar stays."""
import os
import sys

import numpy as np
import pytest

import attn_decode_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HD = R.HD


def slab_gqa_rows(pkg):
    """The slab GQA form's row limit, as attn_decode_gqa_max_seq derives it, from the code object's metadata (no device): (160 KB - static LDS) / 16 bytes."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from kernel_resources import kernel_resources
    k = [r for r in kernel_resources(pkg.build.LIB_PATH) if "attn_decode_gqa_kernel<4, false>" in r["demangled"]]
    assert len(k) == 1
    return (160 * 1024 - int(k[0][".group_segment_fixed_size"])) // 16


@pytest.fixture(scope="module")
def cases(pkg):
    return {R.case_id(c): c for c in R.logical_cases(slab_gqa_rows(pkg))}


def test_slab_gqa_limit_is_the_documented_one(pkg):
    """README.md, DESIGN.md and the header name the limit this build has; it lies between the window (a slab group must reach 8193 keys) and the session limit."""
    rows = slab_gqa_rows(pkg)
    assert R.REAL_WINDOW + 2 < rows < 16384
    shown = f"{rows // 1000} {rows % 1000:03d}"
    for doc in ("README.md", "DESIGN.md", os.path.join("include", "voxtral_hip.h")):
        assert shown in open(os.path.join(ROOT, doc)).read(), (doc, shown)


def test_table_shape():
    """The table's fixed parts: the 37 seam key counts, 40 = a multiple of 8 G for the re-map, the page-edge phases."""
    assert len(R.SEAM_POS) == 37 and len(R.SEAM40_POS) == 40 and len(set(R.SEAM40_POS)) == 40
    for H, KV in R.HEAD_GEOS:
        G = H // KV
        assert G == 1 or ((H * 40) % (8 * G) == 0 and (H * 37) % (8 * G) != 0)
    for P in (16, 64, 1024):
        seen = set()
        for c in R.page_edge_cases((4, 1), P):
            for i, p in enumerate(c.pos[:-1]):
                seen.add((p % P, R.window_of(c, i)[0] % P))
            assert R.window_of(c, len(c.pos) - 1)[0] == 0
        assert seen == {(a, b) for a in (P - 1, 0, P // 2) for b in (P - 1, 0, P // 2)}
    c = R.small_window_case("peaked", (4, 1), 200)
    assert {R.peak_index(c, i) for i in range(len(c.pos))} >= {159, 160, 0} and R.peak_index(c, 2) == R.window_of(c, 2)[1] - 1


def _all_ids():
    # (the ids do not depend on the limit: collected with a stand-in, the cases are built with the library's in the fixture)
    return [R.case_id(c) for c in R.logical_cases(9000)]


@pytest.mark.parametrize("cid", _all_ids())
def test_reference_and_inputs(pkg, orc, cases, cid):
    """One logical case: (a) the oracle, (b) float32 rounding, (c) the mutations."""
    c = cases[cid]
    q, k, v = R.build_inputs(c)
    ref = R.reference(c, q, k, v)
    n_seq = len(c.pos)
    assert np.isfinite(ref).all()
    # the hostile rows are where the docstring says
    for i, p in enumerate(c.pos):
        s = R.slice_of(c, i); j_lo, n = R.window_of(c, i)
        assert np.isnan(k[s, :, p + 1:]).all() and np.isnan(v[s, :, p + 1:]).all() and (v[s, :, :j_lo] == np.float32(R.FRONT_V[c.kind])).all() and np.isfinite(k[s, :, :p + 1]).all()
    unread = sorted(set(range(c.n_slices)) - {R.slice_of(c, i) for i in range(n_seq)})
    assert np.isnan(k[unread]).all() and np.isnan(v[unread]).all()
    # (a) orc_attention, one query row at a time: M = 1, kv_len = pos + 1, offset = pos
    got = np.zeros((n_seq, c.H * HD), np.float32)
    for i, p in enumerate(c.pos):
        s = R.slice_of(c, i)
        kt = np.ascontiguousarray(k[s, :, :p + 1].transpose(1, 0, 2).reshape(p + 1, c.KV * HD)); vt = np.ascontiguousarray(v[s, :, :p + 1].transpose(1, 0, 2).reshape(p + 1, c.KV * HD))
        o = np.zeros((1, c.H * HD), np.float32)
        orc.lib().orc_attention(np.ascontiguousarray(q[i:i + 1]), kt, vt, 1, p + 1, c.H, c.KV, HD, p, 1, c.window, o)
        got[i] = o[0]
    e_orc = R.row_err(got, ref, c.H).max()
    # (b) sequential float32
    e_f32 = R.row_err(R.reference_f32(c, q, k, v), ref, c.H)
    print(f"{cid}: oracle {e_orc:.2e}, sequential f32 {e_f32.max():.2e} of the row's max")
    assert e_orc <= 2e-5
    assert (e_f32 <= R.BAR / 4).all(), e_f32.max()
    # (c) a reference that is wrong by one key at the window's edge
    has = {"first": [i for i in range(n_seq) if R.window_of(c, i)[1] >= 2], "last": [i for i in range(n_seq) if R.window_of(c, i)[1] >= 2],
           "early": [i for i in range(n_seq) if R.window_of(c, i)[0] >= 1]}
    for mut, seqs in has.items():
        if not seqs:
            continue
        moved = R.row_err(R.reference(c, q, k, v, mutate=mut, only=seqs)[seqs], ref[seqs], c.H).max()
        assert moved >= 10 * R.BAR, (mut, moved)
    if c.kind == "uniform":      # ANY single key: with q = 0 the output is the window's mean, so losing key t gives (S - v_t) / (n - 1) -- every t at once
        for i in range(n_seq):
            j_lo, n = R.window_of(c, i)
            if n < 2:
                continue
            w = v[R.slice_of(c, i), 0, j_lo:j_lo + n].astype(np.float64)
            S = w.sum(axis=0)
            moved = np.abs((S[None, :] - w) / (n - 1) - S[None, :] / n).max(axis=1) / np.abs(S / n).max()
            assert moved.min() >= 5 * R.BAR, (i, n, moved.min(), int(moved.argmin()))
