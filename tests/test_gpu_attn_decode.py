"""The decode attention kernels (one query row per sequence; csrc/vox_kernels.hip) against a float64 reference, one launch at a time through vox_debug_attn_decode:
attn_decode_kernel<128, false> (`decode`), its speculative-row form (`decode_spec`, VOX_ATTN_SPEC=1), attn_decode_gqa_kernel<4, false> (`decode_gqa`: the wide batch
step and every slab stream group of a 4:1 model), attn_decode_paged_kernel<128> (`decode_paged`) and attn_decode_gqa_kernel<4, true> (`decode_gqa_paged`).  The
reference, the inputs and the case table are tests/attn_decode_ref.py, pinned on the CPU by tests/test_attn_decode_ref.py.

Bar: per row (one sequence, one head) |out - ref| <= 2e-5 max|ref of that row| -- the suite's f32-class bar, row by row as in tests/test_gpu_linear.py, so a scaled
edge row of one sequence does not loosen the others.  Every case asserts WHICH kernel ran (vox_debug_attn_launches: exactly one launch of the expected form); the last
test fails if a reachable form was never the asserted kernel of a passing case, and prints the worst error per form and input kind (recorded in DESIGN.md).

The table (attn_decode_ref.logical_cases): the key-count seams 1 .. 1024 in one launch of 37 sequences (the 160 prefetched keys, the tail loops of stride 64 / 32
and 32 / 8, the 256-wide softmax loop, the 16-row XF group, per-sequence positions), again with 40 sequences for the per-head kernels (their XCD re-map runs when
n_heads * n_seq is a multiple of 8 G) and once with no_xcd_remap; windows of 20 .. 200 keys at their first moves; the real 8192-key window at positions 8191 .. 8193
and at the last row of the cache; kv_row; page tables with the position and the window's first key at a page's last row, first row and middle (paged == slab bit for
bit there, and wherever a case ran on both); the XF output decoded with a numpy restatement of xf_store4 against the bf16 split of the same case's f32 output.
Rows behind a position are NaN, rows in front of a window hold V = 1e6, unread slices and unnamed pool pages are NaN, table entries outside a window are -1.

UNREACHABLE: the head_dim-64 instantiations (attn_decode_kernel<64, false>, attn_decode_paged_kernel<64>) have no caller -- dec_head_dim is the constant 128 -- and
the entry refuses head_dim != 128; attn_wo_kernel needs a Q4 weight and is held to the oracle at full size, window edge included (tests/test_gpu_fullsize.py).  The
paged per-head kernel cannot see a 4:1 geometry: launch_attn_decode_paged takes the GQA form there.  The live sessions' ring attention (`stream_ring`:
stream_attn_kernel, RoPE + K / V append + windowed softmax in one launch) is no decode attention launch and has no entry here; it is held to its own float64
reference, one launch at a time through vox_debug_stream_attn, by tests/test_gpu_stream_attn.py (both head sizes, the three RoPE modes, the ring seeding too).

That the table can fail was checked once on an MI355X with four temporary mutations of attn_decode_gqa_kernel alone (the paged == slab tests cannot see them: both
sides are that kernel), each changing a value or reading FEWER rows, no address or bound widened:
  * j_lo computed as pos - window + 1 (the window starts one key late) -> every small-window case (win20 .. win200, all three kinds), kvrow and the real-window
    cases of decode_gqa and decode_gqa_paged, 81 tests; the seam cases (no window) and every per-head case pass, as they must;
  * the V tail loop ending at n - 1 -> the cases with more than 160 keys: seam, win160, win200, kvrow, the real window, the 1024-row page edges (54 tests); win20,
    win65 and win159 (at most 160 keys: no tail) pass;
  * wave 3's partial left out of the softmax sum -> the cases with more than 192 keys (that wave's first score index): seam, win200, kvrow, the real window, the
    1024-row page edges (42 tests);
  * the score scale 1 / sqrt(129) -> every normal and peaked case of both GQA forms (65 tests); the uniform kind (q = 0) cannot see a scale and passes.
Each mutation also fails test_every_reachable_form_was_asserted or the refusal test's closing launch; none is seen by a per-head form or by a paged == slab comparison.
"""
import ctypes
from collections import namedtuple
from importlib import import_module

import numpy as np
import pytest

import attn_decode_ref as R
from model_fixtures import ATTN_FORMS, attn_launches, launches_since, tiny_gguf
from stream_helpers import _gain, _t

pytestmark = pytest.mark.gpu

Form = namedtuple("Form", "paged gqa spec geos twin")
FORMS = {"decode": Form(False, False, False, R.HEAD_GEOS, None),
         "decode_spec": Form(False, False, True, R.HEAD_GEOS, None),
         "decode_gqa": Form(False, True, False, R.GQA_GEOS, None),
         "decode_paged": Form(True, False, False, ((4, 2), (2, 2)), "decode"),
         "decode_gqa_paged": Form(True, True, False, R.GQA_GEOS, "decode_gqa")}
REACHABLE = set(FORMS)
UNREACHABLE = set(ATTN_FORMS) - REACHABLE      # no decode attention launch: prefill, attn_wo, engines, the resamplers, and the streams' ring attention, which tests/test_gpu_stream_attn.py holds (module docstring: hd 64)
PAGE_ROWS = 64                                 # the paged runs of the 1024-row cases: 16 pages per slice
REAL_PAGE_ROWS = 256                           # the default page of a paged group

Run = namedtuple("Run", "form case page_rows no_xcd")
RUNS = {}


def add(form, case, page_rows=0, no_xcd=False):
    rid = f"{R.case_id(case)}-{form}" + (f"-p{page_rows}" if page_rows else "") + ("-noremap" if no_xcd else "")
    assert rid not in RUNS and (case.H, case.KV) in FORMS[form].geos and bool(page_rows) == FORMS[form].paged
    RUNS[rid] = Run(form, case, page_rows, no_xcd)


def real_geos(form):
    return [g for g in FORMS[form].geos if g in R.REAL_GEOS]


for form_, f_ in FORMS.items():
    pr_ = PAGE_ROWS if f_.paged else 0
    for geo_ in f_.geos:
        for kind_ in R.KINDS:
            add(form_, R.seam_case(kind_, geo_), pr_)
            if not f_.gqa:
                add(form_, R.seam_case(kind_, geo_, True), pr_)
            for w_ in R.SMALL_WINDOWS:
                add(form_, R.small_window_case(kind_, geo_, w_), pr_)
        add(form_, R.kv_row_case("normal", geo_), pr_)
    if form_ != "decode_gqa":      # (the slab GQA form's real-window case takes the device's row limit: test_real_window_slab_gqa)
        for geo_ in real_geos(form_):
            for kind_ in R.KINDS:
                add(form_, R.real_window_case(kind_, geo_, 16384), REAL_PAGE_ROWS if f_.paged else 0)
add("decode", R.seam_case("normal", (4, 2), True), no_xcd=True)
add("decode_paged", R.seam_case("normal", (4, 2), True), PAGE_ROWS, no_xcd=True)
RUN_IDS = sorted(RUNS, key=lambda r: (R.case_id(RUNS[r].case), list(FORMS).index(RUNS[r].form), r))      # by case: the inputs and the reference are built once, the slab twin runs first

WORST = {}            # (form, kind) -> worst row error, as a multiple of the row's max|ref|
PASSED, ASSERTED = set(), set()
F32_OUT = {}          # (case, form) -> the f32 output, for the paged == slab comparison of cases that ran on both


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def gg(pkg):
    return import_module(pkg.__name__ + ".gguf")


def launch(pkg, gg, ctx, monkeypatch, form, c, q, k, v, page_rows=0, no_xcd=False, out_xf=False):
    """ONE launch of `form` on the case's rows; asserts that exactly that kernel form ran."""
    f = FORMS[form]
    if f.spec:
        monkeypatch.setenv("VOX_ATTN_SPEC", "1")
    before = attn_launches(pkg)
    if f.paged:
        pk, pv, tab = R.to_paged(c, k, v, page_rows)
        out = gg.attn_decode(ctx, q, pk, pv, c.pos, c.H, c.KV, window=c.window, kv_row=c.kv_row, page_tab=tab, score_rows=R.score_rows_of(c), no_xcd_remap=no_xcd, out_xf=out_xf)
    else:
        out = gg.attn_decode(ctx, q, k, v, c.pos, c.H, c.KV, window=c.window, kv_row=c.kv_row, prefer_gqa=f.gqa, spec=f.spec, no_xcd_remap=no_xcd, out_xf=out_xf)
    ran = launches_since(pkg, before)
    assert ran == {form: 1}, f"expected one {form} launch, the launcher ran {ran}"
    return out


def held(form, c, out, ref):
    """The bar, row by row; records the worst error of (form, kind)."""
    e = R.row_err(out, ref, c.H)
    w = float(e.max()); i, h = np.unravel_index(int(np.argmax(e)), e.shape)
    print(f"{form} {R.case_id(c)}: worst row {w:.2e} of its max (sequence {i} at position {c.pos[i]}, {R.window_of(c, i)[1]} keys, head {h})")
    WORST[(form, c.kind)] = max(WORST.get((form, c.kind), 0.0), w)
    bad = np.argwhere(e > R.BAR)
    assert not len(bad), (f"{len(bad)} rows past 2e-5 of their max, worst {w / R.BAR:.1f} x the bar at sequence {i} (position {c.pos[i]}, window from {R.window_of(c, i)[0]}, "
                          f"{R.window_of(c, i)[1]} keys), head {h}; first rows (sequence, head): {bad[:6].tolist()}")


def run_case(pkg, gg, ctx, monkeypatch, form, c, page_rows=0, no_xcd=False):
    q, k, v, ref = R.cached(c)
    out = launch(pkg, gg, ctx, monkeypatch, form, c, q, k, v, page_rows, no_xcd)
    assert out.shape == ref.shape
    held(form, c, out, ref)
    twin = FORMS[form].twin
    if not no_xcd:
        F32_OUT[(c, form)] = out
        if twin and (c, twin) in F32_OUT:
            assert np.array_equal(out.view(np.uint32), F32_OUT[(c, twin)].view(np.uint32)), f"{form} differs from {twin} on the same logical rows"
    else:
        base = F32_OUT[(c, form)] if (c, form) in F32_OUT else launch(pkg, gg, ctx, monkeypatch, form, c, q, k, v, page_rows)
        assert np.array_equal(out.view(np.uint32), base.view(np.uint32)), "the workgroup order changed a row's bits"
    ASSERTED.add(form)
    return out


@pytest.mark.parametrize("rid", RUN_IDS)
def test_attn_decode_case(pkg, gg, ctx, monkeypatch, rid):
    """One row of the table: the expected kernel form ran (one launch, nothing else) and every output row meets the bar."""
    r = RUNS[rid]
    run_case(pkg, gg, ctx, monkeypatch, r.form, r.case, r.page_rows, r.no_xcd)
    PASSED.add(rid)


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("geo", R.GQA_GEOS)
def test_real_window_slab_gqa(pkg, gg, ctx, monkeypatch, geo, kind):
    """The slab GQA form at the real window, on the longest cache it serves (attn_decode_gqa_max_seq): positions 8191, 8192, 8193 and the cache's last row."""
    rows = gg.attn_gqa_max_seq(ctx)
    assert R.REAL_WINDOW + 2 < rows < 16384
    run_case(pkg, gg, ctx, monkeypatch, "decode_gqa", R.real_window_case(kind, geo, rows))
    PASSED.add(f"realgqa-{kind}-{geo}")


@pytest.mark.parametrize("form,geo", [("decode_gqa_paged", (4, 1)), ("decode_paged", (4, 2))])
@pytest.mark.parametrize("P", [16, 64, 1024])
def test_page_edges_and_paged_equals_slab(pkg, gg, ctx, monkeypatch, P, form, geo):
    """Position and first visible key each at a page's last row, first row and middle (six windows, attn_decode_ref.page_edge_cases): the paged form meets the bar and has
    the slab form's bits on the same logical rows -- what launch_attn_decode_paged documents."""
    for c in R.page_edge_cases(geo, P):
        slab = run_case(pkg, gg, ctx, monkeypatch, FORMS[form].twin, c)
        paged = run_case(pkg, gg, ctx, monkeypatch, form, c, P)
        assert np.array_equal(paged.view(np.uint32), slab.view(np.uint32)), (R.case_id(c), np.argwhere(paged != slab)[:4].tolist())
    PASSED.add(f"pages-{P}-{form}")


@pytest.mark.parametrize("form", list(FORMS))
def test_xf_output(pkg, gg, ctx, monkeypatch, form):
    """The seam launch again with out_xf (37 sequences: three 16-row groups, out_xf_gstride apart): every element's bf16 hi + lo pair, read back through a numpy
    restatement of xf_store4's layout, is bit for bit the split of the same launch's f32 output.  A wrong decoder, plane or row placement cannot pass by accident."""
    f = FORMS[form]
    for geo in f.geos:
        c = R.seam_case("normal", geo)
        q, k, v, _ = R.cached(c)
        pr = PAGE_ROWS if f.paged else 0
        f32 = F32_OUT.get((c, form))
        if f32 is None:
            f32 = launch(pkg, gg, ctx, monkeypatch, form, c, q, k, v, pr)
        planes = launch(pkg, gg, ctx, monkeypatch, form, c, q, k, v, pr, out_xf=True)
        assert planes.shape == (3, 2, c.H * 2048) and planes.dtype == np.uint16
        hi, lo = R.xf_decode(planes, len(c.pos), c.H * R.HD)
        want_hi, want_lo = R.bf16_split(f32)
        assert np.array_equal(hi, want_hi) and np.array_equal(lo, want_lo), (geo, np.argwhere(hi != want_hi)[:4].tolist(), np.argwhere(lo != want_lo)[:4].tolist())
        rows_16 = np.arange(48)[len(c.pos):]      # rows 37 .. 47 of the last group belong to no sequence: untouched (zero)
        z_hi, z_lo = R.xf_decode(planes, 48, c.H * R.HD)
        assert not z_hi[rows_16].any() and not z_lo[rows_16].any()
    PASSED.add(f"xf-{form}")


def test_refusals_launch_nothing(pkg, gg, ctx):
    """What the entry refuses ends in a VoxError before any launch: head_dim 64, a position outside the cache, a table entry of the window outside the pool, a window
    wider than score_rows, a slab longer than the GQA form serves -- the limit + 1 case never reaches the device."""
    c = R.make_case("refuse", "normal", 4, 1, 40, 128, (100, 17))
    q, k, v = R.build_inputs(c)
    pk, pv, tab = R.to_paged(c, k, v, 16)
    most = gg.attn_gqa_max_seq(ctx)

    def refused(fn, word):
        before = attn_launches(pkg)
        with pytest.raises(pkg.VoxError) as e:
            fn()
        assert e.value.code == 1 and word in str(e.value), e.value
        assert launches_since(pkg, before) == {}

    refused(lambda: gg.attn_decode(ctx, q, k, v, c.pos, 4, 1, window=40, head_dim=64), "head_dim")
    refused(lambda: gg.attn_decode(ctx, q, k, v, (128, 17), 4, 1, window=40), "outside the cache")
    refused(lambda: gg.attn_decode(ctx, q, k, v, c.pos, 4, 1, window=40, kv_row=(0, 2)), "kv_row")
    bad = tab.copy(); bad[0, 100 >> 4] = pk.shape[0]
    refused(lambda: gg.attn_decode(ctx, q, pk, pv, c.pos, 4, 1, window=40, page_tab=bad, score_rows=41), "outside the pool")
    gone = tab.copy(); gone[0, 60 >> 4] = -1      # the page of the window's first key, released
    refused(lambda: gg.attn_decode(ctx, q, pk, pv, c.pos, 4, 1, window=40, page_tab=gone, score_rows=41), "outside the pool")
    refused(lambda: gg.attn_decode(ctx, q, pk, pv, c.pos, 4, 1, window=40, page_tab=tab, score_rows=40), "score_rows")
    long_k = np.zeros((1, 1, most + 1, R.HD), np.float32)
    refused(lambda: gg.attn_decode(ctx, q[:1], long_k, long_k, (5,), 4, 1, prefer_gqa=True), "at most")
    out = gg.attn_decode(ctx, q, pk, pv, c.pos, 4, 1, window=40, page_tab=tab, score_rows=41)      # the context is still usable
    assert (R.row_err(out, R.reference(c, q, k, v), 4) <= R.BAR).all()


def _device_free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def test_slab_group_limit_of_a_gqa_model(pkg, gg, ctx):
    """A slab stream group of a 4:1 model (the tiny dec_heads = 8 one) takes max_positions up to attn_decode_gqa_max_seq and runs there; one position more is refused
    at creation with VOX_ERR_INVALID, a message that names the limit and points to paged groups, and nothing allocated.  A paged group of the same model and a slab
    group of the 2:1 model are not bound by it."""
    most = gg.attn_gqa_max_seq(ctx)
    m = pkg.Q4ModelLoader.from_file(tiny_gguf(dec_heads=8)[0]).load(ctx)
    m2 = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    try:
        assert m.config.dec_heads == 4 * m.config.dec_kv_heads and m2.config.dec_heads == 2 * m2.config.dec_kv_heads
        t = _t(pkg, m); x = pkg.synth.synth_audio(1.0, seed=77)
        g = m.create_stream_group(t, 2, gains=[_gain(x)] * 2, max_positions=most)
        try:
            before = attn_launches(pkg)
            ids = g.advance({0: x[:9000], 1: x[:6000]})
            ran = launches_since(pkg, before)
            assert len(ids[0]) >= 3 and len(ids[1]) >= 2 and ran.get("decode_gqa", 0) >= m.config.dec_layers and "decode" not in ran
        finally:
            g.close()
        ctx.synchronize()
        free0 = _device_free_bytes()
        with pytest.raises(pkg.VoxError) as e:
            m.create_stream_group(t, 2, max_positions=most + 1)
        assert e.value.code == 1 and f"at most {most} positions" in str(e.value) and "vox_stream_group_create_paged" in str(e.value), e.value
        with pytest.raises(pkg.VoxError) as e:
            m.create_stream_group(t, 2, max_positions=most + 1, sample_rates=[48000, 16000])
        assert e.value.code == 1 and f"at most {most} positions" in str(e.value)
        assert _device_free_bytes() == free0
        for mk, kw in ((m, {"page_rows": 256, "pool_pages": 8}), (m2, {})):
            g = mk.create_stream_group(_t(pkg, mk), 2, max_positions=most + 1, **kw)
            g.close()
    finally:
        m.close(); m2.close()


def test_every_reachable_form_was_asserted():
    """Every row of the table ran and passed, and each of the five reachable forms was the asserted kernel of a passing case.  Prints the worst error per form and kind."""
    for (form, kind), w in sorted(WORST.items()):
        print(f"worst error, {form:17s} {kind:8s}: {w:.2e} of the row's max (bar {R.BAR:.0e})")
    assert set(RUN_IDS) <= PASSED, f"{len(set(RUN_IDS) - PASSED)} rows of the table did not pass: {sorted(set(RUN_IDS) - PASSED)[:8]}"
    missing = set(ATTN_FORMS) - UNREACHABLE - ASSERTED
    assert not missing, f"no passing case asserted {sorted(missing)}"
    assert REACHABLE == {"decode", "decode_spec", "decode_gqa", "decode_paged", "decode_gqa_paged"}
