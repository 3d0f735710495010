"""Live streaming session (vox_stream): samples pushed in pieces, ids handed back as they are determined.

What is asserted, and against what:
 * the concatenated ids equal the offline path's (transcribe_streaming on the log-mel of pad_audio(gain * x), logits tap = the full computation) in the project's usual sense:
   check_greedy_ids with TOL = 2e-4 -- equal up to the first near-tie of the REFERENCE's own logits (top-2 margin below 10 x TOL x max(1, max|logit|)), the rule and the
   numbers of tests/test_gpu_prefix_cache.py -- and outright on every id before that near-tie.  So that the rule cannot hide a failure, the tests that carry an ids claim
   assert that the reference's first near-tie lies at or beyond half of the clip's ids.
 * cut-independence, the ring, isolation between streams and offline calls: bit for bit (==), no rule.
 * every push returns exactly the ids vox_stream_schedule says were due."""
import ctypes as C
import os

import numpy as np
import pytest

from model_fixtures import check_greedy_ids, single_stream_reference, tiny_gguf
from stream_helpers import _full_path, _gain, _pieces, _stop, _t

pytestmark = pytest.mark.gpu
TOL = 2e-4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_16s_peaked_oracle.npz")


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=["tiny", "full"])
def model(request, pkg, ctx):
    """tiny: the synthetic tiny model; full: the full-size PEAKED model (no near-tie on its golden clip: ids claims can be carried end to end)."""
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0] if request.param == "tiny" else _full_path(True)).load(ctx)
    yield m, request.param
    m.close()


@pytest.fixture(scope="module")
def full_model(pkg, ctx):
    """The full-size peaked model alone, for the tests that have no tiny form."""
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    yield m
    m.close()


@pytest.fixture(autouse=True)
def _defaults(request):
    yield
    for name in ("model", "full_model"):
        if name in request.fixturenames:
            m = request.getfixturevalue(name)
            m = m[0] if isinstance(m, tuple) else m
            m.set_prefix_cache(True); m.set_decode_engine(True)


def _loud(seconds, seed):
    rng = np.random.default_rng(seed); n = int(seconds * 16000)
    return (0.4 * rng.standard_normal(n) + 0.3 * np.sin(np.arange(n) * 0.07)).astype(np.float32)


def _run(pkg, st, x, cuts, check_schedule=True):
    """Push x[a:b] for every (a, b) of cuts, then finish: (all ids, ids per call).  Every call must return exactly what the schedule says was due."""
    per = []; pushed = 0; had = 0
    for a, b in cuts:
        ids = st.push(x[a:b]); pushed += b - a
        if check_schedule:
            assert had + len(ids) == pkg.stream_schedule(pushed)[1], (a, b, had, len(ids))
        had += len(ids); per.append(ids)
    ids = st.finish(); had += len(ids); per.append(ids)
    assert pushed == len(x) and had == pkg.stream_schedule(len(x), finished=True)[1]
    return np.concatenate(per), [len(p) for p in per]


def _stream_ids(pkg, m, x, t, size=1600, **kw):
    st = m.create_stream(t, gain=_gain(x), **kw)
    try:
        return _run(pkg, st, x, _pieces(len(x), size))[0]
    finally:
        st.close()


def _reference(pkg, ctx, m, x, t):
    if x.size:
        return single_stream_reference(pkg, ctx, m, x, t)
    mel = pkg.MelSpectrogram.voxtral(ctx).compute_log(pkg.pad_audio(x))      # the pad alone
    return m.transcribe_streaming(np.ascontiguousarray(mel.T)[None], t, return_logits=True)


def _clips(pkg):
    S = pkg.synth
    return {"3s": S.synth_audio(3.0, seed=31), "16s": S.synth_audio(16.0, seed=1234), "33s_past_window": S.synth_audio(33.0, seed=33),
            "loud_from_0": _loud(4.0, 5), "one_sample": np.array([0.3], np.float32), "empty": np.zeros(0, np.float32)}


def _compare_with_offline(pkg, ctx, m, x, t, label, condition):
    rids, rlg = _reference(pkg, ctx, m, x, t)
    stop = _stop(rlg, TOL)
    sids = _stream_ids(pkg, m, x, t)
    print(f"{label}: {len(sids)} ids, stream == reference on {int((sids == rids).sum()) if len(sids) == len(rids) else -1}, first near-tie of the reference at {stop}")
    assert len(sids) == len(rids) and len(sids) >= 8
    if condition:
        assert 2 * stop >= len(rids), f"{label}: the reference's first near-tie ({stop}) lies in the first half of {len(rids)} ids: the clip cannot carry the claim"
    assert (sids[:stop] == rids[:stop]).all()
    check_greedy_ids(sids, rids, rlg, TOL)
    if x.size:      # (transcribe_audio refuses an empty clip)
        for on in (True, False):
            m.set_prefix_cache(on)
            off = m.transcribe_audio(x, t)
            assert (off[:stop] == sids[:stop]).all()
            check_greedy_ids(off, rids, rlg, TOL)
    return sids, rids, stop


# ---- 1. equals the offline path -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("clip", ["3s", "16s", "33s_past_window", "loud_from_0", "one_sample", "empty"])
def test_stream_equals_offline_tiny(pkg, ctx, clip):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    try:
        x = _clips(pkg)[clip]
        sids, rids, stop = _compare_with_offline(pkg, ctx, m, x, _t(pkg, m), f"tiny {clip}", condition=True)
        assert len(sids) == {"3s": 27, "16s": 108, "33s_past_window": 215, "loud_from_0": 33, "one_sample": 9, "empty": 8}[clip]
    finally:
        m.close()


def test_stream_equals_offline_full_bench_model(pkg, ctx):
    """The ordinary full-size model (seed 42) has its first near-tie early in its 16 s clip: the comparison runs, the stop is printed, no condition is claimed."""
    m = pkg.Q4ModelLoader.from_file(_full_path(False)).load(ctx)
    try:
        x = pkg.synth.synth_audio(16.0, seed=1234)
        _compare_with_offline(pkg, ctx, m, x, _t(pkg, m), "full seed 42, 16 s", condition=False)
    finally:
        m.close()


# ---- 2. full size, no forgiveness -----------------------------------------------------------------------------------------------------------------------------------
def test_full_peaked_golden_all_ids(pkg, ctx, full_model):
    m = full_model
    g = np.load(GOLDEN)
    x = pkg.synth.synth_audio(16.0, seed=7049); t = _t(pkg, m)
    rids, top1, top2, amax = g["ids"], g["top1"], g["top2"], float(g["logit_absmax"])
    assert len(rids) == 108 and float((top1 - top2).min()) > 50 * TOL * amax
    st = m.create_stream(t, gain=_gain(x)); st.tap_arm(128)
    try:
        ids, per = _run(pkg, st, x, _pieces(len(x), 2560))
        lg = st.tap_fetch()
    finally:
        st.close()
    assert np.array_equal(ids, rids), f"stream ids differ from the oracle's at {np.flatnonzero(ids != rids)[:8]}"
    assert lg.shape[0] == 108 and np.array_equal(lg.argmax(axis=1), ids)      # the tap holds the row behind each id
    err = float(np.abs(np.sort(lg, axis=1)[:, -1] - top1).max())
    print(f"peaked golden through a stream in 2560-sample pieces: 108 / 108 ids, ids per call {sorted(set(per))}, max top-logit error {err:.3e} at |logit| max {amax:.1f}")
    assert err <= 1e-2 * amax      # the bound of test_full_peaked_golden_all_ids_single_batch16_ragged


# ---- 3. cut-independence, bit for bit -------------------------------------------------------------------------------------------------------------------------------
def test_cut_independence(pkg, ctx, model):
    m, size = model
    x = pkg.synth.synth_audio(16.0, seed=7049 if size == "full" else 1234); t = _t(pkg, m); n = len(x)
    rng = np.random.default_rng(77)
    cuts = {"one piece": [(0, n)], "2560": _pieces(n, 2560), "1600": _pieces(n, 1600),
            "37 then 4001": _pieces(16000, 37) + [(16000 + a, 16000 + b) for a, b in _pieces(n - 16000, 4001)]}
    rnd = [0]
    while rnd[-1] < n:
        rnd.append(min(n, rnd[-1] + int(rng.choice([0, 0, 1, 39, 40, 41, 333, 2559, 2560, 2561, 7000, 30001]))))
    cuts["random with empty pushes"] = list(zip(rnd[:-1], rnd[1:]))
    st = m.create_stream(t, gain=_gain(x))
    try:
        out = {}
        for k, c in cuts.items():
            out[k] = _run(pkg, st, x, c)[0]; st.reset()
        dev = C.c_void_p(); pkg._lib.check(pkg.lib().vox_dev_alloc(ctx.h, n * 4, C.byref(dev)))      # from device memory, 4800-sample pieces
        try:
            pkg._lib.check(pkg.lib().vox_dev_upload(ctx.h, dev, x.ctypes.data, n * 4))
            per = [st.push(device_ptr=dev.value + 4 * a, n_samples=b - a) for a, b in _pieces(n, 4800)] + [st.finish()]
            out["device"] = np.concatenate(per)
        finally:
            pkg._lib.check(pkg.lib().vox_dev_free(ctx.h, dev))
    finally:
        st.close()
    ref = out["one piece"]
    assert len(ref) == 108
    for k, v in out.items():
        assert np.array_equal(v, ref), f"{size}: ids of '{k}' differ from the one-piece push at {np.flatnonzero(v != ref)[:8]}"


# ---- 4. ring wrap ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_ring_wrap_is_exact(pkg, ctx, model):
    """A ring changes addresses, not the order in which a query's keys are visited (stream_attn_kernel walks the window by key index): a 760-row ring, which wraps every
    few ticks past the window, gives the default (768-row) ring's ids and logits bit for bit -- both wrap many times in a 990-row clip."""
    m, size = model
    x = pkg.synth.synth_audio(33.0, seed=33); t = _t(pkg, m)
    res = []
    for cap in (0, 760, 2012):      # default, the smallest useful, the compacting cache's capacity (never wraps here)
        st = m.create_stream(t, gain=_gain(x), enc_capacity_rows=cap); st.tap_arm(256)
        try:
            ids = _run(pkg, st, x, _pieces(len(x), 1600))[0]
            info = st.info(); lg = st.tap_fetch()
        finally:
            st.close()
        assert info["encoder_position"] == 4 * info["positions"] and info["ring_rows"] == min(info["encoder_position"], cap or (m.config.enc_window + 8 + 63) // 64 * 64)
        res.append((ids, lg))
    assert len(res[0][0]) == 215 and res[1][0].size == 215
    for ids, lg in res[1:]:
        assert np.array_equal(res[0][0], ids) and np.array_equal(res[0][1], lg)


# ---- 5. isolation ---------------------------------------------------------------------------------------------------------------------------------------------------
def _piecewise(m, t, cache, calls, nxt=None):
    """`calls` generate_step_with_cache calls on a caller-owned cache: the 38-token prefix when nothing has been fed yet (nxt None), then one token per call, the argmax
    fed back.  (ids, logits of every call, the token the next call takes)."""
    ids, lgs = [], []
    for _ in range(calls):
        lg = m.generate_step_with_cache([1] + [32] * 37 if nxt is None else [nxt], t, cache)
        nxt = int(lg[-1].argmax()); ids.append(nxt); lgs.append(lg)
    return ids, lgs, nxt


def _same_piecewise(got, solo, first):
    assert got[0] == solo[0][first:first + len(got[0])]
    for k, lg in enumerate(got[1]):
        assert np.array_equal(lg, solo[1][first + k]), f"piecewise call {first + k}: logits differ from the undisturbed sequence"


def test_streams_and_offline_calls_do_not_disturb_each_other(pkg, ctx, model):
    """Two streams, offline calls, a batch and a piecewise caller alternate on one model: on the full-size model three clients of the decode engine, each with its own
    layer table (the tiny model has no engine: the same plumbing on the per-operator launches)."""
    m, size = model
    S = pkg.synth; t = _t(pkg, m); t2 = _t(pkg, m, delay=3.0)
    xa = S.synth_audio(9.0, seed=501); xb = _loud(6.5, 502); xo = S.synth_audio(4.0, seed=503)
    batch = [S.synth_audio(2.0 + 0.25 * i, seed=600 + i) for i in range(20)]
    solo_a = _stream_ids(pkg, m, xa, t, size=3200); solo_b = _stream_ids(pkg, m, xb, t2, size=1777)
    off_solo = m.transcribe_audio(xo, t); off2_solo = m.transcribe_audio(xo, t2)
    kc0 = m.create_decoder_cache_preallocated(256)
    try:
        pw_solo = _piecewise(m, t, kc0, 12)      # the prefix call + 11 one-token calls, nothing in between
    finally:
        kc0.close()
    kc = half = None; pw_halves = 0
    os.environ["VOX_BATCH_NO_CALIB"] = "1"      # the plan a function of the lengths alone: batch ids comparable call to call (include/voxtral_hip.h)
    try:
        batch_solo = m.transcribe_batch(batch, t)
        a = m.create_stream(t, gain=_gain(xa)); b = m.create_stream(t2, gain=_gain(xb))
        try:
            ca, cb = _pieces(len(xa), 3200), _pieces(len(xb), 1777)
            ga, gb = [], []
            for i in range(max(len(ca), len(cb))):
                if i < len(ca): ga.append(a.push(xa[ca[i][0]:ca[i][1]]))
                if i == 2:      # the same piecewise sequence on a fresh cache, in two halves between the pushes: bit for bit (the same kernels on the same inputs)
                    kc = m.create_decoder_cache_preallocated(256)
                    half = _piecewise(m, t, kc, 6); _same_piecewise(half, pw_solo, 0); pw_halves += 1
                if i == 6:
                    _same_piecewise(_piecewise(m, t, kc, 6, half[2]), pw_solo, 6); assert kc.seq_len() == 38 + 11; pw_halves += 1
                if i == 3: assert np.array_equal(m.transcribe_audio(xo, t), off_solo)
                if i < len(cb): gb.append(b.push(xb[cb[i][0]:cb[i][1]]))
                if i == 5:
                    for u, v in zip(m.transcribe_batch(batch, t), batch_solo): assert np.array_equal(u, v)
                if i == 7:      # the model's prefix state dropped and another t_embed selected while both streams are live
                    assert not m.set_prefix_cache(False)
                    assert np.array_equal(m.transcribe_audio(xo, t2), off2_solo)
            ga.append(a.finish()); gb.append(b.finish())
            assert pw_halves == 2      # (both halves of the piecewise sequence ran: the loop reached i == 2 and i == 6)
            assert np.array_equal(np.concatenate(ga), solo_a) and np.array_equal(np.concatenate(gb), solo_b)
            a.reset()
            assert np.array_equal(_run(pkg, a, xa, ca)[0], solo_a)      # (the prefix cache is off on the model: the stream builds what it starts from itself)
            assert not m.set_prefix_cache(None)
        finally:
            a.close(); b.close()
            if kc is not None: kc.close()
    finally:
        os.environ.pop("VOX_BATCH_NO_CALIB", None)


# ---- 6. past 1024 decoder positions -----------------------------------------------------------------------------------------------------------------------------------
def test_past_1024_positions_tiny_against_the_oracle(pkg, ctx, orc):
    """170 s: 1071 ids, more than the offline HIP path takes un-chunked (its encoder table ends at 4096 rows).  The CPU oracle takes the whole 17 744-frame mel in one
    piece; its logits have no near-tie in 1071 steps (asserted), so every id must match.  The decoder cache doubles at position 1024 on the way."""
    path = tiny_gguf()[0]
    m = pkg.Q4ModelLoader.from_file(path).load(ctx); om = orc.Model(path)
    try:
        x = pkg.synth.synth_audio(170.0, seed=61); t = _t(pkg, m)
        xn = np.array(x, dtype=np.float32, copy=True); orc.lib().orc_peak_normalize(xn, xn.size, 0.95)
        mel = np.ascontiguousarray(orc.mel_compute_log(orc.pad_audio(xn)).T)
        rids, rlg = om.transcribe_streaming(mel, orc.time_embedding(6.0, m.config.dec_dim), want_logits=True)
        stop = _stop(rlg, TOL)
        st = m.create_stream(t, gain=_gain(x))
        try:
            sids = _run(pkg, st, x, _pieces(len(x), 16000))[0]; info = st.info()
        finally:
            st.close()
        print(f"tiny 170 s: {len(sids)} ids, first near-tie of the oracle at {stop}, stream == oracle on {int((sids == rids).sum())}")
        assert len(rids) == 1071 and len(sids) == 1071 and stop == 1071      # no near-tie anywhere in the oracle's logits: nothing is forgiven
        assert np.array_equal(sids, rids), f"stream ids differ from the oracle's at {np.flatnonzero(sids != rids)[:8]}"
        assert info["positions"] == 37 + 1071 and info["engine_steps"] + info["operator_steps"] == 1071
    finally:
        om.close(); m.close()


def test_past_1024_positions_full_engine_then_operators(pkg, ctx, full_model):
    m = full_model
    x = pkg.synth.synth_audio(170.0, seed=61); t = _t(pkg, m)
    eng = m.set_decode_engine(True)      # (a device without the engine: every step on the launches, the comparison still runs)
    a = m.create_stream(t, gain=_gain(x))
    try:
        ia = _run(pkg, a, x, _pieces(len(x), 16000))[0]; info_a = a.info()
    finally:
        a.close()
    assert not m.set_decode_engine(False)
    b = m.create_stream(t, gain=_gain(x)); b.tap_arm(1071)
    try:
        ib = _run(pkg, b, x, _pieces(len(x), 16000))[0]; info_b = b.info(); lg = b.tap_fetch()
    finally:
        b.close()
    stop = _stop(lg, TOL)
    print(f"full 170 s: engine stream {info_a['engine_steps']} engine + {info_a['operator_steps']} per-operator steps; first near-tie of the per-operator stream at {stop}; equal on {int((ia == ib).sum())} of 1071")
    assert len(ia) == len(ib) == 1071 and 2 * stop >= 1071
    assert (ia[:stop] == ib[:stop]).all()
    check_greedy_ids(ia, ib, lg, TOL)
    n_eng = 1024 - 37 if eng else 0      # positions 37 .. 1023 on the engine, 1024 .. on the launches
    assert info_a["engine_steps"] == n_eng and info_a["operator_steps"] == 1071 - n_eng
    assert info_b["engine_steps"] == 0 and info_b["operator_steps"] == 1071


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_untouched(pkg, ctx, model):
    m, size = model
    L = pkg.lib(); t = _t(pkg, m); x = pkg.synth.synth_audio(3.0, seed=31)
    ref = _stream_ids(pkg, m, x, t, size=len(x))
    st = m.create_stream(t, gain=_gain(x))
    try:
        n = C.c_int32(-1); ids = np.zeros(64, np.int32)
        due = pkg.stream_schedule(len(x))[1]
        assert due > 2
        before = st.info()
        assert L.vox_stream_push(st.h, x.ctypes.data, len(x), 0, ids.ctypes.data, due - 1, C.byref(n)) == 1 and b"capacity" in L.vox_last_error()
        assert st.info() == before
        pkg._lib.check(L.vox_stream_push(st.h, x.ctypes.data, len(x), 0, ids.ctypes.data, due, C.byref(n)))      # the repeated call with room
        assert n.value == due and np.array_equal(ids[:due], ref[:due])
        before = st.info()
        assert L.vox_stream_finish(st.h, ids.ctypes.data, 1, C.byref(n)) == 1 and st.info() == before
        rest = st.finish()
        assert np.array_equal(np.concatenate([ids[:due], rest]), ref)
        with pytest.raises(pkg.VoxError, match="finished"):
            st.push(x[:100])
        with pytest.raises(pkg.VoxError, match="finished"):
            st.finish()
        st.reset()
        assert np.array_equal(_run(pkg, st, x, _pieces(len(x), 999))[0], ref)
    finally:
        st.close()
    with pytest.raises(pkg.VoxError, match="window"):
        m.create_stream(t, enc_capacity_rows=m.config.enc_window + 4)
    with pytest.raises(pkg.VoxError, match="max_positions"):
        m.create_stream(t, max_positions=1 << 20)
    small = m.create_stream(t, gain=_gain(x), max_positions=48)      # positions 37 .. 47 can be reached: 11 ids
    try:
        a = small.push(x[:2560 * 10 + 40])
        assert len(a) == 11 and np.array_equal(a, ref[:11])
        before = small.info()
        with pytest.raises(pkg.VoxError, match="position"):
            small.push(x[2560 * 10 + 40:2560 * 11 + 40])
        assert small.info() == before
        with pytest.raises(pkg.VoxError, match="position"):
            small.finish()
    finally:
        small.close()


# ---- 8. launch accounting -------------------------------------------------------------------------------------------------------------------------------------------
def test_steady_ticks_launch_no_prefill_form(pkg, ctx, model):
    from model_fixtures import GEMM_FORMS
    m, size = model
    L = pkg.lib(); t = _t(pkg, m); x = pkg.synth.synth_audio(12.0, seed=88)
    names = ("prefill_small", "prefill_mfma", "prefill_f32", "decode", "decode_spec", "decode_gqa", "attn_wo", "engine", "stream_ring")

    def counts():
        a = (C.c_uint64 * 9)(); g = (C.c_uint64 * len(GEMM_FORMS))()
        assert L.vox_debug_attn_launches(a, 9) == 0 and L.vox_debug_gemm_launches(g, len(GEMM_FORMS)) == 0
        return dict(zip(names, map(int, a))), dict(zip(GEMM_FORMS, map(int, g)))

    st = m.create_stream(t, gain=_gain(x))
    try:
        st.push(x[:2560 * 8])      # first ticks done: every lazily built table exists
        a0, g0 = counts()
        got = st.push(x[2560 * 8:2560 * 58])
        a1, g1 = counts()
    finally:
        st.close()
    assert len(got) == 50
    da = {k: a1[k] - a0[k] for k in a1 if a1[k] != a0[k]}; dg = {k: g1[k] - g0[k] for k in g1 if g1[k] != g0[k]}
    print(f"{size}: 50 steady ticks: attention {da}, linear {dg}")
    assert da.pop("stream_ring") == 50 * m.config.enc_layers
    assert not {"prefill_small", "prefill_mfma", "prefill_f32"} & set(da)
    assert not {"big", "big_rope", "wide", "skinny", "skinny_mt", "skinny_mt2", "tile_11", "tile_12", "tile_21", "tile_22"} & set(dg)
    assert dg.get("dense2", 0) == 2 * 50      # the conv stem: two small im2col GEMMs per tick


# ---- 9. the front end's values: stream_mel_kernel on the sample ring, the conv stem as two GEMMs on the halo buffer -------------------------------------------------
# (vox_debug_stream_front_tap_*; the float64 reference of tests/frontend_ref.py and the bars of tests/test_gpu_front_end.py; worst errors: DESIGN.md section 4)
FRONT_SECONDS = 9.0      # 144 000 samples: the 65 536-sample ring wraps twice, frames straddle both wrap points


def _front_clip():
    import frontend_ref as F
    x = F.make_clip("noise", 9, FRONT_SECONDS)
    assert len(x) == 144000 and F.pad_len(len(x)) // 2560 == 103
    return x


def _front_tapped(pkg, st, x, cuts):
    """One utterance with the front tap armed: (log-mel [128][16 ticks] of frames 592 .., conv rows [4 ticks][enc_dim] of rows 148 ..), ticks = positions 37 .. S - 2."""
    import frontend_ref as F
    ticks = F.pad_len(len(x)) // 2560 - 1 - 37
    st.front_tap_arm(ticks + 3)
    _run(pkg, st, x, cuts)
    mel, conv = st.front_tap_fetch()
    assert mel.shape[0] == conv.shape[0] == ticks
    return np.ascontiguousarray(mel.reshape(ticks * 16, -1).T), conv.reshape(ticks * 4, -1)


def _front_mel_check(mel, x, gain, tables, label):
    import frontend_ref as F
    ref = F.log_mel(F.pad(np.float64(np.float32(gain)) * x.astype(np.float64)), *tables)[:, 592:592 + mel.shape[1]]
    inside = F.clip_frames(len(x), 592 + mel.shape[1])[592:]
    assert ref.shape == mel.shape and (ref[:, inside] > F.FLOOR + 0.05).mean() >= 0.5      # not floor against floor
    err = np.abs(mel - ref); worst = float(err.max())
    assert worst <= 1e-4, f"{label}: stream log-mel {worst:.3e} off the float64 reference at (mel bin, frame) {np.unravel_index(np.argmax(err), err.shape)} (+592)"
    assert (mel[:, ~inside] == np.float32(F.FLOOR)).all()
    return worst


def test_stream_front_end_values(pkg, ctx, model):
    """The tapped log-mel frames [16 p, 16 p + 16), p = 37 .. S - 2, against log_mel(pad(gain x)) and against the single clip's front end on the same clip (same gain);
    the tapped conv rows against conv_stem on the TAPPED mel (so the bar covers the conv alone): per row 2e-5 max_j |pre_ij|, carried through the GELU
    (linear_ref.carry_bound), the bar of tests/test_gpu_linear.py.  The conv weights are read from the GGUF."""
    import frontend_ref as F
    from linear_ref import EPI_GELU, carry_bound
    from model_fixtures import gguf_conv_weights
    m, size = model
    tables = (pkg.MelSpectrogram.mel_filterbank(), pkg.MelSpectrogram.hann_window(400))
    x = _front_clip(); t = _t(pkg, m); gain = _gain(x)
    st = m.create_stream(t, gain=gain)
    try:
        mel, conv = _front_tapped(pkg, st, x, _pieces(len(x), 2560))
    finally:
        st.close()
    assert mel.shape == (128, 16 * 65) and conv.shape == (4 * 65, m.config.enc_dim)
    worst = _front_mel_check(mel, x, gain, tables, size)
    sc, mels = m.debug_front_end([x], 0)
    assert sc[0] == np.float32(gain)
    off = mels[0][:, 592:592 + mel.shape[1]]
    d = float(np.abs(mel - off).max())
    assert d <= 1e-4
    print(f"{size}: stream log-mel, 65 ticks over two ring wraps: worst error {worst:.2e} vs float64; vs the single clip's front end {d:.2e}, bit-identical: {np.array_equal(mel, off)}")
    w1, b1, w2, b2 = gguf_conv_weights(pkg, tiny_gguf()[0] if size == "tiny" else _full_path(True), m.config.enc_dim, m.config.n_mels)
    full = np.full((128, 592 + mel.shape[1]), np.float32(F.FLOOR), np.float32); full[:, 592:] = mel      # frames below 592 see the left pad's zeros alone
    ref, pre = F.conv_stem(full, w1, b1, w2, b2)
    ref, pre = ref[148:], pre[148:]
    assert ref.shape == conv.shape
    bound = carry_bound(pre, 2e-5 * np.abs(pre).max(axis=1)[:, None], EPI_GELU)
    err = np.abs(conv - ref); ratio = float((err / bound).max())
    print(f"{size}: stream conv rows 148 .. {148 + len(conv) - 1}: worst error {err.max():.2e} at max |row| {np.abs(ref).max():.2f}, {ratio:.3f} x the bound")
    assert (err <= bound).all(), f"{size}: conv row {148 + int(np.argmax((err / bound).max(axis=1)))} is {ratio:.2f} x its bound"


def test_stream_front_end_cut_independence(pkg, ctx, model):
    """The tapped log-mel frames and conv rows do not depend on how the samples were cut into pushes: bit for bit."""
    m, size = model
    x = _front_clip(); t = _t(pkg, m); n = len(x)
    rng = np.random.default_rng(77)
    rnd = [0]
    while rnd[-1] < n:
        rnd.append(min(n, rnd[-1] + int(rng.choice([0, 0, 1, 39, 40, 41, 333, 2559, 2560, 2561, 7000, 30001]))))
    cuts = {"one push": [(0, n)], "2560": _pieces(n, 2560), "30001": _pieces(n, 30001), "70000 then the rest": [(0, 70000), (70000, n)],
            "random with empty pushes": list(zip(rnd[:-1], rnd[1:]))}
    st = m.create_stream(t, gain=_gain(x))
    try:
        out = {}
        for k, c in cuts.items():
            out[k] = _front_tapped(pkg, st, x, c); st.reset()
    finally:
        st.close()
    ref = out["one push"]
    for k, v in out.items():
        assert np.array_equal(v[0], ref[0]), f"{size}: log-mel of '{k}' differs from the one-push run in frames {592 + np.unique(np.nonzero(v[0] != ref[0])[1])[:8]}"
        assert np.array_equal(v[1], ref[1]), f"{size}: conv rows of '{k}' differ from the one-push run in rows {148 + np.unique(np.nonzero(v[1] != ref[1])[0])[:8]}"


def test_stream_gain_reaches_the_mel(pkg, ctx, model):
    """A gain that is not the clip's own (0.5) appears in the log-mel as the reference says."""
    m, size = model
    tables = (pkg.MelSpectrogram.mel_filterbank(), pkg.MelSpectrogram.hann_window(400))
    x = _front_clip()[:40000]; t = _t(pkg, m)
    assert abs(_gain(x) - 0.5) > 0.1
    st = m.create_stream(t, gain=0.5)
    try:
        mel, _ = _front_tapped(pkg, st, x, [(0, len(x))])
    finally:
        st.close()
    print(f"{size}: stream log-mel at gain 0.5: worst error {_front_mel_check(mel, x, 0.5, tables, size):.2e}")
