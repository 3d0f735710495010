"""Alternatives of the live sessions' ids (vox_token_alts; DESIGN.md section 8, "Alternatives"): the kernel through vox_alternatives_rows, then the records a solo
stream and a stream group hand out, against numpy in float64 on the same f32 logits rows (the sessions' rows come from their logits taps).

The reference and what is asked of the kernel:
  id, n      exact: the project's argmax rule (the largest wins, the lowest index wins a tie, a NaN or -inf never wins) applied k times, each time over the columns not
             yet taken; n = how many times something won; the entries behind are {-1, NaN};
  logprob    within 2^-23 (|ref| + V / 256 + 32), the bound of the score records;
  entropy    within 2^-23 (V / 256 + 32) (1 + H_ref): S = sum exp(L - m) and T = sum exp(L - m) (L - m) each carry a relative summation-and-expf error of at most about
             (V / 1024 + 16) 2^-24, and H = log S + A with A = sum p |L - m| <= H, so the error is at most about that rate times (1 + A) plus the roundings of logf, the
             division and the subtraction;
  NaN for both where the row holds a NaN or its maximum is not finite.
The bounds are worst cases; the inputs are chosen such that a lost, doubled or misordered column moves an id, or moves the entropy by far more."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from model_fixtures import tiny_gguf
from stream_helpers import _full_path, _gain, _pieces, _t
from test_gpu_stream_scores import _argmax_rule, _cli_files, _loud, _run, _same_bits, _word_lines

pytestmark = pytest.mark.gpu
F32 = np.float32
KS = (1, 3, 8)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------------------------
def _ref(row, k):
    """(ids of the n winners, their logprobs in float64, the entropy in float64) of one f32 row; NaN values for a flagged row."""
    row = np.asarray(row, dtype=F32).copy(); ids = []
    work = row.copy()
    for _ in range(k):
        t = _argmax_rule(work)
        if t < 0:
            break
        ids.append(t); work[t] = -np.inf
    L = row.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = L[ids[0]] if ids else -np.inf
        if np.isnan(L).any() or not np.isfinite(m):
            return ids, [np.nan] * len(ids), np.nan
        d = L - m; lse = np.log(np.exp(d).sum())
        fin = d > -np.inf
        H = float(-(np.exp(d[fin] - lse) * (d[fin] - lse)).sum())
    return ids, [float(d[t] - lse) for t in ids], max(H, 0.0)


def _tol_lp(ref, V):
    return 2.0 ** -23 * (abs(ref) + V / 256.0 + 32.0)


def _tol_h(ref, V):
    return 2.0 ** -23 * (V / 256.0 + 32.0) * (1.0 + ref)


def _check(rec, rows, k, label, worst=None):
    """Every record of `rec` (made at k; k a sequence: per record) against the reference on its row."""
    V = rows.shape[1]
    assert len(rec) == len(rows), (label, len(rec), len(rows))
    for r, row in enumerate(rows):
        kk = int(k[r]) if np.ndim(k) else int(k)
        ids, lps, H = _ref(row, kk); got = rec[r]; where = f"{label}, row {r} (V {V}, k {kk})"
        assert int(got["n"]) == len(ids) and list(got["alt"]["id"]) == ids + [-1] * (8 - len(ids)), (where, got, ids)
        assert np.isnan(got["alt"]["logprob"][len(ids):]).all(), (where, got)
        for j, lp in enumerate(lps):
            g = float(got["alt"]["logprob"][j])
            if np.isnan(lp):
                assert np.isnan(g), (where, j, got)
            else:
                err = abs(g - lp)
                if worst is not None:
                    worst[0] = max(worst[0], err / _tol_lp(lp, V))
                assert err <= _tol_lp(lp, V), (where, j, g, lp, err, _tol_lp(lp, V))
        if np.isnan(H):
            assert np.isnan(got["entropy"]), (where, got)
        else:
            err = abs(float(got["entropy"]) - H)
            if worst is not None:
                worst[1] = max(worst[1], err / _tol_h(H, V))
            assert got["entropy"] >= 0 and err <= _tol_h(H, V), (where, float(got["entropy"]), H, err, _tol_h(H, V))


def _off(rec):
    """The records of ids handed out while alternatives were off."""
    return len(rec) == 0 or bool(np.isnan(rec["entropy"]).all() and (rec["n"] == 0).all() and (rec["alt"]["id"] == -1).all() and np.isnan(rec["alt"]["logprob"]).all())


def _cut(rec8, k):
    """What the list for k must be, from the list for 8: its first k entries, n capped, the entropy as it is."""
    out = rec8.copy()
    out["n"] = np.minimum(out["n"], k); out["alt"]["id"][:, k:] = -1; out["alt"]["logprob"][:, k:] = np.nan
    return out


def _alts_eq(a, b):
    """Bit for bit (the kernel, the library's off-records and numpy all write the one quiet NaN, 0x7fc00000)."""
    return _same_bits(a, b)


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tiny(pkg, ctx):
    m = pkg.Q4ModelLoader.from_file(tiny_gguf()[0]).load(ctx)
    yield m
    m.close()


def _alts(pkg, ctx, x, k, device):
    if not device:
        return pkg.alternatives_rows(ctx, x, k)
    p = ctx.upload(x)
    try:
        return pkg.alternatives_rows(ctx, None, k, device_ptr=p, shape=x.shape)
    finally:
        ctx.free(p)


def _score_identities(pkg, ctx, x, rec8, label):
    """alt[0].logprob has the bits of vox_score_rows' logprob for the computed id, alt[1].id is its runner_up (rows on which something wins)."""
    sc = pkg.score_rows(ctx, x)
    for r in range(len(x)):
        if rec8["n"][r] >= 1:
            assert int(rec8["alt"]["id"][r][0]) == int(sc["id"][r]) and rec8["alt"]["logprob"][r][:1].tobytes() == sc["logprob"][r:r + 1].tobytes(), (label, r, rec8[r], sc[r])
        assert int(rec8["alt"]["id"][r][1]) == int(sc["runner_up"][r]) or rec8["n"][r] == 0, (label, r, rec8[r], sc[r])


# ---- 1. the kernel's edges through vox_alternatives_rows ---------------------------------------------------------------------------------------------------------------
def _handmade(V, rng):
    rnd = lambda: (3.0 * rng.standard_normal(V)).astype(F32)
    rows = [("all equal", np.full(V, 1.25, F32))]
    if V >= 2:
        a = rnd(); a[[V // 3, V - 1]] = a.max() + F32(1); rows.append(("the maximum at two indices", a))
    a = rnd(); a[::3] = -np.inf; rows.append(("every third column -inf", a))
    a = np.full(V, -np.inf, F32); a[rng.permutation(V)[:min(V, 5)]] = rnd()[:min(V, 5)]; rows.append(("fewer than 8 finite columns", a))
    a = rnd(); a[V // 2] = np.nan; rows.append(("a NaN column", a))
    rows.append(("all -inf", np.full(V, -np.inf, F32)))
    a = (1e4 * np.where(rng.random(V) < 0.5, -1.0, 1.0) + rng.standard_normal(V)).astype(F32); a[V // 2] = abs(a[V // 2]); rows.append(("around +-1e4", a))
    a = rnd(); a[rng.permutation(V)[:min(V, 11)]] = a.max() + F32(0.5); rows.append(("up to eleven equal maxima", a))
    return rows


@pytest.mark.parametrize("V", [1, 2, 3, 5, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4099, 8196])
def test_alternatives_rows_edges(pkg, ctx, V):
    """M in {1, 3, 17} at every V (rows 1 and up of a matrix with V % 4 != 0 are misaligned), k in {1, 3, 8}, host and device logits.  The 17-row matrix carries every
    hand-made row behind a random one.  At every shape: the reference; the list for k is the bit prefix of the list for 8; host and device logits give the same bits;
    the identities with vox_score_rows."""
    rng = np.random.default_rng([2027, V]); worst = [0.0, 0.0]
    hand = _handmade(V, rng)
    rnd = lambda n: (3.0 * rng.standard_normal((n, V))).astype(F32)
    mats = [("M 1", rnd(1)), ("M 3", np.vstack([rnd(1), hand[V % len(hand)][1][None], rnd(1)])), ("M 17", np.vstack([rnd(1)] + [r[None] for _, r in hand] + [rnd(16 - len(hand))]))]
    assert [m.shape[0] for _, m in mats] == [1, 3, 17]
    for name, x in mats:
        x = np.ascontiguousarray(x); rec8 = None
        for k in KS[::-1]:
            host = _alts(pkg, ctx, x, k, False); dev = _alts(pkg, ctx, x, k, True)
            _check(host, x, k, f"{name}, host logits", worst)
            assert _alts_eq(host, dev), (name, k, host, dev)
            if k == 8:
                rec8 = host
            assert _alts_eq(host, _cut(rec8, k)), (name, k, host, rec8)
        _score_identities(pkg, ctx, x, rec8, name)
    print(f"V {V}: largest |logprob - ref| / tol = {worst[0]:.3f}, largest |entropy - ref| / tol = {worst[1]:.3f}")


def test_alternatives_facts_of_the_handmade_rows(pkg, ctx):
    """What the issue states about single rows, spelled out (this pins the reference too)."""
    A = lambda x, k=8: pkg.alternatives_rows(ctx, np.asarray(x, F32)[None], k)[0]
    V = 1025
    for k in KS:
        r = A(np.full(V, 1.25, F32), k)
        assert r["n"] == k and list(r["alt"]["id"][:k]) == list(range(k)) and abs(float(r["entropy"]) - np.log(V)) <= _tol_h(np.log(V), V)
        assert np.all(np.abs(r["alt"]["logprob"][:k].astype(np.float64) + np.log(V)) <= _tol_lp(np.log(V), V))
    x = np.zeros(64, F32); x[[40, 7]] = 3      # the maximum at two indices: the lower first, then the rest from column 0 up
    assert list(A(x, 3)["alt"]["id"][:3]) == [7, 40, 0]
    x = np.full(64, -np.inf, F32); x[[50, 9, 33]] = [1, 2, 1]      # fewer than k finite columns
    r = A(x)
    assert r["n"] == 3 and list(r["alt"]["id"]) == [9, 33, 50, -1, -1, -1, -1, -1] and np.isnan(r["alt"]["logprob"][3:]).all() and np.isfinite(r["alt"]["logprob"][:3]).all()
    r = A(np.full(64, -np.inf, F32))
    assert r["n"] == 0 and _off(np.array([r]))      # nothing can win: the record of an unlisted id, by the rule
    x = np.arange(64, dtype=F32); x[63] = np.nan      # a NaN column is never listed; it flags the row
    r = A(x, 3)
    assert r["n"] == 3 and list(r["alt"]["id"][:3]) == [62, 61, 60] and np.isnan(r["alt"]["logprob"]).all() and np.isnan(r["entropy"])
    x = np.zeros(8, F32); x[3] = np.inf      # a maximum that is not finite
    r = A(x, 3)
    assert list(r["alt"]["id"][:3]) == [3, 0, 1] and np.isnan(r["alt"]["logprob"]).all() and np.isnan(r["entropy"])
    r = A(np.full(1, -3.5, F32))
    assert r["n"] == 1 and r["alt"]["id"][0] == 0 and r["alt"]["logprob"][0] == 0 and r["entropy"] == 0
    x = np.full(16, -1e4, F32); x[5] = 1e4      # around +-1e4: one column holds all the mass that f32 can see
    r = A(x, 3)
    assert list(r["alt"]["id"][:3]) == [5, 0, 1] and r["alt"]["logprob"][0] == 0 and r["alt"]["logprob"][1] == F32(-2e4) and r["entropy"] == 0


def test_one_thread_owns_every_winner_and_ties_across_waves(pkg, ctx):
    """V = 8196: columns {0..3, 4096..4099, 8192..8195} all belong to thread 0.  The top 8 among them in ascending order, in descending order and as eight equal
    values: a per-thread list shorter than k loses some, a wrong tie order misorders the equal ones.  Then eight equal maxima in eight different waves (columns
    256 w + c): the lowest indices first."""
    V = 8196; own = [0, 1, 2, 3, 4096, 4097, 4098, 4099, 8192, 8193, 8194, 8195]; rng = np.random.default_rng(8196)
    base = (rng.standard_normal(V) - 20.0).astype(F32)
    rows = []; want = []
    a = base.copy(); a[own] = np.arange(12, dtype=F32); rows.append(a); want.append(own[::-1][:8])             # ascending values: the last columns win
    a = base.copy(); a[own] = -np.arange(12, dtype=F32); rows.append(a); want.append(own[:8])                   # descending values
    a = base.copy(); a[own[2:10]] = 5; rows.append(a); want.append(own[2:10])                                  # eight equal values: by index
    waves = [15, 2, 9, 0, 22, 7, 12, 4]; cols = [256 * w + (37 * w) % 256 for w in waves]
    a = base.copy(); a[cols] = 5; rows.append(a); want.append(sorted(cols))                                    # eight waves (columns 256 w .. 256 w + 255 belong to wave w % 16)
    x = np.stack(rows)
    for device in (False, True):
        rec = _alts(pkg, ctx, x, 8, device)
        assert [list(r) for r in rec["alt"]["id"]] == [list(w) for w in want] and list(rec["n"]) == [8] * 4
        _check(rec, x, 8, "thread 0's columns")
        for k in (1, 3):
            assert _alts_eq(_alts(pkg, ctx, x, k, device), _cut(rec, k))


# ---- 2. the full vocabulary: boundary spikes ----------------------------------------------------------------------------------------------------------------------------
def test_full_vocabulary_boundary_spikes(pkg, ctx):
    """V = 131072: the boundary-spike row of the scores test -- twelve columns at 0 over N(0, 1) - 30.  The eight listed are the first eight spikes; the entropy is
    about log 12, and a lost spike moves it by 0.087 (tol: about 2e-4).  The same row one float past a 16-byte boundary gives the same bits."""
    V = 131072; spikes = [0, 3, 4, 1023, 1024, 1025, 4095, 4096, 65535, 65536, 131068, 131071]
    rng = np.random.default_rng(131072)
    row = (rng.standard_normal(V) - 30.0).astype(F32); row[spikes] = 0
    H = _ref(row, 8)[2]
    assert abs(H - np.log(12.0)) < 1e-4 and _tol_h(H, V) < 3e-4
    two = np.stack([row, row]); worst = [0.0, 0.0]
    rec = pkg.alternatives_rows(ctx, two, 8)
    _check(rec, two, 8, "aligned rows", worst)
    assert list(rec["n"]) == [8, 8] and [list(r) for r in rec["alt"]["id"]] == [spikes[:8]] * 2
    buf = np.zeros(2 * V + 5, F32); buf[1:V + 1] = row; buf[V + 1:2 * V + 1] = row      # [2][V] from one float past a 16-byte boundary
    p = ctx.upload(buf); assert p % 16 == 0
    try:
        mis = pkg.alternatives_rows(ctx, None, 8, device_ptr=p + 4, shape=(2, V))
        mis3 = pkg.alternatives_rows(ctx, None, 3, device_ptr=p + 4, shape=(2, V))
    finally:
        ctx.free(p)
    assert _alts_eq(mis, rec) and _alts_eq(mis3, _cut(rec, 3)), (mis, rec)
    _score_identities(pkg, ctx, two, rec, "full vocabulary")
    print(f"V {V}: largest |logprob - ref| / tol = {worst[0]:.3f}, largest |entropy - ref| / tol = {worst[1]:.3f}")


# ---- the sessions ----------------------------------------------------------------------------------------------------------------------------------------------------------
def _score_bits(al, sc):
    """With scores on too: alt[0] is the id handed out with the score record's logprob bits, alt[1].id its runner-up."""
    assert np.array_equal(al["alt"]["id"][:, 0], sc["id"]) and al["alt"]["logprob"][:, 0].tobytes() == sc["logprob"].tobytes()
    assert np.array_equal(al["alt"]["id"][:, 1], sc["runner_up"])


def test_solo_tiny_records_equal_the_reference_and_do_not_depend_on_the_cuts(pkg, ctx, tiny):
    """3 s through a tiny solo stream at k = 3 with scores on and the tap armed: every record is the reference's on the tapped row of its id, alt[0] is the id handed
    out.  A stream with alternatives off gives the same ids and the same tapped rows, bit for bit.  Then the same clip cut two other ways with no tap and no scores (the
    rows go through the stream's own logits row): bit-identical records."""
    m = tiny; t = _t(pkg, m); x = _loud(3.0, 11); g = _gain(x)
    st = m.create_stream(t, gain=g); plain = m.create_stream(t, gain=g)
    try:
        st.set_alternatives(3); st.set_scores(True); st.tap_arm(64); plain.tap_arm(64)
        ids = _run(st, x, 1600); al = st.alternatives(); sc = st.scores(); lg = st.tap_fetch()
        pids = _run(plain, x, 1600); plg = plain.tap_fetch()
        assert _off(plain.alternatives()) and len(plain.alternatives()) == len(pids)
    finally:
        st.close(); plain.close()
    assert len(ids) == pkg.stream_schedule(len(x), finished=True)[1] == len(al) == len(lg) and len(ids) >= 20
    assert np.array_equal(pids, ids) and _same_bits(plg, lg)
    worst = [0.0, 0.0]
    _check(al, lg, 3, "tiny solo stream", worst)
    assert np.array_equal(al["alt"]["id"][:, 0], ids) and (al["n"] == 3).all() and np.isfinite(al["entropy"]).all()
    _score_bits(al, sc)
    for size in (2560, 7777):
        st = m.create_stream(t, gain=g)
        try:
            st.set_alternatives(3)
            ids2 = _run(st, x, size); al2 = st.alternatives()
            assert _alts_eq(st.alternatives(3, 5), al2[3:8]) and len(st.alternatives(len(ids2), 0)) == 0
        finally:
            st.close()
        assert np.array_equal(ids2, ids) and _alts_eq(al2, al), f"pieces of {size} samples"
    print(f"tiny solo stream: largest |logprob - ref| / tol = {worst[0]:.3f}, largest |entropy - ref| / tol = {worst[1]:.3f}")


def test_solo_tiny_toggling_reset_refusals_and_bytes(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); x = _loud(3.0, 12); g = _gain(x); L = pkg.lib(); V = m.config.vocab
    full3 = m.create_stream(t, gain=g); full8 = m.create_stream(t, gain=g); st = m.create_stream(t, gain=g, max_positions=256)
    try:
        full3.set_alternatives(3); ids = _run(full3, x, 1600); ref3 = full3.alternatives()
        full8.set_alternatives(8); assert np.array_equal(_run(full8, x, 1600), ids); ref8 = full8.alternatives()
        assert _alts_eq(ref3, _cut(ref8, 3))
        # off -> 3 -> 8 -> off across pushes
        b0 = st.info()["bytes"]
        a, b, c = 12000, 24000, 36000
        got = [st.push(x[:a])]; n0 = len(got[0])
        st.set_alternatives(3); b1 = st.info()["bytes"]
        got.append(st.push(x[a:b])); n1 = n0 + len(got[1])
        st.set_alternatives(8)
        got.append(st.push(x[b:c])); n2 = n1 + len(got[2])
        st.set_alternatives(0)
        got += [st.push(x[c:]), st.finish()]
        got = np.concatenate(got); al = st.alternatives()
        assert np.array_equal(got, ids) and len(al) == len(ids) and 0 < n0 < n1 < n2 < len(ids)
        assert _off(al[:n0]) and _off(al[n2:])      # handed out while off
        assert _alts_eq(al[n0:n1], ref3[n0:n1]) and _alts_eq(al[n1:n2], ref8[n1:n2])      # each record at the k of its call: its own n
        assert (al["n"][n0:n1] == 3).all() and (al["n"][n1:n2] == 8).all()
        assert b1 - b0 == (256 + 2) * 72 + V * 4      # the records of every position the stream was created for + one logits row, at the first k > 0 ...
        st.set_alternatives(5); st.set_alternatives(0); st.set_alternatives(3)
        assert st.info()["bytes"] == b1               # ... only
        st.set_scores(True)
        assert st.info()["bytes"] == b1 + (256 + 2) * 16      # the logits row is there already: scores add their records alone
        # out-of-range requests: refused, nothing written
        n = len(ids); buf = np.full(n + 4, -7, dtype=pkg.ALTS_DTYPE); before = buf.tobytes()
        for first, cnt in ((0, n + 1), (n, 1), (-1, 2), (2, -1), (n + 1, 0), (2 ** 31 - 1, 2 ** 31 - 1)):
            assert L.vox_stream_alternatives(st.h, first, cnt, buf.ctypes.data) == 1 and "handed out" in L.vox_last_error().decode(), (first, cnt)
        assert buf.tobytes() == before
        # reset: the list starts over, k stays
        st.reset()
        assert len(st.alternatives()) == 0 and L.vox_stream_alternatives(st.h, 0, 1, buf.ctypes.data) == 1
        again = _run(st, x, 2560)
        assert np.array_equal(again, ids) and _alts_eq(st.alternatives(), ref3)
        _score_bits(st.alternatives(), st.scores())
    finally:
        full3.close(); full8.close(); st.close()


def test_solo_full_size_engine_path(pkg, ctx):
    """The full-size peaked model, 3 s: every decode step is an engine launch, its logits row written on request; the ids are the plain stream's, the records the
    reference's on the tapped rows at V = 131072."""
    m = pkg.Q4ModelLoader.from_file(_full_path(True)).load(ctx)
    try:
        t = _t(pkg, m); x = _loud(3.0, 13); g = _gain(x)
        a = m.create_stream(t, gain=g); b = m.create_stream(t, gain=g)
        try:
            a.set_alternatives(8); a.tap_arm(64)
            ids = _run(a, x, 2560); al = a.alternatives(); lg = a.tap_fetch(); info = a.info()
            plain = _run(b, x, 2560)
        finally:
            a.close(); b.close()
        assert info["engine_steps"] > 0 and info["engine_steps"] + info["operator_steps"] == len(ids)
        assert lg.shape == (len(ids), 131072) and np.array_equal(plain, ids) and np.array_equal(al["alt"]["id"][:, 0], ids)
        worst = [0.0, 0.0]
        _check(al, lg, 8, "full-size solo stream", worst)
        print(f"full-size solo stream: largest |logprob - ref| / tol = {worst[0]:.3f}, largest |entropy - ref| / tol = {worst[1]:.3f}")
    finally:
        m.close()


def test_group_tiny_rounds_of_three_widths(pkg, ctx, tiny):
    """Three members fed 1.3 s, 2.1 s and 3 s in ONE call that finishes them all: rounds of width 3, 2 and 1.  k = 3, 0 and 8: members 0 and 2 get the reference's
    records on their own tapped rows, member 1 the records of an unlisted id; the ids are those of the same group with alternatives off everywhere."""
    m = tiny; t = _t(pkg, m)
    clips = [_loud(1.3, 21), _loud(2.1, 22), _loud(3.0, 23)]; ks = [3, 0, 8]
    g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips]); plain = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips])
    try:
        b0 = [g.info(k)["bytes"] for k in range(3)]
        for k in range(3):
            g.set_alternatives(k, ks[k])
        b1 = [g.info(k)["bytes"] for k in range(3)]
        assert b1[1] == b0[1] and b1[0] - b0[0] == b1[2] - b0[2] and (b1[0] - b0[0]) % 72 == 0 and b1[0] > b0[0]
        for k in range(3):
            g.tap_arm(k, 64)
        out = g.advance({k: x for k, x in enumerate(clips)}, finish=[0, 1, 2])
        ref = plain.advance({k: x for k, x in enumerate(clips)}, finish=[0, 1, 2])
        n = [len(out[k]) for k in range(3)]
        assert n == [pkg.stream_schedule(len(x), finished=True)[1] for x in clips] and n[0] < n[1] < n[2]
        assert all(np.array_equal(out[k], ref[k]) and _off(plain.alternatives(k)) and len(plain.alternatives(k)) == n[k] for k in range(3))
        for k in (0, 2):
            al = g.alternatives(k); lg = g.tap_fetch(k)
            assert np.array_equal(al["alt"]["id"][:, 0], out[k]) and len(lg) == n[k] and (al["n"] == ks[k]).all()
            _check(al, lg, ks[k], f"group member {k}")
        assert _off(g.alternatives(1)) and len(g.alternatives(1)) == n[1]
        L = pkg.lib(); buf = np.full(4, -7, dtype=pkg.ALTS_DTYPE); before = buf.tobytes()
        assert L.vox_stream_group_alternatives(g.h, 0, n[0] - 1, 2, buf.ctypes.data) == 1 and L.vox_stream_group_alternatives(g.h, 3, 0, 1, buf.ctypes.data) == 1 and buf.tobytes() == before
        g.reset(0, _gain(clips[0]))      # the member's next connection: its list starts over, its k stays
        assert len(g.alternatives(0)) == 0
        again = g.advance({0: clips[0]}, finish=[0])[0]; al = g.alternatives(0)      # (rounds of one now: a group's logits are not bit for bit those of its wider rounds)
        assert np.array_equal(again, out[0]) and len(al) == n[0] and (al["n"] == 3).all() and np.array_equal(al["alt"]["id"][:, 0], again)
    finally:
        g.close(); plain.close()


# ---- peek --------------------------------------------------------------------------------------------------------------------------------------------------------------------
def test_solo_peek_records_are_the_ones_finish_appends(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); x = _loud(3.0, 14); g = _gain(x)
    st = m.create_stream(t, gain=g)
    try:
        st.set_alternatives(3)
        assert len(st.peeked_alternatives()) == 0
        got = [st.push(x[:20000])]
        tail = st.peek(); pa = st.peeked_alternatives()
        assert len(tail) == len(pa) > 0 and np.array_equal(pa["alt"]["id"][:, 0], tail) and len(st.alternatives()) == len(got[0])      # the session's list is not extended
        assert _alts_eq(st.peeked_alternatives(), pa)      # (reading them does not use them up)
        got.append(st.push(x[20000:]))
        assert len(st.peeked_alternatives()) == 0          # gone with the next push
        have = st.info()["ids"]
        tail = st.peek(); pa = st.peeked_alternatives()
        L = pkg.lib(); buf = np.full(len(pa), -7, dtype=pkg.ALTS_DTYPE); before = buf.tobytes(); n = C.c_int32(-3)
        assert L.vox_stream_peeked_alternatives(st.h, buf.ctypes.data, len(pa) - 1, C.byref(n)) == 1 and "capacity" in L.vox_last_error().decode()
        assert buf.tobytes() == before and n.value == -3
        assert len(st.alternatives()) == have == st.info()["ids"]
        fin = st.finish()
        assert np.array_equal(fin, tail) and _alts_eq(st.alternatives(have), pa) and len(st.peeked_alternatives()) == 0
        ids = np.concatenate(got + [fin]); al = st.alternatives()
    finally:
        st.close()
    never = m.create_stream(t, gain=g)      # a session that never had k > 0 keeps no records: a peek's are off-records all the same, and go with the next push
    try:
        never.push(x[:20000]); tail = never.peek()
        assert len(never.peeked_alternatives()) == len(tail) > 0 and _off(never.peeked_alternatives())
        never.push(x[20000:22000])
        assert len(never.peeked_alternatives()) == 0 and _off(never.alternatives()) and len(never.alternatives()) == never.info()["ids"]
    finally:
        never.close()
    ref = m.create_stream(t, gain=g)
    try:
        ref.set_alternatives(3)
        assert np.array_equal(_run(ref, x, 1600), ids) and _alts_eq(ref.alternatives(), al)      # the peeks left the session what it was
    finally:
        ref.close()


def test_group_peek_records_are_the_ones_finish_appends(pkg, ctx, tiny):
    m = tiny; t = _t(pkg, m); clips = [_loud(2.0, 24), _loud(2.6, 25)]
    g = m.create_stream_group(t, 2, gains=[_gain(x) for x in clips])
    try:
        g.set_alternatives(0, 8)      # member 1 stays off
        g.advance({0: clips[0][:20000], 1: clips[1][:20000]})
        have = [g.info(k)["ids"] for k in range(2)]
        tails = g.peek([0, 1]); pa = [g.peeked_alternatives(k) for k in range(2)]
        assert all(len(pa[k]) == len(tails[k]) > 0 and len(g.alternatives(k)) == have[k] for k in range(2))
        assert np.array_equal(pa[0]["alt"]["id"][:, 0], tails[0]) and _off(pa[1])
        g.advance({0: clips[0][20000:20100]})
        assert len(g.peeked_alternatives(0)) == 0 and _alts_eq(g.peeked_alternatives(1), pa[1])      # member 0 was fed: its peeked records are gone, member 1's stay
        have = [g.info(k)["ids"] for k in range(2)]
        tails = g.peek([0, 1]); pa = [g.peeked_alternatives(k) for k in range(2)]
        fin = g.advance({0: clips[0][20100:20100], 1: clips[1][20000:20000]}, finish=[0, 1])
        for k in range(2):
            assert np.array_equal(fin[k], tails[k]) and _alts_eq(g.alternatives(k, have[k]), pa[k]) and len(g.peeked_alternatives(k)) == 0
    finally:
        g.close()


# ---- the CLI ----------------------------------------------------------------------------------------------------------------------------------------------------------------
def _check_word_alternatives(words, k):
    """Every token of the CLI fixture's tokenizer is one word " w<index>" (id 1000 + index): the word's id is known from its text."""
    assert len(words) >= 3
    for w in words:
        assert w["first_id"] == w["last_id"] == w["weakest"]["k"] and np.isfinite(w["entropy"]) and w["entropy"] >= 0
        alts = w["weakest"]["alternatives"]
        assert len(alts) == k and alts[0]["id"] == 1000 + int(w["text"].strip()[1:]) and alts[0]["text"] == w["text"]
        assert abs(alts[0]["logprob"] - w["logprob"]) == 0 and all(a["logprob"] >= b["logprob"] for a, b in zip(alts, alts[1:]))


def test_cli_live_alternatives(pkg, tmp_path):
    """--live --live-words --live-alternatives 3: every word line has its entropy and the alternatives of its weakest id, the first of them that id; stdout and the
    other fields are those of the run without the flag."""
    cmd, wavs = _cli_files(pkg, tmp_path); out = str(tmp_path / "words.jsonl"); out0 = str(tmp_path / "words0.jsonl")
    r = subprocess.run(cmd + ["--audio", wavs[0], "--live", "--live-words", out, "--live-alternatives", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r0 = subprocess.run(cmd + ["--audio", wavs[0], "--live", "--live-words", out0], capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r0.stdout == r.stdout and r.stdout.strip()
    words = _word_lines(out); words0 = _word_lines(out0)
    _check_word_alternatives(words, 3)
    assert [{k: v for k, v in w.items() if k not in ("entropy", "weakest")} for w in words] == words0 and all("entropy" not in w and "weakest" not in w for w in words0)


def test_cli_live_group_alternatives(pkg, tmp_path):
    cmd, wavs = _cli_files(pkg, tmp_path); out = str(tmp_path / "words.jsonl")
    base = cmd + ["--audio", wavs[0], "--audio", wavs[1], "--live", "--live-group", "2"]
    r = subprocess.run(base + ["--live-words", out, "--live-alternatives", "3"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Error" not in r.stderr, r.stderr
    r0 = subprocess.run(base, capture_output=True, text=True, timeout=300)
    assert r0.returncode == 0 and r0.stdout == r.stdout and len(r.stdout.split("\n")) == 3
    words = _word_lines(out)
    assert {w["file"] for w in words} == set(wavs)
    for path in wavs:
        _check_word_alternatives([w for w in words if w["file"] == path], 3)
