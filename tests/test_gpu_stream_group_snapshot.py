"""Snapshot and resume of a stream group's members (vox_stream_group_snapshot / _restore; include/voxtral_hip.h, SNAPSHOT AND RESUME) on the tiny model.

Same slot (tests/snapshot_group_cases.py): group A runs uninterrupted; group B, fed the same calls, snapshots member 1 at a call boundary, RESETS it and restores it.
Every round of B then has A's width and picks A's kernels, so the claim is bit for bit for all three members: ids per call, tapped logits rows, member 1's score and
alternatives records, pool() and the pages held per member after every call (the physical page numbers may differ), info words 0-4.  For slab and paged groups
in-process; for an endless paged group in a worker process (its attention counts in launch slots other tests hold to 0 in their process).
Across slots and kinds (member -> another slot, member -> solo stream, solo stream -> member) the rounds' widths differ from the reference's, so the ids are held by the
group files' rule against the uninterrupted SOLO session (stream_helpers._held, TOL = 2e-4), on a clip for which that rule's precondition holds."""
import numpy as np
import pytest

from model_fixtures import attn_launches, gemm_launches, tiny_gguf
from snapshot_group_cases import KINDS, STEP, same_slot_case
from stream_helpers import _gain, _held, _stop, _t
from worker_tests import check, run_worker

pytestmark = pytest.mark.gpu
TOL = 2e-4


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


@pytest.fixture(scope="module")
def solo(pkg, tiny):
    """(clip, gain, ids, logits rows) of the uninterrupted solo session, the seed moved on until its first near-tie lies at or beyond half of its ids (_held's precondition)"""
    t = _t(pkg, tiny)
    for seed in range(77, 12077, 1000):
        x = pkg.synth.synth_audio(12.0, seed=seed)
        st = tiny.create_stream(t, gain=_gain(x)); st.tap_arm(256)
        try:
            ids = np.concatenate([st.push(x[a:a + STEP]) for a in range(0, len(x), STEP)] + [st.finish()]); lg = st.tap_fetch()
        finally:
            st.close()
        if 2 * _stop(lg, TOL) >= len(ids):
            for a in (x, ids, lg):
                a.setflags(write=False)
            return x, _gain(x), ids, lg
    raise AssertionError("no seed gives a clip that can carry an ids claim")


@pytest.mark.parametrize("kind", ["slab", "paged"])
def test_member_snapshot_reset_restore_in_its_slot(pkg, tiny, kind):
    same_slot_case(pkg, tiny, kind)


def test_endless_member_in_a_worker_process(tmp_path_factory):
    run = run_worker("stream_group_snapshot_worker.py", tmp_path_factory.mktemp("group_snapshot"), 300)
    check(run, "test_endless_member_snapshot_reset_restore_in_its_slot")


def _feed(g, k, x, a, b, out):
    """member k alone is fed x[a:b] in calls of STEP samples (finishing with the clip's last sample)"""
    for p in range(a, b, STEP):
        q = min(p + STEP, b)
        out.extend(g.advance({k: x[p:q]}, finish=[k] if q == len(x) else []).get(k, []))


def test_a_paged_restore_into_a_pool_one_page_short_is_refused_and_changes_nothing(pkg, tiny, solo):
    x, gain, _, _ = solo
    t = _t(pkg, tiny); cut = 26 * STEP      # position 38 + 32 = 70 .. : 5 pages of 16 rows
    src = tiny.create_stream_group(t, 3, gains=[gain] * 3, **KINDS["paged"]); ids = []
    _feed(src, 0, x, 0, cut, ids); blob = src.snapshot(0); need = src.pool()["held"][0]; src.close()
    assert need == -(-pkg.snapshot_info(blob)["positions"] // 16) >= 5
    short = 9 - 3 + need - 1      # three seeds of 3 pages; member 1's own 3 count as free: one page short of `need`
    runs = []
    for attempt in (True, False):      # the group that saw the refused restore, and its twin that never did
        g = tiny.create_stream_group(t, 3, gains=[gain] * 3, max_positions=256, page_rows=16, pool_pages=short)
        try:
            g.tap_arm(0, 64); got = []
            _feed(g, 0, x, 0, 2 * STEP, got)
            if attempt:
                before = (g.pool(), [g.pages(k) for k in range(3)], [g.info(k) for k in range(3)])
                with pytest.raises(pkg.VoxError) as e:
                    g.restore(1, blob)
                assert f"member 1: the restore needs {need} pages of the pool, {need - 1} are free" in str(e.value), str(e.value)
                assert (g.pool(), [g.pages(k) for k in range(3)], [g.info(k) for k in range(3)]) == before
            _feed(g, 0, x, 2 * STEP, 6 * STEP, got)
            runs.append((np.array(got), g.tap_fetch(0), g.pool()))
        finally:
            g.close()
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]
    g = tiny.create_stream_group(t, 3, gains=[gain] * 3, max_positions=256, page_rows=16, pool_pages=short + 1)      # one page more: it fits
    try:
        g.restore(1, blob); assert g.pool()["held"] == [3, need, 3] and g.pool()["free"] == 0
    finally:
        g.close()
    slab = tiny.create_stream_group(t, 2, gains=[gain] * 2, max_positions=60)      # a slab member is refused beyond the slab's max_positions
    try:
        with pytest.raises(pkg.VoxError, match="created for 60"):
            slab.restore(0, blob)
    finally:
        slab.close()


@pytest.mark.parametrize("kind", ["slab", "paged"])
def test_across_slots_and_kinds_the_ids_are_held_against_the_solo_session(pkg, tiny, solo, kind):
    x, gain, rids, rlg = solo
    t = _t(pkg, tiny); cut = 20 * STEP + 123
    # member 1 -> idle member 2 of the same group, fed in member 1's place from there on
    g = tiny.create_stream_group(t, 3, gains=[gain] * 3, **KINDS[kind]); ids = []
    try:
        _feed(g, 1, x, 0, 20 * STEP, ids); ids.extend(g.advance({1: x[20 * STEP:cut]}).get(1, []))
        blob = g.snapshot(1)
        g.restore(2, blob)
        tail = list(g.advance({2: x[cut:21 * STEP]}).get(2, [])); _feed(g, 2, x, 21 * STEP, len(x), tail)
        assert g.info(2)["ids"] == len(ids) + len(tail)
    finally:
        g.close()
    _held(np.array(ids + tail, np.int32), rids, rlg, f"{kind}: member 1 -> member 2", TOL)
    # member -> solo stream
    st = tiny.create_stream(t, gain=0.3, enc_capacity_rows=760)
    try:
        st.restore(blob)
        into_solo = list(st.push(x[cut:])) + list(st.finish())
    finally:
        st.close()
    _held(np.array(ids + into_solo, np.int32), rids, rlg, f"{kind}: member -> solo stream", TOL)
    # solo stream -> member
    st = tiny.create_stream(t, gain=gain); head = list(st.push(x[:cut])); sblob = st.snapshot(); st.close()
    g = tiny.create_stream_group(t, 3, gains=[1.0] * 3, **KINDS[kind]); tail = []
    try:
        a0, g0 = attn_launches(pkg), gemm_launches(pkg)
        g.restore(0, sblob); again = g.snapshot(0)
        assert attn_launches(pkg) == a0 and gemm_launches(pkg) == g0      # a snapshot or restore launches none of the counted attention or GEMM forms
        assert pkg.snapshot_info(again)["positions"] == pkg.snapshot_info(sblob)["positions"] and again.size == sblob.size
        tail = list(g.advance({0: x[cut:21 * STEP]}).get(0, [])); _feed(g, 0, x, 21 * STEP, len(x), tail)
    finally:
        g.close()
    _held(np.array(head + tail, np.int32), rids, rlg, f"{kind}: solo stream -> member", TOL)
