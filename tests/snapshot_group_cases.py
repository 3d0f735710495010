"""The same-slot case of tests/test_gpu_stream_group_snapshot.py as a plain function: the file runs it in-process for slab and paged groups, and
tests/stream_group_snapshot_worker.py runs it for the endless kind in a process of its own (an endless group's decode attention counts in launch slots that other tests
hold to 0 in theirs)."""
import numpy as np

from stream_helpers import _gain, _t

STEP = 3200
KINDS = {"slab": dict(max_positions=256), "paged": dict(max_positions=256, page_rows=16, pool_pages=48), "endless": dict(page_rows=16, pool_pages=48, endless=True)}


def group_clips(pkg):
    return [pkg.synth.synth_audio(s, seed=610 + i) for i, s in enumerate((14.0, 11.0, 8.0))]


def _calls(clips, starts=(0, 1, 3)):
    """the calls of a run: [(feeds {member: samples}, finish [members])]; member k starts in call starts[k] and finishes with its last piece"""
    out = []; c = 0
    while True:
        feeds, fin = {}, []
        for k, x in enumerate(clips):
            i = c - starts[k]
            if i >= 0 and i * STEP < len(x):
                feeds[k] = x[i * STEP:(i + 1) * STEP]
                if (i + 1) * STEP >= len(x):
                    fin.append(k)
        if not feeds and c > max(starts):
            return out
        out.append((feeds, fin)); c += 1


def _state(g, paged):
    if not paged:
        return None
    p = g.pool()
    assert p["free"] + sum(p["held"]) == p["pool_pages"] and [len(g.pages(k)) for k in range(g.n_members)] == p["held"], p
    every = [q for k in range(g.n_members) for q in g.pages(k)]
    assert len(set(every)) == len(every)      # no page in two tables
    return p


def run_group(pkg, m, kind, clips, suspend_after=None, member=1):
    """One group fed the calls of `clips`; suspend_after = c: behind call c, `member` is snapshotted (twice: identical blobs, nothing changed), reset, and restored.
    -> dict(ids per member per call, taps per member, rec / alt of `member`, pool states per call, words per call)"""
    t = _t(pkg, m); paged = kind != "slab"
    g = m.create_stream_group(t, 3, gains=[_gain(x) for x in clips], **KINDS[kind])
    out = dict(ids=[[] for _ in clips], taps=[[] for _ in clips], pools=[], words=[])
    try:
        for k in range(3):
            g.tap_arm(k, 256)
        g.set_scores(member, True); g.set_alternatives(member, 3)
        for c, (feeds, fin) in enumerate(_calls(clips)):
            got = g.advance(feeds, finish=fin)
            for k in range(3):
                out["ids"][k].append(got.get(k, np.zeros(0, np.int32)))
            out["pools"].append(_state(g, paged)); out["words"].append([[g.info(k)[w] for w in ("samples", "positions", "ids", "encoder_position", "ring_rows")] for k in range(3)])
            if c == suspend_after:
                before = (g.info(member), _state(g, paged))
                blob = g.snapshot(member)
                assert g.snapshot(member).tobytes() == blob.tobytes() and (g.info(member), _state(g, paged)) == before
                info = pkg.snapshot_info(blob)
                assert info["positions"] == before[0]["positions"] > 45 and info["scores"] == 1 and info["alternatives"] == 3
                out["taps"][member].append(g.tap_fetch(member))
                g.reset(member, gain=0.5)      # the member's memory is given back; the restore brings the blob's gain
                if paged:
                    assert g.pool()["held"][member] == 3
                g.restore(member, blob)
                g.tap_arm(member, 256)
                assert (g.info(member)["positions"], _state(g, paged)) == (before[0]["positions"], before[1])
                out["blob"] = blob
        for k in range(3):
            out["taps"][k].append(g.tap_fetch(k))
        out["rec"] = g.scores(member); out["alt"] = g.alternatives(member)
    finally:
        g.close()
    out["taps"] = [np.concatenate(v) for v in out["taps"]]
    return out


def same_slot_case(pkg, m, kind):
    clips = group_clips(pkg)
    a = run_group(pkg, m, kind, clips)
    b = run_group(pkg, m, kind, clips, suspend_after=9)
    assert sum(len(v) for v in a["ids"][1][10:]) >= 20      # the restored member has most of its utterance ahead
    for k in range(3):
        for c, (u, v) in enumerate(zip(b["ids"][k], a["ids"][k])):
            assert np.array_equal(u, v), f"{kind}: member {k}, call {c}: {u}, the uninterrupted group's {v}"
        assert a["taps"][k].shape == b["taps"][k].shape and np.array_equal(a["taps"][k].view(np.uint32), b["taps"][k].view(np.uint32)), f"{kind}: member {k}'s logits rows differ"
    assert a["rec"].tobytes() == b["rec"].tobytes() and a["alt"].tobytes() == b["alt"].tobytes(), kind
    assert a["pools"] == b["pools"] and a["words"] == b["words"], kind      # pool() counts and the pages held per member, vox_stream_group_info words 0-4, after every call
    return a, b
