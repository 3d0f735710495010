"""The float64 reference of the live sessions' level records (vox_tick_level; DESIGN.md section 8, "Levels"), and the bound the tests hold the device to.

Record k of an utterance describes the window w_k = [2560 (k - 1), 2560 k) of its 16 kHz samples, each taken as the mel front end reads it: v = f32(gain * x[i]) (one
f32 multiplication), 0 below index 0 (the silent left pad) and, here, 0 behind the end of x (a finish's zero pad).
  peak         max |v|: exact in any order, so the device's must have the reference's bits;
  mean_square  (sum v^2) / 2560.  The device squares in f32 (one rounding each), adds 18 times on every path of its tree (10 in a thread, 6 in a wave, 2 across the
               waves) and divides once: with no underflow its result is within (1 + 2^-24)^20 - 1 < 2^-19 relative of the float64 sum of the exact squares.  A square below 2^-126 rounds on the subnormal
               grid instead -- absolute error at most 2^-150 each, 2560 of them divided by 2560 again, plus the scale's own rounding there: 2^-149 in all, the
               spacing of f32 at zero.  bound() is the sum of the two; on samples whose squares are normal numbers it is the relative bound alone."""
import numpy as np

F32 = np.float32
TICK = 2560
LEVEL_DTYPE = np.dtype([("peak", "<f4"), ("mean_square", "<f4")])      # vox_tick_level
REL = 2.0 ** -19
ABS = 2.0 ** -149


def window(k):
    """w_k as (first, end) in the utterance's own 16 kHz sample index."""
    return TICK * (k - 1), TICK * k


def taken(x, gain, first, end):
    """The samples first .. end - 1 as the front end reads them: f32(gain * x[i]), 0 outside 0 .. len(x) - 1."""
    x = np.asarray(x, dtype=F32); v = np.zeros(end - first, dtype=F32)
    lo, hi = max(first, 0), min(end, len(x))
    if hi > lo:
        with np.errstate(under="ignore", over="ignore"):
            v[lo - first:hi - first] = x[lo:hi] * F32(gain)
    return v


def level_of(v):
    """(peak as f32, mean_square in float64) of one window's f32 samples."""
    v = np.asarray(v, dtype=F32)
    d = v.astype(np.float64)
    return F32(np.abs(v).max()) if v.size else F32(0), float((d * d).sum() / TICK)


def levels(x, gain, n):
    """Records 0 .. n - 1 of the utterance x at `gain`: (peaks f32 [n], mean squares float64 [n])."""
    pk = np.zeros(n, dtype=F32); ms = np.zeros(n, dtype=np.float64)
    for k in range(n):
        pk[k], ms[k] = level_of(taken(x, gain, *window(k)))
    return pk, ms


def bound(ms):
    return REL * np.asarray(ms, dtype=np.float64) + ABS


def check(rec, pk, ms, label):
    """Device records against the reference: peak bit for bit, mean_square within bound(); an exact 0 where the window is all zeros."""
    assert len(rec) == len(pk) == len(ms), (label, len(rec), len(pk))
    got_pk = np.asarray(rec["peak"], dtype=F32); got_ms = np.asarray(rec["mean_square"], dtype=F32)
    bad = np.flatnonzero(got_pk.view(np.uint32) != np.asarray(pk, dtype=F32).view(np.uint32))
    assert bad.size == 0, (label, "peak", bad[:8], got_pk[bad[:8]], pk[bad[:8]])
    err = np.abs(got_ms.astype(np.float64) - ms)
    bad = np.flatnonzero(~(err <= bound(ms)))
    assert bad.size == 0, (label, "mean_square", bad[:8], got_ms[bad[:8]], ms[bad[:8]], err[bad[:8]] / np.maximum(ms[bad[:8]], 1e-300))
    zero = np.flatnonzero(np.asarray(ms) == 0)
    assert (got_ms[zero].view(np.uint32) == 0).all(), (label, "zero windows", got_ms[zero])
    return float((err / bound(ms)).max()) if len(ms) else 0.0
