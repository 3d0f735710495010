"""The cases of the ring decode attention (tests/test_gpu_attn_decode_ring.py and its worker): a ring run is a geometry, a ring capacity and ONE position; its keys
are the window's -- min(pos, window) + 1 of them -- built by attn_decode_ref as a flat case of exactly that many rows with pos = n - 1 and the same window, so the
flat launch and the float64 reference see them from row 0 and the ring launch sees row j of the sequence at ring row j % cap, every other ring row NaN.

Window 200: 201 keys exceed the 160 the kernel requests up front, so the tail loops of the scores and of P.V run across the wrap.  Capacities 256 (a power of two)
and 264 (not one).  Positions: inside the first lap (100, 199, 200: the window starts to move), either side of the first wrap (cap - 1, cap, cap + 1), the window
wholly inside the second lap (cap + 199) and at its end (2 cap - 1), and the last position a session can reach (2^24 - 1)."""
from collections import namedtuple

import numpy as np

import attn_decode_ref as R

WINDOW = 200
GEOS = ((4, 2), (2, 2))
CAPS = (256, 264)
LAST = (1 << 24) - 1

Run = namedtuple("Run", "H KV cap pos")


def positions(cap):
    return (100, 199, 200, cap - 1, cap, cap + 1, cap + 199, 2 * cap - 1, LAST)


RUNS = {f"{H}x{KV}-cap{cap}-pos{p}": Run(H, KV, cap, p) for (H, KV) in GEOS for cap in CAPS for p in positions(cap)}


def window_of(run):
    j_lo = max(0, run.pos - WINDOW)
    return j_lo, run.pos - j_lo + 1


def flat_case(run):
    n = window_of(run)[1]
    return R.make_case(f"ring{run.cap}p{run.pos}", "normal", run.H, run.KV, WINDOW, n, (n - 1,))


def flat_inputs(run):
    """(the flat case, q [1][H*128], K, V [1][KV][n][128]): the window's keys from row 0."""
    c = flat_case(run)
    return (c,) + R.build_inputs(c)


def to_ring(run, k, v):
    """K, V [1][KV][cap][128]: ring[j % cap] = row j for the window's keys, NaN everywhere else."""
    j_lo, n = window_of(run)
    assert k.shape[2] == n and n <= run.cap
    rk = np.full((1, run.KV, run.cap, R.HD), np.nan, np.float32); rv = np.full_like(rk, np.nan)
    at = (j_lo + np.arange(n)) % run.cap
    rk[0][:, at] = k[0]; rv[0][:, at] = v[0]
    return rk, rv
