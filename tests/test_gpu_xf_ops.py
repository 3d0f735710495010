"""The operators of the batched XF decode step, one launch at a time, against float64 (vox_debug_xf_op -> the decode chain's own parameter fill -> launch_q4_gemm on
one XF group / launch_q4_wide on 2..4 slot groups; tests/linear_ref.py, pinned on the CPU by tests/test_linear_ref.py): q|k|v with the folded RMSNorm, RoPE and the
cache write (ROPE_KV, every cache form), wo / w2 (RESID_XF), w1|w3 (SWIGLU_XF), the lm_head (STORE + folded norm); and the encoder's RoPE rows (EPI_ROPE_ROWS in
q4_gemm_big_kernel, the `big_rope` form of vox_debug_gemm_launches).

Every case asserts WHICH form ran: the launch counters (skinny / wide / xf_rows / big / big_rope) and the plan the hook returns, against the launchers' thresholds
restated below as named constants.  The closing test fails if an instantiation of REQUIRED was never the asserted form of a passing case.

Shapes (derived from q4_skinny_plan and q4_wide_plan; K / 128 = K steps, N / 16 = n-tiles):
  one group  n-tiles per wave 1 | 2 | 4 from 0 | 384 | 768 tiles (N 6144 / 12288); split-K waves ks = 1 | 2 | 4 from 1 | 2 | 4 steps, 8 when tiles / ntw < 256 and
             steps >= 16; a straight-line instantiation when steps / ks is whole and listed (VOX_ST_FORMS), else the loop.  ks < ntw (K 128 or 256 at N >= 6144) sends
             tiles through the epilogue's reloading (non-`pre`) path.
  wide       n-tiles per wave 2 from 384 tiles, 4 for STORE from 4096 (N 65536); K slices kz = the smallest divisor of the steps with ceil(tiles / (4 ntw)) kz >= 320,
             capped at 24; N = 128 with K = 128 / 1024 / 1152 / 3072 / 9216 gives kz 1 / 8 / 9 / 24 / 24 (3 steps per slice).
Every group, row and slot has data of its own (rows, partial sums, residuals, positions, cache slices), every output buffer starts as a sentinel, and EVERY element
of every output is compared: with the reference where the operator writes, with the sentinel where it does not (rows >= M, columns >= n_q of the q|k|v rows, cache
cells outside the written (slice, head, row), the gaps of a group stride).  ssq_out rows >= M are written as zeros by the one-group kernel (as
test_gpu_group_delays_op.py pins).

Error bars (derived as in test_gpu_linear.py, carried by linear_ref): before the epilogue 2^-16 mag_ij (the wide step's <= 24 plane additions, 24 * 2^-24 mag, sit
inside that bound's factor of two); the folded norm |ref| (n_part + 8) 2^-24 more; RoPE |c| b_v + |s| b_other + 4 ulp of |a c| + |b s|; SwiGLU as carry_bound has it;
a residual or bias addition half an ulp of the result; the two scale multiplications of RESID_XF's planes one ulp; a value read back from XF planes 2^-17 |a| more.
ssq_out is held to the float64 sum of squares of the kernel's own returned `out` (16 terms: 2^-20 relative), `out` itself to the reference.  A bf16 pool holds,
bit for bit, vox_kv_round_bf16 of the f32-pool run of the same case, which is the run held to float64.  An all-zero row gives exactly zero.

Bit equality of a wide group with the one-group launch is asserted nowhere: the wide step sums K slices across workgroups in slice order, the one-group kernel sums
its waves' ranges, and no comment of either promises equal bits (test_gpu_stream_alternatives.py notes that a group's logits are not those of wider rounds).

The prefill's row-major form of the wide GEMM (VOX_XF_MODE_WIDE_ROWS: launch_q4_skinny_mt2_planes, then launch_splitk_finish_rope_kv / _swiglu_xf / _resid) runs at
M = 17, 38 and 48 for each finishing kernel, with 1, 4, 8, 9 and 24 K slices, a non-zero pos_off and a bias; rows >= M of the outputs keep the sentinel.
Activations: the linear suite's kinds (linear_ref.activations) -- ramp, scales (row scales over six decades, zeros, an all-zero row) and, on one-group and wide cases
of every epilogue, offset3 / offset30, whose non-zero mean makes the -136 sum(x) correction of the 128 + q kernels the large term.

That the table can fail was checked once on an MI355X with temporary value-only mutations (no address, guard, loop bound or synchronisation touched; none committed),
one build each, every one caught:
  * the pair partner's sign in wide_finish_kernel's RoPE -> all 9 wide ROPE_KV cases (the three groups at N = 1024 and 6144, the three K-slice cases at N = 192);
  * rstd taken from group 0 for every group (wide_finish_kernel's partial sums and the DIRECT kernel's s_rstd) -> all 26 wide cases with a folded norm: ROPE_KV,
    SWIGLU_XF and the STORE cases at n-tiles per wave 1, 2 and 4;
  * the last K-slice plane left out of the finishing sum -> all 9 cases with more than one K slice (kz 8, 9, 24 and 24 x 3 steps; RESID_XF, ROPE_KV, SWIGLU_XF);
  * gate and up swapped in q4_skinny_kernel's SWIGLU_XF -> all 11 one-group SWIGLU_XF cases (the loop, the reloading path at ntw 2 and 4, the straight-line
    forms at ntw 1, 2 and 4);
  * kv_bf16_round replaced by truncation in q4_skinny_kernel -> all 5 bf16-pool cases (paged and ring; loop, reloading path, straight-line);
  * the non-`pre` xw missing its xf_w2 factor: not built -- that path cannot run.  launch_q4_skinny forces one n-tile per wave for EPI_RESID_XF (and its per-row
    form), so `t == wave` holds for every tile that is finished and the reloading branch of xw / xwr / the residual is dead code; no shape reaches it.
In every mutated run the closing coverage test failed as well (a failed row is not a passed one)."""
import zlib
from collections import namedtuple

import numpy as np
import pytest

import linear_ref as R
import xf_op_lib as X
from model_fixtures import gemm_launches, gemm_launches_since

pytestmark = pytest.mark.gpu

# ---- the launchers' thresholds (q4_skinny_plan, q4_wide_plan, launch_q4_gemm_epi)
SK_NTW2_TILES, SK_NTW4_TILES, SK_KS8_MAX_WG, SK_KS8_MIN_STEPS = 384, 768, 256, 16
SK_PARTS_PER_WAVE = 48                                     # 12 partial sums per thread, 64 / 16 threads per row and wave
STRAIGHT = {(2, "rope_kv", 1, 3), (2, "swiglu_xf", 1, 6), (1, "swiglu_xf", 1, 6), (4, "swiglu_xf", 1, 6), (1, "resid_xf", 0, 4), (1, "resid_xf", 0, 9), (4, "store", 1, 6)}
WIDE_NTW2_TILES, WIDE_NTW4_TILES, WIDE_MIN_WG, WIDE_KZ_MAX = 384, 4096, 320, 24
BIG_ROPE_MIN_WG = 1024                                     # 64 x 256 workgroups from which the big kernel ropes in its epilogue
EPS = 1e-5
EPI_NAME = {X.EPI_STORE: "store", X.EPI_ROPE_KV: "rope_kv", X.EPI_SWIGLU_XF: "swiglu_xf", X.EPI_RESID_XF: "resid_xf"}
KV_NAME = {"contig": "rope_kv", "slots": "rope_kv", "paged": "rope_kv_paged", "ring": "rope_kv_paged_ring"}
KV_FORM = {"contig": X.KV_CONTIG, "slots": X.KV_SLOTS, "paged": X.KV_PAGED, "ring": X.KV_PAGED_RING}


def skinny_plan(K, N, epi, pro):
    steps, tiles = K // 128, -(-N // 16)
    ntw = 4 if tiles >= SK_NTW4_TILES else 2 if tiles >= SK_NTW2_TILES else 1
    ks = 4 if steps >= 4 else 2 if steps >= 2 else 1
    if tiles // ntw < SK_KS8_MAX_WG and steps >= SK_KS8_MIN_STEPS:
        ks = 8
    if epi == "resid_xf":
        ntw = 1
    per = steps // ks if steps % ks == 0 else 0
    return ntw, ks, -(-steps // ks), int((ntw, epi, int(pro), per) in STRAIGHT)


def wide_plan(K, N, epi):
    steps, tiles = K // 128, N // 16
    ntw, kz = (2 if tiles >= WIDE_NTW2_TILES else 1), 1
    if epi == "store" and tiles >= WIDE_NTW4_TILES:
        ntw = 4
    if epi != "store":
        ranges = -(-tiles // (4 * ntw))
        for d in range(1, steps + 1):
            if steps % d == 0:
                kz = d
                if ranges * d >= WIDE_MIN_WG:
                    break
        if kz > WIDE_KZ_MAX:
            kz = max(d for d in range(1, WIDE_KZ_MAX + 1) if steps % d == 0)
    return ntw, kz, steps // kz, 0


Case = namedtuple("Case", "G M K N epi act n_part kv bf16 bias w2 gaps")
CASES = {}


def add(tag, G, M, K, N, epi, act="ramp", n_part=None, kv="contig", bf16=False, bias=False, w2=True, gaps=False):
    if n_part is None:
        n_part = 0 if epi == X.EPI_RESID_XF else 8
    cid = f"{tag}-g{G}-m{M}-{K}x{N}-{EPI_NAME[epi]}{'-' + kv + ('-bf16' if bf16 else '') if epi == X.EPI_ROPE_KV else ''}-p{n_part}-{act}{'-bias' if bias else ''}{'' if w2 else '-now2'}{'-gaps' if gaps else ''}"
    assert cid not in CASES, cid
    CASES[cid] = Case(G, M, K, N, epi, act, n_part, kv, bf16, bias, w2, gaps)


ST, RK, SW, RX = X.EPI_STORE, X.EPI_ROPE_KV, X.EPI_SWIGLU_XF, X.EPI_RESID_XF
QKV_SMALL = 4 * 128 + 2 * 2 * 128          # hd 128, 4 q heads over 2 kv heads: N = 1024
# 1. one group, the loop at one K step and one wave (K = 128), M in {1, 5, 16}
for M_ in (1, 5, 16):
    add("loop", 1, M_, 128, 256, ST, n_part=1)
    add("loop", 1, M_, 128, 256, ST, n_part=0, bias=True, act="scales")
    add("loop", 1, M_, 128, 256, SW)
    add("loop", 1, M_, 128, 128, RX, w2=(M_ != 5))
    add("loop", 1, M_, 128, QKV_SMALL, RK)
# 2. ks < ntw: tiles through the reloading epilogue path.  ntw 2: N = 6144 (K = 128: ks 1); ntw 4: N = 12288 (K = 256: ks 2; K = 128: ks 1)
for K_, N_ in ((128, 6144), (256, 12288), (128, 12288)):
    add("nonpre", 1, 5, K_, N_, ST, n_part=1, act="scales")
    add("nonpre", 1, 16, K_, N_, SW)
    add("nonpre", 1, 16, K_, N_, RK, kv="slots")
add("nonpre", 1, 5, 128, 6144, RK, kv="ring")
add("nonpre", 1, 16, 128, 6144, RK, kv="paged", bf16=True)
add("nonpre", 1, 5, 128, 6144, RX, w2=True)          # (RESID_XF runs one tile per wave at any N: the prefetched path, at 384 workgroups)
# 3. the straight-line instantiations (VOX_ST_FORMS): (2, ROPE_KV*, 1, 3) N = 6144, K = 3072 (ks 8); (1 | 2, SWIGLU_XF, 1, 6) K = 6144 (ks 8), N = 256 / 6144;
#    (4, SWIGLU_XF | STORE, 1, 6) N = 16384 (1024 tiles / 4 = 256 workgroups: ks 4), K = 3072; (1, RESID_XF, 0, 4 | 9) K = 4096 / 9216 (ks 8), N = 128
for kv_, bf_ in (("contig", False), ("slots", False), ("paged", False), ("ring", False), ("paged", True), ("ring", True)):
    add("st", 1, 16, 3072, 6144, RK, kv=kv_, bf16=bf_, n_part=192)
    add("loop", 1, 5 if kv_ in ("contig", "ring") else 16, 512, QKV_SMALL, RK, kv=kv_, bf16=bf_)
add("st", 1, 5, 3072, 6144, RK, kv="paged", act="scales")
add("st", 1, 1, 3072, 6144, RK, kv="slots")
for M_ in (1, 5, 16):
    add("st", 1, M_, 6144, 256, SW, n_part=192)
    add("st", 1, M_, 4096, 128, RX, w2=(M_ != 1))
    add("st", 1, M_, 9216, 128, RX, w2=(M_ == 1))
add("st", 1, 16, 6144, 6144, SW, n_part=192, act="scales")
add("st", 1, 5, 3072, 16384, SW, n_part=192)
add("st", 1, 16, 3072, 16384, ST, n_part=192)
# 4. the folded norm's partial sums: 1, 8, 192 = the limit of a 4-wave launch (K = 512); 193 and 384 = the limit of an 8-wave launch (K = 2048)
for n_ in (1, 8, 192):
    add("parts", 1, 16, 512, 256, ST, n_part=n_, act="scales")
for n_ in (193, 384):
    add("parts", 1, 16, 2048, 256, ST, n_part=n_, act="scales")
# 5. the wide step.  Plane forms at ntw 1 (N = 128 .. 1024) and 2 (N = 6144), K slices 1 / 8 / 9 / 24 / 24 x 3 steps; a partial last block of four n-tiles
#    in DIRECT (N / 16 = 13 at ntw 1, N = 6160: 385 tiles at ntw 2 -- the plane forms' N constraints admit whole blocks only); DIRECT at ntw 1 / 2 / 4;
#    finishing-kernel n_part 1 / 192 / 193; group strides with gaps
QKV_TINY = 64 + 2 * 64                      # hd 64, one q and one kv head: N = 192, 12 n-tiles
for G_ in (2, 3, 4):
    add("wide", G_, 16 * G_, 128, QKV_SMALL, RK, kv="slots", gaps=True)
    add("wide", G_, 16 * G_, 128, 128, RX, gaps=True, w2=(G_ != 3))
    add("wide", G_, 16 * G_, 128, 256, SW, gaps=True)
    add("wide", G_, 16 * G_, 128, 6144, RK, kv=("contig" if G_ == 3 else "slots"))
    add("wide", G_, 16 * G_, 128, 6144, RX, act="scales")
    add("wide", G_, 16 * G_, 128, 6144, SW)
    add("wide", G_, 16 * G_, 128, 208, ST, n_part=(1, 192, 193)[G_ - 2], gaps=True, act="scales")
    add("wide", G_, 16 * G_, 128, 6144, ST)
    add("wide", G_, 16 * G_, 128, 65536, ST, n_part=1)
for i_, K_ in enumerate((1024, 1152, 3072, 9216)):
    add("wide-kz", 2 + i_ % 3, 16 * (2 + i_ % 3), K_, 128, RX, gaps=(i_ % 2 == 0))
add("wide-kz", 4, 64, 1152, QKV_TINY, RK, n_part=193, kv="slots")
add("wide-kz", 2, 32, 1024, QKV_TINY, RK, n_part=192, kv="contig", act="scales")
add("wide-kz", 3, 48, 3072, QKV_TINY, RK, n_part=1, kv="slots", gaps=True)
add("wide-kz", 3, 48, 1152, 256, SW, n_part=193)
add("wide-kz", 2, 32, 3072, 256, SW, n_part=192, act="scales", gaps=True)
add("wide", 3, 48, 128, 6160, ST, act="scales")          # 385 n-tiles at two per wave: the last wave's second tile does not exist
# 6. activations with a non-zero mean: the -136 sum(x) correction (the skinny kernel's MFMA pair, q4_wide_kernel's s_cs per (group, block)) is the large term
add("offset", 1, 5, 128, 256, ST, n_part=1, act="offset3")
add("offset", 1, 16, 3072, 6144, RK, kv="slots", n_part=192, act="offset30")
add("offset", 1, 16, 128, 12288, SW, act="offset30")
add("offset", 1, 16, 4096, 128, RX, act="offset30")
add("offset", 3, 48, 1152, 128, RX, act="offset30")
add("offset", 2, 32, 128, 6144, SW, act="offset3")
add("offset", 4, 64, 128, 6144, ST, act="offset30")
add("offset", 2, 32, 3072, QKV_TINY, RK, kv="slots", act="offset30")

REQUIRED = ({("st", 2, e) for e in ("rope_kv", "rope_kv_paged", "rope_kv_paged_ring", "rope_kv_paged_bf16", "rope_kv_paged_ring_bf16", "swiglu_xf")}
            | {("st", 1, "swiglu_xf"), ("st", 4, "swiglu_xf"), ("st", 4, "store"), ("st", 1, "resid_xf", 4), ("st", 1, "resid_xf", 9)}
            | {("loop", 1, e, "pre") for e in ("store", "rope_kv", "rope_kv_paged", "rope_kv_paged_ring", "rope_kv_paged_bf16", "rope_kv_paged_ring_bf16", "swiglu_xf", "resid_xf")}
            | {("loop", n, e, "reload") for n in (2, 4) for e in ("store", "rope_kv", "swiglu_xf")}
            | {("loop", 2, "rope_kv_paged_ring", "reload"), ("loop", 2, "rope_kv_paged_bf16", "reload")}
            | {("wide", g, n, "planes") for g in (2, 3, 4) for n in (1, 2)} | {("wide", g, n, "direct") for g in (2, 3, 4) for n in (1, 2, 4)}
            | {("finish", e) for e in ("rope_kv", "swiglu_xf", "resid_xf")} | {("finish-kz", z) for z in (1, 8, 9, 24)} | {("finish-sps", 3)}
            | {("big_rope", p) for p in ("table", "seq_rows", "rows")}
            | {("wide_rows", m, e) for m in (17, 38, 48) for e in ("rope_kv", "swiglu_xf", "resid_xf")} | {("wide_rows-kz", z) for z in (4, 8, 9, 24)})
PASSED, ASSERTED, WORST = set(), set(), {}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    for _, t in _WEIGHTS.values():      # (a tensor is freed on its context: the tensors go first)
        t.close()
    _WEIGHTS.clear()
    c.close()


_WEIGHTS = {}


def weights(pkg, ctx, N, K, swiglu):
    """One weight per (N, K, kind) for the whole module.  synth_q4_blocks with the scales of every third row negated (the positive-only generator is blind to a
    dropped sign); SwiGLU: the gate rows negated, the up rows times three (a swapped pair cannot survive)."""
    key = (N, K, swiglu)
    if key not in _WEIGHTS:
        rng = np.random.default_rng([zlib.crc32(repr(key).encode()), 7])
        raw = pkg.synth.synth_q4_blocks(rng, N * K, 0.04).reshape(N, K // 32, 18)
        if swiglu:
            d = np.ascontiguousarray(raw[:, :, :2]).view(np.float16).reshape(N, K // 32).astype(np.float32)
            d[1::2] *= 3.0; d[0::2] *= -1.0
            raw[:, :, :2] = d.astype(np.float16).view(np.uint8).reshape(N, K // 32, 2)
        else:
            raw[1::3, :, 1] ^= 0x80
        raw = raw.reshape(-1)
        _WEIGHTS[key] = (R.LinearRef(raw, N, K, chunk_rows=2048 if N * K > (1 << 22) else 0), pkg.Q4Tensor.from_q4_bytes(raw, [N, K], ctx))
    return _WEIGHTS[key]


def rope_geometry(N):
    return (64, 64, 1) if N == QKV_TINY else (128, N - 2 * 8 * 128, 8) if N >= 6144 else (128, 4 * 128, 2)      # hd, n_q, n_kv


def make_inputs(c, rng):
    """Everything the operator reads, distinct per group, row and slot; the cache geometry of a ROPE_KV case."""
    rows, G, K, N = 16 * c.G, c.G, c.K, c.N
    x, zrow = R.activations(rng, c.act, rows, K)
    d = dict(x=x, zrow=zrow)
    if c.n_part:
        ss = (x.astype(np.float64) ** 2).sum(axis=1).reshape(G, 1, 16)
        d["ssq_part"] = np.ascontiguousarray((ss / c.n_part * (0.5 + rng.random((G, c.n_part, 16)))).astype(np.float32))
    if c.bias:
        d["bias"] = rng.standard_normal(N).astype(np.float32)
    if c.epi == RX:
        d["resid"] = rng.standard_normal((rows, N)).astype(np.float32)
        d["xf_w"] = (1.0 + 0.1 * rng.standard_normal(N)).astype(np.float32)
        d["xf_w2"] = (1.0 + 0.2 * rng.standard_normal(N)).astype(np.float32) if c.w2 else None
    if c.epi == RK:
        hd, n_q, n_kv = rope_geometry(N)
        Mr = c.M
        d.update(hd=hd, n_q=n_q, n_kv=n_kv)
        if c.kv == "ring":
            members, mask = 5, 15
            ring = np.empty((members, mask + 1, hd), np.float32)
            ang = rng.uniform(0, 2 * np.pi, (members, mask + 1, hd // 2))
            ring[:, :, :hd // 2] = np.cos(ang); ring[:, :, hd // 2:] = np.sin(ang)
            d.update(rope_cos=ring, rope_sin=None, rope_rows=members * (mask + 1), rope_mask=mask, rope_member=rng.integers(0, members, Mr).astype(np.int32),
                     pos=(1000 + 37 * np.arange(Mr) + rng.integers(1, 16, Mr) * 0 + 5).astype(np.int32))      # beyond the ring: pos & rope_mask wraps
            d["pos"] = np.array([p if p % 16 else p + 1 for p in d["pos"]], np.int32)
        else:
            rope_rows = 80
            ang = np.arange(rope_rows)[:, None] * (10000.0 ** (-2.0 * np.arange(hd // 2) / hd))[None, :]
            cand = np.array([p for p in range(1, rope_rows) if p % 16])
            d.update(rope_cos=np.cos(ang).astype(np.float32), rope_sin=np.sin(ang).astype(np.float32), rope_rows=rope_rows, rope_mask=0,
                     pos=rng.permutation(cand)[:Mr].astype(np.int32))
            assert len(set(d["pos"].tolist())) == Mr
        if c.kv in ("paged", "ring"):
            pages, page_rows = 8, 16
            perm = rng.permutation(pages)
            d.update(kv_slices=pages, kv_rows=page_rows, kv_row=perm[np.arange(Mr) % pages].astype(np.int32), kv_pos=((5 * np.arange(Mr) + 3) % page_rows).astype(np.int32))
            assert len({(a, b) for a, b in zip(d["kv_row"], d["kv_pos"])}) == Mr and (d["kv_row"] != np.arange(Mr) % pages).any()
        elif c.kv == "slots":
            d.update(kv_slices=rows + 3, kv_rows=80, kv_row=rng.permutation(rows + 3)[:Mr].astype(np.int32), kv_pos=None)
            assert (d["kv_row"] != np.arange(Mr)).any()
        else:
            d.update(kv_slices=rows, kv_rows=80, kv_row=None, kv_pos=None)
    return d


def run_op(pkg, ctx, t, c, d, bf16):
    """One hook call on sentinel-filled outputs.  Returns (outputs dict, plan, launches, the group strides)."""
    G, K, N, rows = c.G, c.K, c.N, 16 * c.G
    xo_cols = N // 2 if c.epi == SW else N if c.epi == RX else 0
    gs = dict(xf_in_gs=K * 32 + 64, xf_out_gs=xo_cols * 32 + 72, ssq_part_gs=c.n_part * 16 + 16 if c.n_part else 0, ssq_out_gs=N + 48) if c.gaps else \
        dict(xf_in_gs=0, xf_out_gs=0, ssq_part_gs=0, ssq_out_gs=0)
    desc = X.XfOpDesc(mode=X.MODE_STEP, groups=G, M=c.M, epi=c.epi, n_part=c.n_part, norm_eps=EPS, **gs)
    o = dict(out=None if c.epi == SW else X.sentinel32((rows, N)))
    if xo_cols:
        o["xf_out"] = np.full(G * (gs["xf_out_gs"] or xo_cols * 32), X.SENT16, np.uint16)
    if c.epi == RX:
        o["ssq_out"] = X.sentinel32(G * (gs["ssq_out_gs"] or N))
    a = dict(x=d["x"], ssq_part=d.get("ssq_part"), bias=d.get("bias"), resid=d.get("resid"), xf_w=d.get("xf_w"), xf_w2=d.get("xf_w2"))
    if c.epi == RK:
        for k in ("hd", "n_q", "n_kv", "kv_slices", "kv_rows", "rope_rows", "rope_mask"):
            setattr(desc, k, d[k])
        desc.kv_form = KV_FORM[c.kv]; desc.kv_bf16 = int(bf16)
        shape = (d["kv_slices"], d["n_kv"], d["kv_rows"], d["hd"])
        o["kc"], o["vc"] = (np.full(shape, X.SENT16, np.uint16), np.full(shape, X.SENT16, np.uint16)) if bf16 else (X.sentinel32(shape), X.sentinel32(shape))
        a.update(rope_cos=d["rope_cos"], rope_sin=d["rope_sin"], pos=d["pos"], kv_row=d["kv_row"], kv_pos=d["kv_pos"], rope_member=d.get("rope_member"))
    before = gemm_launches(pkg)
    code = X.call(pkg, ctx.h, t.h, desc, **a, **o)
    assert code == 0, (pkg.lib().vox_last_error() or b"").decode()
    return o, (desc.plan_ntw, desc.plan_ks, desc.plan_steps, desc.plan_straight), gemm_launches_since(pkg, before), gs


def note(form, err, bound):
    w = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    WORST[form] = max(WORST.get(form, 0.0), w)
    return w


def held(what, got, ref, bound, form):
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), f"{what}: not finite"
    err = np.abs(got - ref)
    w = note(form, err, bound)
    print(f"{form} {what}: worst |err| / bound {w:.3f}")
    bad = err > bound
    assert not bad.any(), f"{what}: {int(bad.sum())} elements past the bound, worst {w:.2f} x at {np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)}"


def planes_rows(c, planes, cols, gs, form, ref, bound, what):
    """The XF output planes of every group: rows < M against ref / bound [rows][cols] (hi + lo), rows >= M and the gaps between the groups' planes untouched."""
    stride = gs or cols * 32
    planes = planes.reshape(c.G, stride)
    assert (planes[:, cols * 32:] == X.SENT16).all(), f"{what}: the gap behind a group's planes was written"
    for g in range(c.G):
        val, hi, lo = R.xf_unpack(planes[g, :cols * 32], cols)
        m = c.M if c.G == 1 else 16
        assert (hi[m:] == X.SENT16).all() and (lo[m:] == X.SENT16).all(), f"{what}: rows >= M written"
        held(f"{what} group {g}", val[:m], ref[16 * g:16 * g + m], R.xf_bound(ref[16 * g:16 * g + m], bound[16 * g:16 * g + m]), form)


def run_case(pkg, ctx, c):
    G, M, K, N = c.G, c.M, c.K, c.N
    rows, ename = 16 * G, EPI_NAME[c.epi]
    lin, t = weights(pkg, ctx, N, K, c.epi == SW)
    rng = np.random.default_rng([zlib.crc32(repr(tuple(c)).encode()), 3])
    d = make_inputs(c, rng)
    o, plan, ran, gs = run_op(pkg, ctx, t, c, d, False)
    # ---- which form ran
    if G == 1:
        want = skinny_plan(K, N, ename, c.n_part > 0)
        assert ran == {"xf_rows": 1, "skinny": 1}, ran
        assert c.n_part <= SK_PARTS_PER_WAVE * want[1]
        kname = KV_NAME[c.kv] if c.epi == RK else ename
        form = f"skinny-{'st' if want[3] else 'loop'}-ntw{want[0]}-{ename}"
        keys = [("st", want[0], kname) + ((want[2],) if c.epi == RX else ())] if want[3] else [("loop", want[0], kname, "pre")] + ([("loop", want[0], kname, "reload")] if want[1] < want[0] else [])
    else:
        want = wide_plan(K, N, ename)
        assert ran == {"xf_rows": G, "wide": 1}, ran
        form = f"wide-ntw{want[0]}-{ename}"
        keys = [("wide", G, want[0], "direct" if c.epi == ST else "planes")] + ([] if c.epi == ST else [("finish", ename), ("finish-kz", want[1]), ("finish-sps", want[2])])
    assert plan == want, f"plan (ntw, ks | kz, steps, straight) {plan}, the thresholds give {want}"
    # ---- the reference
    Mg = M if G == 1 else 16                                      # rows served per group
    live = np.concatenate([np.arange(16 * g, 16 * g + Mg) for g in range(G)])
    _, pre, _, mag = lin(d["x"])
    bound = 2.0 ** -16 * mag
    if c.n_part:
        rstd = np.concatenate([R.rstd64(d["ssq_part"][g], K, EPS) for g in range(G)])
        pre = pre * rstd[:, None]
        bound = R.norm_bound(pre, bound, rstd, c.n_part)
    if c.bias:
        pre = pre + d["bias"].astype(np.float64)[None, :]
        bound = bound + 0.5 * R.ULP32 * np.abs(pre)
    dead = np.setdiff1d(np.arange(rows), live)
    if c.epi == ST:
        held("out", o["out"][live], pre[live], bound[live], form)
        assert X.is_sentinel32(o["out"][dead]).all(), "rows >= M written"
        if d["zrow"] is not None and d["zrow"] in live and not c.bias:
            assert (o["out"][d["zrow"]] == 0.0).all(), "an all-zero row must give exactly zero"
    elif c.epi == SW:
        ref = R.apply_epilogue(pre, R.EPI_SWIGLU); b = R.carry_bound(pre, bound, R.EPI_SWIGLU)
        planes_rows(c, o["xf_out"], N // 2, gs["xf_out_gs"], form, ref, b, "SwiGLU planes")
    elif c.epi == RX:
        ref = pre + d["resid"].astype(np.float64); b = bound + 0.5 * R.ULP32 * np.abs(ref)
        held("out", o["out"][live], ref[live], b[live], form)
        assert X.is_sentinel32(o["out"][dead]).all(), "rows >= M written"
        xw = d["xf_w"].astype(np.float64) * (d["xf_w2"].astype(np.float64) if d["xf_w2"] is not None else 1.0)
        planes_rows(c, o["xf_out"], N, gs["xf_out_gs"], form, ref * xw[None, :], b * np.abs(xw)[None, :] + R.ULP32 * np.abs(ref * xw[None, :]), "RESID planes")
        so = o["ssq_out"].reshape(G, gs["ssq_out_gs"] or N)
        assert X.is_sentinel32(so[:, N:]).all(), "the gap behind a group's sums of squares was written"
        for g in range(G):
            got = so[g, :N].reshape(N // 16, 16).astype(np.float64)
            own = (o["out"][16 * g:16 * g + Mg].astype(np.float64) ** 2).reshape(Mg, N // 16, 16).sum(axis=2).T
            held(f"ssq_out group {g}", got[:, :Mg], own, 2.0 ** -20 * own, form + "-ssq")
            assert (got[:, Mg:] == 0.0).all(), "sums of squares of rows >= M must be zero"
    else:
        hd, n_q, n_kv = d["hd"], d["n_q"], d["n_kv"]
        kd, P = n_kv * hd, hd // 2
        cs = np.zeros((rows, (n_q + kd) // 2)); sn = np.zeros_like(cs)
        pair = np.arange((n_q + kd) // 2) % P
        for i, r in enumerate(live):
            if c.kv == "ring":
                row = d["rope_cos"][d["rope_member"][i], d["pos"][i] & d["rope_mask"]]
                cs[r], sn[r] = row[:P][pair], row[P:][pair]
            else:
                cs[r], sn[r] = d["rope_cos"][d["pos"][i]][pair], d["rope_sin"][d["pos"][i]][pair]
        roped = R.rope64(pre[:, :n_q + kd], cs, sn); rb = R.carry_bound(pre[:, :n_q + kd], bound[:, :n_q + kd], R.EPI_ROPE, cos=cs, sin=sn)
        held("q rows", o["out"][live][:, :n_q], roped[live][:, :n_q], rb[live][:, :n_q], form)
        assert X.is_sentinel32(o["out"][dead]).all() and X.is_sentinel32(o["out"][:, n_q:]).all(), "q|k|v rows: something outside rows < M, columns < n_q was written"
        kref = np.zeros(o["kc"].shape); vref = np.zeros_like(kref); kb = np.zeros_like(kref); vb = np.zeros_like(kref); mask = np.zeros(o["kc"].shape, bool)
        for i, r in enumerate(live):
            sl = r if c.kv == "contig" else d["kv_row"][i]
            cr = d["kv_pos"][i] if c.kv in ("paged", "ring") else d["pos"][i]
            assert not mask[sl, :, cr].any()
            mask[sl, :, cr] = True
            kref[sl, :, cr] = roped[r, n_q:].reshape(n_kv, hd); kb[sl, :, cr] = rb[r, n_q:].reshape(n_kv, hd)
            vref[sl, :, cr] = pre[r, n_q + kd:].reshape(n_kv, hd); vb[sl, :, cr] = bound[r, n_q + kd:].reshape(n_kv, hd)
        for name, got, ref, b in (("K cache", o["kc"], kref, kb), ("V cache", o["vc"], vref, vb)):
            assert X.is_sentinel32(got[~mask]).all(), f"{name}: a cell outside the written (slice, head, row) was written"
            held(name, got[mask], ref[mask], b[mask], form)
        if c.bf16:
            o2, plan2, ran2, _ = run_op(pkg, ctx, t, c, d, True)
            assert ran2 == ran and plan2[:3] == plan[:3]
            kname = kname + "_bf16"
            keys = keys + [k[:2] + (kname,) + k[3:] for k in keys]
            assert np.array_equal(o2["out"].view(np.uint32), o["out"].view(np.uint32)), "the q rows of a bf16 pool's launch differ from the f32 pool's"
            for name, got, f32 in (("K pool", o2["kc"], o["kc"]), ("V pool", o2["vc"], o["vc"])):
                assert (got[~mask] == X.SENT16).all(), f"bf16 {name}: a cell outside the written ones was written"
                assert np.array_equal(got[mask], pkg.gguf.kv_round_bf16(np.ascontiguousarray(f32[mask]))), f"bf16 {name}: not vox_kv_round_bf16 of the f32 pool's values"
            if G == 1:      # the plan of the bf16 launch is its own instantiation's
                assert plan2[3] == skinny_plan(K, N, ename, True)[3]
    ASSERTED.update(keys)


@pytest.mark.parametrize("cid", list(CASES))
def test_xf_op_case(pkg, orc, ctx, cid):
    """One row of the table: the expected form and plan ran, every element of every output meets its bound or keeps the sentinel."""
    run_case(pkg, ctx, CASES[cid])
    PASSED.add(cid)


def test_limits_are_refused_before_the_device(pkg, orc, ctx):
    """193 partial sums on a 4-wave launch (limit 192), a position outside the table, a slot outside the cache: VOX_ERR_INVALID, no launch, outputs untouched."""
    lin, t = weights(pkg, ctx, 256, 512, False)
    x = np.ones((16, 512), np.float32); out = X.sentinel32((16, 256)); part = np.ones((193, 16), np.float32)
    before = gemm_launches(pkg)
    assert X.call(pkg, ctx.h, t.h, X.XfOpDesc(groups=1, M=16, epi=ST, n_part=193, norm_eps=EPS), x=x, ssq_part=part, out=out) == 1
    assert "n_part 193" in pkg.lib().vox_last_error().decode()
    lin, t = weights(pkg, ctx, QKV_SMALL, 128, False)
    x = np.ones((16, 128), np.float32); out = X.sentinel32((16, QKV_SMALL)); kc = X.sentinel32((16, 2, 8, 128)); vc = X.sentinel32((16, 2, 8, 128))
    tab = np.ones((8, 64), np.float32); part = np.ones((1, 16), np.float32)
    for pos, kv_row, form in (([0, 8], None, X.KV_CONTIG), ([0, -1], None, X.KV_CONTIG), ([0, 1], [0, 16], X.KV_SLOTS), ([0, 1], [0, -1], X.KV_SLOTS)):
        dsc = X.XfOpDesc(groups=1, M=2, epi=RK, n_part=1, norm_eps=EPS, hd=128, n_q=512, n_kv=2, kv_form=form, kv_slices=16, kv_rows=8, rope_rows=8)
        code = X.call(pkg, ctx.h, t.h, dsc, x=x, ssq_part=part, out=out, kc=kc, vc=vc, rope_cos=tab, rope_sin=tab, pos=np.array(pos, np.int32),
                      kv_row=None if kv_row is None else np.array(kv_row, np.int32))
        assert code == 1, (pos, kv_row)
    assert gemm_launches_since(pkg, before) == {} and X.is_sentinel32(out).all() and X.is_sentinel32(kc).all() and X.is_sentinel32(vc).all()


# ---- the prefill's row-major form of the wide GEMM: (M, epilogue, K, N, pos_off, bias); the weights are the table's
WIDE_ROWS = [(17, RK, 1152, QKV_TINY, 0, False), (38, RK, 512, QKV_SMALL, 7, False), (48, RK, 1152, QKV_TINY, 21, False),
             (17, SW, 3072, 256, 0, False), (38, SW, 1152, 256, 0, True), (48, SW, 1152, 256, 0, False),
             (17, RX, 9216, 128, 0, False), (38, RX, 1152, 128, 0, False), (48, RX, 1024, 128, 0, False)]


@pytest.mark.parametrize("M,epi,K,N,pos_off,bias", WIDE_ROWS, ids=[f"m{c[0]}-{EPI_NAME[c[1]]}-{c[2]}x{c[3]}-off{c[4]}{'-bias' if c[5] else ''}" for c in WIDE_ROWS])
def test_wide_rows_case(pkg, orc, ctx, M, epi, K, N, pos_off, bias):
    """launch_q4_skinny_mt2_planes on q4_wide_kernel's row-major planes + the finishing kernel, against float64; rows >= M of the 16-row blocks keep the sentinel."""
    ename, mt = EPI_NAME[epi], -(-M // 16)
    lin, t = weights(pkg, ctx, N, K, epi == SW)
    rng = np.random.default_rng([M, epi, K, N, 4])
    x, _ = R.activations(rng, "scales" if M == 38 else "offset3" if M == 48 else "ramp", M, K)
    b = rng.standard_normal(N).astype(np.float32) if bias else None
    _, pre, _, mag = lin(x)
    bound = 2.0 ** -16 * mag
    if bias:
        pre = pre + b.astype(np.float64)[None, :]; bound = bound + 0.5 * R.ULP32 * np.abs(pre)
    desc = X.XfOpDesc(mode=X.MODE_WIDE_ROWS, M=M, epi=epi, pos_off=pos_off)
    form = f"wide_rows-{ename}"
    a = dict(x=x, bias=b)
    if epi == RK:
        hd, n_q, n_kv = rope_geometry(N)
        rows_c = 80
        ang = np.arange(rows_c)[:, None] * (10000.0 ** (-2.0 * np.arange(hd // 2) / hd))[None, :]
        cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
        for k, v in dict(hd=hd, n_q=n_q, n_kv=n_kv, kv_form=X.KV_CONTIG, kv_slices=1, kv_rows=rows_c, rope_rows=rows_c).items():
            setattr(desc, k, v)
        a.update(out=X.sentinel32((16 * mt, N)), kc=X.sentinel32((n_kv, rows_c, hd)), vc=X.sentinel32((n_kv, rows_c, hd)), rope_cos=cos, rope_sin=sin)
    elif epi == SW:
        a.update(xf_out=np.full(mt * (N // 2) * 32, X.SENT16, np.uint16))
    else:
        resid = rng.standard_normal((M, N)).astype(np.float32)
        a.update(out=X.sentinel32((16 * mt, N))); a["out"][:M] = resid
    before = gemm_launches(pkg)
    code = X.call(pkg, ctx.h, t.h, desc, **a)
    assert code == 0, (pkg.lib().vox_last_error() or b"").decode()
    ran = gemm_launches_since(pkg, before)
    assert ran == dict({"xf_rows": 1, "wide": 1}, **({"splitk_finish": 1} if epi == RX else {})), ran
    want = wide_plan(K, N, "rope_kv")          # (the prefill plans every operator as a plane form)
    assert (desc.plan_ntw, desc.plan_ks, desc.plan_steps) == want[:3], ((desc.plan_ntw, desc.plan_ks, desc.plan_steps), want)
    if epi == RK:
        kd, P = n_kv * hd, hd // 2
        pair = np.arange((n_q + kd) // 2) % P
        cs, sn = cos[pos_off:pos_off + M][:, pair].astype(np.float64), sin[pos_off:pos_off + M][:, pair].astype(np.float64)
        roped = R.rope64(pre[:, :n_q + kd], cs, sn); rb = R.carry_bound(pre[:, :n_q + kd], bound[:, :n_q + kd], R.EPI_ROPE, cos=cs, sin=sn)
        held("q rows", a["out"][:M, :n_q], roped[:, :n_q], rb[:, :n_q], form)
        assert X.is_sentinel32(a["out"][M:]).all() and X.is_sentinel32(a["out"][:, n_q:]).all(), "q rows: something outside rows < M, columns < n_q was written"
        for name, got, ref, bb in (("K cache", a["kc"], roped[:, n_q:], rb[:, n_q:]), ("V cache", a["vc"], pre[:, n_q + kd:], bound[:, n_q + kd:])):
            held(name, got[:, pos_off:pos_off + M], ref.reshape(M, n_kv, hd).transpose(1, 0, 2), bb.reshape(M, n_kv, hd).transpose(1, 0, 2), form)
            assert X.is_sentinel32(got[:, :pos_off]).all() and X.is_sentinel32(got[:, pos_off + M:]).all(), f"{name}: a row outside pos_off .. pos_off + M - 1 was written"
    elif epi == SW:
        ref = R.apply_epilogue(pre, R.EPI_SWIGLU); bb = R.carry_bound(pre, bound, R.EPI_SWIGLU)
        tiles = a["xf_out"].reshape(mt, (N // 2) * 32)
        for g in range(mt):
            val, hi, lo = R.xf_unpack(tiles[g], N // 2)
            m = min(16, M - 16 * g)
            assert (hi[m:] == X.SENT16).all() and (lo[m:] == X.SENT16).all(), "SwiGLU tiles: rows >= M written"
            held(f"SwiGLU tile {g}", val[:m], ref[16 * g:16 * g + m], R.xf_bound(ref[16 * g:16 * g + m], bb[16 * g:16 * g + m]), form)
    else:
        ref = pre + resid.astype(np.float64)
        held("x + sum of the planes", a["out"][:M], ref, bound + 0.5 * R.ULP32 * np.abs(ref), form)
        assert X.is_sentinel32(a["out"][M:]).all(), "rows >= M written"
    ASSERTED.update({("wide_rows", M, ename), ("wide_rows-kz", want[1])})


# ---- the encoder's fused RoPE rows: q4_gemm_big_kernel<EPI_ROPE_ROWS> runs from 1024 workgroups of 64 x 256 (M = 4096 at N = 4096); K = 128 keeps it small
ROWS_K, ROWS_N, ROWS_HD, ROWS_NQ, ROWS_TAB = 128, 4096, 64, 2560, 4096
ROWS_M = 64 * (BIG_ROPE_MIN_WG // (ROWS_N // 256))
assert (ROWS_N // 256) * (ROWS_M // 64) == BIG_ROPE_MIN_WG and 0 < ROWS_NQ < ROWS_N


@pytest.fixture(scope="module")
def rows_op(pkg, orc, ctx):
    """The weight, 4096 rows, the table and the un-roped float64 product with its bound: made once, read-only."""
    rng = np.random.default_rng(77)
    lin, t = weights(pkg, ctx, ROWS_N, ROWS_K, False)
    x, _ = R.activations(rng, "ramp", ROWS_M, ROWS_K)
    ang = np.arange(ROWS_TAB)[:, None] * (10000.0 ** (-2.0 * np.arange(ROWS_HD // 2) / ROWS_HD))[None, :]
    cos, sin = np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)
    _, pre, _, mag = lin(x)
    for a in (x, cos, sin, pre, mag):
        a.setflags(write=False)
    return t, x, cos, sin, pre, 2.0 ** -16 * mag


@pytest.mark.parametrize("form", ["table", "seq_rows", "rows"])
@pytest.mark.parametrize("path", ["fused", "unfused", "below"])
def test_rope_rows(pkg, ctx, rows_op, monkeypatch, form, path):
    """EPI_ROPE_ROWS against float64 under a position table, stacked sequences of 750 rows (750 does not divide M) and plain row positions: fused in the big kernel's
    epilogue; big + rope_kernel behind VOX_NO_ROPE_FUSE=1; and one row block below the threshold, where the call reports fused_rope == 0 and is still right."""
    t, x, cos, sin, pre, bound = rows_op
    M = ROWS_M - 64 if path == "below" else ROWS_M
    if path == "unfused":
        monkeypatch.setenv("VOX_NO_ROPE_FUSE", "1")      # (pkg.lib() re-reads the knobs whenever the VOX_* environment changed)
    rng = np.random.default_rng(5)
    pos = rng.integers(0, ROWS_TAB, M).astype(np.int32) if form == "table" else None
    seq = 750 if form == "seq_rows" else 0
    where = pos if pos is not None else np.arange(M) % seq if seq else np.arange(M)
    out = X.sentinel32((M, ROWS_N))
    dsc = X.XfOpDesc(mode=X.MODE_ROWS, M=M, hd=ROWS_HD, n_q=ROWS_NQ, rope_rows=ROWS_TAB, rope_seq_rows=seq)
    before = gemm_launches(pkg)
    code = X.call(pkg, ctx.h, t.h, dsc, x=np.ascontiguousarray(x[:M]), out=out, rope_cos=cos, rope_sin=sin, pos=pos)
    assert code == 0, (pkg.lib().vox_last_error() or b"").decode()
    ran = gemm_launches_since(pkg, before)
    assert ran == ({"big_rope": 1} if path == "fused" else {"big": 1}), ran
    assert dsc.fused_rope == int(path == "fused")
    pair = np.arange(ROWS_NQ // 2) % (ROWS_HD // 2)
    cs, sn = cos[where][:, pair].astype(np.float64), sin[where][:, pair].astype(np.float64)
    ref = np.concatenate([R.rope64(pre[:M, :ROWS_NQ], cs, sn), pre[:M, ROWS_NQ:]], axis=1)
    b = np.concatenate([R.carry_bound(pre[:M, :ROWS_NQ], bound[:M, :ROWS_NQ], R.EPI_ROPE, cos=cs, sin=sn), bound[:M, ROWS_NQ:]], axis=1)
    held(f"rope rows {form} {path}", out, ref, b, "big_rope" if path == "fused" else "big+rope_kernel")
    if path == "fused":
        ASSERTED.add(("big_rope", form))


def test_every_required_instantiation_was_asserted():
    """Every row of the table passed and every instantiation of REQUIRED was the asserted form of a passing case.  Prints the worst error / bound of every form."""
    for form in sorted(WORST):
        print(f"worst |err| / bound, {form:32s}: {WORST[form]:.3f}")
    assert set(CASES) == PASSED, f"{len(set(CASES) - PASSED)} rows of the table did not pass: {sorted(set(CASES) - PASSED)[:8]}"
    missing = REQUIRED - ASSERTED
    assert not missing, f"no passing case asserted {sorted(missing, key=repr)}"
