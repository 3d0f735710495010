"""Shared helpers for model-level tests: deterministic synthetic GGUFs (cached in the temp dir)."""
import os
import re
import tempfile

import numpy as np

from __graft_entry__ import load_package

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_python_golden.npz")


def cache_dir():
    d = os.path.join(tempfile.gettempdir(), "vox_test_models")
    os.makedirs(d, exist_ok=True)
    return d


def synth_gguf(dims, seed, tag):
    S = load_package().synth
    p = os.path.join(cache_dir(), f"{tag}_{seed}.gguf")
    if not os.path.exists(p):
        tmp = p + f".tmp{os.getpid()}"
        S.write_synthetic_gguf(tmp, dims, seed=seed)
        os.replace(tmp, p)
    return p


def golden():
    return np.load(GOLDEN)


def golden_gguf():
    S = load_package().synth; g = golden()
    dims = S.ModelDims(**{str(k): int(v) for k, v in zip(g["dims_keys"], g["dims"])})
    return synth_gguf(dims, int(g["seed"]), "golden"), dims


def tiny_gguf(seed=7, **kw):
    S = load_package().synth
    tag = "tiny" + "".join(f"_{k}{v}" for k, v in sorted(kw.items()))
    return synth_gguf(S.tiny_dims(**kw), seed, tag), S.tiny_dims(**kw)


def fake_mel(T, seed=0, n_mels=128):
    rng = np.random.default_rng(seed)
    return (0.6 * rng.standard_normal((n_mels, T)) + 0.3).astype(np.float32)


def rel_err(a, b):
    a = np.asarray(a, dtype=np.float64); b = np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(1e-30, np.abs(b).max()))


def tiny_f32_pair(seed=9):
    """(safetensors path for the HIP f32 path, all-F32 GGUF with the same values for the oracle)."""
    S = load_package().synth; d = S.tiny_dims()
    st = os.path.join(cache_dir(), f"tiny_f32_{seed}.safetensors"); gg = os.path.join(cache_dir(), f"tiny_f32_{seed}.gguf")
    if not os.path.exists(st):
        S.write_synthetic_safetensors(st + ".tmp", d, seed); os.replace(st + ".tmp", st)
    if not os.path.exists(gg):
        S.write_synthetic_dense_gguf(gg + ".tmp", d, seed); os.replace(gg + ".tmp", gg)
    return st, gg, d


def check_greedy_ids(ids, rids, rlg, tol):
    """Greedy ids must equal the oracle's; the only admissible first disagreement is at a step whose oracle top-2
    logit margin is below 10x the logit tolerance (a near-tie; after it the autoregressive sequences may diverge)."""
    ids = np.asarray(ids); rids = np.asarray(rids)
    assert ids.shape == rids.shape
    agree = ids == rids
    if agree.all():
        return len(ids)
    first = int(np.argmin(agree))
    srt = np.sort(rlg[first]); margin = srt[-1] - srt[-2]
    assert margin <= 10 * tol * max(1.0, float(np.abs(rlg).max())), f"ids differ at step {first} with a clear margin {margin}"
    return first


def single_stream_reference(pkg, ctx, model, x, t_embed):
    """(ids, logits) of the single-stream EAGER path (logits tap) for 16 kHz samples x: the per-sequence reference the batched paths are
    held to -- same device log-mel kernel as the batch path, then vox_transcribe_streaming with return_logits."""
    mel = pkg.MelSpectrogram.voxtral(ctx).compute_log(pkg.pad_audio(pkg.peak_normalize(x)))
    return model.transcribe_streaming(np.ascontiguousarray(mel.T)[None], t_embed, return_logits=True)


def check_batch_rows(pkg, ctx, model, clips, t_embed, outs, tol):
    """Every sequence of a batched transcription must equal the single-stream ids up to the first near-tie of ITS OWN single-stream logits
    (top-2 margin < 10 x tol x max|logit|); returns how many sequences are identical end to end."""
    assert len(outs) == len(clips)
    identical = 0
    for x, ids in zip(clips, outs):
        rids, rlg = single_stream_reference(pkg, ctx, model, x, t_embed)
        first = check_greedy_ids(ids, rids, rlg, tol)
        identical += int(first == len(rids))
    return identical


def gguf_conv_weights(pkg, path, enc_dim, n_mels):
    """The conv stem's f32 tensors of a GGUF: (w1 [enc_dim][n_mels][3], b1, w2 [enc_dim][enc_dim][3], b2)."""
    r = pkg.GgufReader.open(path); pfx = "mm_streams_embeddings.embedding_module.whisper_encoder.conv_layers."
    try:
        t = {k: r.tensor_data(pfx + k).view(np.float32) for k in ("0.conv.weight", "0.conv.bias", "1.conv.weight", "1.conv.bias")}
    finally:
        r.close()
    assert t["0.conv.weight"].size == enc_dim * n_mels * 3 and t["1.conv.weight"].size == enc_dim * enc_dim * 3 and t["0.conv.bias"].size == t["1.conv.bias"].size == enc_dim
    return t["0.conv.weight"].reshape(enc_dim, n_mels, 3), t["0.conv.bias"], t["1.conv.weight"].reshape(enc_dim, enc_dim, 3), t["1.conv.bias"]


PREFIX = [1] + [32] * 37      # BOS + 37 x STREAMING_PAD: the decoder's 38-token prefix (gguf/model.rs:887-902)


def _dec_positions(T, R=4):
    """Decoder positions of a T-frame log-mel: two stride-2 convolutions, then R frames per position (conv.rs:47-48, adapter.rs:114)."""
    cl = lambda L: (L - 1) // 2 + 1
    return cl(cl(T)) // R


def teacher_forced_logits(pkg, ctx, model, x, t_embed, ids, oracle=None):
    """The logits rows that predicted `ids` ([len(ids)][vocab], row k -> ids[k]) with the sequence's OWN ids fed back as the token inputs: PREFIX + ids[:-1] (the last
    position's input is never read by a kept row, causal).  Default: vox_forward_streaming on the device log-mel the batch path computes (single_stream_reference's mel):
    the prefill / large-M GEMM path, no decode kernel in common with the batched step forms.  oracle = an oracle_lib.Model: the CPU oracle on its own mel -- encode_audio,
    embed_tokens, one causal forward_hidden_with_cache over every position, lm_head (f32, sequential sums)."""
    ids = np.asarray(ids, dtype=np.int32); n = len(ids)
    assert n >= 1
    if oracle is None:
        mel = np.ascontiguousarray(pkg.MelSpectrogram.voxtral(ctx).compute_log(pkg.pad_audio(pkg.peak_normalize(x))).T)
    else:
        import oracle_lib
        xn = np.array(x, dtype=np.float32, copy=True); oracle_lib.lib().orc_peak_normalize(xn, xn.size, 0.95)
        mel = np.ascontiguousarray(oracle_lib.mel_compute_log(oracle_lib.pad_audio(xn)).T)
    S = _dec_positions(mel.shape[1], model.config.reshape_factor)
    assert S >= 38 and n == max(S - 38, 1), (S, n)
    toks = np.array((PREFIX + list(ids[:-1]) + [32] * S)[:S], dtype=np.int32)
    if oracle is None:
        lg = model.forward_streaming(mel[None], toks, t_embed)[0]
    else:
        audio = oracle.encode_audio(mel)
        assert audio.shape[0] == S
        oc = oracle.cache(max(S, 8))
        try:
            h = oracle.forward_hidden_with_cache(audio + oracle.embed_tokens(toks), t_embed, oc)
        finally:
            oracle.cache_free(oc)
        lg = oracle.lm_head(h[37:37 + n])
        return np.asarray(lg, dtype=np.float32)
    return lg[37:37 + n]


def argmax_low(rows):
    """Row-wise argmax with the lowest index winning ties (np.argmax does that)."""
    return np.argmax(np.asarray(rows), axis=1)


def top2_margin(row):
    s = np.sort(np.asarray(row, dtype=np.float64)); return float(s[-1] - s[-2])


def parse_batch_verbose(err):
    """The VOX_BATCH_VERBOSE lines of one batch call: lock-step parts [(rows, groups, steps, form)], continuous sessions [slots], decode steps per continuous step form
    (summed over sessions) and the slot plan of the last continuous session (caller units per slot, in queue order)."""
    out = {"lockstep": [], "slots": [], "forms": {"chains": 0, "engine1": 0, "engine2": 0, "wide": 0, "split": 0}, "plan": None}
    for r, g, st, f in re.findall(r"lock-step batch: (\d+) rows, (\d+) groups, (\d+) steps, step form (\S+)", err):
        out["lockstep"].append((int(r), int(g), int(st), f))
    out["slots"] = [int(x) for x in re.findall(r"continuous batch: \d+ utterances, (\d+) slots", err)]
    for line in re.findall(r"continuous batch step forms: ([^\n]*)", err):
        for k, v in re.findall(r"(\w+) (\d+)", line):
            out["forms"][k] += int(v)
    plans = re.findall(r"slot plan \(caller units per slot\):([^\n]*)", err)
    if plans:
        out["plan"] = [[int(u) for u in q.split()] for q in plans[-1].split("|")]
    return out


def dense_head_sha(path, nbytes=64 << 20):
    """sha256 of the first 64 MB of a (8.9 GB) synthetic dense checkpoint: cheap identity check of the deterministic generator's output."""
    import hashlib
    with open(path, "rb") as f:
        return hashlib.sha256(f.read(nbytes)).digest()


def full_dense_safetensors(seed=7, heavy_tail=False):
    """The full-size synthetic BF16 SafeTensors checkpoint of the f32 path (8.9 GB, written in a few seconds, cached in the temp dir);
    heavy_tail: the stress statistics of synth.dense_checkpoint_tensors."""
    S = load_package().synth
    st = os.path.join(cache_dir(), f"full_dense{'_heavytail' if heavy_tail else ''}_seed{seed}.safetensors")
    if not os.path.exists(st):
        S.write_fast_dense_checkpoint(st + ".tmp", None, S.ModelDims(), seed=seed, heavy_tail=heavy_tail); os.replace(st + ".tmp", st)
    return st


# ---- synthetic checkpoint tensors for the reference's per-component forward script (tests/golden/make_component_golden.py): real shapes, regenerable by name
COMPONENT_SEED = 20260925
_ENC = "mm_streams_embeddings.embedding_module.whisper_encoder."
COMPONENT_SHAPES = {
    _ENC + "transformer.layers.0.feed_forward.w1.weight": (5120, 1280), _ENC + "transformer.layers.0.feed_forward.w2.weight": (1280, 5120),
    _ENC + "transformer.layers.0.feed_forward.w3.weight": (5120, 1280),
    _ENC + "conv_layers.0.conv.weight": (1280, 128, 3), _ENC + "conv_layers.0.conv.bias": (1280,),
    _ENC + "conv_layers.1.conv.weight": (1280, 1280, 3), _ENC + "conv_layers.1.conv.bias": (1280,),
    _ENC + "transformer.layers.0.attention.wq.weight": (2048, 1280), _ENC + "transformer.layers.0.attention.wk.weight": (2048, 1280),
    _ENC + "transformer.layers.0.attention.wv.weight": (2048, 1280), _ENC + "transformer.layers.0.attention.wo.weight": (1280, 2048),
    _ENC + "transformer.layers.0.attention.wq.bias": (2048,), _ENC + "transformer.layers.0.attention.wv.bias": (2048,), _ENC + "transformer.layers.0.attention.wo.bias": (1280,),
    "layers.0.ada_rms_norm_t_cond.0.weight": (32, 3072), "layers.0.ada_rms_norm_t_cond.2.weight": (3072, 32),
}


def component_weight(name):
    """The synthetic tensor `name` of COMPONENT_SHAPES: N(0, sigma^2) f32, sigma = 0.03 (weights) / 0.02 (biases); numpy default_rng keyed by (seed, crc32(name))."""
    import zlib
    shape = COMPONENT_SHAPES[name]
    rng = np.random.default_rng([COMPONENT_SEED, zlib.crc32(name.encode())])
    return ((0.02 if name.endswith(".bias") else 0.03) * rng.standard_normal(shape)).astype(np.float32)


# ---- the decoder's sliding window (8192 positions, models/config.rs) past the point where it starts to move
DEC_WINDOW = 8192
EDGE_V_SCALE = 100.0       # one such key of ~8193 visible ones moves the tiny model's hidden states and logits by >= 60x the suite's 2e-4 (tests/test_oracle_window_edges.py)


def window_edge_rows(positions, window=DEC_WINDOW):
    """The two keys at the window's edge for every query position p: p - window - 1 (the last key a query at p must NOT see: the oracle masks
    |p - j| > window) and p - window (the first key it must see) -- those that exist.  A kernel whose window starts one key early or late adds or
    drops exactly one of them."""
    rows = set()
    for p in positions:
        rows.update(j for j in (p - window - 1, p - window) if j >= 0)
    return np.array(sorted(rows), dtype=np.int64)


def edge_kv(seed, lo, hi, n_kv, hd, edge_rows=(), v_scale=EDGE_V_SCALE, block=256):
    """K / V rows lo .. hi-1 of a synthetic cache layer, [n_kv][hi - lo][hd] (what vox_cache_update / orc_cache_update take): N(0, 1), drawn per
    `block` rows from default_rng([*seed, block index]) so that any row range can be (re)written alike on both sides without the rest of the layer
    (seed: e.g. (base, layer)).  The V rows listed in edge_rows are scaled by v_scale: with ~8193 visible keys one key holds ~1/8193 of the softmax
    weight, and at N(0, 1) an off-by-one in the window's first key would move the result by less than the tolerance."""
    seed = tuple(np.atleast_1d(seed).tolist())
    k = np.empty((n_kv, hi - lo, hd), np.float32); v = np.empty_like(k)
    for b in range(lo // block, (hi + block - 1) // block):
        rng = np.random.default_rng(seed + (b,))
        kb = rng.standard_normal((n_kv, block, hd), dtype=np.float32); vb = rng.standard_normal((n_kv, block, hd), dtype=np.float32)
        r0, r1 = max(lo, b * block), min(hi, (b + 1) * block)
        k[:, r0 - lo:r1 - lo] = kb[:, r0 - b * block:r1 - b * block]; v[:, r0 - lo:r1 - lo] = vb[:, r0 - b * block:r1 - b * block]
    e = np.asarray(edge_rows, dtype=np.int64)
    e = e[(e >= lo) & (e < hi)] - lo
    v[:, e] *= np.float32(v_scale)
    return k, v


def fill_edge_caches(caches, n_layers, n_kv, hd, lo, hi, edge_rows, seed=2026, step=2048):
    """Write rows lo .. hi-1 of every layer of each cache in `caches` (callables (layer, pos, k, v): a vox cache's update, or the oracle's
    cache_update bound to its cache) with edge_kv data -- in slices of `step` rows, so a 26-layer cache never needs its whole host copy at once."""
    for l in range(n_layers):
        for a in range(lo, hi, step):
            b = min(hi, a + step)
            k, v = edge_kv((seed, l), a, b, n_kv, hd, edge_rows)
            for upd in caches:
                upd(l, a, k, v)


# every slot of vox_debug_attn_launches, in the order of include/voxtral_hip.h (AttnForm, csrc/vox_kernels.h)
ATTN_FORMS = ("prefill_small", "prefill_mfma", "prefill_f32", "decode", "decode_spec", "decode_gqa", "attn_wo", "engine", "stream_ring", "group_resample", "stream_resample",
              "decode_paged", "decode_gqa_paged")


def attn_launches(pkg):
    """Attention launches of this process so far by kernel form (vox_debug_attn_launches)."""
    import ctypes
    out = (ctypes.c_uint64 * (len(ATTN_FORMS) + 1))()
    assert pkg.lib().vox_debug_attn_launches(out, len(ATTN_FORMS) + 1) == 0
    assert out[len(ATTN_FORMS)] == 0      # (entries past the last form are written as 0)
    return dict(zip(ATTN_FORMS, (int(x) for x in out)))


def launches_since(pkg, before):
    now = attn_launches(pkg)
    return {k: now[k] - before[k] for k in now if now[k] != before[k]}


GEMM_FORMS = ("gemv_r1", "gemv_r2", "gemv_r4", "dense_gemv", "skinny", "skinny_mt", "skinny_mt2", "xf_rows", "splitk_finish", "tile_11", "tile_12", "tile_21", "tile_22",
              "tile_21_tb", "tile_22_tb", "k32", "big", "big_rope", "dense2", "wide")


def gemm_launches(pkg):
    """Launches of the linear kernels of this process so far by kernel form (vox_debug_gemm_launches; the order of include/voxtral_hip.h)."""
    import ctypes
    out = (ctypes.c_uint64 * (len(GEMM_FORMS) + 1))()
    assert pkg.lib().vox_debug_gemm_launches(out, len(GEMM_FORMS) + 1) == 0
    return dict(zip(GEMM_FORMS, (int(x) for x in out)))


def gemm_launches_since(pkg, before):
    now = gemm_launches(pkg)
    return {k: now[k] - before[k] for k in now if now[k] != before[k]}


# vox_attention at hd 128 past the decoder window's first move: (M, kv_len, offset, window); every case runs at GQA 4:1 and 2:1
EDGE_ATTN_CASES = [
    (1, 8193, 8192, DEC_WINDOW),         # the last position whose window has not moved
    (1, 8194, 8193, DEC_WINDOW),         # the first that has: key 0 out, key 1 in
    (1, 8256, 8255, DEC_WINDOW),         # first visible key 63, the last of a 64-key tile (the MFMA kernel starts at its query block's tile)
    (70, 8263, 8193, DEC_WINDOW),        # two query blocks, both moved
    (80, 8230, 8150, DEC_WINDOW),        # a block that straddles the first move (rows 8150 .. 8213), then one that starts past it
    (38, 16384, 16346, DEC_WINDOW),      # the last rows a decoder cache can hold
    (200, 200, 0, 20),                   # a small window at hd 128
    (200, 200, 0, 65),                   # ... whose third block's first visible key is 63
]


def edge_attention_inputs(M, kv, H, KV, off, win, hd=128, seed=0):
    """q [M][H*hd] (N(0, 1.5^2)), k / v [kv][KV*hd] (edge_kv rows, token-major) for one EDGE_ATTN_CASES case, the V rows at every query's window
    edge scaled (window_edge_rows)."""
    rng = np.random.default_rng([seed, M, kv, off])
    q = (1.5 * rng.standard_normal((M, H * hd))).astype(np.float32)
    k, v = edge_kv((seed, 1, kv, off), 0, kv, KV, hd, window_edge_rows(range(off, off + M), win))
    return q, np.ascontiguousarray(k.transpose(1, 0, 2).reshape(kv, KV * hd)), np.ascontiguousarray(v.transpose(1, 0, 2).reshape(kv, KV * hd))
