"""Host-side mirror of the reference's `src/gguf` module over the C ABI: GgufReader (reader.rs),
Q4Tensor (tensor.rs), q4_matmul (op.rs), Q4Linear (linear.rs), Q4ModelLoader (loader.rs),
Q4VoxtralModel / Q4LanguageModel surface (model.rs).  All tensors cross as numpy float32 / int32."""
from __future__ import annotations

import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import check, lib, VoxError

F32, F16, Q4_0 = 0, 1, 2


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One HIP device + stream (the reference's implicit WgpuDevice::default())."""

    def __init__(self, device: int = 0):
        self.h = C.c_void_p()
        check(lib().vox_ctx_create(device, C.byref(self.h)))
        self.device = device

    def occupy(self, workgroups: int, micros: int):
        """Test hook: `workgroups` x 1024 threads spin for `micros` us on a side stream (returns at once)."""
        check(lib().vox_debug_occupy(self.h, workgroups, micros))

    def set_shared(self, shared: bool = True):
        """vox_ctx_set_shared: this context shares its GPU with other sessions (no batched decode engines, slot planner on the scaled cost table); results unchanged."""
        check(lib().vox_ctx_set_shared(self.h, 1 if shared else 0))

    def synchronize(self):
        check(lib().vox_ctx_synchronize(self.h))

    def stream(self):
        s = C.c_void_p(); check(lib().vox_ctx_stream(self.h, C.byref(s)))
        return s.value

    def alloc(self, nbytes):
        p = C.c_void_p(); check(lib().vox_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, p):
        check(lib().vox_dev_free(self.h, C.c_void_p(p)))

    def upload(self, arr):
        arr = np.ascontiguousarray(arr); p = self.alloc(arr.nbytes)
        check(lib().vox_dev_upload(self.h, C.c_void_p(p), _ptr(arr), arr.nbytes))
        return p

    def download(self, p, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        check(lib().vox_dev_download(self.h, _ptr(out), C.c_void_p(p), out.nbytes))
        return out

    def copy(self, dst, src, nbytes):
        check(lib().vox_dev_copy(self.h, C.c_void_p(dst), C.c_void_p(src), nbytes))

    def close(self):
        if self.h:
            lib().vox_ctx_destroy(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count():
    n = C.c_int32(); check(lib().vox_device_count(C.byref(n)))
    return n.value


class GgufTensorInfo:
    def __init__(self, name, dims, dtype, nbytes):
        self.name, self._dims, self._dtype, self._nbytes = name, dims, dtype, nbytes

    def shape(self):
        return list(self._dims)

    def dtype(self):
        return self._dtype

    def num_elements(self):
        return int(np.prod(self._dims)) if self._dims else 1

    def byte_size(self):
        return self._nbytes


class GgufReader:
    """gguf/reader.rs:98-223 (v2/v3; dtypes F32/F16/Q4_0)"""

    def __init__(self, path=None):
        self.h = C.c_void_p(); self._keep = None
        if path is not None:
            check(lib().vox_gguf_open(str(path).encode(), C.byref(self.h)))

    @classmethod
    def open(cls, path):
        return cls(path)

    @classmethod
    def from_bytes(cls, data):
        """gguf/reader.rs:98-103: parse a GGUF image held in memory (kept alive by this object, not copied)."""
        r = cls(); r._keep = np.frombuffer(data, dtype=np.uint8)
        check(lib().vox_gguf_open_memory(r._keep.ctypes.data, r._keep.size, C.byref(r.h)))
        return r

    @classmethod
    def from_shards(cls, shards):
        """gguf/loader.rs:101-107: consecutive pieces (<= 512 MB each in the reference's WASM loader) of one GGUF image."""
        arrs = [np.frombuffer(s, dtype=np.uint8) for s in shards]; n = len(arrs)
        ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs]); sizes = (C.c_size_t * n)(*[a.size for a in arrs])
        r = cls(); check(lib().vox_gguf_open_shards(ptrs, sizes, n, C.byref(r.h)))
        return r

    def version(self):
        v = C.c_uint32(); check(lib().vox_gguf_version(self.h, C.byref(v))); return v.value

    def tensor_count(self):
        v = C.c_uint64(); check(lib().vox_gguf_tensor_count(self.h, C.byref(v))); return v.value

    def tensor_names(self):
        out = []
        for i in range(self.tensor_count()):
            s = C.c_char_p(); check(lib().vox_gguf_tensor_name(self.h, i, C.byref(s))); out.append(s.value.decode())
        return out

    def tensor_info(self, name):
        dims = (C.c_uint64 * 4)(); nd = C.c_uint32(); dt = C.c_uint32(); nb = C.c_uint64()
        r = lib().vox_gguf_tensor_info(self.h, name.encode(), C.byref(dims), C.byref(nd), C.byref(dt), C.byref(nb))
        if r == 4:
            return None                      # Option::None, reader.rs:200-202
        check(r)
        return GgufTensorInfo(name, [int(dims[i]) for i in range(nd.value)], dt.value, nb.value)

    def tensor_data(self, name):
        info = self.tensor_info(name)
        if info is None:
            raise VoxError(4, f"Tensor '{name}' not found in GGUF")
        out = np.empty(info.byte_size(), dtype=np.uint8)
        check(lib().vox_gguf_tensor_data(self.h, name.encode(), _ptr(out), out.size))
        return out

    def close(self):
        if self.h:
            lib().vox_gguf_close(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Q4Tensor:
    """gguf/tensor.rs:21-113"""

    def __init__(self, ctx, h, shape):
        self.ctx, self.h, self._shape = ctx, h, shape

    @classmethod
    def from_q4_bytes(cls, raw_bytes, shape, ctx: Context):
        raw = np.ascontiguousarray(np.frombuffer(raw_bytes, dtype=np.uint8) if not isinstance(raw_bytes, np.ndarray) else raw_bytes, dtype=np.uint8)
        n, k = shape; h = C.c_void_p()
        check(lib().vox_q4_tensor_from_bytes(ctx.h, _ptr(raw), raw.size, n, k, C.byref(h)))
        return cls(ctx, h, [n, k])

    @classmethod
    def from_f32(cls, w, ctx: Context, other=None):
        """Dense f32-path weight [N, K] (models/weights.rs:16-66) in the f32 model's device format; `other`: a second [N, K] tensor interleaved row by row
        (the fused gate | up operand of SwiGLU, models/layers/swiglu.rs:72-77)."""
        w = _f32(w); n, k = w.shape; h = C.c_void_p()
        o = None if other is None else _f32(other)
        check(lib().vox_dense_tensor_from_f32(ctx.h, _ptr(w), None if o is None else _ptr(o), n, k, C.byref(h)))
        return cls(ctx, h, [n if o is None else 2 * n, k])

    def shape(self):
        return list(self._shape)

    def num_blocks(self):
        v = C.c_int64(); check(lib().vox_q4_tensor_num_blocks(self.h, C.byref(v))); return v.value

    def dequantize(self):
        out = np.empty(self._shape, dtype=np.float32)
        check(lib().vox_q4_tensor_dequantize(self.ctx.h, self.h, _ptr(out)))
        return out

    def close(self):
        if self.h:
            lib().vox_q4_tensor_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def q4_matmul(x, weights: Q4Tensor):
    """gguf/op.rs:86-137: x [B, M, K] float32 -> [B, M, N]; raises on rank/shape mismatch (the reference panics)."""
    x = _f32(x)
    if x.ndim != 3:
        raise VoxError(1, f"q4_matmul expects a 3-D input, got {x.ndim}-D")
    b, m, k = x.shape
    n, kw = weights.shape()
    if k != kw:
        raise VoxError(1, f"q4_matmul: input K={k} != weight K={kw}")
    out = np.empty((b, m, n), dtype=np.float32)
    check(lib().vox_q4_matmul(weights.ctx.h, weights.h, _ptr(x), b, m, _ptr(out), 0))
    return out


def linear_forward(weights: Q4Tensor, x, bias=None, epilogue=0):
    """Linear::forward with a fused epilogue (0 none, 1 GELU, 2 SwiGLU over interleaved gate / up rows -> N / 2 columns); x [B, M, K]."""
    x = _f32(x)
    if x.ndim != 3:
        raise VoxError(1, f"linear_forward expects a 3-D input, got {x.ndim}-D")
    b, m, k = x.shape; n, kw = weights.shape()
    if k != kw:      # the C entry takes K from the tensor: a shorter row would be read past its end
        raise VoxError(1, f"linear_forward: input K={k} != weight K={kw}")
    if bias is not None and np.size(bias) != n:
        raise VoxError(1, f"linear_forward: bias has {np.size(bias)} elements, weight N={n}")
    out = np.empty((b, m, n // 2 if epilogue == 2 else n), dtype=np.float32)
    bb = None if bias is None else _f32(bias)
    check(lib().vox_linear_forward_ex(weights.ctx.h, weights.h, None if bb is None else _ptr(bb), _ptr(x), b, m, _ptr(out), epilogue, 0))
    return out


def conv_downsample(ctx, x, w1, b1, w2, b2):
    """ConvDownsampler::forward (models/layers/conv.rs:78-83): x [C, L] -> [O, L2] through the conv stem's im2col MFMA path."""
    x, w1, b1, w2, b2 = (_f32(a) for a in (x, w1, b1, w2, b2))
    c_, l_ = x.shape; o_ = w1.shape[0]; l2 = ((l_ + 1) // 2 + 1) // 2
    out = np.empty((o_, l2), dtype=np.float32)
    check(lib().vox_conv_downsample(ctx.h, _ptr(x), c_, l_, _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), o_, _ptr(out)))
    return out


def attention(ctx, q, k, v, n_heads, n_kv_heads, offset=0, window=-1):
    """Attention core (gguf/model.rs:100-120,125-198 + masking.rs:9-107): q [M, n_heads*hd], k/v [kv_len, n_kv_heads*hd]
    -> [M, n_heads*hd]; query m sits at position offset+m, causal, optional sliding window."""
    q, k, v = _f32(q), _f32(k), _f32(v)
    if q.ndim != 2 or k.ndim != 2 or k.shape != v.shape or q.shape[1] % n_heads:
        raise VoxError(1, "attention: bad shapes")
    hd = q.shape[1] // n_heads
    if k.shape[1] != n_kv_heads * hd:
        raise VoxError(1, "attention: k/v width != n_kv_heads*head_dim")
    out = np.empty_like(q)
    check(lib().vox_attention(ctx.h, _ptr(q), _ptr(k), _ptr(v), q.shape[0], k.shape[0], n_heads, n_kv_heads, hd, offset, window, _ptr(out), 0))
    return out


def kv_round_bf16(x) -> np.ndarray:
    """vox_kv_round_bf16 (host arithmetic): the bf16 K/V pool's rounding of float32 values -- round to nearest even on the upper 16 bits -- as uint16 of x's shape."""
    x = _f32(x); out = np.empty(x.shape, np.uint16)
    check(lib().vox_kv_round_bf16(_ptr(x), x.size, _ptr(out)))
    return out


class AttnDecodeDesc(C.Structure):
    """vox_attn_decode_desc (include/voxtral_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_seq", "n_heads", "n_kv_heads", "head_dim", "window", "n_slices", "max_seq", "page_rows", "pool_pages", "page_tab_stride",
                                         "score_rows", "prefer_gqa", "spec", "no_xcd_remap", "out_xf")] + [(n, C.c_void_p) for n in ("pos", "kv_row", "page_tab")]


def attn_decode(ctx, q, k, v, pos, n_heads, n_kv_heads, window=-1, kv_row=None, page_tab=None, score_rows=0, prefer_gqa=False, spec=False, no_xcd_remap=False,
                out_xf=False, head_dim=128, page_tab_len=None, bf16=False):
    """vox_debug_attn_decode: ONE decode attention launch.  q [n_seq, n_heads*128], pos [n_seq]; slab: k / v [n_slices, n_kv_heads, max_seq, 128]; paged (page_tab
    [n_slices, stride] int32 given): k / v [pool_pages, n_kv_heads, page_rows, 128].  Returns float32 [n_seq, n_heads*128], or with out_xf the raw XF planes as uint16
    [ceil(n_seq / 16), 2, n_heads*128 / 128 * 256 * 8] (hi plane, lo plane).
    page_tab_len (a paged call): vox_debug_attn_decode_paged_ring -- every table row is a ring of page_tab_len entries, logical page q at entry q % page_tab_len.
    bf16 (a paged call): vox_debug_attn_decode_paged_bf16 -- k / v are uint16 pools of bf16 values (kv_round_bf16); page_tab_len None: a flat table."""
    if bf16:
        q, k, v = _f32(q), np.ascontiguousarray(k, dtype=np.uint16), np.ascontiguousarray(v, dtype=np.uint16)
        if page_tab is None:
            raise VoxError(1, "attn_decode: a bf16 pool belongs to a paged call")
    else:
        q, k, v = _f32(q), _f32(k), _f32(v)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    if q.ndim != 2 or k.ndim != 4 or k.shape != v.shape or pos.shape != (q.shape[0],):
        raise VoxError(1, "attn_decode: bad shapes")
    d = AttnDecodeDesc(n_seq=q.shape[0], n_heads=n_heads, n_kv_heads=n_kv_heads, head_dim=head_dim, window=window, prefer_gqa=int(prefer_gqa), spec=int(spec),
                       no_xcd_remap=int(no_xcd_remap), out_xf=int(out_xf), pos=pos.ctypes.data)
    if kv_row is not None:
        kv_row = np.ascontiguousarray(kv_row, dtype=np.int32)
        if kv_row.shape != pos.shape:
            raise VoxError(1, "attn_decode: bad shapes")
        d.kv_row = kv_row.ctypes.data
    if page_tab is None:
        d.n_slices, d.max_seq = k.shape[0], k.shape[2]
    else:
        page_tab = np.ascontiguousarray(page_tab, dtype=np.int32)
        if page_tab.ndim != 2:
            raise VoxError(1, "attn_decode: bad shapes")
        d.n_slices, d.page_tab_stride = page_tab.shape
        d.pool_pages, d.page_rows, d.score_rows, d.page_tab = k.shape[0], k.shape[2], score_rows, page_tab.ctypes.data
    if k.shape[1] != n_kv_heads or k.shape[3] != 128 or q.shape[1] != n_heads * 128:
        raise VoxError(1, "attn_decode: q / k / v widths do not match the head counts")
    QD = n_heads * 128
    out = np.empty(((q.shape[0] + 15) // 16, 2, QD // 128 * 256 * 8), np.uint16) if out_xf else np.empty((q.shape[0], QD), np.float32)
    if bf16:
        check(lib().vox_debug_attn_decode_paged_bf16(ctx.h, C.byref(d), int(page_tab_len or 0), _ptr(q), _ptr(k), _ptr(v), _ptr(out)))
    elif page_tab_len is not None:
        check(lib().vox_debug_attn_decode_paged_ring(ctx.h, C.byref(d), int(page_tab_len), _ptr(q), _ptr(k), _ptr(v), _ptr(out)))
    else:
        check(lib().vox_debug_attn_decode(ctx.h, C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out)))
    return out


def attn_decode_ring(ctx, q, k, v, pos, n_heads, n_kv_heads, window):
    """vox_debug_attn_decode_ring: ONE ring decode attention launch.  q [n_seq, n_heads*128], pos [n_seq] (any value below 2^24); k / v [n_slices, n_kv_heads, cap, 128]
    with row j of a sequence at ring row j % cap; 0 <= window < cap.  Returns float32 [n_seq, n_heads*128]."""
    q, k, v = _f32(q), _f32(k), _f32(v)
    pos = np.ascontiguousarray(pos, dtype=np.int32)
    if q.ndim != 2 or k.ndim != 4 or k.shape != v.shape or pos.shape != (q.shape[0],):
        raise VoxError(1, "attn_decode_ring: bad shapes")
    if k.shape[1] != n_kv_heads or k.shape[3] != 128 or q.shape[1] != n_heads * 128:
        raise VoxError(1, "attn_decode_ring: q / k / v widths do not match the head counts")
    d = AttnDecodeDesc(n_seq=q.shape[0], n_heads=n_heads, n_kv_heads=n_kv_heads, head_dim=128, window=window, n_slices=k.shape[0], max_seq=k.shape[2], pos=pos.ctypes.data)
    out = np.empty((q.shape[0], n_heads * 128), np.float32)
    check(lib().vox_debug_attn_decode_ring(ctx.h, C.byref(d), _ptr(q), _ptr(k), _ptr(v), _ptr(out)))
    return out


class StreamAttnDesc(C.Structure):
    """vox_stream_attn_desc (include/voxtral_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_slots", "n_members", "rows", "n_heads", "head_dim", "window", "cap", "layers", "layer", "rope_rows", "rope_per_member")] + \
               [("theta", C.c_float), ("order", C.c_void_p), ("enc_pos", C.c_void_p)]


def stream_attn(ctx, qkv, kring, vring, order, enc_pos, rows, window, theta, layer=0, rope_rows=0, rope_per_member=False, _entry="vox_debug_stream_attn"):
    """vox_debug_stream_attn: ONE launch of the live sessions' encoder ring attention (RoPE on q and k, K / V append, windowed softmax).  qkv [n_slots * rows,
    3 * n_heads * hd] not rotated; kring / vring [n_members, layers, n_heads, cap, hd] (hd 64 | 128); order [n_slots] distinct members; enc_pos [n_members].
    rope_rows 0: a flat RoPE table; R: a RoPE ring of R rows, with rope_per_member one per member.  Returns (out [n_slots * rows, n_heads * hd], kring, vring after
    the launch); the arguments are left as they are."""
    qkv = _f32(qkv); kring = _f32(kring).copy(); vring = _f32(vring).copy()
    order = np.ascontiguousarray(order, dtype=np.int32); enc_pos = np.ascontiguousarray(enc_pos, dtype=np.int32)
    if qkv.ndim != 2 or kring.ndim != 5 or kring.shape != vring.shape or order.ndim != 1 or enc_pos.shape != (kring.shape[0],):
        raise VoxError(1, "stream_attn: bad shapes")
    n_members, layers, n_heads, cap, hd = kring.shape
    if qkv.shape != (len(order) * max(int(rows), 0), 3 * n_heads * hd):
        raise VoxError(1, "stream_attn: qkv is not [n_slots * rows][3 * n_heads * head_dim]")
    d = StreamAttnDesc(n_slots=len(order), n_members=n_members, rows=int(rows), n_heads=n_heads, head_dim=hd, window=int(window), cap=cap, layers=layers, layer=int(layer),
                       rope_rows=int(rope_rows), rope_per_member=int(bool(rope_per_member)), theta=float(theta), order=order.ctypes.data, enc_pos=enc_pos.ctypes.data)
    out = np.empty((qkv.shape[0], n_heads * hd), np.float32)
    check(getattr(lib(), _entry)(ctx.h, C.byref(d), _ptr(qkv), _ptr(kring), _ptr(vring), _ptr(out)))
    return out, kring, vring


def stream_attn_burst(ctx, qkv, kring, vring, order, enc_pos, rows, window, theta, layer=0, rope_rows=0, rope_per_member=False):
    """vox_debug_stream_attn_burst: stream_attn's arguments with rows up to 64 (a burst's 4 b rows) -- ONE launch of the burst kernel, which leaves the bits b
    chained stream_attn launches of 4 rows leave."""
    return stream_attn(ctx, qkv, kring, vring, order, enc_pos, rows, window, theta, layer, rope_rows, rope_per_member, _entry="vox_debug_stream_attn_burst")


def stream_attn_group_burst(ctx, qkv, kring, vring, order, enc_pos, rows_per_slot, window, theta, layer=0, rope_rows=0, rope_per_member=False):
    """vox_debug_stream_attn_group_burst: the RAGGED burst attention of a burst group's round -- slot z has rows_per_slot[z] rows (multiples of 4 in 4..64: its b_z
    ticks), qkv [sum rows, 3 * n_heads * hd] and out hold the slots' rows back to back.  ONE launch; for every slot it leaves the bits rows_per_slot[z] / 4 chained
    stream_attn launches of 4 rows leave, and members outside `order` keep their rings.  Returns (out [sum rows, n_heads * hd], kring, vring)."""
    qkv = _f32(qkv); kring = _f32(kring).copy(); vring = _f32(vring).copy()
    order = np.ascontiguousarray(order, dtype=np.int32); enc_pos = np.ascontiguousarray(enc_pos, dtype=np.int32); rps = np.ascontiguousarray(rows_per_slot, dtype=np.int32)
    if qkv.ndim != 2 or kring.ndim != 5 or kring.shape != vring.shape or order.ndim != 1 or rps.shape != order.shape or enc_pos.shape != (kring.shape[0],):
        raise VoxError(1, "stream_attn_group_burst: bad shapes")
    n_members, layers, n_heads, cap, hd = kring.shape
    if qkv.shape != (int(np.maximum(rps, 0).sum()), 3 * n_heads * hd):
        raise VoxError(1, "stream_attn_group_burst: qkv is not [sum rows_per_slot][3 * n_heads * head_dim]")
    d = StreamAttnDesc(n_slots=len(order), n_members=n_members, rows=int(rps.max()) if rps.size else 0, n_heads=n_heads, head_dim=hd, window=int(window), cap=cap, layers=layers,
                       layer=int(layer), rope_rows=int(rope_rows), rope_per_member=int(bool(rope_per_member)), theta=float(theta), order=order.ctypes.data, enc_pos=enc_pos.ctypes.data)
    out = np.empty((qkv.shape[0], n_heads * hd), np.float32)
    check(lib().vox_debug_stream_attn_group_burst(ctx.h, C.byref(d), _ptr(rps), _ptr(qkv), _ptr(kring), _ptr(vring), _ptr(out)))
    return out, kring, vring


def stream_attn_burst_launches() -> int:
    """vox_debug_stream_attn_burst_launches: launches of the burst kernel so far (a counter of its own, in no slot of attn_launches)."""
    v = C.c_uint64(); check(lib().vox_debug_stream_attn_burst_launches(C.byref(v)))
    return int(v.value)


STREAM_BURST_MAX = 16      # VOX_STREAM_BURST_MAX


def stream_burst_len(due: int, burst: int, pos: int, next_stop: int) -> int:
    """vox_stream_burst_len: the next burst of a pass with `due` ticks still to run at position pos -- max(1, min(due, burst, next_stop - pos))."""
    return int(lib().vox_stream_burst_len(int(due), int(burst), int(pos), int(next_stop)))


def stream_group_burst_rounds(due, burst: int) -> list:
    """vox_stream_group_burst_rounds: the rounds of a burst group's pass whose members have `due` ticks due (sorted descending, 1..16 of them) at burst_ticks = burst --
    one tuple of b_z per round: round k gives the first #{due_z > k burst} members min(due_z - k burst, burst) ticks.  ceil(max due / burst) rounds; a round of
    ones is a plain group round."""
    d = np.ascontiguousarray([int(v) for v in due], dtype=np.int32)
    cap = max(1, -(-int(d.max()) // max(int(burst), 1))) if d.size else 1
    out = np.zeros((cap, 17), dtype=np.int32); n = C.c_int32()
    check(lib().vox_stream_group_burst_rounds(_ptr(d), int(d.size), int(burst), _ptr(out), cap, C.byref(n)))
    return [tuple(int(x) for x in row[1:1 + row[0]]) for row in out[:n.value]]


def stream_ring_init(ctx, kv, kring, vring):
    """vox_debug_stream_ring_init: the rings' seeding from token-major rows.  kv [layers, rows, 2 * n_heads * hd] (k row | v row); kring / vring [layers, n_heads, cap,
    hd].  Returns (kring, vring) after the launch; the arguments are left as they are."""
    kv = _f32(kv); kring = _f32(kring).copy(); vring = _f32(vring).copy()
    if kv.ndim != 3 or kring.ndim != 4 or kring.shape != vring.shape or kv.shape[0] != kring.shape[0] or kv.shape[2] != 2 * kring.shape[1] * kring.shape[3]:
        raise VoxError(1, "stream_ring_init: bad shapes")
    layers, n_heads, cap, hd = kring.shape
    check(lib().vox_debug_stream_ring_init(ctx.h, layers, kv.shape[1], n_heads, hd, cap, _ptr(kv), _ptr(kring), _ptr(vring)))
    return kring, vring


def rope_rows(head_dim, theta, first_pos, n):
    """vox_debug_rope_rows (host arithmetic, no device): (inv [head_dim/2], cos [n, head_dim/2], sin [n, head_dim/2]) float32 for positions first_pos .. first_pos + n - 1."""
    half = max(int(head_dim) // 2, 0)
    inv = np.empty(half, np.float32); cos = np.empty((max(int(n), 0), half), np.float32); sin = np.empty_like(cos)
    check(lib().vox_debug_rope_rows(int(head_dim), float(theta), int(first_pos), int(n), _ptr(inv), _ptr(cos), _ptr(sin)))
    return inv, cos, sin


class SnapshotKvDesc(C.Structure):
    """vox_snapshot_kv_desc (include/voxtral_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("layers", "n_heads", "head_dim", "lo", "hi", "layout", "rows", "page_rows", "pool_pages", "page_tab_len")] + \
               [("layer_stride", C.c_int64), ("page_tab", C.c_void_p)]


def snapshot_kv(ctx, cache_k, cache_v, lo, hi, n_heads, head_dim, layout="flat", rows=0, page_tab=None, page_rows=0, blob=None):
    """vox_debug_snapshot_kv: ONE launch of the session blob's K / V kernel over the logical rows lo .. hi - 1.  layout "flat" | "ring": cache_k / cache_v
    [layers, layer_floats] with head h of a layer at h * rows * head_dim (ring: row r at r % rows); "paged" | "paged_ring": [layers, pool_pages, n_heads, page_rows,
    head_dim] with page_tab [entries] int32.  blob None: pack -> the blob [2, layers, n_heads, hi - lo, head_dim]; blob given: unpack it -> (cache_k, cache_v) after the
    launch.  The arguments are left as they are."""
    ck = _f32(cache_k).copy(); cv = _f32(cache_v).copy()
    code = {"flat": 0, "ring": 1, "paged": 2, "paged_ring": 3}[layout]
    if ck.shape != cv.shape or ck.ndim != (2 if code < 2 else 5):
        raise VoxError(1, "snapshot_kv: bad shapes")
    d = SnapshotKvDesc(layers=ck.shape[0], n_heads=int(n_heads), head_dim=int(head_dim), lo=int(lo), hi=int(hi), layout=code)
    if code < 2:
        d.rows, d.layer_stride = int(rows), ck.shape[1]
    else:
        page_tab = np.ascontiguousarray(page_tab, dtype=np.int32)
        if page_tab.ndim != 1 or ck.shape[2] != n_heads or ck.shape[4] != head_dim or ck.shape[3] != page_rows:
            raise VoxError(1, "snapshot_kv: bad shapes")
        d.page_rows, d.pool_pages, d.page_tab_len, d.page_tab = int(page_rows), ck.shape[1], page_tab.size, page_tab.ctypes.data
    shape = (2, ck.shape[0], int(n_heads), max(int(hi) - int(lo), 0), int(head_dim))
    if blob is None:
        out = np.zeros(shape, np.float32)
        check(lib().vox_debug_snapshot_kv(ctx.h, C.byref(d), _ptr(ck), _ptr(cv), _ptr(out), 0))
        return out
    blob = _f32(blob)
    if blob.shape != shape:
        raise VoxError(1, "snapshot_kv: the blob is not [2, layers, n_heads, hi - lo, head_dim]")
    check(lib().vox_debug_snapshot_kv(ctx.h, C.byref(d), _ptr(ck), _ptr(cv), _ptr(blob), 1))
    return ck, cv


def snapshot_info(blob) -> dict:
    """vox_snapshot_describe (host arithmetic, no device): validates the header of a session blob (a numpy uint8 array) and returns it as a dict."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
    v = _lib.SnapshotInfo(); check(lib().vox_snapshot_describe(_ptr(blob) if blob.size else None, blob.size, C.byref(v)))
    out = {n: getattr(v, n) for n, _ in _lib.SnapshotInfo._fields_ if n not in ("reserved", "section_offset", "section_bytes")}
    out["section_offset"] = [int(x) for x in v.section_offset]; out["section_bytes"] = [int(x) for x in v.section_bytes]
    return out


def snapshot_bytes_for(config, positions, sample_rate=16000, n_samples=0, scores=False, alternatives=False) -> int:
    """vox_snapshot_bytes_for: the blob size of a session of this model geometry (a model's .config) at decoder position `positions` after n_samples pushed samples."""
    n = C.c_size_t()
    check(lib().vox_snapshot_bytes_for(C.byref(config), int(positions), int(sample_rate), int(n_samples), int(bool(scores)), int(bool(alternatives)), C.byref(n)))
    return n.value


def attn_gqa_max_seq(ctx):
    """vox_debug_attn_gqa_max_seq: the most rows per KV head the slab GQA decode attention serves (a slab stream group's max_positions on a 4:1 model)."""
    n = C.c_int32(); check(lib().vox_debug_attn_gqa_max_seq(ctx.h, C.byref(n)))
    return n.value


class Q4Linear:
    """gguf/linear.rs:17-40"""

    def __init__(self, weights: Q4Tensor, bias=None):
        self.weights = weights
        self.bias = None if bias is None else _f32(bias)

    @classmethod
    def new(cls, weights, bias=None):
        return cls(weights, bias)

    def forward(self, x):
        x = _f32(x); b, m, k = x.shape; n = self.weights.shape()[0]
        out = np.empty((b, m, n), dtype=np.float32)
        check(lib().vox_q4_linear_forward(self.weights.ctx.h, self.weights.h, None if self.bias is None else _ptr(self.bias),
                                          _ptr(x), b, m, _ptr(out), 0))
        return out


class LayerCaches:
    """create_cache_preallocated, gguf/model.rs:711-723 / kv_cache.rs:221-258"""

    def __init__(self, model, max_seq):
        self.model = model; self.h = C.c_void_p()
        check(lib().vox_decoder_cache_create(model.h, max_seq, C.byref(self.h)))
        model._caches.add(self)

    def seq_len(self):
        v = C.c_int32(); check(lib().vox_cache_seq_len(self.h, C.byref(v))); return v.value

    def reset(self):
        check(lib().vox_cache_reset(self.h))

    def update(self, layer, pos, k, v):
        """KVCache::update on one layer (kv_cache.rs:116-136): k / v [kv_heads][n][head_dim] host arrays -> rows pos .. pos + n"""
        k = _f32(k); v = _f32(v); assert k.shape == v.shape and k.ndim == 3
        check(lib().vox_cache_update(self.h, layer, pos, _ptr(k), _ptr(v), k.shape[1], 0))

    def truncate(self, n):
        check(lib().vox_cache_truncate(self.h, n))

    def close(self):
        if self.h:
            lib().vox_cache_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class EncoderCaches(LayerCaches):
    """Q4AudioEncoder::create_cache (gguf/model.rs:454-459): K / V of the streaming encoder; evicts rows older than the sliding window by itself."""

    def __init__(self, model, capacity_rows=0):
        self.model = model; self.h = C.c_void_p()
        check(lib().vox_encoder_cache_create(model.h, capacity_rows, C.byref(self.h)))
        model._caches.add(self)

    def abs_pos(self):
        v = C.c_int32(); check(lib().vox_cache_abs_pos(self.h, C.byref(v))); return v.value

    def apply_sliding_window(self, window):
        """kv_cache.rs:176-203 (every layer)"""
        check(lib().vox_encoder_cache_apply_sliding_window(self.h, window))


class Q4LanguageModel:
    """The decoder surface used by e2e-bench (gguf/model.rs:566-723)."""

    def __init__(self, model):
        self._m = model

    def n_layers(self):
        return self._m.config.dec_layers

    def d_model(self):
        return self._m.config.dec_dim

    def embed_tokens_from_ids(self, ids, batch=1, seq=None):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        out = np.empty((ids.size, self.d_model()), dtype=np.float32)
        check(lib().vox_embed_tokens_from_ids(self._m.h, _ptr(ids), ids.size, _ptr(out)))
        return out.reshape(batch, -1, self.d_model())

    def create_cache_preallocated(self, max_seq):
        return LayerCaches(self._m, max_seq)

    def forward_hidden_with_cache(self, x, t_embed, caches: LayerCaches):
        x = _f32(x); shp = x.shape; x2 = x.reshape(-1, self.d_model())
        out = np.empty_like(x2)
        check(lib().vox_forward_hidden_with_cache(self._m.h, _ptr(x2), x2.shape[0], _ptr(_f32(t_embed).reshape(-1)), caches.h, _ptr(out)))
        return out.reshape(shp)

    def lm_head(self, hidden):
        h = _f32(hidden); shp = h.shape; h2 = h.reshape(-1, self.d_model())
        out = np.empty((h2.shape[0], self._m.config.vocab), dtype=np.float32)
        check(lib().vox_lm_head(self._m.h, _ptr(h2), h2.shape[0], _ptr(out)))
        return out.reshape(shp[:-1] + (self._m.config.vocab,))


    # ---- device-resident forms (VOX_MEM_DEVICE): raw device pointers in, nothing copied, nothing synchronised -- the loop of bin/e2e_bench.rs:179-224 on "tensors"
    def embed_tokens_from_ids_dev(self, ids, out_ptr):
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
        check(lib().vox_embed_tokens_from_ids_ex(self._m.h, _ptr(ids), ids.size, C.c_void_p(out_ptr), 1))

    def forward_hidden_with_cache_dev(self, x_ptr, rows, t_embed, caches: LayerCaches, out_ptr=None):
        """-> device pointer of the model-owned hidden rows (read-only; valid until the next decoder call).  One row on an engine-eligible cache = one engine launch."""
        ws = C.c_void_p()
        check(lib().vox_forward_hidden_with_cache_ex(self._m.h, C.c_void_p(x_ptr), rows, _ptr(_f32(t_embed).reshape(-1)), caches.h,
                                                     None if out_ptr is None else C.c_void_p(out_ptr), C.byref(ws), 1))
        return ws.value

    def lm_head_dev(self, hidden_ptr, rows, logits_ptr):
        check(lib().vox_lm_head_ex(self._m.h, C.c_void_p(hidden_ptr), rows, C.c_void_p(logits_ptr), 1))

    def lm_head_argmax(self, hidden_ptr, rows):
        """lm_head + argmax(2) + read-back: `rows` token ids (host)."""
        ids = np.zeros(rows, dtype=np.int32)
        check(lib().vox_lm_head_argmax(self._m.h, C.c_void_p(hidden_ptr), rows, _ptr(ids), 1))
        return ids


def tensor_add_dev(ctx, a_ptr, b_ptr, n, out_ptr):
    """out = a + b on device pointers (n floats), on the context's stream"""
    check(lib().vox_tensor_add(ctx.h, C.c_void_p(a_ptr), C.c_void_p(b_ptr), n, C.c_void_p(out_ptr), 1))


def argmax_rows_dev(ctx, logits_ptr, rows, vocab):
    """`logits.argmax(2)` + scalar read-back of device logits [rows][vocab] -> host ids; synchronises the stream"""
    ids = np.zeros(rows, dtype=np.int32)
    check(lib().vox_argmax_rows(ctx.h, C.c_void_p(logits_ptr), rows, vocab, _ptr(ids), 1))
    return ids


SCORE_DTYPE = np.dtype([("logprob", "<f4"), ("margin", "<f4"), ("runner_up", "<i4"), ("id", "<i4")])      # vox_token_score


def score_rows(ctx, logits, ids=None, device_ptr=None, shape=None):
    """vox_score_rows: one vox_token_score per row of f32 logits [rows][vocab] -> a structured array (logprob, margin, runner_up, id).  ids: the id to score in every
    row (None: the row's argmax by the project's rule).  logits: a host array, or device_ptr + shape=(rows, vocab).  Computed on the device; synchronises."""
    if device_ptr is None:
        x = _f32(logits); x = x.reshape(1, -1) if x.ndim == 1 else x
        M, V = x.shape; ptr = _ptr(x); kind = 0
    else:
        M, V = (int(v) for v in shape); ptr = C.c_void_p(device_ptr); kind = 1
    t = None if ids is None else np.ascontiguousarray(ids, dtype=np.int32).reshape(-1)
    if t is not None and t.size != M:
        raise ValueError(f"{t.size} ids for {M} rows")
    out = np.zeros(M, dtype=SCORE_DTYPE)
    check(lib().vox_score_rows(ctx.h, ptr, M, V, None if t is None else _ptr(t), _ptr(out), kind))
    return out


ALTS_DTYPE = np.dtype([("entropy", "<f4"), ("n", "<i4"), ("alt", np.dtype([("id", "<i4"), ("logprob", "<f4")]), (8,))])      # vox_token_alts


def alternatives_rows(ctx, logits, k, device_ptr=None, shape=None):
    """vox_alternatives_rows: one vox_token_alts per row of f32 logits [rows][vocab] -> a structured array (entropy, n, alt[8] of (id, logprob)): the row's k best ids
    by the project's argmax rule with their log-probabilities, and the entropy of its softmax.  logits: a host array, or device_ptr + shape=(rows, vocab).  Computed on
    the device; synchronises."""
    if device_ptr is None:
        x = _f32(logits); x = x.reshape(1, -1) if x.ndim == 1 else x
        M, V = x.shape; ptr = _ptr(x); kind = 0
    else:
        M, V = (int(v) for v in shape); ptr = C.c_void_p(device_ptr); kind = 1
    out = np.zeros(M, dtype=ALTS_DTYPE)
    check(lib().vox_alternatives_rows(ctx.h, ptr, M, V, int(k), _ptr(out), kind))
    return out


def records_rows(ctx, logits, k=0, device_ptr=None, shape=None):
    """vox_records_rows: both records of every row of f32 logits [rows][vocab] from one launch, scored on the row's own argmax -> (scores, alts): the structured arrays
    of score_rows(ctx, logits) and alternatives_rows(ctx, logits, k), bit for bit; k = 0: scores alone, alts is None.  logits: a host array, or device_ptr +
    shape=(rows, vocab).  Computed on the device; synchronises."""
    if device_ptr is None:
        x = _f32(logits); x = x.reshape(1, -1) if x.ndim == 1 else x
        M, V = x.shape; ptr = _ptr(x); kind = 0
    else:
        M, V = (int(v) for v in shape); ptr = C.c_void_p(device_ptr); kind = 1
    k = int(k)
    sc = np.zeros(M, dtype=SCORE_DTYPE); al = np.zeros(M, dtype=ALTS_DTYPE) if k != 0 else None
    check(lib().vox_records_rows(ctx.h, ptr, M, V, k, _ptr(sc), None if al is None else _ptr(al), kind))
    return sc, al


LEVEL_DTYPE = np.dtype([("peak", "<f4"), ("mean_square", "<f4")])      # vox_tick_level


def level_window(k: int):
    """vox_level_window (host arithmetic): the window of level record k as (first, end) in the utterance's own 16 kHz sample index -- [2560 (k - 1), 2560 k), the 2560
    samples new to the tick that chose id k; record 0 covers the silent left pad alone."""
    a = C.c_int64(); b = C.c_int64()
    check(lib().vox_level_window(int(k), C.byref(a), C.byref(b)))
    return a.value, b.value


def level_db(x, power: bool = False):
    """A level record's field in dB relative to full scale: 20 log10(peak), or with power=True 10 log10(mean_square) (the RMS level); -inf at 0, NaN stays NaN.
    Scalars or arrays."""
    v = np.asarray(x, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = (10.0 if power else 20.0) * np.log10(v)
    return float(out) if out.ndim == 0 else out


def _db_peak(db) -> float:
    """The f32 peak threshold of a dBFS figure (what quiet_ticks compares with)."""
    p = float(np.float32(10.0 ** (float(db) / 20.0)))
    if not (np.isfinite(p) and p > 0.0):
        raise ValueError(f"threshold {db!r} dB is not a finite positive peak in f32")
    return p


def quiet_ticks(levels, db: float = -50.0) -> int:
    """The end-of-speech hint as a pure function (vox_stream_quiet's rule on a list of records): the number of trailing records whose peak < 10^(db / 20); a NaN
    record ends the run."""
    thr = np.float32(_db_peak(db)); n = 0
    for pk in np.asarray(levels["peak"], dtype=np.float32)[::-1]:
        if not pk < thr:
            break
        n += 1
    return n


def stream_id_due(k: int, sample_rate: int = 16000) -> int:
    """The smallest number of pushed samples (at `sample_rate`) at which a live session hands out id k of its utterance: 2560 k + 40 at 16 kHz, by the schedule; at
    another rate the smallest n with stream_schedule_rate(n)[1] > k, found by bisection (the schedule is monotone).  This is when the session KNOWS the id, the only time
    the schedule defines: not where in the audio the word was said."""
    k = int(k)
    if k < 0:
        raise ValueError(f"id index {k}")
    if int(sample_rate) == 16000:
        return 2560 * k + 40
    ids = lambda n: stream_schedule_rate(n, sample_rate)[1]
    lo, hi = 0, max(1, int(sample_rate))      # ids(lo) <= k < ids(hi)
    while ids(hi) <= k:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if ids(mid) > k:
            hi = mid
        else:
            lo = mid
    return hi


def words(ids, scores, tokenizer, sample_rate: int = 16000, alternatives=None, levels=None):
    """The ids a live session handed out (ids[k] = id k of the utterance) and their records (LiveStream.scores()) as words.  Text ids are those >= 1000 (control and
    streaming ids are dropped); a word begins at the first text id and at every text id whose bytes begin with ASCII whitespace, so a character split over two ids stays
    in one word.  -> a list of {text (the word's bytes as lossy UTF-8, its leading whitespace included: the texts joined are the decoded transcript), first_id, last_id
    (indices into ids), due_s (stream_id_due(last_id) / sample_rate: when a session fed at that rate hands the word's last id out), logprob (the sum over its ids),
    min_margin (the smallest margin among them)}.
    alternatives (LiveStream.alternatives(), one record per id): every word also gets entropy (the largest over its ids; NaN when one of them has none) and weakest =
    {k: the index of its smallest-margin id (the first of them), alternatives: that id's list as [{id, text, logprob}]}; text is the tokenizer's bytes for the id as
    lossy UTF-8, "" for control ids and ids past the vocabulary.
    levels (LiveStream.levels(), one record per id): every word also gets peak_db (level_db of the largest peak over its ids) and rms_db (level_db of the mean of its
    ids' mean_square): what the model had just heard while it chose the word's ids, not where the word was spoken; NaN when one of the ids has no record."""
    from .tokenizer import TEXT_TOKEN_OFFSET

    def id_text(t):
        v = t - TEXT_TOKEN_OFFSET
        b = tokenizer.vocab_bytes[v] if 0 <= v < len(tokenizer.vocab_bytes) else None
        return "" if b is None else bytes(b).decode("utf-8", errors="replace")
    out = []; cur = None
    for k, t in enumerate(ids):
        t = int(t)
        if t < TEXT_TOKEN_OFFSET:
            continue
        v = t - TEXT_TOKEN_OFFSET
        b = tokenizer.vocab_bytes[v] if v < len(tokenizer.vocab_bytes) else None
        if b is None:      # a control entry, an id past the vocabulary: VoxtralTokenizer.decode skips them
            continue
        if cur is None or b[:1] in (b" ", b"\t", b"\n", b"\r", b"\x0b", b"\x0c"):
            cur = {"bytes": bytearray(), "first_id": k, "last_id": k, "logprob": 0.0, "min_margin": float("inf"), "weakest": k, "ks": []}; out.append(cur)
        cur["bytes"] += b; cur["last_id"] = k; cur["ks"].append(k)
        cur["logprob"] += float(scores["logprob"][k])
        if float(scores["margin"][k]) < cur["min_margin"]:
            cur["min_margin"] = float(scores["margin"][k]); cur["weakest"] = k
    res = []
    for w in out:
        res.append({"text": bytes(w["bytes"]).decode("utf-8", errors="replace"), "first_id": w["first_id"], "last_id": w["last_id"],
                    "due_s": stream_id_due(w["last_id"], sample_rate) / float(sample_rate), "logprob": w["logprob"], "min_margin": w["min_margin"]})
        if alternatives is not None:
            ent = [float(alternatives["entropy"][k]) for k in w["ks"]]
            rec = alternatives[w["weakest"]]
            res[-1]["entropy"] = float("nan") if any(e != e for e in ent) else max(ent)
            res[-1]["weakest"] = {"k": w["weakest"], "alternatives": [{"id": int(a["id"]), "text": id_text(int(a["id"])), "logprob": float(a["logprob"])}
                                                                      for a in rec["alt"][:int(rec["n"])]]}
        if levels is not None:
            pk = np.asarray([levels["peak"][k] for k in w["ks"]], dtype=np.float64); ms = np.asarray([levels["mean_square"][k] for k in w["ks"]], dtype=np.float64)
            res[-1]["peak_db"] = level_db(pk.max() if not np.isnan(pk).any() else np.nan); res[-1]["rms_db"] = level_db(ms.mean(), power=True)
    return res


def stream_schedule_rate(n_samples: int, sample_rate: int, finished: bool = False):
    """vox_stream_schedule_rate (host arithmetic) for a stream fed at `sample_rate`: (decoder positions determined, ids due, 16 kHz samples the stream holds) after
    `n_samples` pushed, or at the end of an n_samples utterance."""
    p = C.c_int32(); i = C.c_int32(); k = C.c_size_t()
    check(lib().vox_stream_schedule_rate(int(n_samples), int(sample_rate), 1 if finished else 0, C.byref(p), C.byref(i), C.byref(k)))
    return p.value, i.value, k.value


def stream_group_pages_for(positions, page_rows=256, window=8192):
    """vox_stream_group_pages_for (host arithmetic, the allocator's own function): (first logical page, number of pages) a paged group's member holds when its next tick
    is at `positions`; window -1: no sliding window."""
    f = C.c_int32(); n = C.c_int32()
    check(lib().vox_stream_group_pages_for(int(positions), int(page_rows), int(window), C.byref(f), C.byref(n)))
    return f.value, n.value


def stream_schedule(n_samples: int, finished: bool = False, sample_rate: int = 16000):
    """vox_stream_schedule (host arithmetic): (decoder positions determined, ids due) after `n_samples` pushed, or at the end of an n_samples utterance; samples counted
    at `sample_rate`, the rate of the stream (vox_stream_schedule_rate)."""
    if int(sample_rate) != 16000:
        return stream_schedule_rate(n_samples, sample_rate, finished)[:2]
    p = C.c_int32(); i = C.c_int32()
    check(lib().vox_stream_schedule(int(n_samples), 1 if finished else 0, C.byref(p), C.byref(i)))
    return p.value, i.value


def stream_peek_ids(n_samples: int, ids_out: int, sample_rate: int = 16000) -> int:
    """vox_stream_peek_ids (host arithmetic): the ids a peek returns after `n_samples` pushed at `sample_rate` with `ids_out` ids handed out -- the finished schedule's
    count minus those."""
    n = C.c_int32()
    check(lib().vox_stream_peek_ids(int(n_samples), int(sample_rate), int(ids_out), C.byref(n)))
    return n.value


class LiveStream:
    """A live streaming session (vox_stream): push samples in pieces of any size, get token ids back as soon as they are determined; after finish() the
    concatenation equals transcribe_streaming on the log-mel of pad_audio(gain * samples).  One decoder position = 2560 samples = 160 ms at 16 kHz.
    sample_rate: the rate of what is pushed (vox_stream_create_rate); other than 16 kHz the session resamples incrementally and gives the ids of a 16 kHz session
    fed resample(samples).
    endless (vox_stream_create_endless): the session goes on past 16 384 positions, up to 2^24: its decoder cache is a ring of dec_ring_rows rows (0: a little more
    than one window) and max_positions does not apply.
    burst (vox_stream_create_burst; None: a plain stream): 1..16 -- a backlog's ticks run in bursts of up to that many (one encoder pass of 4 b rows, then b decode
    steps); ids equal a plain stream's up to near-ties, and bit for bit when the stream is fed one tick per call.  burst_info() counts the bursts."""

    def __init__(self, model, t_embed, gain=1.0, enc_capacity_rows=0, max_positions=0, sample_rate=16000, endless=False, dec_ring_rows=0, burst=None):
        if burst is not None and (isinstance(burst, bool) or not isinstance(burst, (int, np.integer)) or not 1 <= int(burst) <= STREAM_BURST_MAX):
            raise VoxError(1, f"create_stream: burst {burst!r} is not an integer in 1..{STREAM_BURST_MAX}")
        self.model = model; self.h = C.c_void_p(); self.sample_rate = int(sample_rate); self.endless = bool(endless)
        args = (model.h, _ptr(_f32(t_embed).reshape(-1)), float(gain), int(enc_capacity_rows), int(max_positions))
        if self.endless and max_positions:
            raise VoxError(1, "create_stream: an endless session takes no max_positions")
        if burst is not None:
            if dec_ring_rows and not self.endless:
                raise VoxError(1, "create_stream: dec_ring_rows applies with endless=True")
            check(lib().vox_stream_create_burst(*args, self.sample_rate, int(self.endless), int(dec_ring_rows), int(burst), C.byref(self.h)))
        elif self.endless:
            check(lib().vox_stream_create_endless(*args[:4], int(dec_ring_rows), self.sample_rate, C.byref(self.h)))
        elif dec_ring_rows:
            raise VoxError(1, "create_stream: dec_ring_rows applies with endless=True")
        elif self.sample_rate == 16000:
            check(lib().vox_stream_create(*args, C.byref(self.h)))
        else:
            check(lib().vox_stream_create_rate(*args, self.sample_rate, C.byref(self.h)))
        model._caches.add(self)

    def _ids(self, call, n_new, finished):
        due = stream_schedule(self.info()["samples"] + n_new, finished, self.sample_rate)[1] - self.info()["ids"]
        ids = np.zeros(max(due, 1), dtype=np.int32); n = C.c_int32()
        check(call(_ptr(ids), ids.size, C.byref(n)))
        return ids[:n.value].copy()

    def push(self, samples=None, device_ptr=None, n_samples=None, dtype=None) -> np.ndarray:
        """Append samples at the stream's rate -> the ids that became determined (possibly none).  samples: an int16 array (16-bit PCM, vox_stream_push_s16) or
        anything else as float32; or a device pointer + count, of float32 or, with dtype="s16", of 16-bit PCM."""
        if device_ptr is None:
            s16 = isinstance(samples, np.ndarray) and samples.dtype == np.int16
            x = np.ascontiguousarray(samples).reshape(-1) if s16 else _f32(samples).reshape(-1)
            n_samples = x.size; ptr = _ptr(x) if x.size else None; kind = 0
        else:
            if dtype not in (None, "f32", "s16"):
                raise ValueError(f"dtype {dtype!r}: a device pointer holds 'f32' or 's16' samples")
            s16 = dtype == "s16"; ptr = C.c_void_p(device_ptr); kind = 1
        fn = lib().vox_stream_push_s16 if s16 else lib().vox_stream_push
        return self._ids(lambda o, c, n: fn(self.h, ptr, n_samples, kind, o, c, n), n_samples, False)

    def finish(self) -> np.ndarray:
        """End of the utterance: the right pad is appended, the remaining ids come back."""
        return self._ids(lambda o, c, n: lib().vox_stream_finish(self.h, o, c, n), 0, True)

    def peek(self, return_scores=False):
        """vox_stream_peek: the ids finish() would return now; the session stays what it was and goes on with the next push (or finish).  return_scores: -> (ids, the
        records of those ids as scores() gives them; with scores off: NaN, NaN, -1, id).  The session's own record list is not extended."""
        inf = self.info(); due = stream_peek_ids(inf["samples"], inf["ids"], self.sample_rate)
        ids = np.zeros(max(due, 1), dtype=np.int32); rec = np.zeros(max(due, 1), dtype=SCORE_DTYPE); n = C.c_int32()
        check(lib().vox_stream_peek(self.h, _ptr(ids), ids.size, C.byref(n), _ptr(rec) if return_scores else None))
        return (ids[:n.value].copy(), rec[:n.value].copy()) if return_scores else ids[:n.value].copy()

    def reset(self):
        check(lib().vox_stream_reset(self.h))

    def snapshot(self, device_ptr=None, cap=None):
        """vox_stream_snapshot: the session as one position-independent blob (a numpy uint8 array); the stream stays exactly what it was.  With a device pointer
        (16-byte aligned, cap bytes) the blob is written there and its size is returned."""
        n = C.c_size_t(); check(lib().vox_stream_snapshot_size(self.h, C.byref(n)))
        if device_ptr is not None:
            w = C.c_size_t(); check(lib().vox_stream_snapshot(self.h, C.c_void_p(device_ptr), n.value if cap is None else int(cap), C.byref(w), 1))
            return w.value
        blob = np.zeros(n.value if cap is None else int(cap), dtype=np.uint8); w = C.c_size_t()
        check(lib().vox_stream_snapshot(self.h, _ptr(blob), blob.size, C.byref(w), 0))
        return blob[:w.value]

    def restore(self, blob=None, device_ptr=None, nbytes=None):
        """vox_stream_restore: this stream continues the session of the blob (a numpy uint8 array, or a device pointer + size) in place of its own utterance; a
        refused blob leaves the stream untouched."""
        if device_ptr is not None:
            check(lib().vox_stream_restore(self.h, C.c_void_p(device_ptr), int(nbytes), 1)); return
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        check(lib().vox_stream_restore(self.h, _ptr(blob), blob.size, 0))

    def info(self):
        v = (C.c_int64 * 8)(); check(lib().vox_stream_info(self.h, v))
        return dict(zip(("samples", "positions", "ids", "encoder_position", "ring_rows", "bytes", "engine_steps", "operator_steps"), (int(x) for x in v)))

    def burst_info(self):
        """vox_stream_burst_info: burst_ticks (1: a plain stream), the bursts run with b >= 2, the ticks inside them, the ticks run one by one."""
        v = (C.c_int64 * 4)(); check(lib().vox_stream_burst_info(self.h, v))
        return dict(zip(("burst", "bursts", "burst_ticks", "single_ticks"), (int(x) for x in v)))

    def set_scores(self, on: bool = True):
        """vox_stream_set_scores: from the next push / finish on, every id comes with its record (scores()); survives reset()."""
        check(lib().vox_stream_set_scores(self.h, 1 if on else 0))

    def scores(self, first: int = 0, n=None) -> np.ndarray:
        """vox_stream_scores: the records of ids [first, first + n) of the current utterance (n None: up to the last id handed out) as a structured array (logprob,
        margin, runner_up, id); an id handed out while scores were off has NaN, NaN, -1 and its id.  Reads host memory only."""
        n = self.info()["ids"] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=SCORE_DTYPE)
        check(lib().vox_stream_scores(self.h, int(first), n, _ptr(out) if out.size else None))
        return out

    def set_alternatives(self, k: int):
        """vox_stream_set_alternatives: from the next push / finish / peek on, every id comes with its k best alternatives and the step's entropy (alternatives());
        k = 0: off; survives reset()."""
        check(lib().vox_stream_set_alternatives(self.h, int(k)))

    def alternatives(self, first: int = 0, n=None) -> np.ndarray:
        """vox_stream_alternatives: the records of ids [first, first + n) of the current utterance (n None: up to the last id handed out) as a structured array
        (entropy, n, alt[8] of (id, logprob)); an id handed out while alternatives were off has NaN, 0 and (-1, NaN) throughout.  Reads host memory only."""
        n = self.info()["ids"] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=ALTS_DTYPE)
        check(lib().vox_stream_alternatives(self.h, int(first), n, _ptr(out) if out.size else None))
        return out

    def set_levels(self, on: bool = True):
        """vox_stream_set_levels: from the next push / finish on, every id comes with the level of the 160 ms of audio new to its tick (levels()); survives reset()."""
        check(lib().vox_stream_set_levels(self.h, 1 if on else 0))

    def levels(self, first: int = 0, n=None) -> np.ndarray:
        """vox_stream_levels: the records of ids [first, first + n) of the current utterance (n None: up to the last id handed out) as a structured array (peak,
        mean_square) of the window level_window(k), taken on gain * sample as the front end reads it; an id handed out while levels were off has (NaN, NaN).  Refused
        while levels are off.  Reads host memory only."""
        n = self.info()["ids"] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=LEVEL_DTYPE)
        check(lib().vox_stream_levels(self.h, int(first), n, _ptr(out) if out.size else None))
        return out

    def quiet_ticks(self, db: float = -50.0) -> int:
        """vox_stream_quiet, the end-of-speech hint: how many of the last ids handed out had a window whose peak lies below `db` dBFS (of the gained samples); times
        160 ms: the quiet time as of the last id.  A NaN record ends the run.  Reads host memory only."""
        t = C.c_int32(); check(lib().vox_stream_quiet(self.h, _db_peak(db), C.byref(t)))
        return t.value

    def peeked_alternatives(self) -> np.ndarray:
        """vox_stream_peeked_alternatives: the records of the ids the last peek() returned; empty once a push / finish / peek / reset has followed it."""
        cap = max(stream_peek_ids(self.info()["samples"], 0, self.sample_rate), 1)      # (no peek returns more ids than the whole utterance has)
        out = np.zeros(cap, dtype=ALTS_DTYPE); n = C.c_int32()
        check(lib().vox_stream_peeked_alternatives(self.h, _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def tap_arm(self, max_rows):
        check(lib().vox_debug_stream_tap_arm(self.h, int(max_rows))); self._tap_max = int(max_rows)

    def tap_fetch(self):
        """The f32 logits rows behind the ids handed out since tap_arm: [rows][vocab]."""
        buf = np.zeros((self._tap_max, self.model.config.vocab), dtype=np.float32); rows = C.c_int32()
        check(lib().vox_debug_stream_tap_fetch(self.h, _ptr(buf), C.byref(rows)))
        if rows.value > self._tap_max:
            raise VoxError(1, f"stream tap: {rows.value} rows for a tap of {self._tap_max}")
        return buf[:rows.value].copy()

    def tap_peeked(self, rows):
        """vox_debug_stream_tap_peeked: the logits rows behind the ids of the last peek(), [rows][vocab]; the tap goes on."""
        buf = np.zeros((int(rows), self.model.config.vocab), dtype=np.float32)
        check(lib().vox_debug_stream_tap_peeked(self.h, _ptr(buf), int(rows)))
        return buf

    def front_tap_arm(self, max_ticks):
        check(lib().vox_debug_stream_front_tap_arm(self.h, int(max_ticks))); self._ftap_max = int(max_ticks)

    def front_tap_fetch(self):
        """vox_debug_stream_front_tap_fetch: (log-mel [ticks][16][n_mels], conv-stem rows [ticks][4][enc_dim]) of the ticks run since front_tap_arm."""
        c = self.model.config; R = c.reshape_factor
        mel = np.zeros((self._ftap_max, 4 * R, c.n_mels), dtype=np.float32); conv = np.zeros((self._ftap_max, R, c.enc_dim), dtype=np.float32); ticks = C.c_int32()
        check(lib().vox_debug_stream_front_tap_fetch(self.h, _ptr(mel), _ptr(conv), C.byref(ticks)))
        if ticks.value > self._ftap_max:
            raise VoxError(1, f"stream front tap: {ticks.value} ticks for a tap of {self._ftap_max}")
        return mel[:ticks.value].copy(), conv[:ticks.value].copy()

    def close(self):
        if self.h:
            lib().vox_stream_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LiveStreamGroup:
    """A stream group (vox_stream_group): up to 16 live sessions on one model advanced together, every weight matrix read once per tick for all members that have a tick
    due.  Members are numbered 0 .. n_members-1; each has its own gain and its own sample rate (sample_rates, reset(sample_rate=); 16 kHz unless set) and follows
    stream_schedule(..., sample_rate=its rate) on its own sample count.  Samples are float32 or 16-bit PCM at the member's rate."""
    _rates = None      # {member: rate} of the members at another rate than 16 kHz; a member without an entry is fed 16 kHz

    KV_DTYPES = {"f32": 0, "bf16": 1}      # VOX_KV_F32, VOX_KV_BF16

    def __init__(self, model, t_embed, n_members, gains=None, enc_capacity_rows=0, max_positions=0, sample_rates=None, page_rows=None, pool_pages=None, endless=False,
                 kv_dtype=None, burst=None, t_embeds=None):
        if burst is not None and (isinstance(burst, bool) or not isinstance(burst, (int, np.integer)) or not 1 <= int(burst) <= STREAM_BURST_MAX):
            raise VoxError(1, f"create_stream_group: burst {burst!r} is not an integer in 1..{STREAM_BURST_MAX}")
        self.model = model; self.h = C.c_void_p(); self.n_members = int(n_members); self._tap_max = {}; self._rates = {}
        self.burst = None if burst is None else int(burst)      # given: a burst group (vox_stream_group_create_burst) of whatever kind the other arguments make
        if kv_dtype is not None and kv_dtype not in self.KV_DTYPES:
            raise ValueError(f"kv_dtype {kv_dtype!r}: a stream group's K/V pool holds 'f32' or 'bf16'")
        self.kv_dtype = kv_dtype      # given: a paged group made by vox_stream_group_create_kv, whose pool() names the dtype; None: the group the other arguments make
        self.endless = bool(endless)      # an endless paged group (vox_stream_group_create_endless): no max_positions, every member goes on to 2^24 positions
        if self.endless and max_positions:
            raise ValueError(f"an endless stream group has no max_positions (got {max_positions}): every member may go on to 2^24 positions")
        self.paged = self.endless or page_rows is not None or pool_pages is not None or kv_dtype is not None      # either one given: a paged group (vox_stream_group_create_paged; 0 / None: its default)
        g = None if gains is None else _f32(gains).reshape(-1)
        if g is not None and g.size != self.n_members:
            raise ValueError(f"{g.size} gains for {self.n_members} members")
        self.per_member = t_embeds is not None      # a delay per member (vox_stream_group_create_t_embeds): t_embeds [n_members][dec_dim], t_embed unread
        if self.per_member:
            te = _f32(t_embeds)
            if te.ndim != 2 or te.shape[0] != self.n_members:
                raise ValueError(f"t_embeds of shape {tuple(te.shape)} for {self.n_members} members: one row per member")
            r = np.ascontiguousarray([int(v) for v in (sample_rates if sample_rates is not None else [16000] * self.n_members)], dtype=np.uint32)
            if r.size != self.n_members:
                raise ValueError(f"{r.size} sample rates for {self.n_members} members")
            check(lib().vox_stream_group_create_t_embeds(model.h, _ptr(te), self.n_members, None if g is None else _ptr(g), _ptr(r), int(enc_capacity_rows), int(max_positions),
                                                         int(self.paged), int(page_rows or 0), int(pool_pages or 0), int(self.endless), self.KV_DTYPES[kv_dtype or "f32"],
                                                         int(burst or 1), C.byref(self.h)))
            self._rates = {k: int(v) for k, v in enumerate(r) if int(v) != 16000}
            model._caches.add(self)
            return
        args = (model.h, _ptr(_f32(t_embed).reshape(-1)), self.n_members, None if g is None else _ptr(g))
        if burst is not None:
            r = np.ascontiguousarray([int(v) for v in (sample_rates if sample_rates is not None else [16000] * self.n_members)], dtype=np.uint32)
            if r.size != self.n_members:
                raise ValueError(f"{r.size} sample rates for {self.n_members} members")
            check(lib().vox_stream_group_create_burst(*args, _ptr(r), int(enc_capacity_rows), int(max_positions), int(self.paged), int(page_rows or 0), int(pool_pages or 0),
                                                      int(self.endless), self.KV_DTYPES[kv_dtype or "f32"], int(burst), C.byref(self.h)))
            self._rates = {k: int(v) for k, v in enumerate(r) if int(v) != 16000}
        elif sample_rates is None and not self.paged:
            check(lib().vox_stream_group_create(*args, int(enc_capacity_rows), int(max_positions), C.byref(self.h)))
        else:
            r = np.ascontiguousarray([int(v) for v in (sample_rates if sample_rates is not None else [16000] * self.n_members)], dtype=np.uint32)
            if r.size != self.n_members:
                raise ValueError(f"{r.size} sample rates for {self.n_members} members")
            if kv_dtype is not None:
                check(lib().vox_stream_group_create_kv(*args, _ptr(r), int(enc_capacity_rows), int(max_positions), int(page_rows or 0), int(pool_pages or 0), int(self.endless),
                                                       self.KV_DTYPES[kv_dtype], C.byref(self.h)))
            elif self.endless:
                check(lib().vox_stream_group_create_endless(*args, _ptr(r), int(enc_capacity_rows), int(page_rows or 0), int(pool_pages or 0), C.byref(self.h)))
            elif self.paged:
                check(lib().vox_stream_group_create_paged(*args, _ptr(r), int(enc_capacity_rows), int(max_positions), int(page_rows or 0), int(pool_pages or 0), C.byref(self.h)))
            else:
                check(lib().vox_stream_group_create_rates(*args, _ptr(r), int(enc_capacity_rows), int(max_positions), C.byref(self.h)))
            self._rates = {k: int(v) for k, v in enumerate(r) if int(v) != 16000}
        model._caches.add(self)

    def sample_rate(self, member) -> int:
        """The rate of what `member` is fed."""
        return (self._rates or {}).get(int(member), 16000)

    def advance(self, feeds, finish=(), device=False, dtype=None) -> dict:
        """One call for any subset of members: feeds {member: samples at the member's rate} (arrays; device=True: {member: (device pointer, count)} of float32 or, with
        dtype="s16", of 16-bit PCM), finish: the members whose utterance ends with these samples (a member named there alone is fed no samples) -> {member: the ids that
        became due}.  Host arrays: when every fed array is int16 the call is the 16-bit one (vox_stream_group_advance_s16); anything else goes in as float32, int16
        arrays of a mixed call as v / 32768 (exact)."""
        if dtype not in (None, "f32", "s16") or (dtype is not None and not device):
            raise ValueError(f"dtype {dtype!r}: a device pointer holds 'f32' or 's16' samples")
        fin = set(int(k) for k in finish); entries = {int(k): v for k, v in feeds.items()}
        is16 = lambda v: isinstance(v, np.ndarray) and v.dtype == np.int16
        s16 = dtype == "s16" if device else bool(entries) and all(is16(v) for v in entries.values())
        for k in fin:
            entries.setdefault(k, (0, 0) if device else np.zeros(0, np.int16 if s16 else np.float32))
        arr = (_lib.StreamFeed * max(len(entries), 1))(); keep = []
        for e, (k, v) in zip(arr, entries.items()):
            if device:
                ptr, n = int(v[0]) or None, int(v[1])
            else:
                if s16:
                    x = np.ascontiguousarray(v).reshape(-1)
                else:
                    x = (v.astype(np.float32) / np.float32(32768) if is16(v) else _f32(v)).reshape(-1)
                keep.append(x); ptr, n = (x.ctypes.data if x.size else None), x.size
            if not 0 <= k < self.n_members:
                raise ValueError(f"member {k} of a group of {self.n_members}")
            inf = self.info(k)
            due = stream_schedule(inf["samples"] + n, k in fin, self.sample_rate(k))[1] - inf["ids"]      # each cap comes from the member's schedule
            ids = np.zeros(max(due, 1), dtype=np.int32); keep.append(ids)
            e.member = k; e.finish = 1 if k in fin else 0; e.samples = ptr; e.n_samples = n; e.out_ids = ids.ctypes.data; e.cap = ids.size; e.n_ids = 0
        fn = lib().vox_stream_group_advance_s16 if s16 else lib().vox_stream_group_advance
        check(fn(self.h, arr, len(entries), 1 if device else 0))
        out = {}
        for e in arr[:len(entries)]:
            out[e.member] = np.ctypeslib.as_array((C.c_int32 * max(e.cap, 1)).from_address(e.out_ids))[:e.n_ids].copy()
        return out

    def peek(self, members, return_scores=False) -> dict:
        """vox_stream_group_peek: {member: the ids advance(finish=[member]) would hand it now} for every member named, in one call; the group stays what it was.
        return_scores: {member: (ids, records)} as LiveStream.peek."""
        ms = [int(k) for k in members]
        arr = (_lib.StreamFeed * max(len(ms), 1))(); keep = []; recs = []
        for e, k in zip(arr, ms):
            if not 0 <= k < self.n_members:
                raise ValueError(f"member {k} of a group of {self.n_members}")
            inf = self.info(k); due = max(stream_peek_ids(inf["samples"], inf["ids"], self.sample_rate(k)), 1)
            ids = np.zeros(due, dtype=np.int32); keep.append(ids); recs.append(np.zeros(due, dtype=SCORE_DTYPE))
            e.member = k; e.finish = 0; e.samples = None; e.n_samples = 0; e.out_ids = ids.ctypes.data; e.cap = ids.size; e.n_ids = 0
        ptrs = (C.c_void_p * max(len(ms), 1))(*[r.ctypes.data for r in recs])
        check(lib().vox_stream_group_peek(self.h, arr, len(ms), ptrs if return_scores else None))
        out = {}
        for e, ids, rec in zip(arr, keep, recs):
            out[e.member] = (ids[:e.n_ids].copy(), rec[:e.n_ids].copy()) if return_scores else ids[:e.n_ids].copy()
        return out

    def reset(self, member, gain=1.0, sample_rate=None, delay=None, t_embed=None):
        """The member's next connection; sample_rate: what it delivers (None: the member keeps its rate).  delay / t_embed (one of them; a group made with t_embeds= or
        delays= alone): the delay its next utterance runs at (vox_stream_group_reset_t_embed); a refused call leaves the member as it was."""
        if delay is not None and t_embed is not None:
            raise ValueError("reset: delay and t_embed name the same thing, give one")
        if delay is not None:
            from .audio import TimeEmbedding
            t_embed = TimeEmbedding(self.model.config.dec_dim).embed(float(delay))
        if t_embed is not None:
            te = _f32(t_embed).reshape(-1)
            if te.size != self.model.config.dec_dim:
                raise ValueError(f"a t_embed of {te.size} values for a model of dec_dim {self.model.config.dec_dim}")
            check(lib().vox_stream_group_reset_t_embed(self.h, int(member), float(gain), int(sample_rate or 0), _ptr(te)))
            if sample_rate is None:
                return
        elif sample_rate is None:
            check(lib().vox_stream_group_reset(self.h, int(member), float(gain)))
            return
        else:
            check(lib().vox_stream_group_reset_rate(self.h, int(member), float(gain), int(sample_rate)))
        rates = dict(self._rates or {}); rates.pop(int(member), None)
        if int(sample_rate) != 16000:
            rates[int(member)] = int(sample_rate)
        self._rates = rates

    def t_embed(self, member) -> np.ndarray:
        """vox_stream_group_t_embed: the t_embed the member runs at (every group: a group of one delay returns that one for every member)."""
        out = np.zeros(self.model.config.dec_dim, dtype=np.float32)
        check(lib().vox_stream_group_t_embed(self.h, int(member), _ptr(out), out.size))
        return out

    def snapshot(self, member) -> np.ndarray:
        """vox_stream_group_snapshot: the member's session as one blob (LiveStream.snapshot); the group stays exactly what it was."""
        n = C.c_size_t(); check(lib().vox_stream_group_snapshot_size(self.h, int(member), C.byref(n)))
        blob = np.zeros(n.value, dtype=np.uint8); w = C.c_size_t()
        check(lib().vox_stream_group_snapshot(self.h, int(member), _ptr(blob), blob.size, C.byref(w), 0))
        return blob[:w.value]

    def restore(self, member, blob):
        """vox_stream_group_restore: the member continues the session of the blob -- a member's or a solo stream's -- at the blob's rate and gain; a refused blob
        leaves the group untouched."""
        blob = np.ascontiguousarray(blob, dtype=np.uint8).reshape(-1)
        check(lib().vox_stream_group_restore(self.h, int(member), _ptr(blob), blob.size, 0))
        rates = dict(self._rates or {}); rates.pop(int(member), None); sr = snapshot_info(blob)["sample_rate"]
        if sr != 16000:
            rates[int(member)] = sr
        self._rates = rates

    def info(self, member):
        v = (C.c_int64 * 8)(); check(lib().vox_stream_group_info(self.h, int(member), v))
        return dict(zip(("samples", "positions", "ids", "encoder_position", "ring_rows", "bytes", "engine_steps", "operator_steps"), (int(x) for x in v)))

    def burst_info(self):
        """vox_stream_group_burst_info: burst_ticks (1: a plain group), the burst rounds run (rounds in which some member ran 2 or more ticks), the member-ticks inside
        them, the plain rounds run -- since create; a peek's rounds are not counted."""
        v = (C.c_int64 * 4)(); check(lib().vox_stream_group_burst_info(self.h, v))
        return dict(zip(("burst", "burst_rounds", "burst_member_ticks", "plain_rounds"), (int(x) for x in v)))

    def pool(self) -> dict:
        """vox_stream_group_pool of a paged group: page_rows, pool_pages, the free pages, the most pages ever in use, and held: the pages each member holds."""
        v = (C.c_int64 * 4)(); held = np.zeros(self.n_members, dtype=np.int32)
        check(lib().vox_stream_group_pool(self.h, v, _ptr(held)))
        out = {"page_rows": int(v[0]), "pool_pages": int(v[1]), "free": int(v[2]), "peak": int(v[3]), "held": [int(x) for x in held]}
        if self.kv_dtype is not None:      # (a group made with kv_dtype= alone: the dicts of every other group are what they were)
            out["kv_dtype"] = self.kv_dtype
        return out

    def pages(self, member) -> list:
        """vox_debug_stream_group_pages: the member's physical pages, in the order of its logical pages."""
        n = C.c_int32(); check(lib().vox_debug_stream_group_pages(self.h, int(member), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int32)
        check(lib().vox_debug_stream_group_pages(self.h, int(member), _ptr(out), out.size, C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def set_scores(self, member, on: bool = True):
        """vox_stream_group_set_scores: LiveStream.set_scores for one member; survives the member's resets."""
        check(lib().vox_stream_group_set_scores(self.h, int(member), 1 if on else 0))

    def scores(self, member, first: int = 0, n=None) -> np.ndarray:
        """vox_stream_group_scores: LiveStream.scores for one member."""
        n = self.info(member)["ids"] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=SCORE_DTYPE)
        check(lib().vox_stream_group_scores(self.h, int(member), int(first), n, _ptr(out) if out.size else None))
        return out

    def set_alternatives(self, member, k: int):
        """vox_stream_group_set_alternatives: LiveStream.set_alternatives for one member; survives the member's resets."""
        check(lib().vox_stream_group_set_alternatives(self.h, int(member), int(k)))

    def alternatives(self, member, first: int = 0, n=None) -> np.ndarray:
        """vox_stream_group_alternatives: LiveStream.alternatives for one member."""
        n = self.info(member)["ids"] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=ALTS_DTYPE)
        check(lib().vox_stream_group_alternatives(self.h, int(member), int(first), n, _ptr(out) if out.size else None))
        return out

    def set_levels(self, member, on: bool = True):
        """vox_stream_group_set_levels: LiveStream.set_levels for one member; survives the member's resets."""
        check(lib().vox_stream_group_set_levels(self.h, int(member), 1 if on else 0))

    def levels(self, member, first: int = 0, n=None) -> np.ndarray:
        """vox_stream_group_levels: LiveStream.levels for one member -- the bits a solo stream fed the same samples at the same gain has."""
        n = self.info(member)["ids"] - int(first) if n is None else int(n)
        out = np.zeros(max(n, 0), dtype=LEVEL_DTYPE)
        check(lib().vox_stream_group_levels(self.h, int(member), int(first), n, _ptr(out) if out.size else None))
        return out

    def quiet_ticks(self, member, db: float = -50.0) -> int:
        """vox_stream_group_quiet: LiveStream.quiet_ticks for one member."""
        t = C.c_int32(); check(lib().vox_stream_group_quiet(self.h, int(member), _db_peak(db), C.byref(t)))
        return t.value

    def peeked_alternatives(self, member) -> np.ndarray:
        """vox_stream_group_peeked_alternatives: LiveStream.peeked_alternatives for one member."""
        cap = max(stream_peek_ids(self.info(member)["samples"], 0, self.sample_rate(member)), 1)
        out = np.zeros(cap, dtype=ALTS_DTYPE); n = C.c_int32()
        check(lib().vox_stream_group_peeked_alternatives(self.h, int(member), _ptr(out), cap, C.byref(n)))
        return out[:n.value].copy()

    def tap_arm(self, member, max_rows):
        check(lib().vox_debug_stream_group_tap_arm(self.h, int(member), int(max_rows))); self._tap_max[int(member)] = int(max_rows)

    def tap_fetch(self, member):
        """The f32 logits rows behind the ids handed to `member` since tap_arm: [rows][vocab]."""
        mx = self._tap_max[int(member)]
        buf = np.zeros((mx, self.model.config.vocab), dtype=np.float32); rows = C.c_int32()
        check(lib().vox_debug_stream_group_tap_fetch(self.h, int(member), _ptr(buf), C.byref(rows)))
        if rows.value > mx:
            raise VoxError(1, f"stream group tap: {rows.value} rows for a tap of {mx}")
        return buf[:rows.value].copy()

    def close(self):
        if self.h:
            lib().vox_stream_group_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Q4VoxtralModel:
    """gguf/model.rs:759-989"""

    def __init__(self, ctx, h):
        self.ctx, self.h = ctx, h
        self._caches = weakref.WeakSet()
        self.config = _lib.ModelCfg(); check(lib().vox_model_config(h, C.byref(self.config)))

    def decoder(self):
        return Q4LanguageModel(self)

    def create_decoder_cache_preallocated(self, max_seq):
        return LayerCaches(self, max_seq)

    def generate_step_with_cache(self, token_ids, t_embed, caches):
        """gguf/model.rs:857-867: logits [n][vocab] of the text tokens `token_ids` against the decoder cache (which advances by n)."""
        ids = np.ascontiguousarray(token_ids, dtype=np.int32).reshape(-1)
        out = np.empty((ids.size, self.config.vocab), dtype=np.float32)
        check(lib().vox_generate_step_with_cache(self.h, _ptr(ids), ids.size, _ptr(_f32(t_embed).reshape(-1)), caches.h, _ptr(out)))
        return out

    def _mel2(self, mel):
        mel = _f32(mel); return mel.reshape(mel.shape[-2], mel.shape[-1])

    def forward(self, mel, t_embed):
        """gguf/model.rs:820-830: mel -> logits [1, S, vocab], the audio embeddings alone as decoder input."""
        mel = self._mel2(mel); T = mel.shape[1]; cap = T // 16 + 2
        out = np.empty((cap, self.config.vocab), dtype=np.float32); S = C.c_int32()
        check(lib().vox_forward(self.h, _ptr(mel), T, _ptr(_f32(t_embed).reshape(-1)), _ptr(out), cap, C.byref(S), 0))
        return out[:S.value][None].copy()

    def forward_streaming(self, mel, token_ids, t_embed):
        """gguf/model.rs:802-816: mel + one token id per audio position -> logits [1, S, vocab]."""
        mel = self._mel2(mel); T = mel.shape[1]; cap = T // 16 + 2
        ids = np.ascontiguousarray(token_ids, dtype=np.int32).reshape(-1)
        out = np.empty((cap, self.config.vocab), dtype=np.float32); S = C.c_int32()
        check(lib().vox_forward_streaming(self.h, _ptr(mel), T, _ptr(ids), ids.size, _ptr(_f32(t_embed).reshape(-1)), _ptr(out), cap, C.byref(S), 0))
        return out[:S.value][None].copy()

    def forward_with_cache(self, mel, t_embed, encoder_cache, decoder_cache):
        """gguf/model.rs:833-843: one chunk through the streaming encoder and the cached decoder -> logits [1, S_chunk, vocab]."""
        mel = self._mel2(mel); T = mel.shape[1]; cap = T // 16 + 2
        out = np.empty((cap, self.config.vocab), dtype=np.float32); S = C.c_int32()
        check(lib().vox_forward_with_cache(self.h, _ptr(mel), T, _ptr(_f32(t_embed).reshape(-1)), encoder_cache.h, decoder_cache.h, _ptr(out), cap, C.byref(S), 0))
        return out[:S.value][None].copy()

    def set_decode_engine(self, on: bool) -> bool:
        """Persistent decode-step engine (one launch per token) on / off; returns whether it is active (it needs the real decoder geometry on a 256-CU device)."""
        a = C.c_int32(); check(lib().vox_model_set_decode_engine(self.h, 1 if on else 0, C.byref(a))); return bool(a.value)

    def set_prefix_cache(self, on=None) -> bool:
        """Prefix state of transcribe_audio (what the silent left pad makes identical for every utterance, computed once per model) on / off (None: query); returns
        whether it is in use.  Off = the full computation for every call."""
        a = C.c_int32(); check(lib().vox_model_set_prefix_cache(self.h, -1 if on is None else (1 if on else 0), C.byref(a))); return bool(a.value)

    def prefix_info(self):
        """The prefix state: built yet, encoder rows and decoder positions it covers, device bytes it holds."""
        v = (C.c_int32 * 4)(); check(lib().vox_model_prefix_info(self.h, v)); return {"built": bool(v[0]), "encoder_rows": v[1], "decoder_positions": v[2], "bytes": v[3]}

    def memory(self):
        """Device bytes: weight arena, its primary (broadcast) part, the decode engines' weight stream, the engines' edge buffers."""
        v = (C.c_uint64 * 4)(); check(lib().vox_model_memory(self.h, v)); return {"arena": v[0], "arena_primary": v[1], "engine_stream": v[2], "engine_state": v[3]}

    def set_batch_engine(self, on=None):
        """Batched decode-layer engine (one launch per 16-row group and step) on / off (None: query); returns (active, engine launches enqueued so far)."""
        a = C.c_int32(); n = C.c_uint64()
        check(lib().vox_model_set_batch_engine(self.h, -1 if on is None else (1 if on else 0), C.byref(a), C.byref(n))); return bool(a.value), int(n.value)

    def weight_bytes(self):
        v = C.c_uint64(); check(lib().vox_model_weight_bytes(self.h, C.byref(v))); return v.value

    def arena(self):
        p = C.c_void_p(); n = C.c_uint64(); check(lib().vox_model_arena(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def replicate(self, dst_ctx):
        """vox_model_replicate: one more replica of this Q4 model on `dst_ctx` (another GPU or the same one) -- layout from the tensor manifest, one device-to-device
        copy of the primary arena, derived copies rebuilt there; no file, no collective library."""
        h = C.c_void_p(); check(lib().vox_model_replicate(self.h, dst_ctx.h, C.byref(h)))
        return type(self)(dst_ctx, h)

    def set_sessions(self, sessions: int):
        """vox_model_set_sessions: batch calls with >= 128 units per session run as `sessions` concurrent sessions on this model's GPU (hidden contexts + replicas +
        library threads); 1 = off (replicas freed).  Same ids per unit."""
        check(lib().vox_model_set_sessions(self.h, int(sessions)))

    def arena_finalize(self):
        """Receiver side of the multi-GPU start-up: the bytes of arena() have been written (e.g. by an RCCL broadcast); rebuild the derived copies on this GPU."""
        check(lib().vox_model_arena_finalize(self.h))

    def encode_audio(self, mel):
        """mel [1,128,T] or [128,T] -> [1,S,dec_dim] (gguf/model.rs:783-788)"""
        mel = _f32(mel); mel = mel.reshape(mel.shape[-2], mel.shape[-1]); T = mel.shape[1]
        cap = T // 16 + 2
        out = np.empty((cap, self.config.dec_dim), dtype=np.float32); S = C.c_int32()
        check(lib().vox_encode_audio(self.h, _ptr(mel), T, _ptr(out), cap, C.byref(S), 0))
        return out[:S.value].reshape(1, S.value, self.config.dec_dim).copy()

    def debug_encode_batch(self, mels, layout):
        """vox_debug_encode_batch: log-mels [128,T_i] as ONE encoder stack, the way the batch drivers run it (layout 0 padded = lock-step, 1 packed = continuous)
        -> (list of [S4_i, dec_dim] adapter rows, form report {Mtot, ksp, ksp_wo, fused_rope})"""
        arrs = [_f32(x) for x in mels]; arrs = [np.ascontiguousarray(a.reshape(a.shape[-2], a.shape[-1])) for a in arrs]; n = len(arrs)
        Ts = [a.shape[1] for a in arrs]
        cap = sum(T // 16 + 2 for T in Ts)
        D = self.config.dec_dim
        out = np.zeros((cap, D), dtype=np.float32); rows = (C.c_int32 * max(n, 1))(); rep = (C.c_int64 * 4)()
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs])
        check(lib().vox_debug_encode_batch(self.h, n, ptrs, (C.c_int32 * max(n, 1))(*Ts), layout, _ptr(out), cap, rows, rep))
        res, o = [], 0
        for i in range(n):
            res.append(out[o:o + rows[i]].copy()); o += rows[i]
        return res, {"Mtot": rep[0], "ksp": rep[1], "ksp_wo": rep[2], "fused_rope": rep[3]}

    def debug_front_end(self, samples_list, form, norm_group=None, device_ptrs=None, n_samples=None):
        """vox_debug_front_end: the sample front end of the single clip (form 0: one unit) or of the batch drivers (form 1) on its own, for float32 sample arrays (or
        device pointers + lengths) -> (scales [n] f32, list of log-mels [128, T_i] as the encoder receives them)."""
        from .audio import PadConfig
        if device_ptrs is None:
            arrs = [_f32(x).reshape(-1) for x in samples_list]; n = len(arrs)
            ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrs]); lens = [a.size for a in arrs]; kind = 0
        else:
            n = len(device_ptrs); ptrs = (C.c_void_p * max(n, 1))(*device_ptrs); lens = [int(v) for v in n_samples]; kind = 1
        pc = PadConfig.voxtral()
        Ts = [pc.padded_len(v) // 160 for v in lens]
        mels = [np.full((128, T), np.nan, dtype=np.float32) for T in Ts]
        mptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in mels]); scales = np.full(n, np.nan, dtype=np.float32); out_T = (C.c_int32 * max(n, 1))()
        grp = None if norm_group is None else (C.c_int32 * max(n, 1))(*[int(g) for g in norm_group])
        check(lib().vox_debug_front_end(self.h, n, ptrs, (C.c_size_t * max(n, 1))(*lens), grp, int(form), kind, _ptr(scales), mptrs, out_T))
        if [out_T[i] for i in range(n)] != Ts:
            raise VoxError(1, f"front end: frame counts {[out_T[i] for i in range(n)]}, expected {Ts}")
        return scales, mels

    def create_encoder_cache(self, capacity_rows=0):
        return EncoderCaches(self, capacity_rows)

    def encode_audio_with_cache(self, mel, encoder_cache):
        """mel chunk [1,128,T] or [128,T] -> [1, floor(S_chunk/4), dec_dim] (gguf/model.rs:791-799); K / V appended to `encoder_cache`"""
        mel = _f32(mel); mel = mel.reshape(mel.shape[-2], mel.shape[-1]); T = mel.shape[1]
        cap = T // 16 + 2
        out = np.empty((cap, self.config.dec_dim), dtype=np.float32); S = C.c_int32()
        check(lib().vox_encode_audio_with_cache(self.h, _ptr(mel), T, encoder_cache.h, _ptr(out), cap, C.byref(S), 0))
        return out[:S.value].reshape(1, S.value, self.config.dec_dim).copy()

    def transcribe_streaming(self, mel, t_embed, return_logits=False):
        """-> ids of length max(S-38, 1) for S >= 38 decoder positions, empty below (gguf/model.rs:873-963)"""
        mel = _f32(mel); mel = mel.reshape(mel.shape[-2], mel.shape[-1]); T = mel.shape[1]
        cap = T // 16 + 2
        ids = np.zeros(cap, dtype=np.int32); n = C.c_int32()
        t = _f32(t_embed).reshape(-1)
        lg = np.empty((cap, self.config.vocab), dtype=np.float32) if return_logits else None
        check(lib().vox_transcribe_streaming(self.h, _ptr(mel), T, _ptr(t), _ptr(ids), cap, C.byref(n),
                                             None if lg is None else _ptr(lg), 0))
        if return_logits:
            return ids[:n.value].copy(), lg[:n.value].copy()
        return ids[:n.value].copy()

    def transcribe_audio(self, samples, t_embed, device_ptr=None, n_samples=None):
        """Whole path from 16 kHz samples (peak-normalise, pad, mel, encode, decode)."""
        t = _f32(t_embed).reshape(-1)
        if device_ptr is None:
            x = _f32(samples); n_samples = x.size; ptr = _ptr(x); kind = 0
        else:
            ptr = C.c_void_p(device_ptr); kind = 1
        cap = n_samples // 1280 + 128
        ids = np.zeros(cap, dtype=np.int32); n = C.c_int32()
        check(lib().vox_transcribe_audio(self.h, ptr, n_samples, _ptr(t), _ptr(ids), cap, C.byref(n), kind))
        return ids[:n.value].copy()

    def transcribe_audio_scored(self, samples, t_embed, alternatives=0, device_ptr=None, n_samples=None):
        """transcribe_audio with a record per id (vox_transcribe_audio_scored) -> (ids, scores, alts): scores[j] / alts[j] are score_rows / alternatives_rows of the f32
        logits row ids[j] was the argmax of, as SCORE_DTYPE / ALTS_DTYPE arrays; alternatives = 0: scores alone, alts is None; 1..8: that many alternatives per id."""
        t = _f32(t_embed).reshape(-1)
        if device_ptr is None:
            x = _f32(samples); n_samples = x.size; ptr = _ptr(x); kind = 0
        else:
            ptr = C.c_void_p(device_ptr); kind = 1
        k = int(alternatives)
        cap = n_samples // 1280 + 128
        ids = np.zeros(cap, dtype=np.int32); n = C.c_int32()
        sc = np.zeros(cap, dtype=SCORE_DTYPE); al = np.zeros(cap, dtype=ALTS_DTYPE) if k != 0 else None
        check(lib().vox_transcribe_audio_scored(self.h, ptr, n_samples, _ptr(t), _ptr(ids), cap, C.byref(n), _ptr(sc), None if al is None else _ptr(al), k, kind))
        return ids[:n.value].copy(), sc[:n.value].copy(), None if al is None else al[:n.value].copy()

    def create_stream(self, t_embed, gain=1.0, enc_capacity_rows=0, max_positions=0, sample_rate=16000, endless=False, dec_ring_rows=0, burst=None) -> LiveStream:
        """A live session on this model (vox_stream_create / vox_stream_create_rate): push(x) -> ids, finish(), reset(), info(), close().  gain multiplies every sample
        (a stream has no file peak: 0.95 / max|x| of a known file reproduces transcribe_audio).  sample_rate: the rate of the samples that will be pushed.
        endless (vox_stream_create_endless): no 16 384-position limit -- the decoder cache is a ring of dec_ring_rows rows (0: the default, a little more than one window).
        burst (vox_stream_create_burst): 1..16 -- a backlog's ticks run in bursts of up to that many; None: a plain stream."""
        return LiveStream(self, t_embed, gain, enc_capacity_rows, max_positions, sample_rate, endless, dec_ring_rows, burst)

    def create_stream_group(self, t_embed, n_members, gains=None, enc_capacity_rows=0, max_positions=0, sample_rates=None, page_rows=None, pool_pages=None,
                            endless=False, kv_dtype=None, burst=None, t_embeds=None, delays=None) -> LiveStreamGroup:
        """Up to 16 live sessions advanced together (vox_stream_group_create): advance({member: samples}, finish=()) -> {member: ids}, reset(member, gain), info(member),
        close().  gains: one per member (None: 1.0 each); max_positions 0: 2048 decoder positions per member (the group's decoder cache does not grow);
        sample_rates: what each member is fed (None: 16 kHz each; vox_stream_group_create_rates).
        page_rows / pool_pages, either one given: a PAGED group (vox_stream_group_create_paged) -- one pool of pool_pages K / V pages of page_rows rows (0 / None: 256 rows;
        the default slab's memory) that the members grow into and return pages to; max_positions 0 is then the session limit; pool(), pages(member).
        endless (vox_stream_group_create_endless): a paged group (page_rows / pool_pages as above, both optional) whose members are not refused at 16 384 positions
        but go on to 2^24; max_positions must not be given (ValueError).  Everything of a paged group works unchanged.
        kv_dtype "f32" | "bf16" (vox_stream_group_create_kv; implies paged, as endless does; anything else: ValueError): what the K / V pool holds.  "bf16": 16-bit
        pages, half the memory and half the bytes the decode attention reads; ids and logits are close to, not equal to, the f32 group's.  pool() then names it.
        t_embeds [n_members][dec_dim] or delays [n_members] (through TimeEmbedding; vox_stream_group_create_t_embeds, any kind of group): a delay PER MEMBER -- t_embed
        is then unread (None); member k's ids are those of member k in a group whose members all run at its delay.  reset(member, delay=) moves a member to another,
        t_embed(member) reads it back."""
        if delays is not None and t_embeds is not None:
            raise ValueError("create_stream_group: delays and t_embeds name the same thing, give one")
        if delays is not None:
            from .audio import TimeEmbedding
            te = TimeEmbedding(self.config.dec_dim); t_embeds = [te.embed(float(d)) for d in delays]
        if t_embeds is not None:
            t_embeds = _f32(np.stack([_f32(t).reshape(-1) for t in t_embeds])) if len(t_embeds) else np.zeros((0, self.config.dec_dim), np.float32)
            if t_embeds.shape != (int(n_members), self.config.dec_dim):
                raise ValueError(f"{t_embeds.shape[0]} t_embeds of {t_embeds.shape[1]} values for {int(n_members)} members of dec_dim {self.config.dec_dim}: one per member")
        return LiveStreamGroup(self, t_embed, n_members, gains, enc_capacity_rows, max_positions, sample_rates, page_rows, pool_pages, endless, kv_dtype, burst, t_embeds)

    def transcribe_batch(self, samples_list, t_embed, device_ptrs=None, n_samples=None, norm_group=None, tap_units=None):
        """Batched whole-path transcription of independent utterances (<= 4096; wider than 16: continuous batching over decode slots): list of float32 sample arrays
        (or device pointers + lengths) -> list of id arrays.  Decode steps are batched so weights stream once per step.
        norm_group (vox_transcribe_batch_ex): per unit, the id of the FILE whose peak normalises it (the CLI's semantics: normalise the file, then chunk it,
        bin/transcribe.rs:207-226); < 0 = use the unit as it is; None = every unit normalises itself.
        tap_units (vox_debug_batch_tap_*): unit indices whose logits rows are tapped -> (outs, taps), taps[j] [len(outs[tap_units[j]])][vocab] f32: row k is the row
        out_ids[tap_units[j]][k] was the argmax of."""
        return self._transcribe_batch(samples_list, t_embed, device_ptrs, n_samples, norm_group, tap_units, None)

    def transcribe_batch_scored(self, samples_list, t_embed, alternatives=0, norm_group=None, tap_units=None, device_ptrs=None, n_samples=None):
        """transcribe_batch with a record per id (vox_transcribe_batch_scored) -> (ids, scores, alts_or_None[, taps]): per unit, scores[i][j] / alts[i][j] are score_rows /
        alternatives_rows of the f32 logits row ids[i][j] was the argmax of (SCORE_DTYPE / ALTS_DTYPE arrays, one per unit, as long as the unit's ids).
        alternatives = 0: scores alone and None for the alternatives; 1..8: that many alternatives per id.  The ids are transcribe_batch's; tap_units as there."""
        return self._transcribe_batch(samples_list, t_embed, device_ptrs, n_samples, norm_group, tap_units, int(alternatives))

    def _transcribe_batch(self, samples_list, t_embed, device_ptrs, n_samples, norm_group, tap_units, alternatives):
        """the two calls above; alternatives None: the unscored entry points"""
        t = _f32(t_embed).reshape(-1)
        if device_ptrs is None:
            arrs = [_f32(x) for x in samples_list]; n = len(arrs)
            ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs]); lens = (C.c_size_t * n)(*[a.size for a in arrs]); kind = 0
        else:
            n = len(device_ptrs); ptrs = (C.c_void_p * n)(*device_ptrs); lens = (C.c_size_t * n)(*n_samples); kind = 1
        caps = [int(lens[i]) // 1280 + 128 for i in range(n)]
        outs = [np.zeros(cp, dtype=np.int32) for cp in caps]
        optrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs]); ccaps = (C.c_int32 * n)(*caps); nids = (C.c_int32 * n)()
        if tap_units is not None:
            units = [int(u) for u in tap_units]
            if not units or any(u < 0 or u >= n for u in units):
                raise ValueError("tap_units: indices into this call's units")
            from .audio import PadConfig
            pc = PadConfig.voxtral()
            max_rows = max(1, max(pc.padded_len(int(lens[u])) // 2560 - 35 for u in units))      # >= max(S - 38, 1): S <= padded / 2560 + 1 decoder positions
            check(lib().vox_debug_batch_tap_arm(self.h, (C.c_int32 * len(units))(*units), len(units), max_rows))
        if norm_group is not None and len(norm_group) != n:
            raise ValueError("norm_group needs one entry per unit")
        grp = None if norm_group is None else (C.c_int32 * n)(*[int(g) for g in norm_group])
        if alternatives is not None:
            scs = [np.zeros(cp, dtype=SCORE_DTYPE) for cp in caps]; als = [np.zeros(cp, dtype=ALTS_DTYPE) for cp in caps] if alternatives != 0 else None
            sptrs = (C.c_void_p * n)(*[a.ctypes.data for a in scs]); aptrs = None if als is None else (C.c_void_p * n)(*[a.ctypes.data for a in als])
            check(lib().vox_transcribe_batch_scored(self.h, n, ptrs, lens, grp, _ptr(t), optrs, ccaps, nids, sptrs, aptrs, alternatives, kind))
        elif norm_group is None:
            check(lib().vox_transcribe_batch(self.h, n, ptrs, lens, _ptr(t), optrs, ccaps, nids, kind))
        else:
            check(lib().vox_transcribe_batch_ex(self.h, n, ptrs, lens, grp, _ptr(t), optrs, ccaps, nids, kind))
        res = [outs[i][:nids[i]].copy() for i in range(n)]
        if alternatives is not None:
            recs = ([scs[i][:nids[i]].copy() for i in range(n)], None if als is None else [als[i][:nids[i]].copy() for i in range(n)])
        if tap_units is None:
            return res if alternatives is None else (res, *recs)
        V = self.config.vocab
        buf = np.zeros((len(units), max_rows, V), dtype=np.float32); rows = (C.c_int32 * len(units))()
        check(lib().vox_debug_batch_tap_fetch(self.h, buf.ctypes.data, rows))
        taps = []
        for j, u in enumerate(units):
            if rows[j] != len(res[u]):
                raise VoxError(1, f"batch tap: unit {u} has {rows[j]} tapped rows for {len(res[u])} ids (max_rows {max_rows})")
            taps.append(buf[j, :rows[j]].copy())
        return (res, taps) if alternatives is None else (res, *recs, taps)

    def timings(self):
        t = _lib.Timings(); check(lib().vox_get_stage_timings(self.h, C.byref(t)))
        return {k: getattr(t, k) for k, _ in _lib.Timings._fields_}

    def bench_decode_gemv(self, which, iters=200):
        us = C.c_double(); by = C.c_double(); nm = C.c_char_p()
        check(lib().vox_bench_decode_gemv(self.h, which, iters, C.byref(us), C.byref(by), C.byref(nm)))
        return us.value, by.value, (nm.value or b"").decode()

    def close(self):
        if self.h:
            for c in list(self._caches):
                c.close()
            lib().vox_model_free(self.h); self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Q4ModelLoader:
    """gguf/loader.rs:67-128"""

    def __init__(self, path=None, reader=None):
        self.path = None if path is None else str(path); self.reader = reader

    @classmethod
    def from_file(cls, path):
        return cls(path)

    @classmethod
    def from_bytes(cls, data):
        """gguf/loader.rs:92-99"""
        return cls(reader=GgufReader.from_bytes(data))

    @classmethod
    def from_shards(cls, shards):
        """gguf/loader.rs:101-107"""
        return cls(reader=GgufReader.from_shards(shards))

    def load(self, ctx: Context, layout_only: bool = False) -> Q4VoxtralModel:
        """`layout_only`: allocate the device arena without reading tensor data (multi-GPU ranks > 0
        receive the arena bytes from rank 0 with one RCCL broadcast)."""
        h = C.c_void_p()
        if self.reader is not None:
            check(lib().vox_q4_model_load_gguf(ctx.h, self.reader.h, 1 if layout_only else 0, C.byref(h)))
        else:
            check(lib().vox_q4_model_load_ex(ctx.h, self.path.encode(), 1 if layout_only else 0, C.byref(h)))
        return Q4VoxtralModel(ctx, h)
