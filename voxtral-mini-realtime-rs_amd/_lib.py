"""ctypes loader for libvoxtral_hip.so (the C ABI in include/voxtral_hip.h).  Fails loudly if the
HIP library has not been built -- there is no fallback implementation."""
from __future__ import annotations

import ctypes as C
import os

from .build import LIB_PATH


class VoxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[vox error {code}] {msg}")
        self.code = code


class PadCfg(C.Structure):
    _fields_ = [("sample_rate", C.c_uint32), ("n_left_pad_tokens", C.c_uint32), ("frame_rate", C.c_float),
                ("extra_right_pad_tokens", C.c_uint32)]


class ChunkCfg(C.Structure):
    _fields_ = [("max_mel_frames", C.c_uint32), ("hop_length", C.c_uint32), ("sample_rate", C.c_uint32),
                ("overlap_frames", C.c_uint32)]


class Chunk(C.Structure):
    _fields_ = [("start_sample", C.c_size_t), ("end_sample", C.c_size_t), ("index", C.c_size_t), ("is_last", C.c_int32)]


class StreamFeed(C.Structure):
    """vox_stream_feed: one member's entry of a vox_stream_group_advance call"""
    _fields_ = [("member", C.c_int32), ("finish", C.c_int32), ("samples", C.c_void_p), ("n_samples", C.c_size_t), ("out_ids", C.c_void_p), ("cap", C.c_int32),
                ("n_ids", C.c_int32)]


class TokenScore(C.Structure):
    """vox_token_score: what a live session knows about one id it handed out"""
    _fields_ = [("logprob", C.c_float), ("margin", C.c_float), ("runner_up", C.c_int32), ("id", C.c_int32)]


class Alt(C.Structure):
    """vox_alt: one alternative of a step, its id and log-probability"""
    _fields_ = [("id", C.c_int32), ("logprob", C.c_float)]


class TokenAlts(C.Structure):
    """vox_token_alts: the k best ids of a step's logits row and the row's entropy"""
    _fields_ = [("entropy", C.c_float), ("n", C.c_int32), ("alt", Alt * 8)]


class ModelCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("enc_layers", "enc_dim", "enc_heads", "enc_head_dim", "enc_ffn", "enc_window",
                                         "dec_layers", "dec_dim", "dec_heads", "dec_kv_heads", "dec_head_dim", "dec_ffn",
                                         "dec_window", "vocab", "n_mels", "reshape_factor", "t_cond_dim")] + \
               [("rope_theta", C.c_float), ("norm_eps", C.c_float)]


class SnapshotInfo(C.Structure):
    """vox_snapshot_info: a session blob's decoded header"""
    _fields_ = [("version", C.c_int32), ("sample_rate", C.c_uint32), ("gain", C.c_float), ("token", C.c_int32),
                ("total_bytes", C.c_uint64), ("fingerprint", C.c_uint64), ("t_embed_hash", C.c_uint64),
                ("samples_pushed", C.c_int64), ("samples_16k", C.c_int64), ("samples_in", C.c_int64)] + \
               [(n, C.c_int32) for n in ("positions", "enc_position", "ids", "scores", "alternatives", "n_scores", "n_alts", "enc_rows", "dec_rows", "reserved")] + \
               [("section_offset", C.c_uint64 * 9), ("section_bytes", C.c_uint64 * 9)]


class Timings(C.Structure):
    _fields_ = [("preprocess_ms", C.c_double), ("encode_ms", C.c_double), ("decode_ms", C.c_double), ("total_ms", C.c_double),
                ("decode_tokens", C.c_int32), ("graph_replays", C.c_int32)]


vp, i32, i64, u32, u64, sz, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_uint64, C.c_size_t, C.c_float
P = C.POINTER

# every symbol include/voxtral_hip.h declares (tests check the .so exports all of them)
SIGNATURES = {
    "vox_last_error": (C.c_char_p, []),
    "vox_abi_version": (i32, []),
    "vox_device_count": (i32, [P(i32)]),
    "vox_ctx_create": (i32, [i32, P(vp)]),
    "vox_ctx_destroy": (i32, [vp]),
    "vox_debug_reload_knobs": (i32, []),
    "vox_ctx_synchronize": (i32, [vp]),
    "vox_ctx_set_shared": (i32, [vp, i32]),
    "vox_ctx_stream": (i32, [vp, P(vp)]),
    "vox_dev_alloc": (i32, [vp, sz, P(vp)]),
    "vox_dev_free": (i32, [vp, vp]),
    "vox_dev_upload": (i32, [vp, vp, vp, sz]),
    "vox_dev_download": (i32, [vp, vp, vp, sz]),
    "vox_dev_copy": (i32, [vp, vp, vp, sz]),
    "vox_peak_normalize": (i32, [vp, sz, f32]),
    "vox_pad_cfg_voxtral": (i32, [P(PadCfg)]),
    "vox_pad_len": (i32, [sz, P(PadCfg), P(sz)]),
    "vox_pad_audio": (i32, [vp, sz, P(PadCfg), vp]),
    "vox_num_audio_tokens": (i32, [sz, P(PadCfg), P(sz)]),
    "vox_needs_chunking": (i32, [sz, P(ChunkCfg), P(i32)]),
    "vox_chunk_plan": (i32, [sz, P(ChunkCfg), P(Chunk), sz, P(sz)]),
    "vox_mel_num_frames": (i32, [sz, P(sz)]),
    "vox_mel_filterbank": (i32, [vp]),
    "vox_hann_window": (i32, [i32, vp]),
    "vox_mel_compute_log": (i32, [vp, vp, sz, vp, i32]),
    "vox_time_embedding": (i32, [f32, i32, vp]),
    "vox_gguf_open": (i32, [C.c_char_p, P(vp)]),
    "vox_gguf_open_memory": (i32, [vp, C.c_size_t, P(vp)]),
    "vox_gguf_open_shards": (i32, [vp, vp, i32, P(vp)]),
    "vox_q4_model_load_gguf": (i32, [vp, vp, C.c_uint32, P(vp)]),
    "vox_gguf_close": (i32, [vp]),
    "vox_gguf_version": (i32, [vp, P(u32)]),
    "vox_gguf_tensor_count": (i32, [vp, P(u64)]),
    "vox_gguf_tensor_name": (i32, [vp, u64, P(C.c_char_p)]),
    "vox_gguf_tensor_info": (i32, [vp, C.c_char_p, P(u64 * 4), P(u32), P(u32), P(u64)]),
    "vox_gguf_tensor_data": (i32, [vp, C.c_char_p, vp, sz]),
    "vox_q4_tensor_from_bytes": (i32, [vp, vp, sz, i64, i64, P(vp)]),
    "vox_q4_tensor_shape": (i32, [vp, P(i64), P(i64)]),
    "vox_q4_tensor_num_blocks": (i32, [vp, P(i64)]),
    "vox_q4_tensor_dequantize": (i32, [vp, vp, vp]),
    "vox_q4_tensor_free": (i32, [vp]),
    "vox_q4_matmul": (i32, [vp, vp, vp, i32, i32, vp, i32]),
    "vox_q4_linear_forward": (i32, [vp, vp, vp, vp, i32, i32, vp, i32]),
    "vox_dense_tensor_from_f32": (i32, [vp, vp, vp, i64, i64, P(vp)]),
    "vox_linear_forward_ex": (i32, [vp, vp, vp, vp, i32, i32, vp, i32, i32]),
    "vox_conv_downsample": (i32, [vp, vp, i32, i32, vp, vp, vp, vp, i32, vp]),
    "vox_attention": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, i32]),
    "vox_q4_model_load": (i32, [vp, C.c_char_p, P(vp)]),
    "vox_q4_model_load_ex": (i32, [vp, C.c_char_p, u32, P(vp)]),
    "vox_f32_model_load": (i32, [vp, C.c_char_p, P(vp)]),
    "vox_model_free": (i32, [vp]),
    "vox_model_config": (i32, [vp, P(ModelCfg)]),
    "vox_model_weight_bytes": (i32, [vp, P(u64)]),
    "vox_model_arena": (i32, [vp, P(vp), P(u64)]),
    "vox_model_set_t_embed": (i32, [vp, vp]),
    "vox_model_set_decode_engine": (i32, [vp, i32, P(i32)]),
    "vox_model_set_prefix_cache": (i32, [vp, i32, P(i32)]),
    "vox_model_prefix_info": (i32, [vp, P(i32 * 4)]),
    "vox_debug_occupy": (i32, [vp, i32, i32]),
    "vox_model_memory": (i32, [vp, P(C.c_uint64)]),
    "vox_model_set_batch_engine": (i32, [vp, i32, P(i32), P(C.c_uint64)]),
    "vox_model_arena_finalize": (i32, [vp]),
    "vox_model_replicate": (i32, [vp, vp, P(vp)]),
    "vox_model_set_sessions": (i32, [vp, i32]),
    "vox_generate_step_with_cache": (i32, [vp, vp, i32, vp, vp, vp]),
    "vox_encode_audio": (i32, [vp, vp, i32, vp, i32, P(i32), i32]),
    "vox_transcribe_streaming": (i32, [vp, vp, i32, vp, vp, i32, P(i32), vp, i32]),
    "vox_transcribe_audio": (i32, [vp, vp, sz, vp, vp, i32, P(i32), i32]),
    "vox_transcribe_batch": (i32, [vp, i32, P(vp), P(sz), vp, P(vp), P(i32), P(i32), i32]),
    "vox_transcribe_batch_ex": (i32, [vp, i32, P(vp), P(sz), vp, vp, P(vp), P(i32), P(i32), i32]),
    "vox_decoder_cache_create": (i32, [vp, i32, P(vp)]),
    "vox_cache_free": (i32, [vp]),
    "vox_cache_seq_len": (i32, [vp, P(i32)]),
    "vox_cache_reset": (i32, [vp]),
    "vox_cache_update": (i32, [vp, i32, i32, vp, vp, i32, i32]),
    "vox_cache_truncate": (i32, [vp, i32]),
    "vox_resample_len": (i32, [sz, C.c_uint32, C.c_uint32, P(sz)]),
    "vox_resample": (i32, [vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, P(sz), i32]),
    "vox_resample_plan": (i32, [C.c_uint32, C.c_uint32, P(i32), P(i32), P(i32), P(C.c_float), vp, sz]),
    "vox_encoder_cache_create": (i32, [vp, i32, P(vp)]),
    "vox_encoder_cache_apply_sliding_window": (i32, [vp, i32]),
    "vox_cache_abs_pos": (i32, [vp, P(i32)]),
    "vox_encode_audio_with_cache": (i32, [vp, vp, i32, vp, vp, i32, P(i32), i32]),
    "vox_embed_tokens_from_ids": (i32, [vp, vp, i32, vp]),
    "vox_forward_hidden_with_cache": (i32, [vp, vp, i32, vp, vp, vp]),
    "vox_lm_head": (i32, [vp, vp, i32, vp]),
    "vox_embed_tokens_from_ids_ex": (i32, [vp, vp, i32, vp, i32]),
    "vox_tensor_add": (i32, [vp, vp, vp, sz, vp, i32]),
    "vox_forward_hidden_with_cache_ex": (i32, [vp, vp, i32, vp, vp, vp, P(vp), i32]),
    "vox_lm_head_ex": (i32, [vp, vp, i32, vp, i32]),
    "vox_argmax_rows": (i32, [vp, vp, i32, i32, vp, i32]),
    "vox_lm_head_argmax": (i32, [vp, vp, i32, vp, i32]),
    "vox_forward": (i32, [vp, vp, i32, vp, vp, i32, P(i32), i32]),
    "vox_forward_streaming": (i32, [vp, vp, i32, vp, i32, vp, vp, i32, P(i32), i32]),
    "vox_forward_with_cache": (i32, [vp, vp, i32, vp, vp, vp, vp, i32, P(i32), i32]),
    "vox_get_stage_timings": (i32, [vp, P(Timings)]),
    "vox_bench_decode_gemv": (i32, [vp, i32, i32, P(C.c_double), P(C.c_double), P(C.c_char_p)]),
    "vox_bench_wide": (i32, [vp, i32, i32, i32, P(C.c_double)]),
    "vox_debug_attn_launches": (i32, [P(C.c_uint64), i32]),
    "vox_debug_attn_decode": (i32, [vp, vp, vp, vp, vp, vp]),
    "vox_debug_attn_decode_ring": (i32, [vp, vp, vp, vp, vp, vp]),
    "vox_debug_attn_decode_paged_ring": (i32, [vp, vp, i32, vp, vp, vp, vp]),      # a paged launch on a ring page table of page_tab_len entries
    "vox_debug_attn_decode_paged_bf16": (i32, [vp, vp, i32, vp, vp, vp, vp]),      # the paged launch (flat table: page_tab_len 0) on uint16_t pools
    "vox_debug_rope_rows": (i32, [i32, C.c_float, C.c_int64, i32, vp, vp, vp]),
    "vox_debug_stream_attn": (i32, [vp, vp, vp, vp, vp, vp]),      # (ctx, vox_stream_attn_desc, qkv, kring, vring, out): ONE launch of the streams' ring attention
    "vox_debug_stream_attn_burst": (i32, [vp, vp, vp, vp, vp, vp]),      # the same arguments, rows up to 64: ONE launch of the burst kernel
    "vox_debug_stream_attn_burst_launches": (i32, [P(C.c_uint64)]),
    "vox_debug_stream_attn_group_burst": (i32, [vp, vp, vp, vp, vp, vp, vp]),      # (ctx, desc, rows_per_slot, qkv, kring, vring, out): ONE launch of the ragged burst kernel
    "vox_debug_stream_ring_init": (i32, [vp, i32, i32, i32, i32, i32, vp, vp, vp]),      # (ctx, layers, rows, n_heads, head_dim, cap, kv, kring, vring)
    "vox_debug_attn_gqa_max_seq": (i32, [vp, P(i32)]),
    "vox_debug_gemm_launches": (i32, [P(C.c_uint64), i32]),
    "vox_debug_timeline_start": (i32, [vp, i32, i32]),
    "vox_debug_timeline_fetch": (i32, [vp, vp, sz, P(i32), vp]),
    "vox_debug_batch_tap_arm": (i32, [vp, P(i32), i32, i32]),
    "vox_debug_batch_tap_fetch": (i32, [vp, vp, P(i32)]),
    "vox_debug_encode_batch": (i32, [vp, i32, P(vp), P(i32), i32, vp, C.c_int64, P(i32), P(C.c_int64)]),
    "vox_stream_create": (i32, [vp, vp, f32, i32, i32, P(vp)]),
    "vox_stream_push": (i32, [vp, vp, sz, i32, vp, i32, P(i32)]),
    "vox_stream_finish": (i32, [vp, vp, i32, P(i32)]),
    "vox_stream_reset": (i32, [vp]),
    "vox_stream_free": (i32, [vp]),
    "vox_stream_info": (i32, [vp, P(i64 * 8)]),
    "vox_debug_step_costs": (i32, [P(C.c_double), P(C.c_double), i32, i32, P(C.c_double)]),
    "vox_debug_plan_slots": (i32, [P(i32), i32, i32, i32, P(C.c_double), P(i32), P(i32), P(i32), P(i32), P(i32), P(C.c_double)]),
    "vox_stream_schedule": (i32, [sz, i32, P(i32), P(i32)]),
    "vox_debug_stream_tap_arm": (i32, [vp, i32]),
    "vox_debug_stream_tap_fetch": (i32, [vp, vp, P(i32)]),
    "vox_debug_stream_front_tap_arm": (i32, [vp, i32]),
    "vox_debug_stream_front_tap_fetch": (i32, [vp, vp, vp, P(i32)]),
    "vox_debug_front_end": (i32, [vp, i32, P(vp), P(sz), P(i32), i32, i32, vp, P(vp), P(i32)]),
    "vox_stream_create_rate": (i32, [vp, vp, f32, i32, i32, u32, P(vp)]),
    "vox_stream_create_endless": (i32, [vp, vp, f32, i32, i32, u32, P(vp)]),
    "vox_stream_create_burst": (i32, [vp, vp, f32, i32, i32, u32, i32, i32, i32, P(vp)]),      # (..., sample_rate, endless, dec_ring_rows, burst_ticks, out)
    "vox_stream_burst_info": (i32, [vp, P(i64 * 4)]),
    "vox_stream_burst_len": (i32, [i64, i32, i64, i64]),      # returns the length itself (a pure function)
    "vox_stream_group_burst_rounds": (i32, [vp, i32, i32, vp, i32, P(i32)]),      # (due, n, burst, out [max_rounds][17], max_rounds, n_rounds)
    "vox_stream_group_create_burst": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, P(vp)]),      # (..., rates, cap, max_pos, paged, page_rows, pool_pages, endless, kv_dtype, burst_ticks, out)
    "vox_stream_group_burst_info": (i32, [vp, P(i64 * 4)]),
    "vox_stream_push_s16": (i32, [vp, vp, sz, i32, vp, i32, P(i32)]),
    "vox_stream_schedule_rate": (i32, [sz, u32, i32, P(i32), P(i32), P(sz)]),
    "vox_stream_group_create": (i32, [vp, vp, i32, vp, i32, i32, P(vp)]),
    "vox_stream_group_advance": (i32, [vp, vp, i32, i32]),
    "vox_stream_group_reset": (i32, [vp, i32, f32]),
    "vox_stream_group_info": (i32, [vp, i32, P(i64 * 8)]),
    "vox_stream_group_free": (i32, [vp]),
    "vox_debug_stream_group_tap_arm": (i32, [vp, i32, i32]),
    "vox_debug_stream_group_tap_fetch": (i32, [vp, i32, vp, P(i32)]),
    "vox_stream_group_create_rates": (i32, [vp, vp, i32, vp, vp, i32, i32, P(vp)]),
    "vox_stream_group_reset_rate": (i32, [vp, i32, f32, u32]),
    "vox_stream_group_advance_s16": (i32, [vp, vp, i32, i32]),
    "vox_debug_stream_feed_passes": (i32, [u32, P(sz), P(i32), i32, sz, P(i64), i32, P(i32)]),
    "vox_score_rows": (i32, [vp, vp, i32, i32, vp, vp, i32]),
    "vox_stream_set_scores": (i32, [vp, i32]),
    "vox_stream_scores": (i32, [vp, i32, i32, vp]),
    "vox_stream_group_set_scores": (i32, [vp, i32, i32]),
    "vox_stream_group_scores": (i32, [vp, i32, i32, i32, vp]),
    "vox_alternatives_rows": (i32, [vp, vp, i32, i32, i32, vp, i32]),
    "vox_stream_set_alternatives": (i32, [vp, i32]),
    "vox_stream_alternatives": (i32, [vp, i32, i32, vp]),
    "vox_stream_peeked_alternatives": (i32, [vp, vp, i32, P(i32)]),
    "vox_stream_group_set_alternatives": (i32, [vp, i32, i32]),
    "vox_stream_group_alternatives": (i32, [vp, i32, i32, i32, vp]),
    "vox_stream_group_peeked_alternatives": (i32, [vp, i32, vp, i32, P(i32)]),
    "vox_stream_peek": (i32, [vp, vp, i32, P(i32), vp]),
    "vox_stream_peek_ids": (i32, [sz, u32, i32, P(i32)]),
    "vox_debug_stream_tap_peeked": (i32, [vp, vp, i32]),
    "vox_stream_group_peek": (i32, [vp, vp, i32, vp]),
    "vox_stream_group_create_paged": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, P(vp)]),
    # an endless paged group: (model, t_embed, n_members, gains, rates or null, enc_capacity_rows, page_rows or 0, pool_pages or 0, out) -- no max_positions
    "vox_stream_group_create_endless": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, P(vp)]),
    # a paged / endless paged group with a K/V pool dtype: (model, t_embed, n_members, gains, rates, enc_capacity_rows, max_positions, page_rows, pool_pages, endless, kv_dtype, out)
    "vox_stream_group_create_kv": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, P(vp)]),
    "vox_kv_round_bf16": (i32, [vp, i64, vp]),      # (f32 in, n, uint16 out): the pool's rounding as host arithmetic
    "vox_stream_group_pool": (i32, [vp, P(i64 * 4), vp]),
    "vox_stream_group_pages_for": (i32, [i64, i32, i32, P(i32), P(i32)]),
    "vox_debug_stream_group_pages": (i32, [vp, i32, vp, i32, P(i32)]),
    "vox_records_rows": (i32, [vp, vp, i32, i32, i32, vp, vp, i32]),
    # snapshot and resume: (blob, nbytes, vox_snapshot_info); (cfg, positions, sample_rate, n_samples, scores, alternatives, out); the streams' three calls
    "vox_snapshot_describe": (i32, [vp, sz, P(SnapshotInfo)]),
    "vox_snapshot_bytes_for": (i32, [P(ModelCfg), i64, u32, sz, i32, i32, P(sz)]),
    "vox_stream_snapshot_size": (i32, [vp, P(sz)]),
    "vox_stream_snapshot": (i32, [vp, vp, sz, P(sz), i32]),
    "vox_stream_restore": (i32, [vp, vp, sz, i32]),
    "vox_stream_group_snapshot_size": (i32, [vp, i32, P(sz)]),
    "vox_stream_group_snapshot": (i32, [vp, i32, vp, sz, P(sz), i32]),
    "vox_stream_group_restore": (i32, [vp, i32, vp, sz, i32]),
    "vox_debug_snapshot_kv": (i32, [vp, vp, vp, vp, vp, i32]),      # (ctx, vox_snapshot_kv_desc, cache_k, cache_v, blob, restore): ONE launch of the blob's K / V kernel
    # a delay per member: (model, t_embeds [n][dec_dim], n_members, gains, rates, cap, max_pos, paged, page_rows, pool_pages, endless, kv_dtype, burst_ticks, out);
    # (group, member, gain, sample_rate or 0, t_embed); (group, member, out, cap)
    "vox_stream_group_create_t_embeds": (i32, [vp, vp, i32, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, P(vp)]),
    "vox_stream_group_reset_t_embed": (i32, [vp, i32, f32, u32, vp]),
    "vox_stream_group_t_embed": (i32, [vp, i32, vp, i32]),
    # (ctx, w, vox_resid_xf_desc, x, resid, xf_w, scales, order or null, out, xf_out, ssq_out): ONE launch of the wo GEMM's EPI_RESID_XF epilogue
    "vox_debug_resid_xf": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
    # (ctx, w, vox_xf_op_desc, vox_xf_op_bufs): ONE operator of the batched XF decode step (one group or the wide step), or the encoder's RoPE rows
    "vox_debug_xf_op": (i32, [vp, vp, vp, vp]),
    # levels: (stream, on); (stream, first_id, n, out); (stream, peak_below, ticks); the same with a member; (k, first, end);
    # (ctx, n_members, rings, ring_n, gains, pos, frame, order, n_slots, ticks, burst_b or null, list_len, out): ONE launch of the level kernel
    "vox_stream_set_levels": (i32, [vp, i32]),
    "vox_stream_levels": (i32, [vp, i32, i32, vp]),
    "vox_stream_quiet": (i32, [vp, f32, P(i32)]),
    "vox_stream_group_set_levels": (i32, [vp, i32, i32]),
    "vox_stream_group_levels": (i32, [vp, i32, i32, i32, vp]),
    "vox_stream_group_quiet": (i32, [vp, i32, f32, P(i32)]),
    "vox_level_window": (i32, [i32, P(i64), P(i64)]),
    "vox_debug_stream_level": (i32, [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, i32, vp]),
    "vox_transcribe_audio_scored": (i32, [vp, vp, sz, vp, vp, i32, P(i32), vp, vp, i32, i32]),
    "vox_transcribe_batch_scored": (i32, [vp, i32, P(vp), P(sz), vp, vp, P(vp), P(i32), P(i32), vp, vp, i32, i32]),
}

_LIB = None
_KNOBS = None


def _knob_env():
    return tuple(sorted((k, v) for k, v in os.environ.items() if k.startswith("VOX_")))


def lib():
    """dlopen libvoxtral_hip.so and bind every declared symbol.  Raises if the library is missing.
    The library snapshots its VOX_* measurement knobs at vox_ctx_create; this Python mirror (tests and tools flip knobs between two calls) asks it to
    re-read them whenever the VOX_* part of os.environ has changed since the last call."""
    global _LIB, _KNOBS
    if _LIB is not None:
        k = _knob_env()
        if k != _KNOBS:
            _KNOBS = k; _LIB.vox_debug_reload_knobs()
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise VoxError(-1, f"{LIB_PATH} not built: run `python __graft_entry__.py build` (hipcc, gfx950). "
                           "There is no CPU fallback for the HIP path.")
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)   # AttributeError here == missing export == ABI drift; fail loudly
        fn.restype = res
        fn.argtypes = args
    _LIB = L; _KNOBS = _knob_env()
    return L


def check(code: int):
    if code != 0:
        raise VoxError(code, (lib().vox_last_error() or b"").decode(errors="replace"))
