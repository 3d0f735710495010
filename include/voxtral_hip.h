/*
 * voxtral_hip.h -- C ABI of libvoxtral_hip.so: the MI355X (gfx950) implementation of the
 * Voxtral-Mini realtime ASR hot path of TrevorS/voxtral-mini-realtime-rs (reference v0.2.0).
 *
 * This is the drop-in boundary: every entry point is what a Rust `-sys` crate for the
 * reference's model-forward surface (src/audio, src/gguf, src/models) would bind.  The
 * reference interface each function replaces is cited as file:line (paths relative to the
 * reference repository).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - every function returns int32_t status: 0 = VOX_OK, non-zero = error; the message is
 *     available from vox_last_error() (thread-local).  Where the reference panics (shape
 *     mismatch in q4_matmul, gguf/op.rs:92-100) or returns anyhow::Error, we return a status.
 *   - opaque handles; caller-owned host buffers; plain pointers and sizes only.
 *   - a vox_ctx binds one HIP device + one stream.  Handles created from a ctx are not
 *     thread-safe; distinct ctxs are independent (one ctx per GPU for multi-GPU sharding).
 *   - `mem_kind`: VOX_MEM_HOST = pointers are host memory (copied in/out, synchronous),
 *     VOX_MEM_DEVICE = pointers are device memory on the ctx's device (asynchronous on the
 *     ctx stream; call vox_ctx_synchronize before reading results from another stream).
 *   - layouts follow the reference: weights [N,K] = [out,in] row-major (gguf/tensor.rs:32-34);
 *     Q4_0 block = {f16 d; u8 qs[16]}, element i <-> low nibble of qs[i], element i+16 <-> high
 *     nibble (gguf/tensor.rs:98-109); mel handed to the model as [128][T] (time fastest,
 *     bin/transcribe.rs:295-305) while compute_log returns [T][128] (audio/mel.rs:128); ids are i32.
 *   - there is NO CPU fallback anywhere behind this ABI: compute entry points fail with
 *     VOX_ERR_HIP if no gfx950 device is usable.
 */
#ifndef VOXTRAL_HIP_H
#define VOXTRAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VOX_OK 0
#define VOX_ERR_INVALID 1   /* bad argument / shape mismatch            */
#define VOX_ERR_IO 2        /* file / GGUF parse error                  */
#define VOX_ERR_HIP 3       /* HIP runtime error or no device           */
#define VOX_ERR_NOTFOUND 4  /* tensor name not present                  */
#define VOX_ERR_UNSUPPORTED 5

#define VOX_MEM_HOST 0
#define VOX_MEM_DEVICE 1

typedef struct vox_ctx vox_ctx;
typedef struct vox_gguf vox_gguf;
typedef struct vox_q4 vox_q4;
typedef struct vox_model vox_model;
typedef struct vox_cache vox_cache;
typedef struct vox_graph vox_graph;

const char* vox_last_error(void);
int32_t vox_abi_version(void);                      /* bumps on any signature change */
int32_t vox_device_count(int32_t* n);

/* ---- context (reference: the implicit `WgpuDevice::default()`, bin/transcribe.rs:67) ---- */
int32_t vox_ctx_create(int32_t device, vox_ctx** out);
int32_t vox_ctx_destroy(vox_ctx* ctx);
int32_t vox_ctx_synchronize(vox_ctx* ctx);
/* shared != 0: this context SHARES its GPU with other sessions (more contexts of this process -- one host thread each, see vox_model_replicate -- or other processes).
 * The batch entry points then stay off the batched decode engines (their 256 persistent workgroups need the GPU to themselves: next to another session their bounded
 * hand-off waits expire and the session is run twice) and the slot planner prices its steps with the table scaled by ONE measured factor instead of per-form
 * measurements (which scatter under contention) and records none.  Per step the logits stay within f32 summation-order noise (2e-4 of the largest, what the tests assert
 * against the single-stream path) whatever the plan, so ids change only after a near-tie; the plan (hence the order of the sums) may differ from an unshared call's.  Default 0.  (No reference counterpart: the reference runs one utterance at a
 * time, bin/transcribe.rs:112-126; this is what a multi-threaded host sets on every context of a GPU it runs more than one session on.) */
int32_t vox_ctx_set_shared(vox_ctx* ctx, int32_t shared);
int32_t vox_ctx_stream(vox_ctx* ctx, void** hip_stream_out);   /* hipStream_t, for event timing */
/* device memory helpers so non-HIP callers can use VOX_MEM_DEVICE */
int32_t vox_dev_alloc(vox_ctx* ctx, size_t nbytes, void** out);
int32_t vox_dev_free(vox_ctx* ctx, void* p);
int32_t vox_dev_upload(vox_ctx* ctx, void* dst_dev, const void* src_host, size_t nbytes);
int32_t vox_dev_download(vox_ctx* ctx, void* dst_host, const void* src_dev, size_t nbytes);
int32_t vox_dev_copy(vox_ctx* ctx, void* dst_dev, const void* src_dev, size_t nbytes);   /* device -> device, synchronous */

/* ---- audio front-end (src/audio) ------------------------------------------------------- */
/* resample / resample_to_16k, audio/resample.rs:10-52.  The reference's resampler is rubato 1.0's synchronous FFT resampler
 * (`Fft::<f32>::new(sr_in, sr_out, 1024, 2, 1, FixedSync::Input)` + `process_all_into_buffer`, resample.rs:22-45).  This is that crate's published algorithm on
 * the GPU: blocks of fft_in samples through a Blackman-Harris^2 windowed-sinc filter in the frequency domain, the low bins re-synthesised at length 2 fft_out,
 * overlap-added, the fft_out / 2 samples of delay dropped; n_out = ceil(n_in * (f64(sr_out) / f64(sr_in))); same rate -> copy (resample.rs:17-19).  rubato is not
 * in the reference's tree, so parity against the crate itself is unpinned; the CPU oracle restates the same algorithm independently.
 * Rate pairs whose blocks would not fit a 64 MB matrix (co-prime rates) are refused with VOX_ERR_UNSUPPORTED.  in / out host or device buffers (mem_kind). */
int32_t vox_resample_len(size_t n_in, uint32_t sr_in, uint32_t sr_out, size_t* n_out);
int32_t vox_resample(vox_ctx* ctx, const float* in, size_t n_in, uint32_t sr_in, uint32_t sr_out, float* out, size_t cap, size_t* n_out,
                     int32_t mem_kind);
/* the plan rubato derives from the two rates, and the filter taps (fft_in floats, already divided by 2 fft_in) when taps_or_null is given */
int32_t vox_resample_plan(uint32_t sr_in, uint32_t sr_out, int32_t* fft_in, int32_t* fft_out, int32_t* delay, float* cutoff, float* taps_or_null, size_t cap);
/* AudioBuffer::peak_normalize, audio/io.rs:59-68 (host, in place) */
int32_t vox_peak_normalize(float* samples, size_t n, float target_peak);

/* PadConfig, audio/pad.rs:20-46 */
typedef struct {
    uint32_t sample_rate;             /* 16000 */
    uint32_t n_left_pad_tokens;       /* 76    */
    float    frame_rate;              /* 12.5  */
    uint32_t extra_right_pad_tokens;  /* 17    */
} vox_pad_cfg;
int32_t vox_pad_cfg_voxtral(vox_pad_cfg* cfg);                                   /* PadConfig::voxtral, pad.rs:50-52 */
int32_t vox_pad_len(size_t n, const vox_pad_cfg* cfg, size_t* out);              /* pad.rs:89-93 */
int32_t vox_pad_audio(const float* in, size_t n, const vox_pad_cfg* cfg, float* out); /* pad_audio, pad.rs:89-103 */
int32_t vox_num_audio_tokens(size_t n, const vox_pad_cfg* cfg, size_t* out);     /* pad.rs:106-108 */

/* ChunkConfig / chunk_audio / needs_chunking, audio/chunk.rs:9-166 */
typedef struct {
    uint32_t max_mel_frames;  /* 1500; CLI default 1200 (bin/transcribe.rs:55-57) */
    uint32_t hop_length;      /* 160 */
    uint32_t sample_rate;     /* 16000 */
    uint32_t overlap_frames;  /* 0 */
} vox_chunk_cfg;
typedef struct { size_t start_sample, end_sample, index; int32_t is_last; } vox_chunk;
int32_t vox_needs_chunking(size_t n, const vox_chunk_cfg* cfg, int32_t* out);
int32_t vox_chunk_plan(size_t n, const vox_chunk_cfg* cfg, vox_chunk* out, size_t cap, size_t* n_chunks);

/* MelSpectrogram (MelConfig::voxtral), audio/mel.rs:63-350 */
int32_t vox_mel_num_frames(size_t n_samples, size_t* out);                       /* mel.rs:175-182 */
int32_t vox_mel_filterbank(float* out_128x201);                                  /* mel.rs:288-339 */
int32_t vox_hann_window(int32_t length, float* out);                             /* mel.rs:345-349 */
/* compute_log, mel.rs:128-165: samples (already padded by the caller) -> [T][128].  STFT + mel
 * filterbank + log run on the GPU. */
int32_t vox_mel_compute_log(vox_ctx* ctx, const float* samples, size_t n, float* out_Tx128, int32_t mem_kind);

/* TimeEmbedding::embed, models/time_embedding.rs:41-71 (theta 10000) */
int32_t vox_time_embedding(float t, int32_t dim, float* out);

/* ---- GGUF reader (src/gguf/reader.rs:98-223) -------------------------------------------- */
int32_t vox_gguf_open(const char* path, vox_gguf** out);                         /* GgufReader::open */
/* GgufReader::from_bytes (gguf/reader.rs:98-103): parse an image already in host memory (BORROWED until vox_gguf_close) */
int32_t vox_gguf_open_memory(const void* data, size_t size, vox_gguf** out);
/* Q4ModelLoader::from_shards (gguf/loader.rs:101-107, the WASM <= 512 MB pieces): consecutive pieces of one GGUF image (copied) */
int32_t vox_gguf_open_shards(const void* const* shards, const size_t* sizes, int32_t n, vox_gguf** out);
int32_t vox_gguf_close(vox_gguf* g);
int32_t vox_gguf_version(const vox_gguf* g, uint32_t* out);
int32_t vox_gguf_tensor_count(const vox_gguf* g, uint64_t* out);
int32_t vox_gguf_tensor_name(const vox_gguf* g, uint64_t index, const char** out); /* tensor_names */
/* tensor_info: dims in file order (GGUF = reversed PyTorch order), dtype 0 F32 / 1 F16 / 2 Q4_0 */
int32_t vox_gguf_tensor_info(const vox_gguf* g, const char* name, uint64_t dims[4], uint32_t* ndims,
                             uint32_t* dtype, uint64_t* nbytes);
int32_t vox_gguf_tensor_data(const vox_gguf* g, const char* name, void* dst, size_t cap); /* tensor_data */

/* ---- Q4 operator boundary (src/gguf/tensor.rs, op.rs, linear.rs) ------------------------ */
/* Q4Tensor::from_q4_bytes, gguf/tensor.rs:35-71: validates N*K % 32 == 0 and nbytes == blocks*18 */
int32_t vox_q4_tensor_from_bytes(vox_ctx* ctx, const uint8_t* raw, size_t nbytes, int64_t N, int64_t K, vox_q4** out);
int32_t vox_q4_tensor_shape(const vox_q4* q, int64_t* N, int64_t* K);            /* tensor.rs:74-76 */
int32_t vox_q4_tensor_num_blocks(const vox_q4* q, int64_t* out);                 /* tensor.rs:79-81 */
int32_t vox_q4_tensor_dequantize(vox_ctx* ctx, const vox_q4* q, float* out_NxK); /* tensor.rs:88-113 (host out) */
int32_t vox_q4_tensor_free(vox_q4* q);
/* q4_matmul, gguf/op.rs:86-137: out[B,M,N] = x[B,M,K] x W[N,K]^T, f32 accumulate.
 * B*M <= 4 runs the GEMV kernel (reference: tiled shader), larger the MFMA GEMM (reference: naive). */
int32_t vox_q4_matmul(vox_ctx* ctx, const vox_q4* w, const float* x, int32_t B, int32_t M, float* out, int32_t mem_kind);
/* Q4Linear::forward, gguf/linear.rs:34-40: q4_matmul (+ bias[N], may be NULL; same mem_kind) */
int32_t vox_q4_linear_forward(vox_ctx* ctx, const vox_q4* w, const float* bias_or_null, const float* x,
                              int32_t B, int32_t M, float* out, int32_t mem_kind);

/* ---- dense (f32 SafeTensors path) layer operators on their own (src/models/layers) ------ */
/* The device form of an F32 burn `Linear` weight [N][K] as models/weights.rs:16-66 loads it: the exact f32 plane + bf16 hi / lo planes (what vox_f32_model_load builds
 * for a checkpoint that is not bf16-representable).  w_other_or_null: a second [N][K] tensor interleaved row by row with the first (row 2 i = w[i], 2 i + 1 =
 * other[i]) -- the fused gate | up operand SwiGLU::forward (models/layers/swiglu.rs:72-77) runs on.  The handle is a vox_q4: vox_q4_tensor_shape / _free apply,
 * vox_q4_linear_forward / vox_q4_matmul multiply by it. */
int32_t vox_dense_tensor_from_f32(vox_ctx* ctx, const float* w_NxK, const float* w_other_or_null, int64_t N, int64_t K, vox_q4** out);
/* Linear::forward with a fused epilogue, Q4 or dense weight: 0 none, 1 GELU (the Ada t_cond MLP, models/layers/rms_norm.rs:109-118), 2 SwiGLU over interleaved
 * gate / up rows: out[.][i] = silu(row 2 i) * row 2 i + 1, N / 2 columns (swiglu.rs:72-77; no bias). */
int32_t vox_linear_forward_ex(vox_ctx* ctx, const vox_q4* w, const float* bias_or_null, const float* x, int32_t B, int32_t M, float* out, int32_t epilogue, int32_t mem_kind);
/* ConvDownsampler::forward, models/layers/conv.rs:78-83: gelu(conv1d k = 3, s = 2, p = 1) twice; x [C][L], w1 [O][C][3], w2 [O][O][3] -> out [O][L2], L2 = ((L + 1) / 2 + 1) / 2
 * (host pointers; the im2col MFMA path the encoder's conv stem runs on). */
int32_t vox_conv_downsample(vox_ctx* ctx, const float* x_CxL, int32_t C, int32_t L, const float* w1, const float* b1, const float* w2, const float* b2, int32_t O, float* out_OxL2);

/* ---- model-forward surface (src/gguf/loader.rs, src/gguf/model.rs) ---------------------- */
typedef struct {
    int32_t enc_layers, enc_dim, enc_heads, enc_head_dim, enc_ffn, enc_window;
    int32_t dec_layers, dec_dim, dec_heads, dec_kv_heads, dec_head_dim, dec_ffn, dec_window, vocab;
    int32_t n_mels, reshape_factor, t_cond_dim;
    float rope_theta, norm_eps;
} vox_model_cfg;

/* Attention core of both stacks: softmax(q k^T * head_dim^-0.5 + causal/sliding-window mask) v with grouped-query heads
 * (gguf/model.rs:100-120 encoder MHA, :125-198 decoder GQA without materialising the x4 KV expansion; masking.rs:9-107:
 * query at position offset+m sees keys j <= offset+m and, when window >= 0, offset+m-j <= window).
 * q [M][n_heads*head_dim], k / v [kv_len][n_kv_heads*head_dim], out [M][n_heads*head_dim]; head_dim 64 or 128. */
int32_t vox_attention(vox_ctx* ctx, const float* q, const float* k, const float* v, int32_t M, int32_t kv_len, int32_t n_heads,
                      int32_t n_kv_heads, int32_t head_dim, int32_t offset, int32_t window, float* out, int32_t mem_kind);

/* Q4ModelLoader::from_file(..).load(), gguf/loader.rs:82-128 */
int32_t vox_q4_model_load(vox_ctx* ctx, const char* gguf_path, vox_model** out);
/* flags: VOX_LOAD_LAYOUT_ONLY parses the GGUF header and allocates the identical device arena layout but does
 * not read or upload tensor data -- the caller fills the arena (vox_model_arena) e.g. from an RCCL broadcast. */
#define VOX_LOAD_LAYOUT_ONLY 1u
int32_t vox_q4_model_load_ex(vox_ctx* ctx, const char* gguf_path, uint32_t flags, vox_model** out);
/* Q4ModelLoader::from_bytes / from_shards -> load (gguf/loader.rs:92-128): from an open reader (file, memory image or shards);
 * the reader is only read during the call and stays owned by the caller. */
int32_t vox_q4_model_load_gguf(vox_ctx* ctx, vox_gguf* g, uint32_t flags, vox_model** out);
/* VoxtralModelLoader::from_file(..).load(), models/loader.rs:35-78: the f32 SafeTensors path (F32 / F16 / BF16 tensors,
 * models/weights.rs:16-66).  Same vox_model handle and the same forward entry points as the Q4 model.  A linear weight whose values
 * are all bf16-representable (the published checkpoint is BF16) is stored as one bf16 plane; any other F32 / F16 tensor keeps its EXACT
 * values on device (f32 plane for the decode GEMV and the embedding lookup, bf16 hi + lo planes for the MFMA GEMMs) -- tested at full size
 * against the oracle (tests/test_gpu_f32_path.py, test_gpu_fullsize.py: 108 / 108 and 196 / 196 greedy ids). */
int32_t vox_f32_model_load(vox_ctx* ctx, const char* safetensors_path, vox_model** out);
int32_t vox_model_free(vox_model* m);
int32_t vox_model_config(const vox_model* m, vox_model_cfg* out);
int32_t vox_model_weight_bytes(const vox_model* m, uint64_t* out);   /* device bytes of the weight arena */
/* Multi-GPU: export / import the packed device weight arena so rank 0 can parse the GGUF once and
 * the other ranks receive it with one RCCL broadcast over xGMI (no data-path collective). */
int32_t vox_model_arena(const vox_model* m, void** dev_ptr, uint64_t* nbytes);
/* Receiver side: after the bytes of vox_model_arena (the PRIMARY part of the arena: every tensor as parsed from the file, 2.5 GB for the
 * Q4 model) have been written into a VOX_LOAD_LAYOUT_ONLY model, rebuild what is derived from them on this GPU (the tile-ordered copies
 * of the Q4 linears; the decode engine's weight stream is packed lazily at the first decode step on every rank). */
int32_t vox_model_arena_finalize(vox_model* m);
/* In-process multi-GPU start-up (one host thread + one vox_ctx + one replica per GPU: the shape SURVEY.md section 8(e) gives the reference's serial loop,
 * bin/transcribe.rs:112-126): one more replica of a loaded Q4 model on `dst_ctx` -- another GPU or the same one -- without the file and without a collective library.
 * The destination arena is laid out from the source's tensor manifest, its primary part is copied device to device (hipMemcpyPeerAsync: xGMI between two GPUs) and the
 * derived copies are rebuilt on the destination (as vox_model_arena_finalize).  The replica is independent of the source afterwards (own arena, own workspaces); distinct
 * contexts may be driven from distinct host threads concurrently (tests/test_gpu_model.py::test_two_contexts_two_threads). */
int32_t vox_model_replicate(const vox_model* src, vox_ctx* dst_ctx, vox_model** out);
/* Device memory the model holds besides caches and workspaces, bytes: out[0] weight arena (= vox_model_weight_bytes), out[1] its primary part (what a multi-GPU start-up
 * broadcasts), out[2] the decode engines' weight stream (a third copy of the decoder's Q4 bytes in consumption order; 0 until the first decode step builds it),
 * out[3] the engines' edge buffers (single-stream granules + one block per 16-row group of the batched engine). */
int32_t vox_model_memory(const vox_model* m, uint64_t out[4]);

/* the delay conditioning used by every decoder call: t_embed = TimeEmbedding(dec_dim).embed(delay)
 * (bin/transcribe.rs:104-105).  Ada scales 1 + w2(gelu(w0 t_embed)) (gguf/model.rs:250-255) are
 * loop-invariant and cached per t_embed. */
int32_t vox_model_set_t_embed(vox_model* m, const float* t_embed_host);
/* Single-stream decode loop of transcribe_streaming (gguf/model.rs:938-960): by default every step is ONE launch of the persistent decode engine
 * (all 26 layers + final norm + lm_head; real decoder geometry, Q4 weights, 256-CU device); on = 0 selects the per-operator launches (4 per layer),
 * which other geometries / dense checkpoints always use.  *active_or_null reports whether the engine will be used.  Results of both paths agree to
 * summation-order noise (same ids; tests/test_gpu_fullsize.py).  The engine's 256 workgroups wait for each other with bounded (20 ms) waits: if the GPU is shared and a wait expires,
 * the utterance is decoded again on the per-operator launches (a warning on stderr), the engine is re-armed for the next utterance and switched off after three such
 * strikes.  Environment VOX_ENGINE=0 sets the default to off at load time. */
int32_t vox_model_set_decode_engine(vox_model* m, int32_t on, int32_t* active_or_null);
/* Prefix state of vox_transcribe_audio (default on).  That entry pads every utterance on the left with the same silence (vox_pad_cfg_voxtral), so the first encoder rows
 * and -- the decoder's prefix tokens being fixed -- the first decoder positions are the same for every utterance: functions of the weights (and of t_embed) alone.  The
 * model computes them once from a silent mel (at its first vox_transcribe_audio call, or here when a t_embed is already set; again for the decoder part when t_embed
 * changes) and afterwards runs the encoder layers over the remaining rows only and one ordinary decode step in place of the 38-token prefill.  Results do not depend on
 * which call came first; they agree with the full computation to summation-order noise.  Entries that take a caller's mel or embeddings, the logits tap and the batch
 * entries always run the full computation.  on = 0: the full computation everywhere (the state is freed); on < 0: query only.  *active_or_null: will it be used. */
int32_t vox_model_set_prefix_cache(vox_model* m, int32_t on, int32_t* active_or_null);
/* out = { state built (0 / 1), encoder rows held per layer, decoder positions held, device bytes held }; rows / positions are 0 for a geometry without a prefix. */
int32_t vox_model_prefix_info(const vox_model* m, int32_t out[4]);
/* Batched decode loop of vox_transcribe_batch (BASELINE configs[3] / [4]; the reference's model.rs:938-960 is batch-1): the 26 decoder layers of a step run as ONE
 * launch of the batched decode-layer engine (same eligibility as above) whenever one or two 16-row groups are active -- a batch of n <= 16 rows (one group per
 * launch), and in a wider batch's continuous decode the steps with one or two active slot groups (TWO groups per launch: group B's phase runs while group A's
 * hand-off resolves; DESIGN.md sections 3.3c / 3.3e).  Steps with three or four active groups take the launch-based step (4 launches per layer and group, the groups'
 * chains back to back on the session stream, as every chain of a batched step since the corpus crash fix; measured, with the chains then forked on side
 * streams, faster than engine launches back to back).  on = 0 selects the launch-based step everywhere, on < 0 only queries.
 * *active_or_null: is the engine armed; *launches_or_null: engine launches enqueued so far (eager + graph replays) -- the number that says whether a given call used
 * it.  A hand-off timeout inside the engine re-runs the batch (the session, for a wide batch) on the launch-based step (a warning on stderr); three such strikes
 * switch the engine off for the model.  Environment VOX_BATCH_ENGINE=0: off at load time. */
int32_t vox_model_set_batch_engine(vox_model* m, int32_t on, int32_t* active_or_null, uint64_t* launches_or_null);

/* Q4VoxtralModel::encode_audio, gguf/model.rs:783-788: mel [128][T] -> [S][dec_dim]; *S = floor(S_enc/4) */
int32_t vox_encode_audio(vox_model* m, const float* mel_128xT, int32_t T, float* out, int32_t cap_rows,
                         int32_t* S, int32_t mem_kind);
/* Q4VoxtralModel::transcribe_streaming, gguf/model.rs:873-963 -> ids, length S-38 (0 if S < 38).
 * logits_or_null (host, [n_ids][vocab]) is a parity/debug tap for the per-step decoder logits. */
int32_t vox_transcribe_streaming(vox_model* m, const float* mel_128xT, int32_t T, const float* t_embed,
                                 int32_t* out_ids, int32_t cap, int32_t* n_ids, float* logits_or_null,
                                 int32_t mem_kind);
/* Whole hot path from 16 kHz samples: peak_normalize(0.95) -> pad -> log-mel -> transcribe_streaming
 * (bin/e2e_bench.rs:98-232 un-chunked pipeline).  samples may be device-resident (VOX_MEM_DEVICE). */
int32_t vox_transcribe_audio(vox_model* m, const float* samples, size_t n, const float* t_embed,
                             int32_t* out_ids, int32_t cap, int32_t* n_ids, int32_t mem_kind);

/* Batched transcription (BASELINE.json configs[3] "Batch=16 x 16 s utterances" and configs[4], a rank's share of a corpus; extension -- the reference's callers
 * loop over files, bin/transcribe.rs:112-126).  n <= 4096 independent utterances, each through the whole path of vox_transcribe_audio; the decode loop advances
 * many sequences per step so the weights are streamed once per step for all of them.  samples[i] / out_ids[i] are per-utterance buffers (samples host or device per
 * mem_kind, ids always host); n_ids[i] receives S_i - 38 (or 0).  Batches may be ragged and results always land in the caller's slot i.
 * n <= 16: one 16-row group, one decode-layer engine launch per step.  n > 16: CONTINUOUS BATCHING -- every utterance is encoded (stacked, packed: no padding to the
 * longest) and prefilled up front; the decode step then runs over 16 .. 128 SLOTS, and a slot whose utterance has its last token takes the next utterance of its
 * host-planned queue inside the same step (token counts are a pure function of the sample count: there is no EOS, gguf/model.rs:936-960), so the groups stay full
 * until the queues run dry; steps with one or two active groups are one engine launch for all their layers (vox_model_set_batch_engine).  Per decode step, every
 * utterance's logits are within f32 summation-order noise (2e-4 of the largest logit, asserted for every step form against the teacher-forced single-stream logits:
 * vox_debug_batch_tap_*) of the single-stream path, whatever n, the slot, the neighbours or the plan; so its ids equal the single-stream ids except after a near-tie,
 * where the forms' different K-split summation orders may break the tie differently.  Ids are bit-identical call to call only with the same slot plan:
 * VOX_BATCH_NO_CALIB=1 makes the plan a function of the input lengths alone (otherwise measured step costs steer it). */
int32_t vox_transcribe_batch(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const float* t_embed,
                             int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind);
/* The same call with the CLI's normalisation semantics (bin/transcribe.rs:207-265): the reference peak-normalises the FILE once, splits it into chunks of
 * --max-mel-frames (default 1200, :55-57; audio/chunk.rs:125-166) and transcribes every chunk as an independent unit (own padding, own 38-token prefix), joining the
 * chunk texts with " " (:261-275).  Here a chunk is a unit of this call: units naming the same norm_group[i] >= 0 share ONE peak scale 0.95 / max|x| taken over all of
 * them (the chunks tile their file, so that is the file's peak: one device reduction per unit folded per group, exact); norm_group[i] < 0: the unit is used as handed
 * over (the caller normalised it); norm_group == NULL: every unit normalises itself (= vox_transcribe_batch, the un-chunked e2e-bench pipeline).  Units may be views
 * into one file buffer (host or device).  Ids per unit equal vox_transcribe_streaming's on the chunk's mel (tests/test_gpu_fullsize.py, test_tokenizer_cli.py). */
int32_t vox_transcribe_batch_ex(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const int32_t* norm_group_or_null, const float* t_embed,
                                int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, int32_t mem_kind);
/* sessions = 2..4: vox_transcribe_batch / _ex calls with at least 128 units per session run as that many CONCURRENT sessions on the model's GPU -- the calling thread on the
 * model's context, the others on library threads with hidden contexts and replicas of the model (made here, device to device: 2.5 GB each; freed with the model or by
 * sessions = 1).  One session leaves the GPU idle wherever its launch-bound decode steps wait; a second one fills the gaps: 647 FLEURS-like clips x 1.16 - 1.20 over a 64-slot session on one
 * MI355X (the plain call now plans up to 128 slots as two chains per step -- the same overlap -- so sessions add ~1 % there: they are for one GPU shared by
 * independent callers).  Units that share a norm_group stay in one session; every context involved counts as shared for the call (vox_ctx_set_shared); results are per
 * unit: a unit's logits stay within f32 summation-order noise of the single-stream path whichever session runs it, so its ids depend on the split only after a near-tie.  vox_get_stage_timings then reports the longest session's stage times and the call's wall time.  Smaller calls and every other
 * entry point are unchanged.  (No reference counterpart -- the reference transcribes one file at a time, bin/transcribe.rs:112-126; a host that prefers its own threads
 * uses vox_model_replicate + vox_ctx_set_shared instead.)  Q4 (GGUF) models. */
int32_t vox_model_set_sessions(vox_model* m, int32_t sessions);

/* Q4LanguageModel pieces used directly by e2e-bench / WASM (gguf/model.rs:566,665,680,711) */
int32_t vox_decoder_cache_create(vox_model* m, int32_t max_seq, vox_cache** out);   /* create_cache_preallocated */
int32_t vox_cache_free(vox_cache* c);
int32_t vox_cache_seq_len(const vox_cache* c, int32_t* out);                         /* KVCache::seq_len */
int32_t vox_cache_reset(vox_cache* c);
/* KVCache::update on layer `layer` of a pre-allocated cache (models/layers/kv_cache.rs:116-136: slice_assign of k / v [1][heads][n_rows][head_dim] at rows pos ..
 * pos + n_rows); the length shared by all layers (LayerCaches::seq_len, :242-244) becomes max(len, pos + n_rows).  heads = dec_kv_heads (decoder cache) / enc_heads. */
int32_t vox_cache_update(vox_cache* c, int32_t layer, int32_t pos, const float* k_HxNxhd, const float* v_HxNxhd, int32_t n_rows, int32_t mem_kind);
/* forget the rows from `len` on (0 <= len <= seq_len): the next forward appends at `len` again.  vox_cache_update / _truncate / _reset first settle the decoder steps of
 * this cache that have not been verified yet (see vox_forward_hidden_with_cache_ex): a hand-off timeout found then is THIS call's error (VOX_ERR_HIP) and ALL steps since
 * the last synchronisation are taken back. */
int32_t vox_cache_truncate(vox_cache* c, int32_t len);
/* Streaming encoder: Q4AudioEncoder::create_cache + Q4VoxtralModel::encode_audio_with_cache (gguf/model.rs:437-459,791-799; per layer
 * :299-317,125-174), eviction KVCache::apply_sliding_window (kv_cache.rs:176-203).  The chunk's conv output rows are run through the 32 layers
 * against the cached K / V (RoPE at the absolute stream position; the cache evicts rows older than the 750-row window by itself when a chunk
 * does not fit), then reshaped / adapted like encode_audio: floor(S_chunk / 4) rows of [dec_dim].  capacity_rows 0 = 2 * window + 512.
 * LIMIT: positions are ABSOLUTE stream positions (the reference offsets RoPE by cache.seq_len(), which restarts after an eviction); the position table
 * holds 65 536 rows = 21.8 minutes of audio per cache -- later chunks are refused (VOX_ERR_INVALID) until vox_cache_reset.  A too small `cap_rows` is refused
 * BEFORE the chunk is appended (the stream cache is untouched and the call can be repeated with a larger buffer). */
int32_t vox_encoder_cache_create(vox_model* m, int32_t capacity_rows, vox_cache** out);
int32_t vox_encoder_cache_apply_sliding_window(vox_cache* enc_cache, int32_t window);
int32_t vox_cache_abs_pos(const vox_cache* c, int32_t* out);      /* encoder cache: stream positions seen so far; decoder cache: == seq_len */
int32_t vox_encode_audio_with_cache(vox_model* m, const float* mel_128xT, int32_t T, vox_cache* enc_cache, float* out, int32_t cap_rows,
                                    int32_t* S, int32_t mem_kind);
int32_t vox_embed_tokens_from_ids(vox_model* m, const int32_t* ids, int32_t n, float* out_nxD);      /* host out */
int32_t vox_forward_hidden_with_cache(vox_model* m, const float* x_MxD, int32_t M, const float* t_embed,
                                      vox_cache* cache, float* out_MxD);                              /* host in/out */
int32_t vox_lm_head(vox_model* m, const float* hidden_MxD, int32_t M, float* logits_MxV);            /* host in/out */
/* Device-resident forms of the same surface (mem_kind as everywhere else; VOX_MEM_DEVICE copies nothing and synchronises nothing), for a caller that drives
 * decode piece by piece the way bin/e2e_bench.rs:179-224 and web/bindings.rs:357-424 do on Burn tensors:
 *     embed_tokens_from_ids -> audio_pos + text_embed -> forward_hidden_with_cache -> lm_head -> argmax(2) -> into_scalar
 * All workspaces are model-owned (no allocation per call).  A single-row forward_hidden_with_cache against a decoder cache of <= 1024 rows runs as ONE launch of the
 * persistent decode engine when that is active (vox_model_set_decode_engine) -- the launch that also computes the row's lm_head; vox_lm_head_ex / vox_lm_head_argmax
 * on the hidden buffer it handed out (`*hidden_ws`, READ-ONLY for the caller, valid until the next decoder call on the model) then return those logits / that token
 * instead of streaming the lm_head again.  Any other hidden pointer is multiplied for real.  Engine hand-off timeouts (shared GPU) surface as VOX_ERR_HIP at the next
 * synchronising call -- vox_lm_head_argmax, vox_argmax_rows, vox_ctx_synchronize, host-kind outputs -- i.e. in the step that failed when the caller reads a token per
 * step as the reference's loop does.  The library remembers which rows of the cache it has not verified yet (the engine steps since the last synchronisation and
 * anything appended behind them) and takes exactly those back: after the error vox_cache_seq_len() is the length before the failed step, REPEAT THE STEP (same
 * token, same position) and the ids are those of an undisturbed run (tests/test_gpu_fullsize.py::test_full_piecewise_surface_recovers_from_an_engine_timeout).
 * ids are always host memory (the reference passes &[i32]). */
int32_t vox_embed_tokens_from_ids_ex(vox_model* m, const int32_t* ids_host, int32_t n, float* out_nxD, int32_t mem_kind);
/* `audio_pos + text_embed` (bin/e2e_bench.rs:212, gguf/model.rs:902,946): out[i] = a[i] + b[i] on the context's stream */
int32_t vox_tensor_add(vox_ctx* ctx, const float* a, const float* b, size_t n, float* out, int32_t mem_kind);
/* out_MxD_or_null: where to copy the rows (may be NULL with VOX_MEM_DEVICE when hidden_ws_or_null is given); *hidden_ws_or_null: the model-owned device buffer holding them */
int32_t vox_forward_hidden_with_cache_ex(vox_model* m, const float* x_MxD, int32_t M, const float* t_embed, vox_cache* cache, float* out_MxD_or_null,
                                         const float** hidden_ws_or_null, int32_t mem_kind);
int32_t vox_lm_head_ex(vox_model* m, const float* hidden_MxD, int32_t M, float* logits_MxV, int32_t mem_kind);
/* `logits.argmax(2)` + the scalar read-back (bin/e2e_bench.rs:219-220; lowest index wins ties): ids_host[M]; synchronises the stream */
int32_t vox_argmax_rows(vox_ctx* ctx, const float* logits_MxV, int32_t M, int32_t V, int32_t* ids_host, int32_t mem_kind);
/* ---- scores: what the model thought of an id (no reference counterpart).  For a logits row L[V] (f32) and an id t:
 *   logprob   = L[t] - (m + log sum_v exp(L[v] - m)), m = max_v L[v]: the id's log-probability under the row's softmax, in f32 with expf / logf;
 *   runner_up = the argmax over the columns v != t by the rule of every decode form (the largest wins, the lowest index wins a tie, a NaN or -inf never wins); -1 when
 *               no column can win (V == 1, or nothing but NaN / -inf besides t);
 *   margin    = L[t] - L[runner_up], one f32 subtraction: 0 on an exact tie, negative when t is not the row's argmax, L[t] + inf (+inf for a finite L[t]) without a
 *               runner-up;
 *   id        = t.
 * A -inf column adds 0 to the sum.  A row that holds a NaN, or whose maximum is not finite (+inf, or all -inf), has logprob = NaN; id and runner_up follow the rule all the
 * same.  The record is a function of the row's values and V alone -- one scan order and one reduction tree whatever the row's address or alignment, its slot, the rows
 * next to it or the launch -- so everything a live session claims bit for bit about its ids (cuts, ring wrap, isolation, capture rate) holds for its scores. */
typedef struct { float logprob; float margin; int32_t runner_up; int32_t id; } vox_token_score;
/* rows of logits -> one record per row, the piecewise caller's companion to vox_argmax_rows (same mem_kind for the logits).  ids_or_null (host, M entries, each in [0, V)):
 * the id to score; null: the row's argmax as vox_argmax_rows gives it.  out: host, M records.  Computed on the device either way (host logits are uploaded).  Synchronises. */
int32_t vox_score_rows(vox_ctx* ctx, const float* logits_MxV, int32_t M, int32_t V, const int32_t* ids_or_null, vox_token_score* out, int32_t mem_kind);
/* ---- levels: what the model had just heard when it chose an id (live sessions only; no reference counterpart).  Record k of an utterance goes with id k and describes
 * the 2560 samples at 16 kHz that are new to the tick that chose it: the window [2560 (k - 1), 2560 k) of the utterance's own 16 kHz sample index (vox_level_window).
 * Each sample is taken as the mel front end reads it -- v = gain * sample in f32, 0 below index 0 (the silent left pad; record 0 is (0, 0)), behind the utterance whatever
 * a finish or a peek put there (its zero pad) -- so a rate stream's records are taken on the 16 kHz samples its resampler produced.
 *   peak        = max |v| over the window: exact;
 *   mean_square = (sum v * v) / 2560 in f32, by ONE scan order and ONE reduction tree ("Levels"): every square rounds once, 18 additions lie on
 *                 every path from a sample to the root, one division follows -- within (1 + 2^-24)^20 - 1 < 2^-19 relative of the float64 value on the same f32 v
 *                 while no square underflows; a square below 2^-126 rounds on the subnormal grid, which adds at most 2^-149 (absolute) to the record.
 * A window with a non-finite sample has a non-finite mean_square; nothing else is promised of it -- in particular a NaN sample is dropped from the peak, which stays
 * the largest of the other samples, and vox_stream_quiet counts such a record by that peak.  The record is a function of the window's samples and the gain alone:
 * bit for bit independent of how the samples were cut into pushes, of solo stream versus group member, of the other members, of the ring and of burst versus plain. */
typedef struct { float peak; float mean_square; } vox_tick_level;
/* host arithmetic, no device: the window of record k >= 0 as [*first_sample, *end_sample) -- first_sample is -2560 for k = 0.  Id k is due at 2560 k + 40 pushed samples
 * (vox_stream_schedule), so every sample of its window has been pushed when the id is handed out. */
int32_t vox_level_window(int32_t k, int64_t* first_sample, int64_t* end_sample);
/* ---- alternatives: what else the model weighed at a step, and how spread the step's distribution was (no reference counterpart).  For a logits row L[V] (f32) and
 * k in 1 .. VOX_MAX_ALTERNATIVES:
 *   alt[0].id = the row's argmax by the rule of every decode form (the largest wins, the lowest index wins a tie, a NaN or -inf never wins); alt[j].id = the argmax by
 *               the same rule over the columns not yet taken;
 *   n         = min(k, the number of columns that can win); the entries j >= n are {-1, NaN} (V < k, rows of -inf or NaN: n < k, possibly 0);
 *   alt[j].logprob = (L[id_j] - m) - logf(S), with vox_token_score's m and S = sum_v exp(L[v] - m), summed in the same order: when the scored id is the row's argmax,
 *               alt[0].logprob has the bits of the score record's logprob, and alt[1].id is its runner_up;
 *   entropy   = max(0, logf(S) - T / S), T = sum_v exp(L[v] - m) (L[v] - m) over the columns above -inf, in f32, summed in S's order: the entropy of the row's softmax
 *               in nats.
 * A row that holds a NaN, or whose maximum is not finite, has entropy = NaN and every logprob = NaN; ids and n follow the rule all the same.  The record is a function
 * of the row's values, V and k alone (never of the row's address or alignment, its slot, the launch or the rows next to it), and the list for k is bit for bit the
 * first k entries of the list for a larger k: what a live session claims bit for bit about its ids holds for these records too. */
#define VOX_MAX_ALTERNATIVES 8
typedef struct { int32_t id; float logprob; } vox_alt;
typedef struct { float entropy; int32_t n; vox_alt alt[VOX_MAX_ALTERNATIVES]; } vox_token_alts;   /* 72 bytes */
/* rows of logits -> one record per row, vox_score_rows' companion (same mem_kind for the logits).  k: 1 .. VOX_MAX_ALTERNATIVES.  out: host, M records.  Computed on the
 * device either way (host logits are uploaded).  Synchronises. */
int32_t vox_alternatives_rows(vox_ctx* ctx, const float* logits_MxV, int32_t M, int32_t V, int32_t k, vox_token_alts* out, int32_t mem_kind);
/* ---- both records of a row from ONE launch, scored on the row's own argmax (vox_score_rows with ids_or_null == NULL): the kernel the offline and batch paths below
 * take their records from.  k == 0: scores alone (alts_or_null must be NULL, scores_or_null given); k in 1 .. VOX_MAX_ALTERNATIVES: alts_or_null is required,
 * scores_or_null optional -- both records then come from the two scans of the alternatives (id = alt[0].id, runner_up = alt[1].id, margin = L[id] - L[runner_up],
 * logprob = alt[0].logprob) instead of four.  The records are bit for bit vox_score_rows' and vox_alternatives_rows' on the same row.  Records: host, M each.
 * Computed on the device either way (host logits are uploaded).  Synchronises. */
int32_t vox_records_rows(vox_ctx* ctx, const float* logits_MxV, int32_t M, int32_t V, int32_t k, vox_token_score* scores_or_null, vox_token_alts* alts_or_null,
                         int32_t mem_kind);
/* ---- offline and batch transcription with a record per id (no reference counterpart): vox_transcribe_audio / vox_transcribe_batch_ex and, besides the ids, for id j of
 * a unit the vox_token_score and / or vox_token_alts of the f32 logits row the id was taken from -- bit for bit what vox_score_rows(row, id) and
 * vox_alternatives_rows(row, k) return for that row, and record j's id (alt[0].id) is out_ids[j].  k == 0: scores alone (alts must be NULL); k in 1 ..
 * VOX_MAX_ALTERNATIVES: alts is required, scores optional; both NULL is refused (VOX_ERR_INVALID: the unscored calls serve that).  The record arrays are host memory:
 * `cap` entries (single clip), caps[i] entries for unit i (batch: scores[i] / alts[i]); the entries from n_ids on are left untouched.  Every argument is checked before
 * a device is touched.
 *   batch: the ids are those of vox_transcribe_batch_ex under the same slot plan; the records are written by one more launch per decode step (and one per prefill
 *   stack), in front of the step's argmax, into device arrays that come down once behind the call's last synchronisation.  Every step form, calls split by
 *   vox_model_set_sessions and a call with the debug tap armed are served.  A call of the unscored entry points launches and allocates nothing for this.
 *   single clip: the clip is decoded as vox_transcribe_streaming decodes it with its logits tap (the full prefill, a logits row per step kept on the device), and
 *   vox_records_rows' kernel runs once over all rows; the ids are vox_transcribe_audio's.
 * (A row nothing can win on -- NaN and -inf only, never seen from a model -- has record id 0 where the ids hold the argmax sentinel.) */
int32_t vox_transcribe_audio_scored(vox_model* m, const float* samples, size_t n, const float* t_embed, int32_t* out_ids, int32_t cap, int32_t* n_ids,
                                    vox_token_score* scores_or_null, vox_token_alts* alts_or_null, int32_t k, int32_t mem_kind);
int32_t vox_transcribe_batch_scored(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const int32_t* norm_group_or_null, const float* t_embed,
                                    int32_t* const* out_ids, const int32_t* caps, int32_t* n_ids, vox_token_score* const* scores_or_null,
                                    vox_token_alts* const* alts_or_null, int32_t k, int32_t mem_kind);
/* lm_head + argmax + read-back in one call: M token ids come back instead of M x 512 KB of logits; synchronises the stream */
int32_t vox_lm_head_argmax(vox_model* m, const float* hidden_MxD, int32_t M, int32_t* ids_host, int32_t mem_kind);
/* Q4VoxtralModel::generate_step_with_cache, gguf/model.rs:857-867 (text tokens only: embed -> decoder against the cache -> final norm -> lm_head) in one call;
 * token_ids[n] host, logits[n][vocab] host; the cache advances by n. */
int32_t vox_generate_step_with_cache(vox_model* m, const int32_t* token_ids, int32_t n, const float* t_embed, vox_cache* cache, float* logits_nxV);

/* Composite forwards, mel [128][T] -> logits [S][vocab] in one call (nothing leaves the device between the stages); *S = decoder positions = floor(S_enc / 4):
 *   vox_forward             Q4VoxtralModel::forward            gguf/model.rs:820-830   the audio embeddings alone are the decoder input
 *   vox_forward_streaming   Q4VoxtralModel::forward_streaming  gguf/model.rs:802-816   audio embeddings + embed(token_ids); n_ids must equal S (vox_num_audio_tokens tells it in advance)
 *   vox_forward_with_cache  Q4VoxtralModel::forward_with_cache gguf/model.rs:833-843   encode_audio_with_cache + forward_hidden_with_cache against the caller's two caches
 * mel / logits host or device per mem_kind; token ids and t_embed host. */
int32_t vox_forward(vox_model* m, const float* mel_128xT, int32_t T, const float* t_embed, float* logits_SxV, int32_t cap_rows, int32_t* S, int32_t mem_kind);
int32_t vox_forward_streaming(vox_model* m, const float* mel_128xT, int32_t T, const int32_t* token_ids, int32_t n_ids, const float* t_embed, float* logits_SxV,
                              int32_t cap_rows, int32_t* S, int32_t mem_kind);
int32_t vox_forward_with_cache(vox_model* m, const float* mel_128xT, int32_t T, const float* t_embed, vox_cache* enc_cache, vox_cache* dec_cache, float* logits_SxV,
                               int32_t cap_rows, int32_t* S, int32_t mem_kind);

/* stage timers, BenchmarkResult parity (bin/e2e_bench.rs:62-74): ms of the last transcribe call */
typedef struct { double preprocess_ms, encode_ms, decode_ms, total_ms; int32_t decode_tokens; int32_t graph_replays; } vox_timings;
int32_t vox_get_stage_timings(const vox_model* m, vox_timings* out);

/* The VOX_* measurement knobs (kernel-selection overrides used by tools/ and by the A/B tests) are read from the environment ONCE, at vox_ctx_create;
 * this re-reads them (tests that flip a knob between two calls).  Not part of the reference surface. */
int32_t vox_debug_reload_knobs(void);
/* Test hook: attention launches enqueued by this process so far, by kernel form (host-side counts; the replays of a captured graph are not counted):
 * out[0] short-sequence prefill, [1] MFMA prefill, [2] f32 VALU prefill (VOX_ATTN_F32), [3] single-query decode, [4] its speculative-row form (VOX_ATTN_SPEC),
 * [5] batched GQA decode, [6] fused attention + wo, [7] single-stream decode-engine launches (the whole step), [8] the live stream's ring attention (RoPE + K / V append + windowed
 * attention in one launch: exactly enc_layers per tick of a vox_stream, one per vox_debug_stream_attn call; a refused launch counts nothing).  Behind them, not attention: [9] a stream group's resampling ingest (one launch per pass for
 * all fed members), [10] a solo stream's.  Behind those, attention again: [11] paged single-query decode, [12] paged batched GQA decode (a paged stream group's step:
 * PAGED DECODER CACHE below).  [13] ring single-query decode (vox_debug_attn_decode_ring below): 0 unless a ring launch ran.  [14] paged single-query decode on a RING page table, [15] paged batched
 * GQA decode on one (an endless paged group's step, ENDLESS PAGED GROUPS below; vox_debug_attn_decode_paged_ring): such a launch counts here and not in [11] [12].
 * [16] paged single-query decode on a bf16 pool, [17] paged batched GQA decode on one, [18] [19] their ring-table forms (a bf16 paged group's step, A BF16 K/V POOL
 * below; vox_debug_attn_decode_paged_bf16): a bf16 launch counts there and never in [11] [12] [14] [15].  Entries past [19] are written as 0. */
int32_t vox_debug_attn_launches(uint64_t* out, int32_t cap);
/* One decode attention launch on its own (tests): one query row per sequence against a decoder cache, through the launcher and with the parameters of the batched decode
 * steps -- exactly ONE launch; which kernel ran is the launcher's choice and is read from vox_debug_attn_launches ([3] [4] [5] slab, [11] [12] paged).
 *   Geometry: n_seq sequences, n_heads query heads over n_kv_heads KV heads, head_dim 128 (anything else is refused), window (-1: none): sequence s at position pos[s]
 *   attends the keys max(0, pos[s] - window) .. pos[s].  q: host [n_seq][n_heads * 128].
 *   Slab cache (page_rows == 0): k / v host [n_slices][n_kv_heads][max_seq][128]; sequence s reads slice s, or slice kv_row[s] (n_slices >= n_seq without kv_row).
 *   Paged cache (page_rows a power of two in 16..1024; max_seq 0): k / v host [pool_pages][n_kv_heads][page_rows][128], page_tab host [n_slices][page_tab_stride]:
 *   entry q of row s (row kv_row[s] with kv_row) = the physical page of that sequence's rows q * page_rows ..; score_rows >= the most keys any sequence attends.
 *   Only the entries of a sequence's window are read, and they are checked against the pool here; the others may hold anything.
 *   Forms: prefer_gqa: the batched steps' flag (slab; the paged launcher takes the GQA form whenever n_heads == 4 n_kv_heads).  spec (slab): offer the speculative
 *   rows (spec_rows = max_seq) -- the launcher takes that form only with VOX_ATTN_SPEC=1, as in the product.  no_xcd_remap: the measurement knob of the per-head kernels.
 *   out: out_xf == 0: host float [n_seq][n_heads * 128] (a row the launch did not write comes back NaN); out_xf != 0: host uint16_t, the raw XF planes the wo GEMM reads,
 *   ceil(n_seq / 16) groups of 2 * (n_heads * 128 / 128) * 256 * 8 uint16_t each (hi plane, then lo plane; sequence s = row s % 16 of group s / 16).
 * Every argument is checked before the context is bound (VOX_ERR_INVALID); a slab call that would take the GQA form with max_seq above vox_debug_attn_gqa_max_seq is
 * refused before the launch.  vox_debug_attn_gqa_max_seq: the most rows per KV head the slab GQA form serves on the context's device (SLAB LIMIT below). */
typedef struct {
    int32_t n_seq, n_heads, n_kv_heads, head_dim, window;
    int32_t n_slices, max_seq;
    int32_t page_rows, pool_pages, page_tab_stride, score_rows;
    int32_t prefer_gqa, spec, no_xcd_remap, out_xf;
    const int32_t* pos;
    const int32_t* kv_row;       /* may be NULL */
    const int32_t* page_tab;     /* paged calls only */
} vox_attn_decode_desc;
int32_t vox_debug_attn_decode(vox_ctx* ctx, const vox_attn_decode_desc* desc, const float* q, const float* k, const float* v, void* out);
int32_t vox_debug_attn_gqa_max_seq(vox_ctx* ctx, int32_t* out);
/* One RING decode attention launch on its own (tests): vox_debug_attn_decode's slab call with every cache slice used as a ring.  max_seq is the ring capacity (any
 * value in 1..16384, a power of two or not); k / v host [n_slices][n_kv_heads][max_seq][128]; row j of a sequence lives at ring row j % max_seq; pos[s] may be any
 * value below 2^24; window >= 0 and window + 1 <= max_seq (a key outside the window may have been overwritten: without a window a ring has no meaning).  Sequence s
 * attends the logical rows max(0, pos[s] - window) .. pos[s] in that order -- the flat kernel's scan order and reduction trees, so the output has the bits of
 * vox_debug_attn_decode on the same keys laid out from row 0; ring rows outside the window are never read.  The per-head kernel, f32 rows out: prefer_gqa, spec,
 * out_xf and the paged fields must be 0.  Exactly ONE launch, counted in vox_debug_attn_launches [13].  Every argument is checked before the context is bound. */
int32_t vox_debug_attn_decode_ring(vox_ctx* ctx, const vox_attn_decode_desc* desc, const float* q, const float* k, const float* v, void* out);
/* One paged decode attention launch on a RING page table (tests): vox_debug_attn_decode's paged call, the descriptor's layout and meaning unchanged, with every table
 * row used as a ring of page_tab_len entries (1..1024, <= page_tab_stride, a power of two or not): logical page q of a sequence is entry q % page_tab_len of its row.
 * pos[s] may be any value below 2^24; window >= 0; page_tab_len >= window / page_rows + 4 -- the window / page_rows + 2 pages a window's keys can touch, + 2 -- is
 * required, a smaller table is refused.  The entries of every sequence's window are checked against the pool; the others may hold anything (-1) and are never read.
 * The paged kernels with the ring index in their staging loop alone: the output has the bits of vox_debug_attn_decode on a flat table naming the same pages.
 * Exactly ONE launch, counted in vox_debug_attn_launches [14] (per-head) or [15] (GQA), never in [11] [12].  Every argument is checked before the context is bound. */
int32_t vox_debug_attn_decode_paged_ring(vox_ctx* ctx, const vox_attn_decode_desc* desc, int32_t page_tab_len, const float* q, const float* k, const float* v, void* out);
/* One paged decode attention launch on a bf16 pool (tests): vox_debug_attn_decode's paged call, the descriptor's layout and meaning unchanged, with k_bf16 / v_bf16 host
 * uint16_t [pool_pages][n_kv_heads][page_rows][128] -- the upper halves of f32 values (vox_kv_round_bf16).  page_tab_len 0: a flat table, as vox_debug_attn_decode;
 * page_tab_len 1..1024: a ring table under vox_debug_attn_decode_paged_ring's conditions (window >= 0, page_tab_len <= page_tab_stride and >= window / page_rows + 4,
 * pos below 2^24).  The kernels load 16-bit rows (16 bytes of K, 8 of V per load), widen them in registers and run the f32 forms' arithmetic in the f32 forms' order:
 * the output has the bits of vox_debug_attn_decode / _paged_ring on the same pages holding the widened f32 values.  Exactly ONE launch, counted in
 * vox_debug_attn_launches [16] (per-head) / [17] (GQA), on a ring table [18] / [19], in no other slot.  Every argument is checked before the context is bound. */
int32_t vox_debug_attn_decode_paged_bf16(vox_ctx* ctx, const vox_attn_decode_desc* desc, int32_t page_tab_len, const float* q, const uint16_t* k_bf16, const uint16_t* v_bf16, void* out);
/* RoPE rows on their own (tests; host arithmetic, no device): rows first_pos .. first_pos + n - 1 (positions below 2^24) of the tables the kernels read, cos_out /
 * sin_out [n][head_dim / 2], and in inv_out [head_dim / 2] the f32 factors 1 / theta^(2 j / head_dim) they were made from.  The ONE function that produces RoPE rows:
 * the load-time tables and the streaming encoder's table are filled by it.  head_dim 128 is the decoder's geometry, whose load-time table has 16 384 rows; any other
 * head_dim is taken as the encoder's, whose streaming table has 65 536.  Below that length a row has the table's bits (f32 product pos * inv, f32 cos / sin); from
 * there on cos / sin are taken of double(pos) * double(inv) and rounded to f32 -- the f32 product loses the angle at large positions (its spacing is about 0.5 rad
 * at position 4 M). */
int32_t vox_debug_rope_rows(int32_t head_dim, float theta, int64_t first_pos, int32_t n, float* inv_out, float* cos_out, float* sin_out);
/* One launch of the live sessions' encoder ring attention on its own (tests): RoPE on q and k, the K / V append into each served session's ring and the windowed
 * softmax, as every tick of a vox_stream or a stream group runs it once per encoder layer -- exactly ONE launch, counted in vox_debug_attn_launches [8]; nothing of a
 * model is needed.
 *   Geometry: n_slots (1..16) slots serve the DISTINCT members order[z] of n_members (n_slots..64) sessions; member c stands at encoder position enc_pos[c] and slot
 *   z's `rows` (1..8) new rows are the positions enc_pos[order[z]] + m.  n_heads (1..32) heads of head_dim 64 or 128; row m attends the keys
 *   max(0, p - window) .. p of its position p, window 0..1023; every ring holds cap rows per head, window + rows < cap <= 16384; the launch works on layer `layer` of
 *   `layers` (1..8): the ring offset layer * n_heads * cap * head_dim.
 *   qkv: host [n_slots * rows][q | k | v], each n_heads * head_dim wide, NOT rotated.  kring / vring: host [n_members][layers][n_heads][cap][head_dim], in and out:
 *   position j of a member lives at ring row j % cap; after the launch rows (enc_pos + r) % cap, r < rows, of the served members' layer hold the rotated k and the
 *   raw v, every other word its bits from before.  out: host [n_slots * rows][n_heads * head_dim]; it is NaN before the launch, so an unwritten row shows.
 *   RoPE rows (theta; made by the function behind vox_debug_rope_rows, so they have that call's bits for the same head_dim):
 *     rope_rows == 0: a flat table of the rows 0 .. the largest position; enc_pos[c] + rows <= 65536, the streaming encoder's table length, for every member.
 *     rope_rows == R (a power of two, rows <= R <= 4096): a RoPE ring of R rows holding the rows (enc_pos[c] + r) & (R - 1), r < rows, of every SERVED member and
 *       NaN everywhere else -- what an endless session's refill writes; positions below 2^24 (enc_pos[c] + rows <= 2^24); two served members that need one ring row
 *       for different positions are refused.  rope_per_member != 0: one such ring per member, R rows apart, indexed by the member and not by the slot (an endless
 *       group's rings).
 * Every argument is checked before the context is bound (VOX_ERR_INVALID with a message): what the launcher would refuse -- rows 0 or 9, 17 slots, window + 1 >
 * 1024, cap <= window + rows, head_dim 32, a RoPE ring shorter than `rows` or no power of two -- never reaches it, and nothing the kernel reads or writes lies outside
 * the uploaded buffers. */
typedef struct {
    int32_t n_slots, n_members, rows, n_heads, head_dim, window, cap;
    int32_t layers, layer;
    int32_t rope_rows, rope_per_member;
    float theta;
    const int32_t* order;        /* [n_slots] */
    const int32_t* enc_pos;      /* [n_members] */
} vox_stream_attn_desc;
int32_t vox_debug_stream_attn(vox_ctx* ctx, const vox_stream_attn_desc* desc, const float* qkv, float* kring, float* vring, float* out);
/* The BURST form of the same attention (a burst stream's encoder layers: vox_stream_create_burst), on its own: vox_debug_stream_attn's arguments and checks with `rows`
 * 1..64 (b ticks' 4 b rows at enc_pos + m; window + rows < cap; a RoPE ring of at least `rows` rows) -- exactly ONE launch of the burst kernel, counted in
 * vox_debug_stream_attn_burst_launches and in no slot of vox_debug_attn_launches; a refused call counts nothing.  One workgroup serves a head and a tile of 4 query
 * rows and reads every ring row once for the tile.  One call with rows = 4 b leaves the bits in `out`, kring and vring that b successive vox_debug_stream_attn calls
 * with rows = 4 leave when enc_pos moves by 4 between them. */
int32_t vox_debug_stream_attn_burst(vox_ctx* ctx, const vox_stream_attn_desc* desc, const float* qkv, float* kring, float* vring, float* out);
/* launches of the burst kernel enqueued by the host so far (a burst stream: enc_layers per burst with b >= 2) */
int32_t vox_debug_stream_attn_burst_launches(uint64_t* out);
/* The RAGGED burst form (a burst group's round: vox_stream_group_create_burst), on its own: vox_debug_stream_attn_burst's arguments and checks, plus
 * rows_per_slot[n_slots] -- slot z has rows_per_slot[z] rows (a multiple of 4 in 4..64: its b_z ticks), desc->rows is the largest of them (window + rows < cap), and qkv
 * [sum rows][3 n_heads hd] and out [sum rows][n_heads hd] hold the slots' rows back to back, slot after slot.  Exactly ONE launch of the ragged burst kernel (grid:
 * heads x ceil(rows / 4) x n_slots; tiles beyond a slot's rows leave at once), counted in vox_debug_stream_attn_burst_launches; a refused call counts nothing.  For
 * every slot the launch leaves in out and in every word of that member's K and V ring the bits rows_per_slot[z] / 4 successive vox_debug_stream_attn calls with rows = 4
 * leave (enc_pos moving by 4); members not in `order` keep every ring word. */
int32_t vox_debug_stream_attn_group_burst(vox_ctx* ctx, const vox_stream_attn_desc* desc, const int32_t* rows_per_slot, const float* qkv, float* kring, float* vring, float* out);
/* The seeding of a session's encoder rings from the model's prefix state, on its own (tests): kv host [layers][rows][k row | v row], token-major, each row n_heads *
 * head_dim wide; kring / vring host [layers][n_heads][cap][head_dim], in and out: ring rows 0 .. rows - 1 of every layer and head receive the input's bits, every
 * other word keeps its own.  layers 1..64, n_heads 1..64, head_dim 64 | 128, cap 1..16384; rows <= 0 and rows > cap are refused, like every argument, before the
 * context is bound. */
int32_t vox_debug_stream_ring_init(vox_ctx* ctx, int32_t layers, int32_t rows, int32_t n_heads, int32_t head_dim, int32_t cap, const float* kv, float* kring, float* vring);
/* The sessions' level kernel on its own, without a model (tests): ONE launch for n_slots slots of n_members hand-made sessions.  rings: host [n_members][ring_n] f32
 * (ring_n a power of two, 4096 .. 2^20; sample i of a session lives at ring[i & (ring_n - 1)]); gains [n_members]; pos and frame [n_members]: each session's
 * STRM_POS (>= 37, the prefix positions) and STRM_FRAME (>= 0) words; order [n_slots]: the member slot z works for (distinct).  ticks 1 .. 16: the grid's tick
 * dimension; burst_b null: every slot runs `ticks` ticks (1: the plain form, more: a solo burst's); burst_b [n_slots]: the ragged form, slot z runs burst_b[z] ticks,
 * 1 .. ticks, descending.  Block (t, z) writes record pos - 37 + t of its session from the window starting at 160 frame - 97280 + 2560 t (the product's left pad
 * and first position).  out: host [n_members][list_len] records, list_len 1 .. 65536 -- every record the launch does not write comes back as (NaN, NaN), an index
 * outside the list is not written.  Every check before the context is bound. */
int32_t vox_debug_stream_level(vox_ctx* ctx, int32_t n_members, const float* rings, int32_t ring_n, const float* gains, const int32_t* pos, const int32_t* frame,
                               const int32_t* order, int32_t n_slots, int32_t ticks, const int32_t* burst_b, int32_t list_len, vox_tick_level* out);
/* One launch of the session blob's K / V kernel on its own (tests; SNAPSHOT AND RESUME below): the logical rows lo .. hi - 1 of every (layer, head) of K and V
 * between the blob's dense layout and a cache in one of the four layouts a session's K / V can have -- exactly ONE launch (none when lo == hi), host arrays in and out.
 *   blob: host [2][layers][n_heads][hi - lo][head_dim], K then V.  restore == 0 packs the cache's rows into it, restore != 0 unpacks it into the cache; cache_k /
 *   cache_v are copied back in both directions (a pack leaves them as they were; after an unpack every word outside the named rows has its bits from before).
 *   layout 0, flat: cache host [layers][layer_rows][...]: layer l starts at l * layer_stride floats, head h of it at h * rows * head_dim, row r at r * head_dim;
 *     layer_stride >= n_heads * rows * head_dim, a multiple of 4; hi <= rows.
 *   layout 1, ring: the same planes with row r at (r % rows) * head_dim -- rows is the ring's capacity, any value (a power of two or not); hi - lo <= rows, hi < 2^24.
 *   layout 2, page table: cache host [layers][pool_pages][n_heads][page_rows][head_dim] (layer_stride = pool_pages * n_heads * page_rows * head_dim, given as 0 or as
 *     that), page_rows a power of two in 16..1024, page_tab host [page_tab_len]: row r lives in page page_tab[r / page_rows]; (hi - 1) / page_rows < page_tab_len.
 *   layout 3, ring table: the same with page_tab[(r / page_rows) % page_tab_len]; the range touches at most page_tab_len pages; hi < 2^24.
 *   The table entries the range touches are checked against pool_pages here, on the host; the others may hold anything and are never read.
 * head_dim 64 | 128, layers 1..64, n_heads 1..64.  Every argument is checked before the context is bound (VOX_ERR_INVALID with a message): hi < lo, head_dim 32, a
 * ring shorter than hi - lo, an entry outside the pool never reach a launch, and nothing the kernel reads or writes lies outside the uploaded buffers. */
typedef struct {
    int32_t layers, n_heads, head_dim, lo, hi;
    int32_t layout, rows;
    int32_t page_rows, pool_pages, page_tab_len;
    int64_t layer_stride;
    const int32_t* page_tab;     /* layouts 2 and 3 only */
} vox_snapshot_kv_desc;
int32_t vox_debug_snapshot_kv(vox_ctx* ctx, const vox_snapshot_kv_desc* desc, float* cache_k, float* cache_v, float* blob, int32_t restore);
/* Test hook: launches of the linear kernels enqueued by this process so far, by kernel form (host-side counts, as above; nothing is dispatched by them):
 * out[0..2] Q4 GEMV with 1 / 2 / 4 rows per wave, [3] dense GEMV, [4] 5..16-row skinny GEMM, [5] 17..48-row skinny GEMM (one-dimensional form), [6] its split-K form,
 * [7] rows -> XF tiles (helper of [5] / [6]), [8] split-K finishing sum (helper of [6]), [9..12] 16 x 64, 16 x 128, 32 x 64, 32 x 128 tile GEMM, [13] [14] the 32 x 64 and
 * 32 x 128 tile GEMM on tile-ordered weights, [15] K % 128 != 0 GEMM, [16] 64 x 256 large-M GEMM, [17] its RoPE-epilogue form, [18] dense hi + lo GEMM, [19] wide
 * batched-decode GEMM.  Entries past [19] are written as 0. */
int32_t vox_debug_gemm_launches(uint64_t* out, int32_t cap);
/* Test hook: launch `workgroups` x 1024-thread workgroups that spin for `micros` microseconds on a side stream of the context and return at once (vox_ctx_synchronize does
 * not wait for them; vox_ctx_destroy does).  Used to test the decode engines against a GPU that is not theirs alone (tests/test_gpu_fullsize.py). */
int32_t vox_debug_occupy(vox_ctx* ctx, int32_t workgroups, int32_t micros);

/* ---- measurement hooks (bench.py roofline leg; not part of the reference surface) -------- */
/* Launch the decode-step Q4 GEMV of decoder layer `layer` (`which`: 0 qkv, 1 wo, 2 w1w3, 3 w2, 4 lm_head; 5 = the whole step as one decode-engine launch)
 * `iters` times on the ctx stream, cycling layers so weights stay HBM-cold; returns the average
 * launch duration measured with hipEvents on that stream and the algorithmic bytes per launch. */
int32_t vox_bench_decode_gemv(vox_model* m, int32_t which, int32_t iters, double* avg_us, double* bytes_per_launch,
                              const char** kernel_name);

/* The wide decode step's operators on their own (tools/wide_bench.py): operator `which` (0 q|k|v, 1 wo, 2 w1|w3, 3 w2, 4 lm_head) over `mt` = 2..4 slot groups of 16 rows,
 * `iters` launches cycling the layers; out_us[0] the GEMM launch, [1] its finishing launch, [2] both, [3] the same operator as `mt` 16-row launches back to back. */
int32_t vox_bench_wide(vox_model* m, int32_t which, int32_t mt, int32_t iters, double out_us[4]);

/* Measurement builds only (the library compiled with -DVOX_TIMELINE; VOX_ERR_UNSUPPORTED otherwise): every decode-step GEMV /
 * attention launch after _start takes the next of `n_slots` slots and each of its first `n_waves` waves stamps the 100 MHz
 * s_memrealtime counter at 4 points; _fetch copies out[n_slots][n_waves][4] back and switches the instrumentation off. */
int32_t vox_debug_timeline_start(vox_ctx* ctx, int32_t n_slots, int32_t n_waves);
int32_t vox_debug_timeline_fetch(vox_ctx* ctx, uint64_t* out, size_t cap_words, int32_t* slots_used, int32_t* meta /* [n_slots][4] {0 gemv / 1 attention, epilogue, N, K}, may be NULL */);
/* Logits tap of the batched decoder (tests).  _arm: the NEXT vox_transcribe_batch / _ex call on m (and only that one, whatever its outcome) copies, for each caller
 * index units[j] (the i of samples[i]; distinct, < that call's n), the f32 logits row each of its ids was taken from: row k of unit j is the row whose argmax is
 * out_ids[units[j]][k] -- row 0 the prefill's lm_head row, rows 1.. the decode steps', whatever the step form, the slot or a refill.  One small kernel per step in
 * front of the argmax launch, captured into the step graphs with it; without an armed tap nothing is launched.  A call that would split into sessions
 * (vox_model_set_sessions) fails with VOX_ERR_UNSUPPORTED.  _fetch (after a successful tapped call): out [n_units][max_rows][vocab] (rows past a unit's count are
 * zero), rows_per_unit[j] = rows the call produced for unit j -- more than max_rows: the rest were dropped.  VOX_ERR_INVALID: bad arguments, or nothing to fetch. */
int32_t vox_debug_batch_tap_arm(vox_model* m, const int32_t* units, int32_t n_units, int32_t max_rows);
int32_t vox_debug_batch_tap_fetch(vox_model* m, float* out, int32_t* rows_per_unit);
/* One stacked encoder + adapter run (tests): the n <= 128 host log-mels mels[i] ([128][T[i]]) through the encoder stack exactly as the batch drivers run it, layout 0 =
 * padded (every clip S_pad rows: the lock-step vox_transcribe_batch of <= 16 units), 1 = packed (every clip its own rows: one stack of the continuous batch).  out receives
 * every clip's adapter rows back to back ([rows_per_clip[i]][dec_dim] each, rows_per_clip[i] = floor(S_enc_i / 4)); cap_rows = rows out can hold.  report[4]: stacked
 * encoder rows, w2 split-K slices, wo split-K slices (0 = unsplit), q|k|v launches that ran RoPE in the GEMM's epilogue.  VOX_ERR_INVALID on bad arguments. */
int32_t vox_debug_encode_batch(vox_model* m, int32_t n, const float* const* mels, const int32_t* T, int32_t layout, float* out, int64_t cap_rows,
                               int32_t* rows_per_clip, int64_t* report);
/* The sample front ends on their own (tests), through the functions the drivers run.  form 0: the single clip's (vox_transcribe_audio: peak scale, virtual pad, log-mel;
 * n == 1, norm_group NULL); form 1: the batch drivers' (vox_transcribe_batch / _ex: host samples packed back to back -- with norm_group each unit 16-byte aligned and
 * the group peaks reduced first --, device samples read where they are).  n <= 128 units; samples[i] host or device (mem_kind), the outputs are always host memory:
 * out_scales[i] the scale unit i was multiplied by (0.95 / peak of the unit or of its group; 1 for silence or a negative group), out_mels[i] its log-mel [128][out_T[i]]
 * as the encoder receives it (room for 128 * vox_pad_len(n_samples[i]) / 160 floats), out_T[i] its frame count.  VOX_ERR_INVALID on bad arguments, before any device is touched. */
int32_t vox_debug_front_end(vox_model* m, int32_t n, const float* const* samples, const size_t* n_samples, const int32_t* norm_group_or_null, int32_t form,
                            int32_t mem_kind, float* out_scales, float* const* out_mels, int32_t* out_T);
/* The continuous batch driver's planner on its own (tests): host arithmetic only -- no context, no device.  _step_costs: the per-step cost in ms of 1..8 lock-step
 * groups (index 0 unused, written as 0) the planner prices a call with, from a cost table `base` and the step times `meas` a context has measured (0 = form not seen
 * yet); calib 0: the table alone; shared != 0: a GPU shared with other sessions (the common measured / table ratio only).  _plan_slots: job i needs steps[i] >= 1 decode
 * steps; force_G 0 = the cost model picks the group count (<= max_groups, 1..8).  Returns the group count G, for every job its slot (0 .. 16 G - 1) and its position in
 * that slot's queue, steps_g[k] / run_g[k] = the steps group k's longest slot needs / the steps group k stays active (entries past G - 1: 0), and the plan's cost. */
int32_t vox_debug_step_costs(const double base[9], const double meas[9], int32_t calib, int32_t shared, double out[9]);
int32_t vox_debug_plan_slots(const int32_t* steps, int32_t n, int32_t force_G, int32_t max_groups, const double step_ms[9], int32_t* G, int32_t* job_slot,
                             int32_t* job_qpos, int32_t steps_g[8], int32_t run_g[8], double* cost_ms);

/* ---- live streaming session (no reference counterpart: the reference transcribes finished files, bin/transcribe.rs:112-126) ------------------------------------------
 * A vox_stream is fed 16 kHz samples (or samples at its capture rate: CAPTURE RATE below) in pieces of any size and hands back token ids as soon as they are determined.  After vox_stream_finish the concatenation of
 * everything it handed back is the id sequence vox_transcribe_streaming gives for the log-mel of pad_audio(gain * x) of the concatenated samples x (gain = 0.95 / max|x|:
 * vox_transcribe_audio(x)) -- per step the logits agree to f32 summation-order noise, so the ids agree up to the first near-tie of the offline path's own logits.
 *   Cut-independence: the session advances in TICKS of one decoder position (16 mel frames -> 4 encoder rows -> 1 adapter row -> 1 decode step) however much audio a
 *   push brought, so the ids, and which call returns which id, are a function of the samples and the gain alone -- not of how they were cut into pushes, nor of what
 *   else ran on the model in between (other streams, offline calls).
 *   Schedule: decoder position p >= 37 is determined once n >= 2560 (p - 37) + 40 samples have been pushed; the step at position p yields id p - 37.  The first id is
 *   due after 40 samples, the second after 2 600; a push returns every id that became due, no later.  vox_stream_finish appends the right pad (vox_pad_cfg_voxtral) and
 *   runs the remaining ticks: vox_pad_len(n) / 2560 - 38 ids in all, the offline count.  vox_stream_schedule is the same arithmetic on the host.
 *   State: a stream owns its encoder K / V (a ring of enc_capacity_rows rows per layer and head, addressed modulo the capacity: eviction costs nothing), its decoder
 *   cache, a 65 536-sample ring, its tokens and a 16-int device block with the per-tick integers, and starts from the model's prefix state (built for its t_embed at
 *   create / reset if the model does not hold it; copied, so later changes of the model's prefix cache or t_embed do not disturb a live stream).  Several streams may live
 *   on one model (same context, one thread) in any interleaving with each other and with offline calls.  A stream may not outlive its model.
 *   Decode step: one launch of the decode engine while the stream's decoder cache has <= 1024 rows (164 s of audio; vox_model_set_decode_engine), the per-operator
 *   launches after.  An engine hand-off timeout (shared GPU) is not the caller's error: the unverified steps of the push are decoded again on the per-operator launches.
 *   One stream synchronisation per call, none per tick (a push of more than 1024 positions synchronises every 1024, and once where the decoder cache doubles: 1024, 2048,
 *   ...; host samples are copied with hipMemcpyAsync from the caller's pageable memory, which the runtime stages: the call may block there as well; a t_embed other than the
 *   model's current one is re-selected first, which synchronises).
 *   Side effects on the model: create and reset build the model's prefix state for the stream's t_embed when the model does not hold it (vox_model_set_prefix_cache's setting
 *   is restored afterwards: a model with the cache off gets it freed again) -- that runs a prefill through the model-owned decoder cache and replaces a prefix state built
 *   for another t_embed, which the next offline call with that t_embed rebuilds; results never depend on it.  As everywhere, a prefix state that cannot be allocated
 *   switches the model's prefix cache off (create / reset then fail with VOX_ERR_HIP).
 * LIMITS: one decoder position = 2560 samples = 160 ms.  A session ends at 16 384 decoder positions (the decoder RoPE table; the encoder's 65 536-position table ends at
 * the same point), about 43 minutes: later pushes are refused until vox_stream_reset -- an ENDLESS session (vox_stream_create_endless below) goes on to 2^24.  Input: 16 kHz, or the capture rate of a stream made by vox_stream_create_rate
 * (every rate pair vox_resample serves), as f32 or as signed 16-bit PCM; mono.  Q4 (GGUF) models whose conv stem
 * runs as im2col GEMMs (3 n_mels and 3 enc_dim multiples of 128); dense SafeTensors models: VOX_ERR_UNSUPPORTED.
 *
 * CAPTURE RATE (vox_stream_create_rate).  A stream created for rate sr and fed x hands back the ids of a 16 kHz stream fed vox_resample(x, sr, 16000) with the same gain:
 * every 16 kHz sample the session consumes is bit for bit the one vox_resample produces for the concatenated input -- hence the agreement with the offline path that
 * 16 kHz streams carry.  The ids, and which call returns which id (vox_stream_schedule_rate), are functions of the samples, the rate and the gain alone: not of the cuts,
 * not of the f32 / s16 mix, not of what else ran on the model or the context in between (vox_resample at other rates included: the stream owns its block matrix).
 *   Why an exact incremental form exists: the resampler is one fixed matrix applied block by block (fft_in input samples -> fft_out output samples, vox_resample_plan);
 *   output sample i reads block c = (i + delay) / fft_out in full and the tail of block c - 1, nothing else.  So after n input samples the first
 *       avail16(n) = max(0, floor(n / fft_in) * fft_out - delay)
 *   output samples are final; the stream produces exactly those (stream_resample_kernel, from a ring of input samples) and runs the ticks they make due.  At
 *   vox_stream_finish the rest, up to vox_resample_len(n) = ceil(n * 16000 / sr), is produced with the blocks clipped at n as vox_resample clips them at the end of a file;
 *   then the right pad follows.
 *   Added latency, from the plan alone: (fft_in + delay * fft_in / fft_out) / sr seconds --
 *       48 kHz 16 ms | 44.1 kHz 30 ms | 32 kHz 24 ms | 22.05 kHz 60 ms | 8 kHz 96 ms | 11.025 kHz 120 ms          (a tick has 160 ms)
 *   State: in addition to a 16 kHz stream's, a ring of input-rate samples (a power of two holding two blocks and a feed chunk) and the rate pair's block matrix
 *   (2 fft_out x fft_in f32, e.g. 0.7 MB at 48 kHz, 2.3 MB at 44.1 kHz); both are counted in vox_stream_info's bytes.  Still one synchronisation per call.
 * 16-BIT PCM (vox_stream_push_s16) works on every stream: sample v enters as float(v) / 32768 (exact in f32; the mono 16-bit scale of audio/io.rs:110-113), so a push of v
 * equals vox_stream_push of those floats, and the two may alternate on one stream. */
typedef struct vox_stream vox_stream;
/* gain: every sample is multiplied by it before the mel (a stream has no file peak; 1.0 = as given).
 * enc_capacity_rows: rows of the encoder K / V ring, 0 = enc_window + 8 rounded up to a multiple of 64 (768: 0.4 GB of K / V per stream at full size; a ring needs no
 *   slack, any capacity above enc_window + 4 gives the same bits); must exceed enc_window + 4.
 * max_positions: decoder positions the session can reach, 0 = the decoder RoPE table (16 384). */
int32_t vox_stream_create(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, vox_stream** out);
/* vox_stream_create for input at sample_rate Hz.  16000: vox_stream_create itself.  Any other rate: the stream also owns its input ring and its block matrix (built here;
 * synchronises).  Rate pairs vox_resample refuses (block matrix above 64 MB: rates without a large common divisor, e.g. 44101 Hz) and blocks that do not fit the input
 * ring: VOX_ERR_UNSUPPORTED; rate 0: VOX_ERR_INVALID. */
int32_t vox_stream_create_rate(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, uint32_t sample_rate, vox_stream** out);
/* ENDLESS SESSIONS.  vox_stream_create_rate for a session whose limit is 2^24 decoder positions (31 days) instead of 16 384: its decoder cache is a RING of dec_ring_rows
 * rows and its RoPE rows are made for the positions it is at, so device memory stops growing once the ring is full.  Every other vox_stream_* call works on it unchanged
 * (push, push_s16, finish, peek, reset, info, scores, alternatives, the taps); everything vox_stream_create_rate refuses is refused here; a push that would pass 2^24
 * positions is refused before anything changes.
 *   dec_ring_rows: 0 = dec_window + 1 + TAIL rounded up to a multiple of 64 (8256 rows: 1.7 GB of K / V at full size, against the 3.4 GB of a 16 384-row flat cache).
 *   TAIL = 63 is the most ticks one finish / peek tail may run: the backlog of the rate's unfinished block plus the right pad (vox_stream_peek_ids' arithmetic), computed
 *   for the session's rate at create -- a rate whose tail is longer: VOX_ERR_UNSUPPORTED.  A given value must be at least dec_window + 1 + TAIL (VOX_ERR_INVALID, the
 *   message names the minimum) and at most 16 384; it need not be a power of two.
 *   Up to position dec_ring_rows the session runs a bounded session's code -- the engine up to 1024 rows, then the per-operator step on a flat cache that doubles up to
 *   dec_ring_rows rows, the load-time RoPE tables -- and its logits are a bounded session's, bit for bit.  From position dec_ring_rows on, position p lives at cache row
 *   p % dec_ring_rows: the q|k|v GEMV appends there and takes its RoPE row from the session's ring, the per-head ring attention follows, then the wo GEMV; the encoder's
 *   ring attention reads its RoPE rows from the session's ring as well.  The fused attention + wo launch has no ring form: on the full-size model the step changes from
 *   fused to unfused sums at the wrap, so logits stay within the 2e-4 bound there and are not bit-equal; geometries that never fuse stay bit-equal throughout.
 *   RoPE rows: two device rings per session (1024 decoder rows, 4096 encoder rows), refilled by the host in front of each pass for exactly the positions the pass
 *   runs; below the load-time table lengths a row has the table's bits, beyond them the angle is formed in double (vox_debug_rope_rows).
 *   Peek: past the wrap a peek's tail overwrites ring rows that lay outside the window of every later position -- what the TAIL rows are for; nothing is saved.
 *   Memory: vox_stream_info [5] is constant once the ring is full, apart from the position-indexed device lists -- the tokens (4 bytes per position) and, when on,
 *   the score (16) and alternatives (72) records -- which GROW BY DOUBLING (from dec_ring_rows positions, at a verification point: one more synchronisation per
 *   doubling) and are counted as they are.  The host record lists behind vox_stream_scores / vox_stream_alternatives grow with the utterance, 88 bytes per id, and are
 *   not trimmed.  vox_stream_info [1] keeps counting positions.
 *   Not served: stream groups (slab or paged), a ring form of the fused attention + wo launch, paging for a solo stream, trimming the host record lists. */
int32_t vox_stream_create_endless(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t dec_ring_rows, uint32_t sample_rate, vox_stream** out);
/* A BURST stream ("Bursts"): a stream that runs a backlog's ticks in bursts of up to burst_ticks (1..VOX_STREAM_BURST_MAX; 1: exactly the stream
 * the creators above make -- the same launches and allocations).  When one pass of a push / finish / peek has several ticks due (a chunked feed, a file, a session
 * that fell behind or was restored with audio waiting), the encoder of b of them runs as ONE pass of 4 b rows -- every weight matrix read once, the ring attention
 * in its burst form (vox_debug_stream_attn_burst) -- followed by the b decode steps, one by one as in a tick.  A burst is the smallest of the ticks still due, burst_ticks
 * and the distance to the next position where the host acts between ticks (decoder cache growth, an endless session's wrap, list growth, the verification limit:
 * vox_stream_burst_len); a burst of 1 is a plain tick, so a burst stream fed one tick per call has a plain stream's bits.  In a burst the row count selects other GEMM
 * kernels than a tick's 4 rows do (as in a stream group): ids equal a plain stream's up to near-ties, and so depend on how the samples were cut, up to near-ties.
 *   endless (0 / 1), dec_ring_rows: vox_stream_create_endless's (dec_ring_rows 0 unless endless); max_positions: a bounded stream's, ignored when endless.
 *   enc_capacity_rows: 0 = max(window + 4 burst_ticks + 4, prefix rows) rounded up to 64 (832 rows at 16 for the 750 window); a given value must exceed window +
 *   4 burst_ticks (VOX_ERR_INVALID before anything is allocated; the message names the bound).
 * Scores, alternatives, taps, peek, reset, snapshot and restore work as on any stream (a blob does not know its ring capacity).  Stream groups have bursts of their own: vox_stream_group_create_burst.  Not served: burst_ticks above 16. */
#define VOX_STREAM_BURST_MAX 16
int32_t vox_stream_create_burst(vox_model* m, const float* t_embed, float gain, int32_t enc_capacity_rows, int32_t max_positions, uint32_t sample_rate, int32_t endless,
                                int32_t dec_ring_rows, int32_t burst_ticks, vox_stream** out);
/* burst_ticks of the stream (1: a plain stream), the bursts run with b >= 2 since create / reset / restore, the ticks inside them, the ticks run one by one (a peek's
 * tail is not counted: the peek takes it back) */
int32_t vox_stream_burst_info(const vox_stream* s, int64_t out[4]);
/* host only, a pure function: the length of the next burst of a pass with `due` ticks still to run, at decoder position pos, of a stream with burst_ticks = burst, when
 * next_stop is the nearest position above pos where the host must act between ticks: max(1, min(due, burst, next_stop - pos)).  A burst never spans next_stop. */
int32_t vox_stream_burst_len(int64_t due, int32_t burst, int64_t pos, int64_t next_stop);
/* samples host or device (mem_kind), ids host.  cap smaller than the ids the call will produce (known from the schedule before any work), a push after finish, a push
 * that would pass max_positions: VOX_ERR_INVALID BEFORE any state changes -- the call can be repeated. */
int32_t vox_stream_push(vox_stream* s, const float* samples, size_t n, int32_t mem_kind, int32_t* out_ids, int32_t cap, int32_t* n_ids);
/* vox_stream_push for signed 16-bit PCM at the stream's rate (host or device memory; host samples pass through a bounded device staging buffer, allocated at the first
 * such push and counted in vox_stream_info's bytes from then on).  The same refusals, before any state changes. */
int32_t vox_stream_push_s16(vox_stream* s, const int16_t* samples, size_t n, int32_t mem_kind, int32_t* out_ids, int32_t cap, int32_t* n_ids);
int32_t vox_stream_finish(vox_stream* s, int32_t* out_ids, int32_t cap, int32_t* n_ids);
int32_t vox_stream_reset(vox_stream* s);          /* back to the state after create: the next push starts a new utterance */
int32_t vox_stream_free(vox_stream* s);
/* samples pushed (as pushed: at the stream's input rate), decoder positions done, ids handed out, encoder stream position, encoder ring rows in use, device bytes held,
 * decode steps run on the engine, decode steps run per operator */
int32_t vox_stream_info(const vox_stream* s, int64_t out[8]);
/* host only: after n_samples pushed (finished = 0) or at the end of an n_samples utterance (finished = 1): decoder positions determined, ids due */
int32_t vox_stream_schedule(size_t n_samples, int32_t finished, int32_t* positions, int32_t* ids);
/* the same for a stream fed at sample_rate Hz: *samples_16k = avail16(n_samples) (finished = 0) or vox_resample_len(n_samples) (finished = 1), positions and ids are
 * vox_stream_schedule's for that many 16 kHz samples.  Rate 16000 gives vox_stream_schedule's answers.  Push and finish check `cap` against this schedule. */
int32_t vox_stream_schedule_rate(size_t n_samples, uint32_t sample_rate, int32_t finished, int32_t* positions, int32_t* ids, size_t* samples_16k);
/* SCORES.  With scores on, every id the stream hands out comes with a vox_token_score (above) computed from the f32 logits row of its decode step: one more launch per
 * tick behind the tick's last kernel (plus, on the per-operator decode step, the logits row written out) and one more copy in front of the call's one synchronisation;
 * the ids themselves do not change, and a stream that never turns scores on allocates and launches nothing.  The records are bit for bit a function of what the ids are a
 * function of.  vox_stream_set_scores: on = 0 / 1, takes effect with the next push / finish, survives vox_stream_reset; the first on = 1 allocates the records (16 bytes
 * per position the stream was created for) and one logits row on the device, counted in vox_stream_info [5] from then on.
 * vox_stream_scores: the records of ids [first_id, first_id + n) of the current utterance from a host array the stream keeps (no device is touched); the range must lie
 * within the ids handed out so far (vox_stream_info [2]), else VOX_ERR_INVALID and nothing is written.  An id handed out while scores were off has logprob = margin = NaN,
 * runner_up = -1 and its id.  Steps a decode-engine hand-off timeout takes back are scored again from the re-run's logits. */
int32_t vox_stream_set_scores(vox_stream* s, int32_t on);
int32_t vox_stream_scores(const vox_stream* s, int32_t first_id, int32_t n, vox_token_score* out);
/* PEEK.  vox_stream_peek returns the ids vox_stream_finish would return now -- vox_stream_peek_ids of them: vox_stream_schedule_rate(samples pushed, rate, finished = 1)
 * minus the ids handed out -- and leaves the stream what it was, bit for bit: the ids and logits of every later call, the decoder cache's size and engine binding,
 * vox_stream_info [0..4], [6], [7].  It takes no samples: push first, then peek; it may be repeated, and followed by a push, a finish or a reset alike.  The stream runs
 * finish's ticks (the right pad, the rest of a rate stream's last block) and takes them back: the encoder ring rows they overwrite and the state block are saved in front
 * of them and restored behind them by one launch each (the save area, 21 MB at full size, is allocated at the first peek and counted in vox_stream_info [5] from
 * then on), the host takes back its own counters, and a decoder cache that grew inside the tail gets its old planes back.  Still one synchronisation per call.
 * Refusals are vox_stream_finish's, before anything changes: a finished stream, cap below the count, a tail past max_positions.
 * scores_or_null: the records of the peeked ids (with scores off: NaN, NaN, -1, id); the stream's own list (vox_stream_scores) is not extended. */
int32_t vox_stream_peek(vox_stream* s, int32_t* out_ids, int32_t cap, int32_t* n_ids, vox_token_score* scores_or_null);
/* host only: the ids a peek returns after n_samples pushed at sample_rate Hz with ids_out ids handed out (more than the utterance has: VOX_ERR_INVALID) */
int32_t vox_stream_peek_ids(size_t n_samples, uint32_t sample_rate, int32_t ids_out, int32_t* n);
/* ALTERNATIVES.  With k > 0, every id the stream hands out also comes with a vox_token_alts (above) of its decode step's logits row: one more launch per tick, behind the
 * score launch if there is one, and one more copy in front of the call's one synchronisation; the ids do not change, and a stream that never asks allocates and launches
 * nothing.  vox_stream_set_alternatives: k = 0 (off, the default) .. VOX_MAX_ALTERNATIVES, takes effect with the next push / finish / peek, survives vox_stream_reset; the
 * first k > 0 allocates the records (72 bytes per position the stream was created for) and, unless scores did, one logits row, counted in vox_stream_info [5] from then on.
 * vox_stream_alternatives: the records of ids [first_id, first_id + n) of the current utterance from a host array the stream keeps (no device is touched); the range must
 * lie within the ids handed out so far, else VOX_ERR_INVALID and nothing is written.  An id handed out while alternatives were off has entropy = NaN, n = 0 and every entry
 * {-1, NaN}; a record made at k has n <= k whatever k is now.  vox_stream_reset starts the list over.
 * vox_stream_peeked_alternatives: the records of the ids the LAST vox_stream_peek returned (*n of them; cap < that: VOX_ERR_INVALID), copied in front of that peek's one
 * synchronisation into a host array of the stream's; they equal bit for bit what finish then appends for the same ids, never enter the stream's own list, and are valid
 * until the next push / finish / peek / reset -- after that *n = 0. */
int32_t vox_stream_set_alternatives(vox_stream* s, int32_t k);
int32_t vox_stream_alternatives(const vox_stream* s, int32_t first_id, int32_t n, vox_token_alts* out);
int32_t vox_stream_peeked_alternatives(const vox_stream* s, vox_token_alts* out, int32_t cap, int32_t* n);
/* LEVELS.  With levels on, every id the stream hands out also comes with a vox_tick_level (above): one more launch per tick -- per burst, with a block per tick -- in
 * front of the tick's mel launch, reading the tick's 2560 new samples (10 KB), and one more copy in front of the call's one synchronisation; the ids and logits do not
 * change, and a stream that never turns levels on allocates and launches nothing.  vox_stream_set_levels: on = 0 / 1, takes effect with the next push / finish / peek,
 * survives vox_stream_reset (which starts the records over); the first on = 1 allocates the records (8 bytes per position the stream was created for; an endless
 * stream's list grows with its others), counted in vox_stream_info [5] from then on.
 * vox_stream_levels: the records of ids [first_id, first_id + n) of the current utterance from a host array the stream keeps (no device is touched); the range must lie
 * within the ids handed out so far, else VOX_ERR_INVALID and nothing is written; while levels are off: VOX_ERR_INVALID.  An id handed out while levels were
 * off has (NaN, NaN).  A decode-engine hand-off timeout repeats decode steps, never a tick: level records are not computed again.  A peek's tail ticks write their
 * records behind the stream's position, where the stream's own ticks overwrite them; the stream's list is not extended and there is no call for a peek's records (a
 * tail is mostly pad).  A session blob carries no level records: after vox_stream_restore the ids handed out so far have (NaN, NaN), later ids the records of the
 * uninterrupted session; the restored stream's own flag is what counts.
 * vox_stream_quiet: the end-of-speech hint -- *ticks = the number of trailing records of the ids handed out in the current utterance whose peak < peak_below (finite,
 * > 0); a NaN record ends the run.  Host memory only.  ticks x 160 ms is the quiet time as of the last id k handed out, that is as of sample 2560 k. */
int32_t vox_stream_set_levels(vox_stream* s, int32_t on);
int32_t vox_stream_levels(const vox_stream* s, int32_t first_id, int32_t n, vox_tick_level* out);
int32_t vox_stream_quiet(const vox_stream* s, float peak_below, int32_t* ticks);
/* test tap, modelled on vox_debug_batch_tap_*: from now on keep the f32 logits row behind each id handed out (up to max_rows); fetch copies them to the host
 * ([min(rows, max_rows)][vocab]; *rows = rows produced since arm) and ends the tap */
int32_t vox_debug_stream_tap_arm(vox_stream* s, int32_t max_rows);
int32_t vox_debug_stream_tap_fetch(vox_stream* s, float* out_rows_x_vocab, int32_t* rows);
/* while a tap is armed: the `rows` logits rows the last vox_stream_peek left behind the tap's position ([rows][vocab]; the tap must have room for them).  The tap goes on. */
int32_t vox_debug_stream_tap_peeked(vox_stream* s, float* out_rows_x_vocab, int32_t rows);
/* front-end tap (tests), same rules as the logits tap (an arm drops the rows of an earlier arm, fetch ends the tap, vox_stream_reset starts the count again): while armed
 * every tick copies, device to device on the stream and without synchronising, its 16 fresh log-mel frames ([16][n_mels], token-major: frames 16 p .. 16 p + 15 of the
 * tick at decoder position p) and its 4 conv-stem rows ([4][enc_dim], the encoder's input rows 4 p .. 4 p + 3); nothing is launched when no tap is armed.  A decode
 * engine hand-off re-run repeats decode steps, never ticks, so the tick count and the rows do not depend on it.  _fetch: out_mel [min(ticks, max_ticks)][16][n_mels],
 * out_conv [min(ticks, max_ticks)][4][enc_dim], *ticks = ticks run since arm. */
int32_t vox_debug_stream_front_tap_arm(vox_stream* s, int32_t max_ticks);
int32_t vox_debug_stream_front_tap_fetch(vox_stream* s, float* out_mel, float* out_conv, int32_t* ticks);

/* ---- SNAPSHOT AND RESUME (no reference counterpart): a live session taken off the GPU as one byte string and put back into any stream of the same model -----------------
 * Between two calls a session is a closed set of device arrays and a small host mirror.  vox_stream_snapshot writes what a LATER TICK CAN STILL READ of them, in logical
 * order, into one contiguous, position-independent blob; vox_stream_restore makes a stream continue from it.  The stream that restores need not be the one that
 * snapshotted, nor have its encoder ring capacity, its max_positions or its kind (bounded / endless): a parked session holds no device memory at all (free the
 * stream), a session can move to another process or GPU with the same model file, survive a restart, or be forked into two.
 *   Blob: a header of VOX_SNAPSHOT_HEADER_BYTES, then up to VOX_SNAPSHOT_SECTIONS sections, each at a 16-byte boundary, the padding zero:
 *     [0] [1] encoder K, V   [enc_layers][enc_heads][We][enc_head_dim] f32, the rows E - We .. E - 1 of the encoder stream position E, We = min(E, enc_window): the keys
 *                            the next query row attends;
 *     [2] [3] decoder K, V   [dec_layers][dec_kv_heads][Wd][dec_head_dim] f32, the rows D - Wd .. D - 1 of the decoder position D, Wd = min(D, dec_window) (no window: D);
 *     [4] the 16 kHz sample ring in logical order: the last min(samples written, 65 536) samples;  [5] a rate stream's input-rate ring likewise (empty at 16 kHz);
 *     [6] the utterance's tokens 0 .. D (i32);  [7] the vox_token_score records of the ids handed out, when scores are on;  [8] the vox_token_alts records, when k > 0.
 *   The header holds: magic, format version (VOX_SNAPSHOT_VERSION), total bytes; a model fingerprint and a hash of the bits of the session's t_embed; gain, sample
 *   rate, samples pushed and the other feed counters a later call depends on; D and E; the ids handed out, the scores flag and the alternatives k; the token at
 *   position D; the model geometry the K / V sections are laid out by; offset and length of every section.  Byte order and float format are the writing machine's.
 *   NOT in the blob (rebuilt, or simply absent after a restore): test taps, the peek save area, the decode engine's binding, RoPE rings, staging buffers, the kept
 *   adapter rows (a snapshot is taken at a verification point), K / V rows outside the windows.  Two snapshots of an untouched session are byte-identical.
 *   The model fingerprint covers the vox_model_cfg words, the byte count of the weights as parsed from the file and a 64-bit hash of a few KB of them (read back once
 *   per model, at its first snapshot or restore).  It is there to stop a blob from going into the WRONG MODEL BY MISTAKE; it proves nothing about integrity, and a blob
 *   is not inspected beyond its header's arithmetic.
 * vox_stream_snapshot_size: the bytes vox_stream_snapshot would write now (host arithmetic: vox_snapshot_bytes_for on the session's counters).
 * vox_stream_snapshot: leaves the stream exactly as it was (nothing of it is written; a finished stream is refused: a reset starts its next utterance).  mem_kind
 *   VOX_MEM_DEVICE: the K / V sections are packed straight into the caller's device buffer (16-byte aligned) by one kernel launch per stack, everything else by copies;
 *   VOX_MEM_HOST: the K / V sections pass through a device staging area of at most 64 MB -- two halves used alternately, each packed by one launch and then downloaded
 *   -- allocated for the call and freed at its end: vox_stream_info[5] is afterwards what it was.  Synchronisations: one at the start (the token at D), one at the end.
 *   cap < the size is refused.
 * vox_stream_restore: replaces the target's utterance, as vox_stream_reset followed by a replay of the blob's samples would; takes the blob's gain; keeps the target's
 *   own scores / alternatives settings (records the blob does not hold read as "off" records).  Everything is checked before anything changes -- a refused call leaves
 *   the target bit for bit what it was: the header's magic, version, length and section table (vox_snapshot_describe's refusals), the fingerprint, the t_embed hash, a
 *   sample rate other than the stream's, D at or beyond the target's max_positions, a token outside the vocabulary.  With a device blob the header is downloaded and
 *   checked first.  After the payload copies the header's VALIDATED token is written at tokens[D]: the embedding lookup never reads an unchecked index.
 *   Placement: a bounded target gets the decoder cache size the doubling rule gives an uninterrupted session at D (the decode engine serves exactly the positions it
 *   would have served); an endless target places the rows at row % dec_ring_rows (flat below the wrap) and grows its lists as its own rule would have; the encoder
 *   rows go to row % capacity of the target's ring.  Everything after a restore into a stream of the same kind is bit for bit what the uninterrupted session gives
 *   (an endless target past its wrap: the relation ENDLESS SESSIONS documents).
 * Members of a stream group (vox_stream_group_snapshot_size / _snapshot / _restore, declared behind the group's own entries): the same three calls with (group,
 *   member) in front, on slab, paged and endless paged groups.  The format does not know the difference: a solo stream's blob restores into a member and the other
 *   way round.  A restore sets the member's rate from the blob, as vox_stream_group_reset_rate does (so a rate mismatch is no refusal here), and takes the blob's
 *   gain.  A paged restore is planned like an advance: the pages the member holds now count as free, the pages vox_stream_group_pages_for(D) names are needed; a pool
 *   without room refuses (the message names the member, the pages needed and the pages free) and the group is untouched.  A slab member refuses a blob at or beyond
 *   the slab's max_positions.  A member restored into the SAME slot of a group fed the same calls continues bit for bit (ids, logits, records, pool counts and pages
 *   held; the physical page numbers may differ); across slots or kinds the continuation is the session's up to f32 summation order (the round width selects the GEMM
 *   kernels), as between a group and a solo stream anyway.
 * Out of scope: blobs across model geometries or t_embeds, compression or a narrower dtype in the blob, the offline and batch paths, incremental snapshots.
 * vox_snapshot_describe (host arithmetic, no device): validates the header at the start of a blob of nbytes bytes -- reads at most VOX_SNAPSHOT_HEADER_BYTES of it;
 *   a caller that holds only the header of a longer blob passes the blob's length -- and decodes it.  vox_snapshot_bytes_for: the blob size of a session of this
 *   geometry at decoder position `positions` (>= 37) after n_samples pushed samples at sample_rate, with (1) or without (0) its score / alternatives records: what a
 *   server budgets its host memory by. */
#define VOX_SNAPSHOT_VERSION 1
#define VOX_SNAPSHOT_HEADER_BYTES 288
#define VOX_SNAPSHOT_SECTIONS 9
typedef struct {
    int32_t version; uint32_t sample_rate; float gain; int32_t token;
    uint64_t total_bytes, fingerprint, t_embed_hash;
    int64_t samples_pushed, samples_16k, samples_in;
    int32_t positions, enc_position, ids, scores, alternatives, n_scores, n_alts, enc_rows, dec_rows, reserved;
    uint64_t section_offset[VOX_SNAPSHOT_SECTIONS], section_bytes[VOX_SNAPSHOT_SECTIONS];
} vox_snapshot_info;
int32_t vox_snapshot_describe(const void* blob, size_t nbytes, vox_snapshot_info* out);
int32_t vox_snapshot_bytes_for(const vox_model_cfg* cfg, int64_t positions, uint32_t sample_rate, size_t n_samples, int32_t scores, int32_t alternatives, size_t* out);
int32_t vox_stream_snapshot_size(const vox_stream* s, size_t* nbytes);
int32_t vox_stream_snapshot(vox_stream* s, void* blob, size_t cap, size_t* nbytes, int32_t mem_kind);
int32_t vox_stream_restore(vox_stream* s, const void* blob, size_t nbytes, int32_t mem_kind);

/* ---- stream group: up to 16 live sessions advanced together (no reference counterpart) ---------------------------------------------------------------------------------
 * A vox_stream_group holds n_members member sessions on one model -- at one t_embed for all, or, made by vox_stream_group_create_t_embeds, each at its own (A DELAY PER
 * MEMBER below) --, each with its own gain, sample ring, encoder K / V ring and slice of the group's
 * decoder cache.  vox_stream_group_advance feeds any subset of the members (f32 samples at each member's rate, host or device memory: mem_kind holds for the whole
 * call; vox_stream_group_advance_s16: signed 16-bit PCM) and advances them together: every weight matrix is read by ONE launch per tick for all members that have a tick due, and the call synchronises once.
 *   Contract: a member's schedule is vox_stream_schedule's on that member's own sample count; every call hands each fed member exactly the ids that became due, and a
 *   member fed with finish = 1 ends its utterance with those samples (right pad, remaining ids: vox_pad_len(n) / 2560 - 38 in all).  A member's ids are those of a solo
 *   vox_stream with the same gain fed the same samples in the project's usual sense -- its logits stay within f32 summation-order noise (2e-4 of the largest logit) of the
 *   teacher-forced logits, so its ids change only after a near-tie.  They are NOT claimed bit-identical to the solo stream's: the number of members that tick together
 *   selects the GEMM kernels (4 rows per member through the encoder, 1 through the decoder), so a member's last bits depend on who else is due.  A solo vox_stream keeps
 *   its bit-for-bit claims.
 *   Refusals happen before anything changes (the call can be repeated, vox_stream_group_info is unchanged): cap below the ids due for an entry, a member fed twice in one
 *   call, a finished member fed before its vox_stream_group_reset, a push past max_positions, a bad member or mem_kind.
 *   Decode step: the batched step's launch chain on the group's cache slab [layer][member][kv_head][max_positions][head_dim], which does not grow: max_positions = 0
 *   selects 2048 (5.4 minutes; at full size 0.21 MB per position, 0.44 GB per member) and a member that reaches it is refused until its reset.  Each member also holds an
 *   encoder ring (enc_capacity_rows as vox_stream_create's: 0.4 GB at full size).  The decode engine is not used.  SLAB LIMIT: on a model whose step takes the GQA
 *   decode attention (head_dim 128, dec_heads == 4 dec_kv_heads: the full-size model) that kernel keeps 16 max_positions bytes of scores in LDS, of which a workgroup
 *   may ask for 160 KB less the kernel's static share: creation refuses (VOX_ERR_INVALID, nothing allocated) a slab group above that many positions -- 9 976 with this
 *   build; the message names the limit, vox_debug_attn_gqa_max_seq returns it.  Other models' slab groups take up to the session limit (16 384), and
 *   a paged group (PAGED DECODER CACHE below) has no such bound and grows into a pool.
 *   Creation refuses (VOX_ERR_UNSUPPORTED) what vox_stream_create refuses and models without tile-ordered Q4 weights; n_members outside 1..16 is invalid.
 *   gains: one per member, null = 1.0 each.
 * CAPTURE RATE AND 16-BIT PCM.  The rate is member state (vox_stream_group_create_rates, vox_stream_group_reset_rate; 16000 unless set), the sample format belongs to the
 * call, as mem_kind does: vox_stream_group_advance_s16 reads every entry's samples as int16_t (sample v enters as float(v) / 32768, exact), and the two calls may alternate
 * on one group.  A member at rate sr follows vox_stream_schedule_rate on its own count of input-rate samples (cap, max_positions and the finish target are checked against
 * it; vox_stream_group_info [0] counts samples as pushed) and consumes, bit for bit, the 16 kHz samples vox_resample gives for its concatenated input: CAPTURE RATE above
 * holds for a member unchanged, the added-latency table included.
 *   Invariant: a call in which every entry fits its rings in one pass runs exactly the rounds -- the same order, the same widths -- that a 16 kHz group runs when fed,
 *   in the same call, x16[a:b] per member, x16 = vox_resample(x, sr, 16000), a and b the member's 16 kHz sample counts before and after the call (the third value of
 *   vox_stream_schedule_rate; vox_resample_len at finish).  So such a group equals that 16 kHz group bit for bit, ids and logits.
 *   How: in every pass all fed members' samples become 16 kHz samples in ONE resampling launch (behind ONE conversion launch when the call is 16-bit), in front of the
 *   pass's rounds; the call still synchronises once.  Host 16-bit samples pass through a device staging area of the group (65 536 samples per member, allocated at the
 *   first such call and counted in the bytes from then on); device samples are read in place.
 *   State per rate != 16000: the group owns ONE block matrix per rate in use (vox_resample's bits, never the context's matrix), shared by the members at that rate and freed
 *   when the last of them leaves it or with the group; each such member owns an input ring sized as a solo stream's.  vox_stream_group_info [5] counts the member's ring
 *   and its share of the matrix.  Rates vox_stream_create_rate refuses: VOX_ERR_UNSUPPORTED; rate 0: VOX_ERR_INVALID; a refused vox_stream_group_reset_rate leaves the
 *   member, its rate and its state as they were. */
typedef struct vox_stream_group vox_stream_group;
typedef struct {
    int32_t member;            /* 0 .. n_members-1, at most one entry per member per call */
    int32_t finish;            /* 1: after these samples the member's utterance ends (right pad, remaining ids) */
    const float* samples;      /* at the member's rate, mem_kind of the call: f32, or int16_t for vox_stream_group_advance_s16; may be null when n_samples == 0 */
    size_t n_samples;
    int32_t* out_ids; int32_t cap;
    int32_t n_ids;             /* out */
} vox_stream_feed;
int32_t vox_stream_group_create(vox_model* m, const float* t_embed, int32_t n_members, const float* gains /* null: 1.0 */,
                                int32_t enc_capacity_rows, int32_t max_positions, vox_stream_group** out);
/* vox_stream_group_create with a rate per member (null: 16000 each); a member at another rate also owns its input ring, the group one block matrix per rate */
int32_t vox_stream_group_create_rates(vox_model* m, const float* t_embed, int32_t n_members, const float* gains /* null: 1.0 */, const uint32_t* rates /* null: 16000 each */,
                                      int32_t enc_capacity_rows, int32_t max_positions, vox_stream_group** out);
int32_t vox_stream_group_advance(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, int32_t mem_kind);
/* vox_stream_group_advance with every entry's `samples` pointing at int16_t samples at that member's rate; the same refusals, before anything changes */
int32_t vox_stream_group_advance_s16(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, int32_t mem_kind);
int32_t vox_stream_group_reset(vox_stream_group* g, int32_t member, float gain);   /* member back to the prefix state: the next connection, at the member's current rate */
/* the same for a connection that delivers sample_rate Hz (may build that rate's matrix: synchronises) */
int32_t vox_stream_group_reset_rate(vox_stream_group* g, int32_t member, float gain, uint32_t sample_rate);
/* vox_stream_info's eight words for the member; [5] is the member's share of the group's device bytes, [6] is 0 (no engine step), [7] counts the member's ticks */
int32_t vox_stream_group_info(const vox_stream_group* g, int32_t member, int64_t out[8]);
int32_t vox_stream_group_free(vox_stream_group* g);
/* vox_stream_set_scores / vox_stream_scores for one member (SCORES above): the flag survives the member's resets; a round launches the score kernel once for all its
 * slots, and only while some member has scores on; the member's records are counted in vox_stream_group_info [5] */
int32_t vox_stream_group_set_scores(vox_stream_group* g, int32_t member, int32_t on);
int32_t vox_stream_group_scores(const vox_stream_group* g, int32_t member, int32_t first_id, int32_t n, vox_token_score* out);
/* vox_stream_peek (PEEK above) for any subset of the members in one call: every entry names a member, out_ids and cap and gets n_ids; its n_samples and finish must be 0.
 * The entries' ids are those vox_stream_group_advance would hand the same members finishing now, and the group -- the peeked members and the others -- stays what it
 * was.  One ring save and one restore launch for all entries, one synchronisation, as advance.  Refusals are advance's for finishing entries (and samples or a finish
 * flag in an entry), before anything changes.  scores_or_null: one array per entry (entries whose pointer is null get none), as vox_stream_peek's.  The save area
 * holds a slot per entry of the largest peek so far and is counted in the group's device bytes. */
int32_t vox_stream_group_peek(vox_stream_group* g, vox_stream_feed* feeds, int32_t n_feeds, vox_token_score* const* scores_or_null);
/* vox_stream_set_alternatives / vox_stream_alternatives / vox_stream_peeked_alternatives for one member (ALTERNATIVES above): k survives the member's resets; a round
 * launches the alternatives kernel once for all its slots, and only while some member has k > 0; the member's records are counted in vox_stream_group_info [5] */
int32_t vox_stream_group_set_alternatives(vox_stream_group* g, int32_t member, int32_t k);
int32_t vox_stream_group_alternatives(const vox_stream_group* g, int32_t member, int32_t first_id, int32_t n, vox_token_alts* out);
int32_t vox_stream_group_peeked_alternatives(const vox_stream_group* g, int32_t member, vox_token_alts* out, int32_t cap, int32_t* n);
/* vox_stream_set_levels / vox_stream_levels / vox_stream_quiet for one member (LEVELS above): the flag survives the member's resets; a round -- a burst round with a
 * block per tick and slot -- launches the level kernel once for all its slots, and only while some member has levels on; the member's records have the bits a solo
 * stream fed the same samples at the same gain has, and are counted in vox_stream_group_info [5] */
int32_t vox_stream_group_set_levels(vox_stream_group* g, int32_t member, int32_t on);
int32_t vox_stream_group_levels(const vox_stream_group* g, int32_t member, int32_t first_id, int32_t n, vox_tick_level* out);
int32_t vox_stream_group_quiet(const vox_stream_group* g, int32_t member, float peak_below, int32_t* ticks);
/* vox_debug_stream_tap_* for one member (the rows are copied by the tick's last kernel; a reset of the member starts the count again) */
int32_t vox_debug_stream_group_tap_arm(vox_stream_group* g, int32_t member, int32_t max_rows);
int32_t vox_debug_stream_group_tap_fetch(vox_stream_group* g, int32_t member, float* out, int32_t* rows);
/* PAGED DECODER CACHE.  vox_stream_group_create_paged makes a group whose decoder cache is ONE pool of fixed-size K / V pages instead of a slab slice per member: K and V
 * pools [layer][pool_pages][kv_head][page_rows][head_dim], page_rows a power of two in 16..1024 (0: 256).  Logical page q of a member holds its cache rows q * page_rows ..
 * (q + 1) * page_rows - 1.  A member holds only the pages its positions occupy: it takes a page when a call's ticks cross a page boundary, returns every page at its
 * reset (and takes the seed's), and returns the pages that have fallen out of the decoder's sliding window after each committed call -- for a member at position P the
 * logical pages below max(0, P - window) / page_rows, which no later step reads.  So a member's memory follows its length and stops growing at the window, and
 * max_positions may be anything up to the session limit (the RoPE tables: 16 384 positions; 0 selects it); the refusal at max_positions stays per member.
 *   pool_pages: 0 selects n_members * ceil(2048 / page_rows), the memory of the default slab.  A pool that cannot hold every member's seed (ceil(37 / page_rows) pages
 *   each) is refused, as are a page_rows that is no power of two in range and a max_positions above the session limit.
 *   A call is planned before anything changes: the logical pages its entries' ticks enter are counted, and a call that needs more than the pool has free is refused
 *   (VOX_ERR_INVALID, the message names the pool, the member and both counts); the group is untouched and the call can be repeated, e.g. after another member's reset.
 *   Pages are not freed inside a call.  A peek takes the pages its tail enters and returns them when the tail is taken back: pool and tables are what they were.
 *   Contract: the same sequence of calls gives a paged group and a slab group the same ids and the same logits, bit for bit -- the decode step is the slab group's launch
 *   chain, its attention reading K / V through the members' page tables (one launch per layer, as the slab's) and its q|k|v GEMM appending into the member's page.
 *   Everything else of a group -- advance, its 16-bit form, peek, reset, info, scores, alternatives, taps -- works on a paged group unchanged.
 * vox_stream_group_pool: out = page_rows, pool_pages, free pages, the most pages ever in use; held_or_null[member] = the pages each member holds.  A slab group:
 *   VOX_ERR_UNSUPPORTED.
 * vox_stream_group_pages_for: host arithmetic only, the allocator's own function: a member whose next tick is at `positions` holds the logical pages *first_page ..
 *   *first_page + *n_pages - 1 = max(0, positions - window) / page_rows .. ceil(positions / page_rows) - 1 (window -1: no window).  During a call from position a to b a
 *   member holds pages_for(a).first .. pages_for(b).first + pages_for(b).n - 1: what a pool must have room for.
 * vox_debug_stream_group_pages (tests): the member's physical pages in logical order, *n of them (at most cap are written). */
int32_t vox_stream_group_create_paged(vox_model* m, const float* t_embed, int32_t n_members, const float* gains /* null: 1.0 */, const uint32_t* rates /* null: 16000 each */,
                                      int32_t enc_capacity_rows, int32_t max_positions, int32_t page_rows, int32_t pool_pages, vox_stream_group** out);
int32_t vox_stream_group_pool(const vox_stream_group* g, int64_t out[4], int32_t* held_or_null);
int32_t vox_stream_group_pages_for(int64_t positions, int32_t page_rows, int32_t window, int32_t* first_page, int32_t* n_pages);
int32_t vox_debug_stream_group_pages(const vox_stream_group* g, int32_t member, int32_t* out, int32_t cap, int32_t* n);
/* ENDLESS PAGED GROUPS.  vox_stream_group_create_endless makes a paged group (everything of PAGED DECODER CACHE above holds) whose members are not refused at 16 384
 * positions: every member may go on to 2^24 decoder positions (31 days), the limit of an endless solo session, and still gives back its pages as they leave the
 * decoder window -- so a member's K / V memory stops growing at the window as before.  There is no max_positions.  rates may be null (16 kHz each); page_rows and
 * pool_pages take 0 for the paged group's defaults.  A model without a sliding decoder window is refused (VOX_ERR_INVALID), as by vox_stream_create_endless.
 *   What differs inside: a member's page table is a RING of pool_pages entries (logical page q at entry q % pool_pages; a member never holds more pages than the pool
 *   has, so its pages never collide -- a call that would make it hold more is the pool refusal itself); the RoPE rows of the positions each pass runs are computed on
 *   the host by the function behind the load-time tables and copied into per-member device rings in front of the pass, at EVERY position (one code path: below the
 *   tables' lengths the rows have the tables' bits by construction); the per-member token row and the score / alternatives records start at 2048 positions and
 *   grow by doubling (a doubling synchronises up to four times: once per list and once for the descriptor), are never trimmed, and are counted in vox_stream_group_info[5] as they are.
 *   Contract: up to the bounded limit, the same sequence of calls gives an endless group and a bounded paged group the same ids, logits, records and pool() -- bit for
 *   bit.  Everything else of a group -- advance, its 16-bit form, peek, reset, info, scores, alternatives, taps, capture rates, pool, pages_for -- works unchanged.
 *   Not served: endless slab groups, freeing pages inside a call, more than 16 members. */
int32_t vox_stream_group_create_endless(vox_model* m, const float* t_embed, int32_t n_members, const float* gains /* null: 1.0 */, const uint32_t* rates /* null: 16000 each */,
                                        int32_t enc_capacity_rows, int32_t page_rows /* 0: 256 */, int32_t pool_pages /* 0: the default */, vox_stream_group** out);
/* A BF16 K/V POOL.  vox_stream_group_create_kv makes a paged (endless == 0) or endless paged (endless == 1, max_positions must be 0) group whose decoder K / V pool
 * holds kv_dtype elements.  VOX_KV_F32: exactly vox_stream_group_create_paged / _create_endless -- the same checks, the same refusals, the same object.  VOX_KV_BF16: the
 * K and V pools are [layer][pool_pages][kv_head][page_rows][head_dim] of uint16_t, half the memory per page (vox_stream_group_info [5] follows), half the bytes the decode
 * attention reads at every tick.  Any other kv_dtype is refused (VOX_ERR_INVALID) before anything is allocated.  Everything of PAGED DECODER CACHE and ENDLESS PAGED
 * GROUPS holds: the allocator, the tables, pool_pages' default, every refusal, the peek's borrowed pages -- the same calls give a bf16 group and an f32 paged group the
 * same vox_stream_group_pool and the same pages per member.
 *   The rounding: f32 -> bf16, round to nearest even on the upper 16 bits, (u + 0x7fff + ((u >> 16) & 1)) >> 16; a NaN stays a quiet NaN, a value that rounds past
 *   the largest finite becomes inf, the sign of zero and denormals are kept.  bf16 has f32's range: no finite value of a checkpoint overflows.  Widening is u << 16.
 *   ONE function (csrc/vox_kv_bf16.h) serves the append, the seed, the restore and vox_kv_round_bf16, which is host arithmetic: no context, no device.
 *   Invariants: (1) a group not made with VOX_KV_BF16 runs the launches and allocations it ran before.  (2) The bf16 decode attention is the f32 attention on the
 *   widened values, bit for bit (vox_debug_attn_decode_paged_bf16).  (3) Rows are rounded where they are appended (the q|k|v epilogue, after RoPE in f32; the seed of
 *   the prefix rows) and nowhere else: while the ids agree, a bf16 member's layer-0 rows are the rounded layer-0 rows of the f32 member, exactly.  (4) A session blob
 *   holds f32 rows whatever its container: a bf16 member packs its rows widened (exact); a restore rounds (exact for a blob of a bf16 member) -- bf16 to bf16 of the
 *   same kind continues bit for bit.  (5) A bf16 group's ids and logits are NOT the f32 group's; how far apart they are is measured (profiles/stream_group_kv_bf16.txt),
 *   not promised.  Not served: bf16 for slab groups and solo streams, the encoder ring, the offline caches, f16 / fp8, mixed dtypes in one group. */
#define VOX_KV_F32 0
#define VOX_KV_BF16 1
int32_t vox_stream_group_create_kv(vox_model* m, const float* t_embed, int32_t n_members, const float* gains /* null: 1.0 */, const uint32_t* rates /* null: 16000 each */,
                                   int32_t enc_capacity_rows, int32_t max_positions /* endless: 0 */, int32_t page_rows /* 0: 256 */, int32_t pool_pages /* 0: the default */,
                                   int32_t endless, int32_t kv_dtype, vox_stream_group** out);
int32_t vox_kv_round_bf16(const float* in, int64_t n, uint16_t* out);
/* BURST GROUPS ("Bursts in stream groups").  vox_stream_group_create_burst makes any group kind the creators above make -- paged 0: a slab group
 * (page_rows, pool_pages, endless 0 and kv_dtype VOX_KV_F32 required); paged 1: a paged group with the arguments of vox_stream_group_create_kv -- with burst_ticks B in
 * 1..VOX_STREAM_BURST_MAX fixed for its life.  B = 1 is exactly the group the other creators make.  With B >= 2 a pass no longer runs one round per due tick: round k of
 * a pass runs every due member's next b_z = min(ticks still due to it, B) ticks as ONE encoder pass of 4 sum b_z rows -- every encoder weight matrix read once, the
 * attention in its ragged burst form (vox_debug_stream_attn_group_burst) -- followed by max b_z decode rounds, decode round t serving the members with b_z > t
 * (vox_stream_group_burst_rounds is the schedule).  A round whose b_z are all 1 is a plain group round, launch for launch; the host never acts between the ticks of a
 * pass, so a pass is never cut anywhere else.
 *   enc_capacity_rows: 0 = max(window + 4 B + 4, prefix rows) rounded up to 64; a given value must exceed window + 4 B (VOX_ERR_INVALID before anything is allocated).
 *   Memory: the round buffers hold n_members x B ticks instead of n_members.
 * Contract: fed so that no member ever has two ticks due in a pass, a burst group is bit for bit the plain group of the same ring capacity (ids, logits, records, the
 * pool).  With backlogs a member's ids are the solo plain stream's up to near-ties: the row count of the encoder pass selects the GEMM kernels, so how the samples were
 * cut can decide an id whose two best logits nearly tie (the solo burst stream's caveat).  A paged and a slab burst group given the same calls agree bit for bit, and so
 * do an endless and a bounded paged one up to the bounded limit.  Peek, reset, snapshot and restore, scores, alternatives, taps, capture rates and 16-bit PCM work as in
 * any group.  Not served: burst_ticks above 16; overlapping a round's decode rounds with the next round's encoder pass. */
int32_t vox_stream_group_create_burst(vox_model* m, const float* t_embed, int32_t n_members, const float* gains /* null: 1.0 */, const uint32_t* rates /* null: 16000 each */,
                                      int32_t enc_capacity_rows, int32_t max_positions /* endless: 0 */, int32_t paged, int32_t page_rows /* 0: 256 */,
                                      int32_t pool_pages /* 0: the default */, int32_t endless, int32_t kv_dtype, int32_t burst_ticks, vox_stream_group** out);
/* burst_ticks of the group (1: a plain group), the burst rounds run since create (rounds in which some member ran 2 or more ticks), the member-ticks inside them, the
 * plain rounds run (every group counts those); a peek's rounds are not counted */
int32_t vox_stream_group_burst_info(const vox_stream_group* g, int64_t out[4]);
/* host only, a pure function: the rounds of a burst group's pass.  due[n]: the ticks due to the pass's n members (1..16 of them, each >= 1, sorted descending); burst:
 * burst_ticks (1..16).  Row k of out ([max_rounds][17]: n_r, b_0 .. b_15, zeros behind b_{n_r - 1}) is round k: the first n_r = #{due_z > k burst} members run
 * b_z = min(due_z - k burst, burst) ticks.  *n_rounds = ceil(due[0] / burst); more than max_rounds: VOX_ERR_INVALID, nothing written. */
int32_t vox_stream_group_burst_rounds(const int32_t* due, int32_t n, int32_t burst, int32_t* out, int32_t max_rounds, int32_t* n_rounds);
/* Snapshot and resume of a member (SNAPSHOT AND RESUME above: the format, the refusals, the contracts): vox_stream_snapshot_size / _snapshot / _restore for member
 * `member` of a slab, paged or endless paged group.  Only that member is read or changed. */
int32_t vox_stream_group_snapshot_size(const vox_stream_group* g, int32_t member, size_t* nbytes);
int32_t vox_stream_group_snapshot(vox_stream_group* g, int32_t member, void* blob, size_t cap, size_t* nbytes, int32_t mem_kind);
int32_t vox_stream_group_restore(vox_stream_group* g, int32_t member, const void* blob, size_t nbytes, int32_t mem_kind);
/* A DELAY PER MEMBER ("A delay per member").  The delay enters the computation through t_embed alone: the decoder's Ada scales
 * 1 + w2(gelu(w0 t_embed)), one [dec_dim] vector per decoder layer, and the decoder half of the prefix state a member starts from.  Every other creator gives the group
 * ONE t_embed; vox_stream_group_create_t_embeds takes vox_stream_group_create_burst's argument list with t_embeds [n_members][dec_dim], member i's t_embed in row i, and
 * makes any group kind (slab, paged, endless paged, bf16 pool; burst_ticks 1: a plain group).  The group owns a device block [n_members][dec_layers][dec_dim] of Ada
 * scales (dec_layers x dec_dim x 4 bytes per member, counted in vox_stream_group_info's bytes), filled per member at create and at reset with the bits
 * vox_model_set_t_embed computes for the member's t_embed; the decode round's wo GEMM multiplies row r by the scales of the member in row r (one epilogue instantiation;
 * no launch is added), and a member is seeded from the prefix state of its own t_embed.
 *   Contract: member k's ids, logits and records are bit for bit those of member k of a group made by vox_stream_group_create_burst at member k's t_embed and given the
 *   same calls; with n_members equal t_embeds the group IS that group, bit for bit.  advance and peek never select the model's t_embed: offline calls with their own
 *   t_embed may be interleaved freely, and after create / reset the model's current t_embed and prefix state are those of the member seeded last (the side effect every
 *   stream's create has).  Members with bit-equal t_embeds seeded one after another share one computation of the scales and of the prefix state.
 *   vox_stream_group_reset_t_embed: the member's next utterance at another delay; gain as vox_stream_group_reset, sample_rate 0: the member keeps its rate, else as
 *   vox_stream_group_reset_rate.  A refused call (null t_embed, member out of range, a rate vox_stream_create_rate refuses, a group of one t_embed:
 *   VOX_ERR_UNSUPPORTED) leaves the member, its delay and its state as they were.  vox_stream_group_t_embed: the member's t_embed (any group; cap >= dec_dim floats).
 *   Snapshot / restore: a member's blob carries the hash of the MEMBER's t_embed; a restore into a member at another t_embed is refused (VOX_ERR_INVALID, the message
 *   names the member) before anything changes.  The blob format and VOX_SNAPSHOT_VERSION are unchanged.
 * Not served: solo vox_stream sessions (they select the model's t_embed per call), the offline and batch paths, a change of delay inside an utterance, more than 16
 * members, the batched persistent engine. */
int32_t vox_stream_group_create_t_embeds(vox_model* m, const float* t_embeds /* [n_members][dec_dim] */, int32_t n_members, const float* gains /* null: 1.0 */,
                                         const uint32_t* rates /* null: 16000 each */, int32_t enc_capacity_rows, int32_t max_positions /* endless: 0 */, int32_t paged,
                                         int32_t page_rows /* 0: 256 */, int32_t pool_pages /* 0: the default */, int32_t endless, int32_t kv_dtype, int32_t burst_ticks,
                                         vox_stream_group** out);
int32_t vox_stream_group_reset_t_embed(vox_stream_group* g, int32_t member, float gain, uint32_t sample_rate /* 0: keep */, const float* t_embed);
int32_t vox_stream_group_t_embed(const vox_stream_group* g, int32_t member, float* out, int32_t cap);
/* debug (tests): ONE launch of the decode round's wo operator on caller data -- out [M][N] = x [M][K] W^T + resid [M][N] as f32 rows, xf_out the XF planes
 * (2 (N / 128) 256 8 16-bit values) of out * xf_w [N] * scale, ssq_out [(N / 16)][16] the per-tile sums of squares of out.  scales holds n_sets vectors of N floats.
 * order null: the per-column form, every row multiplied by scale set `set`; order [M] given: the per-row form of a group with a delay per member, row m multiplied by
 * scale set order[m] (0 .. n_sets - 1, checked).  w: a Q4 tensor with K and N multiples of 128; M 1..16; host pointers. */
typedef struct {
    int32_t M, n_sets, set, reserved;
} vox_resid_xf_desc;
int32_t vox_debug_resid_xf(vox_ctx* ctx, const vox_q4* w, const vox_resid_xf_desc* desc, const float* x, const float* resid, const float* xf_w, const float* scales,
                           const int32_t* order_or_null, float* out, uint16_t* xf_out, float* ssq_out);
/* debug (tests): ONE operator of the batched XF decode step on caller data, no model -- the launch the decode chain makes for q|k|v (ROPE_KV), wo / w2 (RESID_XF),
 * w1|w3 (SWIGLU_XF) or the lm_head (STORE), through the chain's own parameter fill.  w: a tile-ordered Q4 tensor [N][K], K % 128 == 0.  Host pointers throughout.
 *   mode VOX_XF_MODE_STEP: groups = 1 runs launch_q4_gemm on one XF group of M rows (1..16); groups = 2..4 runs the wide step (launch_q4_wide), M = 16 * groups.
 *     x [16 * groups][K] f32 rows -> the groups' XF planes (launch_xf_rows; group g's planes xf_in_gs 16-bit elements after group 0's).
 *     n_part > 0: the fused RMSNorm, ssq_part [groups][n_part][16] (on the device ssq_part_gs floats apart); ROPE_KV needs it, RESID_XF takes none, the wide STORE /
 *     SWIGLU_XF need it.  bias: STORE with one group only.
 *     STORE: out [16 * groups][N].  ROPE_KV (N = n_q + 2 n_kv hd): out [16 * groups][N], columns < n_q written; kc / vc [kv_slices][n_kv][kv_rows][hd], f32 or (kv_bf16,
 *       the paged forms) 16-bit; kv_form CONTIG: row r -> slice r at row pos[r]; SLOTS: slice kv_row[r]; PAGED: page kv_row[r], row kv_pos[r] inside it; PAGED_RING:
 *       PAGED with the RoPE row read from a ring rope_cos [rope_rows / (rope_mask + 1)][rope_mask + 1][hd] (cos | sin), member rope_member[r], row pos[r] & rope_mask.
 *       Every other form reads rope_cos / rope_sin [rope_rows][hd / 2] at pos[r].  One group: CONTIG .. PAGED_RING; the wide step: CONTIG and SLOTS.
 *     SWIGLU_XF (N % 256 == 0): xf_out = the XF planes of N / 2 columns.  RESID_XF (N % 128 == 0): out = x W^T + resid [16 * groups][N], xf_out the planes of
 *       out * xf_w * xf_w2 (xf_w2 may be null), ssq_out [groups][N / 16][16].  Group g's planes xf_out_gs 16-bit elements, its sums ssq_out_gs floats after group 0's.
 *     A group stride of 0 means packed.  out, kc, vc, xf_out and ssq_out are uploaded as they come and copied back whole: what the operator does not write keeps
 *     the caller's contents.  Every index (pos, kv_row, kv_pos, rope_member) is checked against the buffers' sizes.
 *     The plan that ran comes back in the descriptor: plan_ntw (n-tiles per wave); one group: plan_ks (split-K waves), plan_steps (K steps per wave),
 *     plan_straight (a straight-line instantiation, else the loop); wide: plan_ks = K slices, plan_steps = K steps per slice.
 *   mode VOX_XF_MODE_WIDE_ROWS: the decoder prefill's 17..48-row form of the same GEMM -- x [M][K] -> ceil(M / 16) XF tiles (launch_xf_rows), launch_q4_skinny_mt2_planes
 *     (q4_wide_kernel storing row-major K-slice planes [slice][M][N]; refused where the wide plan does not take the weight), then the finishing kernel of `epi`:
 *     ROPE_KV launch_splitk_finish_rope_kv -- one sequence, row m at position pos_off + m: out [16 * ceil(M / 16)][N] (rows < M, columns < n_q written), kc / vc
 *       [n_kv][kv_rows][hd] f32 (kv_slices = 1), rope_cos / rope_sin [rope_rows][hd / 2];
 *     SWIGLU_XF launch_splitk_finish_swiglu_xf (optional bias [N]): xf_out = ceil(M / 16) XF tiles of N / 2 columns (rows >= M of the last tile untouched);
 *     RESID_XF launch_splitk_finish_resid: out [16 * ceil(M / 16)][N] holds the residual rows on entry and residual + x W^T on return (rows >= M untouched).
 *     No fused norm (n_part 0), no group strides.  plan_ntw / plan_ks (K slices) / plan_steps come back as for the wide step.
 *   mode VOX_XF_MODE_ROWS: launch_q4_gemm's EPI_ROPE_ROWS (the encoder's q|k|v) on f32 rows x [M][K]: out [M][N], interleaved-pair RoPE on columns < n_q at row m's
 *     position -- pos[m], or m % rope_seq_rows, or m; rope_cos / rope_sin [rope_rows][hd / 2].  fused_rope: the RoPE ran in the GEMM's epilogue. */
#define VOX_XF_EPI_STORE 0
#define VOX_XF_EPI_ROPE_KV 1
#define VOX_XF_EPI_SWIGLU_XF 2
#define VOX_XF_EPI_RESID_XF 3
#define VOX_XF_KV_CONTIG 0
#define VOX_XF_KV_SLOTS 1
#define VOX_XF_KV_PAGED 2
#define VOX_XF_KV_PAGED_RING 3
#define VOX_XF_MODE_STEP 0
#define VOX_XF_MODE_ROWS 1
#define VOX_XF_MODE_WIDE_ROWS 2
typedef struct {
    int32_t mode, groups, M, epi;
    int32_t n_part; float norm_eps; int32_t hd, n_q;
    int32_t n_kv, kv_form, kv_bf16, kv_slices;
    int32_t kv_rows, rope_rows, rope_mask, rope_seq_rows;
    int32_t xf_in_gs, xf_out_gs, ssq_part_gs, ssq_out_gs;
    int32_t plan_ntw, plan_ks, plan_steps, plan_straight;      /* out */
    int32_t fused_rope /* out */, pos_off /* WIDE_ROWS ROPE_KV */, reserved[2] /* 0 */;
} vox_xf_op_desc;
typedef struct {
    const float* x; const float* ssq_part; const float* bias; const float* resid; const float* xf_w; const float* xf_w2; const float* rope_cos; const float* rope_sin;
    const int32_t* pos; const int32_t* kv_row; const int32_t* kv_pos; const int32_t* rope_member;
    float* out; void* kc; void* vc; uint16_t* xf_out; float* ssq_out;
} vox_xf_op_bufs;
int32_t vox_debug_xf_op(vox_ctx* ctx, const vox_q4* w, vox_xf_op_desc* desc, const vox_xf_op_bufs* bufs);
/* The live sessions' feed planner on its own (tests): host arithmetic only -- no context, no device, no model.  A fresh session fed at sample_rate (4 encoder rows per
 * position, the Voxtral left pad, no position limit to speak of) takes the calls (n_samples[c], finish[c] 0 / 1) exactly as vox_stream_push / _finish and a group's advance
 * plan and pass them, every due tick taken as run; finish[c] = 2 is a peek (n_samples[c] must be 0): planned as a finish, its one pass emitted, the session as it was.  One row of five words per pass: call index, input samples appended, 16 kHz samples that entered the 16 kHz ring (a
 * 16 kHz session: the appended ones), right-pad zeros written, ticks that became due.  pass_cap: most input samples per pass (0: no cap; a group's 16-bit staging: 65536).
 * A call after a finish, a bad rate or more than max_rows passes are refused. */
int32_t vox_debug_stream_feed_passes(uint32_t sample_rate, const size_t* n_samples, const int32_t* finish, int32_t n_calls, size_t pass_cap, int64_t* rows, int32_t max_rows,
                                     int32_t* n_rows);

#ifdef __cplusplus
}
#endif
#endif /* VOXTRAL_HIP_H */
