// vox_dev_base.h -- what the device-side host units share: HIPCHK, the context, the model and the cache as the units see them, the decode engines' bindings,
// and the declarations of the functions that another unit calls.  The device-side counterpart of vox_host_base.h: no unit built as plain C++ includes it.
#pragma once
#include "vox_host_base.h"
#include "vox_kernels.h"

#include <hip/hip_runtime_api.h>

#define HIPCHK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail(VOX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); } while (0)
struct vox_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // mel tables (device)
    float *d_window = nullptr, *d_cos = nullptr, *d_sin = nullptr, *d_fb = nullptr;
    int *d_fb_lo = nullptr, *d_fb_hi = nullptr;
    float* d_scale = nullptr;   // peak-normalise scale scratch
    bool mel_ready = false;
    // grow-only pool of per-call device workspaces (batched transcription): hipMalloc/hipFree of a few hundred MB per call cost
    // tens of ms and serialise the device; buffers are handed back after the call's final stream synchronisation
    struct PoolEntry { void* p; size_t cap; bool used; };
    std::vector<PoolEntry> pool;
    hipStream_t occupy_stream = nullptr;      // vox_debug_occupy's busy kernel (a batched decode step runs all its chains on `stream`)
    hipStream_t fe_stream = nullptr; hipEvent_t ev_fe[2] = {nullptr, nullptr}, ev_enc[2] = {nullptr, nullptr};      // continuous batch: the next chunk's upload + log-mel under this chunk's encoder
    // continuous batch, self-calibration of the planner (the step costs were constants measured on one box): milliseconds per step of 1..4 active groups as
    // MEASURED on this context (HIP events around the runs of equal active sets of earlier sessions, exponentially averaged; [0] = engine forms on, [1] = off), 0 = not seen yet
    double step_ms_meas[2][9] = {{0, 0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0, 0}}; hipEvent_t ev_seg[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    uint32_t warm_forms = 0;      // continuous batch: step chains whose kernels have run once on this context's device (bit 0 launch chains, bit 1 one-group engine, bit 2 two-group engine, bits 3..5 wide chains of 2 / 3 / 4 groups)
    // XF tiles of a 17..48-row GEMM input (the 38-token prefill): 3 tiles x K columns x 64 B; sized once for K <= 16384, reused by every such GEMM of the stream
    static constexpr size_t XF_SCRATCH_BYTES = (size_t)3 * 16384 * 64; uint16_t* xf_scratch = nullptr; size_t xf_scratch_bytes = 0;
    bool shared = false;      // vox_ctx_set_shared: other sessions run on this GPU (no batched engines, planner on the scaled table)
    static constexpr size_t KZ_SCRATCH_BYTES = (size_t)8 * 48 * 18432 * 4; float* kz_scratch = nullptr; size_t kz_scratch_bytes = 0;      // K-slice planes of the 17..48-row GEMMs (q4_skinny_mt2_kernel): 8 x 48 x 18432 floats
    // The one owner of the two buffers above: allocates those asked for that are not there yet.  A failed allocation is not an error: the buffer stays null, size 0 (the caller takes a form without it)
    void want_scratch(bool xf, bool kz) {
        auto get = [](void** p, size_t* bytes, size_t want) { if (*p) return; *bytes = want; if (hipMalloc(p, want) != hipSuccess) { (void)hipGetLastError(); *p = nullptr; *bytes = 0; } };
        if (xf) get(reinterpret_cast<void**>(&xf_scratch), &xf_scratch_bytes, XF_SCRATCH_BYTES);
        if (kz) get(reinterpret_cast<void**>(&kz_scratch), &kz_scratch_bytes, KZ_SCRATCH_BYTES);
    }
    float* rs_matrix = nullptr; uint32_t rs_in = 0, rs_out = 0;    // block matrix of the last resampled rate pair (vox_resample)
    struct vox_model* pw_model = nullptr;      // the model with decode-engine steps of the piecewise surface enqueued on `stream` and not yet verified (see pw_after_sync)
};
namespace vox_host {
static int32_t ctx_bind(const vox_ctx* c) { HIPCHK(hipSetDevice(c->device)); return VOX_OK; }
// small RAII device buffer for host-pointer entry points
struct DevBuf {
    void* p = nullptr; vox_ctx* pool_ctx = nullptr;
    ~DevBuf() {
        if (!p) return;
        if (pool_ctx) { for (auto& e : pool_ctx->pool) if (e.p == p) { e.used = false; return; } }
        (void)hipFree(p);
    }
    hipError_t alloc(size_t n) { return hipMalloc(&p, n ? n : 1); }
    // from the context's workspace pool (best fit, at most 2x oversize); the caller must have synchronised the stream before the
    // buffer goes out of scope
    hipError_t alloc_pooled(vox_ctx* c, size_t n) {
        n = n ? n : 1;
        int best = -1;
        for (size_t i = 0; i < c->pool.size(); i++) {
            const auto& e = c->pool[i];
            if (!e.used && e.cap >= n && e.cap <= 2 * n + (1u << 20) && (best < 0 || e.cap < c->pool[best].cap)) best = (int)i;
        }
        if (best >= 0) { c->pool[best].used = true; p = c->pool[best].p; pool_ctx = c; return hipSuccess; }
        if (c->pool.size() >= 96) {          // bound the pool: drop idle entries
            for (size_t i = 0; i < c->pool.size();) { if (!c->pool[i].used) { (void)hipFree(c->pool[i].p); c->pool.erase(c->pool.begin() + i); } else i++; }
        }
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) { c->pool.push_back({p, n, true}); pool_ctx = c; }
        return e;
    }
    template <class T> T* as() { return reinterpret_cast<T*>(p); }
};
struct Lin { vox::Q4W w{}; const float* bias = nullptr; };
struct EncLayer { const float *attn_norm = nullptr, *ffn_norm = nullptr; Lin wqkv, wo, w13, w2; };
struct DecLayer { const float *attn_norm = nullptr, *ffn_norm = nullptr; Lin wqkv, wo, w13, w2, ada0, ada2; float* ada_mul = nullptr; };
}  // namespace vox_host
struct vox_cache { vox_model* m; vox_ctx* ctx = nullptr; float *k = nullptr, *v = nullptr; int max_seq = 0, len = 0; size_t layer_stride = 0;
                   int kind = 0, abs_pos = 0; uint64_t gen = 0; };   // kind 0: decoder cache, 1: encoder (streaming) cache; abs_pos: positions seen so far (RoPE offset of the next chunk)   // layer_stride in floats   // per layer: [n_kv][max_seq][hd]
namespace vox_host {
// What one client of the single-stream decode engine (the offline path, the piecewise decoder surface, a live stream) holds of it: the device layer table for ITS cache,
// where the launch leaves its 256 argmax partials, and the pinned host word the engine's error word is copied to.  `host` is what `tab` holds, valid for exactly
// (cache, gen): engine_bind rebuilds it for another cache or generation and leaves it alone otherwise, so clients that alternate on one model never disturb each other.
struct EngBinding {
    vox::EngLayerTab* tab = nullptr; float* part_val = nullptr; int* part_idx = nullptr; unsigned* err_word = nullptr; const vox_cache* cache = nullptr; uint64_t gen = 0; std::vector<vox::EngLayerTab> host;
};
struct TensorMeta { std::vector<uint64_t> shape; int dtype = 0; uint64_t nbytes = 0; };
// What vox_transcribe_audio computes identically for EVERY utterance, held once per model.  The library itself pads every utterance on the left
// with silence (vox_pad_cfg_voxtral), the log-mel of silence is the constant floor, the conv stem is local, the encoder attention causal, and the decoder's prefix tokens
// are fixed: encoder rows [0, RC) and decoder positions [0, PC) are functions of the weights (and of t_embed) alone.  Built from a silent mel, never from a caller's clip.
struct PrefixState {
    bool on = true;                        // vox_model_set_prefix_cache
    int RC = 0, PC = 0;                    // encoder rows / decoder positions held; 0: this geometry has no prefix (prefix_bounds)
    float* enc_kv = nullptr;               // [enc_layers][RC][k row | v row]: the RoPE'd keys and the values of rows 0 .. RC-1 of every encoder layer
    float* audio = nullptr;                // [PC][dec_dim]: adapter rows 0 .. PC-1
    float *dec_k = nullptr, *dec_v = nullptr;      // [dec_layers * dec_kv_heads][PC][head_dim]: decoder cache rows 0 .. PC-1 for the t_embed below
    bool enc_built = false, dec_built = false;
    std::vector<float> t_embed;            // the t_embed the decoder part was built with
    float* capture = nullptr; int capture_rows = 0;      // while the encoder part is being built: encode_batch_dev stores every layer's k | v rows here
    uint64_t enc_bytes = 0, dec_bytes = 0;
};
// What decode_step_enqueue launches.  StepAndArgmax: the step and the launch that turns its argmax partials into the next token + input (every path).  Engine only --
// EngineAlone: the engine launch, its partials left for whoever comes next; EngineArgmaxFirst: an engine launch that BEGINS with the argmax of the previous launch's partials
// (flags 65536): [EngineAlone] [EngineArgmaxFirst] ... [EngineArgmaxFirst] [argmax_final] is the token sequence of StepAndArgmax steps with one launch per token, not two.
enum class StepLaunch { StepAndArgmax, EngineAlone, EngineArgmaxFirst };
// the single-clip decode graphs: [0] = one step, [1] = key.unroll steps (fewer graph boundaries).  Both bake the key's cache / audio (and the model's token) pointers
// and its launch form in: graphs_for re-keys them, graphs_destroy drops them (the key stays: the next graphs_for with it captures afresh)
struct DecodeGraphs {
    struct Key { const vox_cache* cache; const float* audio; int unroll; StepLaunch launch; } key{nullptr, nullptr, 0, StepLaunch::StepAndArgmax};
    hipGraph_t graph[2] = {nullptr, nullptr}; hipGraphExec_t exec[2] = {nullptr, nullptr};
};
}  // namespace vox_host
struct vox_model {
    vox_host::PrefixState pfx;
    vox_ctx* ctx = nullptr; vox_model_cfg cfg{};
    std::vector<vox_model*> twins;      // vox_model_set_sessions: replicas on hidden contexts of the same device (owned: freed with the model)
    std::map<std::string, vox_host::TensorMeta> manifest; bool is_q4 = false;      // name -> shape / dtype of every tensor the loader looked up (vox_model_replicate lays a second arena out from it, without the file)
    uint8_t* arena = nullptr; uint64_t arena_bytes = 0, arena_primary_bytes = 0;      // [0, primary): everything parsed from the file; [primary, bytes): copies derived from it on the GPU
    std::vector<vox::Q4W*> tiled;                                 // Q4 linears that own a tile-ordered copy in the derived part
    const float *conv1_w = nullptr, *conv1_b = nullptr, *conv2_w = nullptr, *conv2_b = nullptr, *enc_norm = nullptr, *dec_norm = nullptr;
    vox::Q4W conv1_g{}, conv2_g{};                               // conv weights as im2col GEMM operands (two bf16 planes), optional
    const float *enc_cos = nullptr, *enc_sin = nullptr, *dec_cos = nullptr, *dec_sin = nullptr;
    int enc_rope_len = 4096, dec_rope_len = 16384;                         // gguf/loader.rs:196-198,284-286
    std::vector<vox_host::EncLayer> enc; std::vector<vox_host::DecLayer> dec; vox_host::Lin ad0, ad2, tok;
    // derived (not in the arena)
    float* ada_mul = nullptr; bool t_embed_set = false; std::vector<float> t_embed_host;
    // workspaces
    float* ws = nullptr; size_t ws_floats = 0;            // encoder / prefill workspace
    float *d_audio = nullptr; int audio_cap = 0;          // [S][dec_dim]
    float *d_mel = nullptr; size_t mel_cap = 0;           // [128][T]
    float *d_samples = nullptr; size_t samples_cap = 0;
    // decode state
    vox_cache* cache = nullptr;                           // internal cache for transcribe_streaming
    int *d_tokens = nullptr, *d_pos = nullptr; int tokens_cap = 0;
    float* d_prefix = nullptr;                            // [38][dec_dim] prefill inputs (prefill_prefix_rows)
    float *enc_cos_s = nullptr, *enc_sin_s = nullptr; int enc_rope_s_len = 0;   // RoPE tables for the streaming encoder (positions beyond the 4096-row load-time table)
    int* d_seq_len = nullptr; std::vector<int> h_seq_len;  // per-utterance encoder rows of a stacked batch
    int *d_seq_off = nullptr, *d_row_pos = nullptr; size_t row_pos_cap = 0; std::vector<int> h_seq_off, h_row_pos;      // packed stack: start row per utterance, position per row
    float *d_h = nullptr, *d_q = nullptr, *d_att = nullptr, *d_act = nullptr, *d_logits = nullptr, *d_part_val = nullptr; int* d_part_idx = nullptr;
    float* d_h2 = nullptr; long long* d_wo_acc = nullptr;      // fused attention + wo decode launch: residual stream after wo; per-layer fixed-point accumulators [dec_layers][dec_dim]
    int n_parts = 0, argmax_R = 8;
    // persistent decode-step engine (vox_engine.hip): one launch per token for the real decoder geometry; eng_ok = eligible, eng_ready = stream packed + state allocated
    bool eng_ok = false, eng_on = true, eng_ready = false; unsigned char* eng_stream = nullptr; unsigned char* eng_state = nullptr; unsigned long long eng_launches = 0;
    vox_host::EngBinding eng_offline, eng_pw;      // the engine against the model's own cache (partials: d_part_val / d_part_idx, not owned) and against a piecewise caller's cache
    int eng_flags = 128 | 512 | 1, eng_pace = 50;      // XCD-local edges; probe-less all-gather, swept 0.5 us after the CU's own rows went out; one LDS-DMA packet in flight while the CU polls memory
    int eng_strikes = 0; bool eng_suspended = false;      // hand-off timeouts so far (3: the engine is switched off for good); suspended: the current utterance is being re-run on the per-operator path
    // batched decode-layer engine (vox_engine_b16.hip): one launch per 16-row group and step on the same packet stream; per-group edge buffers + layer tables
    unsigned char* eng_wob = nullptr;      // the batched engine's wo stream (XCD-group K split, launch_eng_pack op 5): 7 MB per layer
    bool engb_ok = false; unsigned char* engb_state[4] = {nullptr, nullptr, nullptr, nullptr}; vox::EngLayerTab* engb_tab[4] = {nullptr, nullptr, nullptr, nullptr};
    bool engb_on = true; unsigned long long engb_launches = 0; int engb_strikes = 0;
    int batch_sessions = 0;      // parts the last vox_transcribe_batch call ran in
    int engb_flags = 128 | 1 | 64 | 2048;
    int engb_flags2 = 128 | 1024;      // two-group launch: loader depth 2, never paused or thinned -- with two chains interleaved the stream is what a phase waits for (profiles/r05_b32_engine.txt: 61.4 us per layer against 65.4 with the one-group flags)
    unsigned engb_err_host[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};
    vox_host::DecodeGraphs graphs;
    // piecewise decoder surface (embed_tokens_from_ids / forward_hidden_with_cache / lm_head on caller-owned caches): model-owned workspaces, and the decode engine's
    // layer table for the caller's cache (eng_pw).  pw_memo: row 0 of pw_hidden is the final norm's output of an engine launch that ALSO produced that row's logits (pw_logits)
    // and argmax partials (eng_pw.part_*): lm_head on that very buffer has nothing left to compute.  eng_pw.err_word is refreshed (async) behind every engine launch: no round trip.
    float *pw_x = nullptr, *pw_hidden = nullptr, *pw_logits = nullptr; size_t pw_x_cap = 0, pw_hidden_cap = 0, pw_logits_cap = 0;
    int* pw_ids = nullptr; int pw_ids_cap = 0; int* pw_zero = nullptr;
    bool pw_memo = false, pw_eng_used = false;
    // rows appended to a caller's cache by engine steps (and by anything run behind them) whose error word has not been read behind a stream synchronisation yet: a
    // hand-off timeout found later takes exactly these rows back (cache length -= pw_pend_rows), so "repeat the step" appends at the failed position again
    vox_cache* pw_pend_cache = nullptr; uint64_t pw_pend_gen = 0; int pw_pend_rows = 0; bool pw_verdict_failed = false;
    vox_timings timings{};
    uint64_t snap_fingerprint = 0; bool snap_fingerprint_set = false;      // the session blobs' model fingerprint (vox_snapshot.h), computed at the first snapshot or restore
    // vox_debug_batch_tap_*: units (caller indices) armed for the next batch call; `on` during that call; out / rows hold the call's rows until fetched
    struct { std::vector<int> units; int max_rows = 0; bool armed = false, on = false, ready = false; float* out = nullptr; int* rows = nullptr; } tap;
};
namespace vox_host {
// ---- vox_ctx.cpp
void roctx_push(const char* name);
void roctx_pop();
double now_ms();
int32_t ctx_mel_tables(vox_ctx* c, vox::MelTables* t);
int32_t resample_matrix_build(vox_ctx* c, const ResamplePlan& p, size_t bytes, float** out);
// ---- vox_tensor.cpp
int32_t upload_repack(vox_ctx* c, const uint8_t* raw, int64_t n_blocks, int nb, uint4* qs, uint16_t* sc, int row_mul, int row_add,
                             void* staging, size_t staging_cap);
int32_t q4_linear_dev(vox_ctx* c, const vox::Q4W& w, const float* bias, const float* x, int x_stride, int rows, float* out, int out_stride,
                             int epi = vox::EPI_STORE, const float* resid = nullptr, int resid_stride = 0, int ksplit = 0);
// ---- vox_api.cpp
void binding_release(EngBinding& b);
void prefix_release(vox_model* m);
void graphs_destroy(vox_model* m);
int32_t pw_after_sync(vox_model* m);
int32_t pw_sync(vox_model* m);
// ---- vox_model.cpp (the loader; of vox_api.cpp it calls only the three release functions above)
void model_release(vox_model* m);
// ---- vox_cache.cpp
void cache_register(vox_cache* k);
void cache_unregister(const vox_cache* k);
bool cache_alive(const vox_cache* k, uint64_t gen);
void cache_release(vox_cache*& k);
int32_t cache_alloc(vox_model* m, int max_seq, vox_cache** out);
struct RoctxScope { explicit RoctxScope(const char* n) { roctx_push(n); } ~RoctxScope() { roctx_pop(); } };
// consecutive stages of one function: begin() closes the previous stage; every exit path (error returns included) closes the open one
struct RoctxStage { bool open = false; void begin(const char* n) { end(); roctx_push(n); open = true; } void end() { if (open) { roctx_pop(); open = false; } } ~RoctxStage() { end(); } };
}  // namespace vox_host
