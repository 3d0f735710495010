// vox_cache.cpp -- the decoder KV cache and the vox_cache_* entries
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the host units: DESIGN.md, "Host units")
#include "vox_dev_base.h"

#include <mutex>
#include <unordered_map>

using namespace vox;
using namespace vox_host;

// Every caller-visible cache carries a generation number from one process-wide counter and is listed while it lives: code that remembers a cache across calls (the
// piecewise engine's layer table, the record of unverified engine steps) keys on (address, generation) -- a freed cache's address may be handed out again by the
// allocator, with another max_seq behind the same K base -- and asks cache_alive() before it dereferences one it did not receive in the current call.
static std::mutex g_cache_mu; static std::unordered_map<const vox_cache*, uint64_t> g_cache_live; static uint64_t g_cache_gen = 0;
namespace vox_host {
void cache_register(vox_cache* k) { std::lock_guard<std::mutex> l(g_cache_mu); k->gen = ++g_cache_gen; g_cache_live[k] = k->gen; }
void cache_unregister(const vox_cache* k) { std::lock_guard<std::mutex> l(g_cache_mu); g_cache_live.erase(k); }
bool cache_alive(const vox_cache* k, uint64_t gen) { std::lock_guard<std::mutex> l(g_cache_mu); auto it = g_cache_live.find(k); return it != g_cache_live.end() && it->second == gen; }
// frees a cache nothing on the GPU reads any more: synchronising first, and dropping whatever remembers it, is the caller's
void cache_release(vox_cache*& k) { if (!k) return; cache_unregister(k); (void)hipFree(k->k); (void)hipFree(k->v); delete k; k = nullptr; }
}  // namespace vox_host

// ---- KV cache (models/layers/kv_cache.rs:52-65,221-234)
namespace vox_host {
int32_t cache_alloc(vox_model* m, int max_seq, vox_cache** out) {
    const vox_model_cfg& c = m->cfg;
    ARGCHK(max_seq > 0 && max_seq <= m->dec_rope_len, "max_seq %d out of range (1..%d)", max_seq, m->dec_rope_len);
    vox_cache* k = new vox_cache(); k->m = m; k->ctx = m->ctx; k->max_seq = max_seq;
    const size_t n = (size_t)c.dec_layers * c.dec_kv_heads * max_seq * c.dec_head_dim * 4;
    if (hipMalloc((void**)&k->k, n) != hipSuccess || hipMalloc((void**)&k->v, n) != hipSuccess) { if (k->k) (void)hipFree(k->k); delete k; return fail(VOX_ERR_HIP, "hipMalloc of KV cache failed"); }
    HIPCHK(hipMemsetAsync(k->k, 0, n, m->ctx->stream)); HIPCHK(hipMemsetAsync(k->v, 0, n, m->ctx->stream));
    k->layer_stride = (size_t)c.dec_kv_heads * max_seq * c.dec_head_dim;
    cache_register(k);
    *out = k; return VOX_OK;
}
}  // namespace vox_host
extern "C" int32_t vox_decoder_cache_create(vox_model* m, int32_t max_seq, vox_cache** out) { ARGCHK(m && out, "null argument"); VOXCHK(ctx_bind(m->ctx)); return cache_alloc(m, max_seq, out); }
extern "C" int32_t vox_cache_free(vox_cache* k) {
    if (!k) return VOX_OK;
    (void)hipSetDevice(k->ctx->device); (void)hipStreamSynchronize(k->ctx->stream);   // never dereferences k->m: the model may be gone
    cache_release(k); return VOX_OK;
}
// KVCache::update on one layer of a pre-allocated cache (kv_cache.rs:116-136: slice_assign of k / v [1][heads][new_seq][hd] at rows pos .. pos + new_seq) -- for callers
// that own their K / V (and for tests that need a cache at a position no prefill has reached).  The length shared by all layers (LayerCaches::seq_len,
// kv_cache.rs:242-244) becomes max(len, pos + n_rows).
// The piecewise decoder surface remembers the rows of a cache it has not verified yet (engine steps since the last synchronisation; see pw_note_pending, vox_api.cpp).  An entry
// point that moves the cache's length by hand settles them first: a hand-off timeout found LATER would otherwise subtract a stale row count from the new length.
// A failure found here is reported by this call (VOX_ERR_HIP; the cache is back at the length before the failed step, nothing else was changed).
static int32_t cache_settle_pending(vox_cache* kc) {
    vox_model* m = kc->m;
    if (m && m->pw_pend_rows > 0 && m->pw_pend_cache == kc) { VOXCHK(ctx_bind(kc->ctx)); VOXCHK(pw_sync(m)); }
    return VOX_OK;
}
extern "C" int32_t vox_cache_update(vox_cache* kc, int32_t layer, int32_t pos, const float* k, const float* v, int32_t n_rows, int32_t mem_kind) {
    ARGCHK(kc && k && v && n_rows > 0 && pos >= 0, "bad argument"); VOXCHK(ctx_bind(kc->ctx)); VOXCHK(cache_settle_pending(kc));
    const vox_model_cfg& c = kc->m->cfg;
    const int L = kc->kind == 1 ? c.enc_layers : c.dec_layers, H = kc->kind == 1 ? c.enc_heads : c.dec_kv_heads, hd = kc->kind == 1 ? c.enc_head_dim : c.dec_head_dim;
    ARGCHK(layer >= 0 && layer < L, "layer %d out of range (0..%d)", layer, L - 1);
    ARGCHK(pos + n_rows <= kc->max_seq, "KV cache overflow: %d + %d > %d", pos, n_rows, kc->max_seq);
    hipStream_t s = kc->ctx->stream; const hipMemcpyKind kind = mem_kind == VOX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    for (int h = 0; h < H; h++) {
        const size_t dst = (size_t)layer * kc->layer_stride + ((size_t)h * kc->max_seq + pos) * hd, src = (size_t)h * n_rows * hd, nb = (size_t)n_rows * hd * 4;
        HIPCHK(hipMemcpyAsync(kc->k + dst, k + src, nb, kind, s)); HIPCHK(hipMemcpyAsync(kc->v + dst, v + src, nb, kind, s));
    }
    if (mem_kind != VOX_MEM_DEVICE) HIPCHK(hipStreamSynchronize(s));      // the host buffers may be reused when the call returns
    kc->len = std::max(kc->len, pos + n_rows);
    return VOX_OK;
}
// forget every row from `len` on (0 <= len <= seq_len): the next forward appends at `len` again.  What a caller of the device-resident entries does after ITS OWN failed step;
// the library's own engine timeouts roll the length back themselves (see vox_forward_hidden_with_cache_ex).
extern "C" int32_t vox_cache_truncate(vox_cache* kc, int32_t len) {
    ARGCHK(kc, "null cache"); VOXCHK(cache_settle_pending(kc)); ARGCHK(len >= 0 && len <= kc->len, "truncate to %d: the cache holds %d rows", len, kc->len);
    if (kc->kind == 1) kc->abs_pos -= kc->len - len;
    kc->len = len; return VOX_OK;
}
extern "C" int32_t vox_cache_seq_len(const vox_cache* k, int32_t* out) { ARGCHK(k && out, "null argument"); *out = k->len; return VOX_OK; }
extern "C" int32_t vox_cache_reset(vox_cache* k) {
    ARGCHK(k, "null cache");
    (void)cache_settle_pending(k);      // (a failed verdict only shortens a cache that is being emptied anyway: the strike is counted, the reset goes through)
    k->len = 0; k->abs_pos = 0; return VOX_OK;
}
