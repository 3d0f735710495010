// vox_snapshot.h -- the session blob's header and section plan (vox_stream_snapshot / vox_stream_restore; DESIGN.md section 8, "Snapshot and resume"): pure host
// arithmetic on bytes, no device, no allocation, no other unit -- vox_snapshot_plan.cpp wraps it into the C ABI, vox_api.cpp fills and reads headers through it, and
// tools/snapshot_check.cpp includes it alone under the host sanitizers.
//   The blob: [header, VOX_SNAPSHOT_HEADER_BYTES][sections, each at a 16-byte boundary, in the order of SnapSection, the padding between them zero].  Everything is
//   in the byte order and float format of the machine that wrote it.  The header says what every section holds and where, so a blob does not know which container
//   (solo stream, slab / paged / endless member) it came from.
//   The model fingerprint (and the t_embed hash) stop a blob from going into the WRONG MODEL BY MISTAKE.  They are FNV-1a sums, prove nothing about integrity, and
//   are no defence against a blob made up on purpose: a blob is trusted as far as its arithmetic goes (snap_parse), its payload is not inspected.
#pragma once
#include "../../include/voxtral_hip.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

namespace vox_snap {
enum SnapSection { SEC_ENC_K = 0, SEC_ENC_V, SEC_DEC_K, SEC_DEC_V, SEC_SAMPLES, SEC_IN_SAMPLES, SEC_TOKENS, SEC_SCORES, SEC_ALTS, SEC_COUNT };
static_assert(SEC_COUNT == VOX_SNAPSHOT_SECTIONS, "the section count of the header");
static const uint32_t SNAP_MAGIC = 0x50534f56u;      // "VOSP"
static const int SNAP_SAMPLE_RING = 1 << 16, SNAP_IN_RING_MAX = 1 << 20, SNAP_POS_LIMIT = 1 << 24, SNAP_PREFIX_POS = 37;
static const size_t SNAP_SCORE_BYTES = 16, SNAP_ALTS_BYTES = 8 + 8 * VOX_MAX_ALTERNATIVES;      // sizeof(vox_token_score), sizeof(vox_token_alts)
// the header as it lies in the blob
struct SnapHeader {
    uint32_t magic, version; uint64_t total_bytes;
    uint64_t fingerprint, t_embed_hash;                   // of the model (snap_fingerprint) and of the bits of the session's t_embed
    float gain; uint32_t sample_rate; int64_t n_pushed;   // FeedState: what a later call depends on
    int64_t n_written, in_written;
    int32_t D, E, ids_out, token;                         // decoder position, encoder stream position, ids handed out, tokens[D]
    int32_t scores_on, alts_k, n_scores, n_alts;          // the flags; the records the two record sections hold
    int32_t enc_layers, enc_heads, enc_head_dim, enc_window, dec_layers, dec_kv_heads, dec_head_dim, dec_window;      // the geometry the K / V sections are laid out by
    int32_t vocab, reshape_factor, We, Wd;                // We / Wd: the rows per (layer, head) of the encoder / decoder sections
    uint64_t sec_off[SEC_COUNT], sec_len[SEC_COUNT];
};
static_assert(sizeof(SnapHeader) == VOX_SNAPSHOT_HEADER_BYTES && VOX_SNAPSHOT_HEADER_BYTES % 16 == 0, "the header's size is part of the format");

inline uint64_t fnv1a(const void* p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; i++) { h ^= b[i]; h *= 0x100000001b3ull; }
    return h;
}
// the model fingerprint: the configuration words, the primary arena's byte count and a hash of a few KB of weights (read back once per model by the caller)
inline uint64_t snap_fingerprint(const vox_model_cfg& c, uint64_t arena_primary_bytes, uint64_t weights_hash) {
    uint64_t h = fnv1a(&c, sizeof c);
    h = fnv1a(&arena_primary_bytes, sizeof arena_primary_bytes, h);
    return fnv1a(&weights_hash, sizeof weights_hash, h);
}
inline int64_t snap_enc_rows(int64_t E, int enc_window) { return E < enc_window ? E : enc_window; }      // We: the keys E - We .. E - 1 the next query row attends
inline int64_t snap_dec_rows(int64_t D, int dec_window) { return dec_window < 0 || D < dec_window ? D : dec_window; }
inline uint64_t snap_align(uint64_t x) { return (x + 15) & ~(uint64_t)15; }

// what a session in this state puts into its sections; `in_samples`: the samples of a rate session's input ring (0 at 16 kHz)
struct SnapShape { int64_t D = 0, E = 0, n_written = 0, in_samples = 0; int32_t n_scores = 0, n_alts = 0; };
// fills the geometry words, We / Wd and the section table of h from the configuration and the shape; returns the blob's total bytes
inline uint64_t snap_layout(const vox_model_cfg& c, const SnapShape& s, SnapHeader* h) {
    h->enc_layers = c.enc_layers; h->enc_heads = c.enc_heads; h->enc_head_dim = c.enc_head_dim; h->enc_window = c.enc_window;
    h->dec_layers = c.dec_layers; h->dec_kv_heads = c.dec_kv_heads; h->dec_head_dim = c.dec_head_dim; h->dec_window = c.dec_window;
    h->vocab = c.vocab; h->reshape_factor = c.reshape_factor;
    h->We = (int32_t)snap_enc_rows(s.E, c.enc_window); h->Wd = (int32_t)snap_dec_rows(s.D, c.dec_window);
    h->n_scores = s.n_scores; h->n_alts = s.n_alts;
    const uint64_t enc = (uint64_t)c.enc_layers * c.enc_heads * (uint64_t)h->We * c.enc_head_dim * 4, dec = (uint64_t)c.dec_layers * c.dec_kv_heads * (uint64_t)h->Wd * c.dec_head_dim * 4;
    const uint64_t len[SEC_COUNT] = {enc, enc, dec, dec, (uint64_t)(s.n_written < SNAP_SAMPLE_RING ? s.n_written : SNAP_SAMPLE_RING) * 4, (uint64_t)s.in_samples * 4,
                                     (uint64_t)(s.D + 1) * 4, (uint64_t)s.n_scores * SNAP_SCORE_BYTES, (uint64_t)s.n_alts * SNAP_ALTS_BYTES};
    uint64_t o = sizeof(SnapHeader);
    for (int i = 0; i < SEC_COUNT; i++) { h->sec_off[i] = o; h->sec_len[i] = len[i]; o = snap_align(o + len[i]); }
    return o;
}

// Validates the first bytes of a blob of `nbytes` bytes and copies its header out.  Reads min(nbytes, sizeof(SnapHeader)) bytes of p and nothing else.  On refusal
// writes the reason to msg and returns false.  An accepted header satisfies everything a restore relies on:
//   the geometry is within the kernels' bounds (head dims 64 | 128, counts positive and small enough that no product below overflows 64 bits);
//   0 <= ids_out <= D < 2^24, E = reshape_factor * D, We = min(E, enc_window), Wd = min(D, dec_window), 0 <= token < vocab;
//   every section starts at a 16-byte boundary at or behind the end of the one before, has exactly the length its contents need, and ends inside nbytes = total_bytes.
inline bool snap_parse(const void* p, size_t nbytes, SnapHeader* out, char* msg, size_t msg_n) {
#define SNAP_REFUSE(...) do { std::snprintf(msg, msg_n, __VA_ARGS__); return false; } while (0)
    if (!p || nbytes < sizeof(SnapHeader)) SNAP_REFUSE("snapshot: %zu bytes are shorter than the %zu-byte header", nbytes, sizeof(SnapHeader));
    SnapHeader h; std::memcpy(&h, p, sizeof h);
    if (h.magic != SNAP_MAGIC) SNAP_REFUSE("snapshot: bad magic 0x%08x", h.magic);
    if (h.version != VOX_SNAPSHOT_VERSION) SNAP_REFUSE("snapshot: format version %u, this library reads version %d", h.version, VOX_SNAPSHOT_VERSION);
    if (h.total_bytes != (uint64_t)nbytes) SNAP_REFUSE("snapshot: the blob says %llu bytes, %zu were given", (unsigned long long)h.total_bytes, nbytes);
    auto in = [](int64_t v, int64_t lo, int64_t hi) { return v >= lo && v <= hi; };
    if (!in(h.enc_layers, 1, 1024) || !in(h.enc_heads, 1, 1024) || !in(h.dec_layers, 1, 1024) || !in(h.dec_kv_heads, 1, 1024) || (h.enc_head_dim != 64 && h.enc_head_dim != 128) ||
        (h.dec_head_dim != 64 && h.dec_head_dim != 128) || !in(h.enc_window, 0, 1 << 20) || !in(h.dec_window, -1, 1 << 24) || !in(h.vocab, 1, 1 << 24) || !in(h.reshape_factor, 1, 16))
        SNAP_REFUSE("snapshot: the header's model geometry is out of range");
    if (!in(h.D, 0, SNAP_POS_LIMIT - 1) || (int64_t)h.E != (int64_t)h.reshape_factor * h.D) SNAP_REFUSE("snapshot: decoder position %d, encoder position %d (reshape factor %d)", h.D, h.E, h.reshape_factor);
    if (!in(h.ids_out, 0, h.D)) SNAP_REFUSE("snapshot: %d ids handed out at position %d", h.ids_out, h.D);
    if (h.token < 0 || h.token >= h.vocab) SNAP_REFUSE("snapshot: token %d at position %d is outside the vocabulary of %d", h.token, h.D, h.vocab);
    if (h.We != snap_enc_rows(h.E, h.enc_window) || h.Wd != snap_dec_rows(h.D, h.dec_window)) SNAP_REFUSE("snapshot: %d encoder rows and %d decoder rows do not follow from the positions", h.We, h.Wd);
    if (!std::isfinite(h.gain) || h.sample_rate == 0) SNAP_REFUSE("snapshot: gain or sample rate out of range");
    if (h.n_pushed < 0 || h.n_written < 0 || h.in_written < 0 || h.n_pushed > ((int64_t)1 << 50) || h.n_written > ((int64_t)1 << 50) || h.in_written > h.n_pushed) SNAP_REFUSE("snapshot: sample counts out of range");
    if (!in(h.scores_on, 0, 1) || !in(h.alts_k, 0, VOX_MAX_ALTERNATIVES) || (h.n_scores != 0 && h.n_scores != h.ids_out) || (h.n_alts != 0 && h.n_alts != h.ids_out))
        SNAP_REFUSE("snapshot: record flags or counts out of range (%d score records, %d alternatives records, %d ids)", h.n_scores, h.n_alts, h.ids_out);
    const uint64_t in_len = h.sec_len[SEC_IN_SAMPLES];
    if (in_len % 4 || in_len > (uint64_t)SNAP_IN_RING_MAX * 4 || in_len > (uint64_t)h.in_written * 4 || (h.sample_rate == 16000 && in_len)) SNAP_REFUSE("snapshot: an input ring section of %llu bytes", (unsigned long long)in_len);
    SnapHeader want = h; vox_model_cfg c{};
    c.enc_layers = h.enc_layers; c.enc_heads = h.enc_heads; c.enc_head_dim = h.enc_head_dim; c.enc_window = h.enc_window; c.dec_layers = h.dec_layers; c.dec_kv_heads = h.dec_kv_heads;
    c.dec_head_dim = h.dec_head_dim; c.dec_window = h.dec_window; c.vocab = h.vocab; c.reshape_factor = h.reshape_factor;
    SnapShape s; s.D = h.D; s.E = h.E; s.n_written = h.n_written; s.in_samples = (int64_t)(in_len / 4); s.n_scores = h.n_scores; s.n_alts = h.n_alts;
    (void)snap_layout(c, s, &want);
    uint64_t end = sizeof(SnapHeader);
    for (int i = 0; i < SEC_COUNT; i++) {
        const uint64_t o = h.sec_off[i], n = h.sec_len[i];
        if (n != want.sec_len[i]) SNAP_REFUSE("snapshot: section %d holds %llu bytes, its contents need %llu", i, (unsigned long long)n, (unsigned long long)want.sec_len[i]);
        if (o % 16) SNAP_REFUSE("snapshot: section %d starts at %llu, not a 16-byte boundary", i, (unsigned long long)o);
        if (o < end) SNAP_REFUSE("snapshot: section %d at %llu overlaps what lies before it (up to %llu)", i, (unsigned long long)o, (unsigned long long)end);
        if (o > (uint64_t)nbytes || n > (uint64_t)nbytes - o) SNAP_REFUSE("snapshot: section %d (%llu bytes at %llu) runs past the blob's %zu bytes", i, (unsigned long long)n, (unsigned long long)o, nbytes);
        end = o + n;
    }
#undef SNAP_REFUSE
    *out = h; return true;
}
inline void snap_info(const SnapHeader& h, vox_snapshot_info* o) {
    std::memset(o, 0, sizeof *o);
    o->version = (int32_t)h.version; o->sample_rate = h.sample_rate; o->gain = h.gain; o->token = h.token; o->total_bytes = h.total_bytes; o->fingerprint = h.fingerprint; o->t_embed_hash = h.t_embed_hash;
    o->samples_pushed = h.n_pushed; o->samples_16k = h.n_written; o->samples_in = h.in_written; o->positions = h.D; o->enc_position = h.E; o->ids = h.ids_out;
    o->scores = h.scores_on; o->alternatives = h.alts_k; o->n_scores = h.n_scores; o->n_alts = h.n_alts; o->enc_rows = h.We; o->dec_rows = h.Wd;
    for (int i = 0; i < SEC_COUNT; i++) { o->section_offset[i] = h.sec_off[i]; o->section_bytes[i] = h.sec_len[i]; }
}
}  // namespace vox_snap
