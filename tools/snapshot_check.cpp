// The session blob's header arithmetic (csrc/vox_snapshot.h) on its own: randomised headers as snap_layout writes them, then mutated -- single fields set to edge
// values, random bytes flipped, the buffer cut short -- through snap_parse, each in a heap buffer of EXACTLY the bytes offered, so that a read past them is the
// sanitizer's to report.  Checked: a header as written is accepted and decodes to what was written; a header cut anywhere is refused; and EVERY accepted header,
// mutated or not, satisfies what a restore relies on without looking again -- sections 16-byte aligned, in order, disjoint, inside the blob, of exactly the length
// their contents need (so no launch or copy sized by them leaves the blob), 0 <= token < vocab, ids <= D < 2^24, E = R D, the window row counts.
// Host code only, no device call: build it with the host sanitizers and run it on the CPU:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I voxtral-mini-realtime-rs_amd/csrc tools/snapshot_check.cpp -o snapshot_check && ./snapshot_check
#include "vox_snapshot.h"

#include <cstdlib>
#include <memory>
#include <random>

using namespace vox_snap;

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "snapshot_check: %s failed at line %d (seed %u, case %d)\n", #cond, __LINE__, seed, kase); return 1; } } while (0)

static unsigned seed = 0; static int kase = 0;

// snap_parse on a heap copy of exactly n bytes of src
static bool parse_exact(const unsigned char* src, size_t n, size_t claimed, SnapHeader* out) {
    std::unique_ptr<unsigned char[]> buf(new unsigned char[n ? n : 1]);
    std::memcpy(buf.get(), src, n);
    char msg[256]; msg[0] = 0;
    const bool ok = snap_parse(buf.get(), claimed, out, msg, sizeof msg);
    if (!ok && !msg[0]) { std::fprintf(stderr, "snapshot_check: a refusal without a message\n"); std::abort(); }
    return ok;
}
// what a restore relies on
static int invariants(const SnapHeader& h, size_t nbytes) {
    CHECK(h.magic == SNAP_MAGIC && h.version == VOX_SNAPSHOT_VERSION && h.total_bytes == nbytes);
    CHECK(h.D >= 0 && h.D < SNAP_POS_LIMIT && (int64_t)h.E == (int64_t)h.reshape_factor * h.D && h.ids_out >= 0 && h.ids_out <= h.D);
    CHECK(h.token >= 0 && h.token < h.vocab);
    CHECK(h.We == std::min<int64_t>(h.E, h.enc_window) && h.Wd == (h.dec_window < 0 ? h.D : std::min(h.D, h.dec_window)));
    CHECK((h.enc_head_dim == 64 || h.enc_head_dim == 128) && (h.dec_head_dim == 64 || h.dec_head_dim == 128));
    CHECK(h.sec_len[SEC_ENC_K] == (uint64_t)h.enc_layers * h.enc_heads * h.We * h.enc_head_dim * 4 && h.sec_len[SEC_ENC_V] == h.sec_len[SEC_ENC_K]);
    CHECK(h.sec_len[SEC_DEC_K] == (uint64_t)h.dec_layers * h.dec_kv_heads * h.Wd * h.dec_head_dim * 4 && h.sec_len[SEC_DEC_V] == h.sec_len[SEC_DEC_K]);
    CHECK(h.sec_len[SEC_SAMPLES] == (uint64_t)std::min<int64_t>(h.n_written, SNAP_SAMPLE_RING) * 4 && h.sec_len[SEC_TOKENS] == (uint64_t)(h.D + 1) * 4);
    CHECK(h.sec_len[SEC_IN_SAMPLES] % 4 == 0 && h.sec_len[SEC_IN_SAMPLES] <= (uint64_t)SNAP_IN_RING_MAX * 4 && (h.sample_rate != 16000 || h.sec_len[SEC_IN_SAMPLES] == 0));
    CHECK((h.n_scores == 0 || h.n_scores == h.ids_out) && (h.n_alts == 0 || h.n_alts == h.ids_out));
    CHECK(h.sec_len[SEC_SCORES] == (uint64_t)h.n_scores * SNAP_SCORE_BYTES && h.sec_len[SEC_ALTS] == (uint64_t)h.n_alts * SNAP_ALTS_BYTES);
    uint64_t end = sizeof(SnapHeader);
    for (int i = 0; i < SEC_COUNT; i++) {
        CHECK(h.sec_off[i] % 16 == 0 && h.sec_off[i] >= end && h.sec_off[i] <= nbytes && h.sec_len[i] <= nbytes - h.sec_off[i]);
        end = h.sec_off[i] + h.sec_len[i];
    }
    CHECK(std::isfinite(h.gain) && h.sample_rate > 0 && h.n_pushed >= 0 && h.n_written >= 0 && h.in_written >= 0);
    return 0;
}

static int run(unsigned sd, int cases) {
    seed = sd; std::mt19937 rng(sd);
    auto pick = [&](int64_t lo, int64_t hi) { return (int64_t)(lo + rng() % (uint64_t)(hi - lo + 1)); };
    int accepted_mutants = 0;
    for (kase = 0; kase < cases; kase++) {
        vox_model_cfg c{};
        c.enc_layers = (int)pick(1, 32); c.enc_heads = (int)pick(1, 32); c.enc_head_dim = pick(0, 1) ? 64 : 128; c.enc_window = (int)pick(0, 1500);
        c.dec_layers = (int)pick(1, 26); c.dec_kv_heads = (int)pick(1, 8); c.dec_head_dim = pick(0, 3) ? 128 : 64; c.dec_window = pick(0, 4) ? (int)pick(0, 9000) : -1;
        c.vocab = (int)pick(1, 200000); c.reshape_factor = (int)pick(1, 4);
        SnapHeader h{}; h.magic = SNAP_MAGIC; h.version = VOX_SNAPSHOT_VERSION; h.fingerprint = rng(); h.t_embed_hash = rng(); h.gain = (float)pick(1, 400) / 100.f;
        const bool rate = pick(0, 2) == 0; h.sample_rate = rate ? (uint32_t)pick(8000, 96000) : 16000; if (h.sample_rate == 16000 && rate) h.sample_rate = 48000;
        SnapShape s; s.D = pick(0, 3) ? pick(SNAP_PREFIX_POS, 20000) : pick(0, SNAP_POS_LIMIT - 1); s.E = (int64_t)c.reshape_factor * s.D;
        h.n_pushed = pick(0, (int64_t)1 << 34); h.in_written = rate ? h.n_pushed : 0; s.n_written = rate ? pick(0, h.n_pushed) : h.n_pushed; h.n_written = s.n_written;
        s.in_samples = rate ? std::min<int64_t>(h.in_written, (int64_t)1 << pick(10, 20)) : 0;
        h.D = (int32_t)s.D; h.E = (int32_t)s.E; h.ids_out = (int32_t)pick(0, s.D); h.token = (int32_t)pick(0, c.vocab - 1); h.scores_on = (int32_t)pick(0, 1); h.alts_k = pick(0, 1) ? (int32_t)pick(1, 8) : 0;
        s.n_scores = h.scores_on ? h.ids_out : 0; s.n_alts = h.alts_k ? h.ids_out : 0;
        h.total_bytes = snap_layout(c, s, &h);
        const size_t total = (size_t)h.total_bytes;
        unsigned char raw[sizeof(SnapHeader)]; std::memcpy(raw, &h, sizeof h);
        // as written: accepted, decoded to itself, the invariants hold
        SnapHeader got{};
        CHECK(parse_exact(raw, sizeof raw, total, &got));
        CHECK(std::memcmp(&got, &h, sizeof h) == 0);
        if (invariants(got, total)) return 1;
        vox_snapshot_info info; snap_info(got, &info);
        CHECK(info.positions == h.D && info.total_bytes == h.total_bytes && info.section_bytes[SEC_TOKENS] == h.sec_len[SEC_TOKENS]);
        // cut anywhere: refused, and nothing behind the cut is read (the buffer ends there)
        for (int t = 0; t < 6; t++) { const size_t n = t == 0 ? 0 : t == 1 ? sizeof raw - 1 : (size_t)pick(0, sizeof raw - 1); CHECK(!parse_exact(raw, n, n, &got)); }
        CHECK(!parse_exact(raw, sizeof raw, total - 1, &got) && !parse_exact(raw, sizeof raw, total + 16, &got));
        // mutated: refused, or accepted with the invariants intact
        for (int t = 0; t < 48; t++) {
            unsigned char mut[sizeof raw]; std::memcpy(mut, raw, sizeof raw);
            SnapHeader* q = reinterpret_cast<SnapHeader*>(mut);
            size_t claimed = total;
            switch (pick(0, 9)) {
                case 0: for (int k = (int)pick(1, 4); k > 0; k--) mut[pick(0, sizeof raw - 1)] ^= (unsigned char)(1u << pick(0, 7)); break;
                case 1: for (int k = (int)pick(1, 8); k > 0; k--) mut[pick(0, sizeof raw - 1)] = (unsigned char)rng(); break;
                case 2: q->sec_off[pick(0, SEC_COUNT - 1)] = pick(0, 3) ? (uint64_t)pick(0, (int64_t)total + 64) : ~(uint64_t)0 - (uint64_t)pick(0, 64); break;
                case 3: q->sec_len[pick(0, SEC_COUNT - 1)] = pick(0, 3) ? (uint64_t)pick(0, (int64_t)total + 64) : ~(uint64_t)0 - (uint64_t)pick(0, 64); break;
                case 4: q->token = pick(0, 1) ? q->vocab + (int32_t)pick(0, 3) : -(int32_t)pick(1, 3); break;
                case 5: { int32_t* w = &q->D + pick(0, 19); *w = (int32_t)(pick(0, 1) ? pick(-3, 3) : (int64_t)(int32_t)rng()); break; }      // any of the 20 words from D to Wd
                case 6: q->total_bytes = (uint64_t)pick(0, 2 * (int64_t)total); claimed = (size_t)q->total_bytes; break;      // a consistent lie about the length
                case 7: q->n_written = (int64_t)rng() * (pick(0, 1) ? 1 : -1); break;
                case 8: { uint64_t a = pick(0, SEC_COUNT - 1), b2 = pick(0, SEC_COUNT - 1); std::swap(q->sec_off[a], q->sec_off[b2]); break; }
                default: q->version = (uint32_t)pick(0, 3); q->magic ^= (uint32_t)pick(0, 1); break;
            }
            if (parse_exact(mut, sizeof mut, claimed, &got)) { accepted_mutants++; if (invariants(got, claimed)) return 1; }
        }
    }
    std::printf("seed %u: %d headers as written accepted, %d of %d mutants accepted, every accepted header within the invariants\n", sd, cases, accepted_mutants, cases * 48);
    return 0;
}

int main(int argc, char** argv) {
    const int cases = argc > 1 ? std::atoi(argv[1]) : 4000;
    for (unsigned sd = 1; sd <= 4; sd++) if (run(sd, cases)) return 1;
    std::printf("snapshot_check: ok\n");
    return 0;
}
