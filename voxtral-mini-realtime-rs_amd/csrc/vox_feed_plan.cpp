// vox_feed_plan.cpp -- the feed planner and the stream schedules (no device)
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the device-free host units: DESIGN.md, "Host units")
#include "vox_host_base.h"
#include "vox_page_pool.h"
#include "vox_kv_bf16.h"

using namespace vox_host;

static const int STREAM_IN_RING_MAX = 1 << 20;      // largest input ring (samples): rate pairs whose two blocks + a feed chunk do not fit are refused at create

static long stream_spp(int R) { return 640L * R; }      // samples per decoder position: R encoder rows x 4 frames x 160
// decoder positions determined after n samples of an unfinished stream: position p's last frame 4 R p + 4 R - 1 reads padded samples up to 640 R (p + 1) + 40
static long stream_positions(long left, int R, int64_t n) { const int64_t a = left + n - 40; return a < 0 ? 0 : (long)(a / stream_spp(R)); }

// the 16 kHz samples final after n input samples at the plan's rate: output i reads block (i + delay) / fft_out in full and the tail of the block before, nothing else
static int64_t stream_avail16(const ResamplePlan& p, int64_t n) { return std::max<int64_t>(0, n / p.fft_in * p.fft_out - p.delay); }
// the 16 kHz samples a stream at rate sr holds after n input samples (finished: of an n-sample utterance)
static int32_t stream_samples16(uint32_t sr, const ResamplePlan& p, size_t n, bool finished, size_t* n16) {
    if (sr == 16000) { *n16 = n; return VOX_OK; }
    if (finished) return vox_resample_len(n, sr, 16000, n16);
    *n16 = (size_t)stream_avail16(p, (int64_t)n); return VOX_OK;
}
static int32_t stream_schedule16(size_t n16, bool finished, int32_t* positions, int32_t* ids) {
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
    const long left = (long)pad_left(&pc); const int R = 4;
    long P;
    if (finished) { size_t total; VOXCHK(vox_pad_len(n16, &pc, &total)); P = (long)(total / (size_t)stream_spp(R)); *ids = (int32_t)std::max(P - VOX_PREFIX_TOKENS, 0L); }
    else { P = stream_positions(left, R, (int64_t)n16); *ids = (int32_t)std::max(P - (VOX_PREFIX_TOKENS - 1), 0L); }
    *positions = (int32_t)P;
    return VOX_OK;
}
extern "C" int32_t vox_stream_schedule(size_t n_samples, int32_t finished, int32_t* positions, int32_t* ids) {
    ARGCHK(positions && ids, "null argument"); ARGCHK(n_samples <= ((size_t)1 << 40), "sample count out of range");
    return stream_schedule16(n_samples, finished != 0, positions, ids);
}
extern "C" int32_t vox_stream_schedule_rate(size_t n_samples, uint32_t sample_rate, int32_t finished, int32_t* positions, int32_t* ids, size_t* samples_16k) {
    ARGCHK(positions && ids && samples_16k, "null argument"); ARGCHK(sample_rate > 0, "bad sample rate 0"); ARGCHK(n_samples <= ((size_t)1 << 40), "sample count out of range");
    ResamplePlan p;
    if (sample_rate != 16000) { p = resample_plan_make(sample_rate, 16000); size_t bytes; VOXCHK(resample_matrix_bytes(sample_rate, 16000, p, &bytes)); }
    VOXCHK(stream_samples16(sample_rate, p, n_samples, finished != 0, samples_16k));
    return stream_schedule16(*samples_16k, finished != 0, positions, ids);
}
// what a session fed at sample_rate != 16000 needs (a solo stream, a group's member): the plan, the size of its block matrix, the size of its input ring -- a power of
// two holding two blocks and a feed chunk -- or the refusal of a rate pair vox_resample refuses or whose blocks do not fit the ring
namespace vox_host {
int32_t stream_rate_plan(uint32_t sample_rate, ResamplePlan* rp, size_t* rs_bytes, int* in_ring_n) {
    *rp = resample_plan_make(sample_rate, 16000);
    VOXCHK(resample_matrix_bytes(sample_rate, 16000, *rp, rs_bytes));
    if (2 * rp->fft_in + STREAM_FEED_CHUNK > STREAM_IN_RING_MAX)
        return fail(VOX_ERR_UNSUPPORTED, "a stream at %u Hz: two blocks of %ld samples do not fit its input ring of %d", sample_rate, rp->fft_in, STREAM_IN_RING_MAX);
    int n = 1; while (n < 2 * rp->fft_in + STREAM_FEED_CHUNK) n <<= 1;
    *in_ring_n = n;
    return VOX_OK;
}
}  // namespace vox_host
// ---- the feed planner: ONE implementation for a solo stream and for every member of a group ("The feed planner").  feed_plan is what a push / finish /
// advance entry decides before anything changes; feed_pass is one pass of the call, bounded by the session's two rings -- a call may be larger than both.  Pure host
// arithmetic: the callers turn a pass's amounts into copies, launches and ticks (stream_run; group_stage_pass), vox_debug_stream_feed_passes into rows of numbers.
// 16 kHz samples a session's ring can take: everything from the oldest sample its next tick (at position pos) reads stays
static size_t ring_room16(int R, long left, int pos, int64_t n_written) {
    const long lo = std::max(0L, (4L * R * pos - 3) * 160 - 200 - left);
    return (size_t)STREAM_SAMPLE_RING - (size_t)(n_written - lo);
}
// every check of a call on one session, nothing changed: a refused call can be repeated.  `who`: the message's subject ("the stream", "entry 2: member 5")
namespace vox_host {
int32_t feed_plan(const FeedState& f, int R, long left, int max_pos, size_t n, bool finish, int cap, const char* who, FeedPlan* out) {
    ARGCHK(!f.finished, "%s is finished: a reset starts its next utterance", who);
    FeedPlan p; p.n = n; p.finish = finish;
    VOXCHK(stream_samples16(f.sr, f.rp, (size_t)f.n_pushed + n, finish, &p.goal16));
    if (finish) {
        vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc); size_t total; VOXCHK(vox_pad_len(p.goal16, &pc, &total));
        const int S = (int)(total / (size_t)stream_spp(R));      // the steps at positions 37 .. S - 2 yield the S - 38 ids of the offline path
        ARGCHK(S - 1 <= max_pos, "%s: finishing would reach decoder position %d of a session created for %d", who, S - 1, max_pos);
        p.target = std::max(S - 1, f.pos); p.right = total - (size_t)left - p.goal16;
    } else {
        const long P = stream_positions(left, R, (int64_t)p.goal16);
        ARGCHK(P <= max_pos, "%s: the push would reach decoder position %ld of a session created for %d (a reset starts over)", who, P, max_pos);
        p.target = std::max((int)P, f.pos);
    }
    p.due = p.target - f.pos;
    ARGCHK(cap >= p.due, "%s: out_ids capacity %d < %d ids due", who, cap, p.due);
    *out = p; return VOX_OK;
}
// the most ticks one pass can have due: the ticks whose samples the 16 kHz ring holds at once, and the one a pass's first samples complete
int feed_pass_max_ticks(int R) { return (int)(STREAM_SAMPLE_RING / stream_spp(R)) + 2; }
bool feed_open(const FeedState& f, const FeedPlan& p) { return p.done < p.n + p.right || f.n_written < (int64_t)p.goal16 || f.pos < p.target; }
}  // namespace vox_host
// Advances in_written, n_written and p.done; NOT pos -- the caller runs the ticks.  in_cap: most input samples this pass (a group's 16-bit staging slot).
// A rate session's input ring keeps everything from block c_next - 1 on, c_next the block of the next 16 kHz sample to be produced: that sample reads the tail of the
// block before its own.  Its 16 kHz samples are the ones whose blocks are complete -- at the end of the utterance (finish, the last input sample in) all goal16, blocks
// clipped at its length.  The right pad follows the utterance's last 16 kHz sample, in the same pass where the ring has room.
namespace vox_host {
FeedPass feed_pass(FeedState& f, FeedPlan& p, int R, long left, size_t in_cap) {
    FeedPass q; q.at = p.done;
    size_t room = ring_room16(R, left, f.pos, f.n_written);
    const size_t rest = std::min(p.n - std::min(p.done, p.n), in_cap);
    if (f.sr != 16000) {
        const int64_t c_next = (f.n_written + f.rp.delay) / f.rp.fft_out, keep_from = std::max<int64_t>(0, c_next - 1) * f.rp.fft_in;
        q.n_in = std::min(rest, (size_t)f.in_ring_n - (size_t)std::max<int64_t>(0, f.in_written - keep_from));
        q.in_w0 = f.in_written; f.in_written += (int64_t)q.n_in; p.done += q.n_in;
        const int64_t have16 = p.finish && p.done >= p.n ? (int64_t)p.goal16 : stream_avail16(f.rp, f.in_written);
        q.n16 = std::min((size_t)std::max<int64_t>(0, have16 - f.n_written), room); q.i0 = f.n_written;
    } else {
        q.n_in = q.n16 = std::min(rest, room); q.in_w0 = q.i0 = f.n_written; p.done += q.n_in;
    }
    f.n_written += (int64_t)q.n16; room -= q.n16;
    if (p.done >= p.n && p.done < p.n + p.right && f.n_written >= (int64_t)p.goal16) {
        q.pad = std::min(p.n + p.right - p.done, room); q.pad_w0 = f.n_written; f.n_written += (int64_t)q.pad; p.done += q.pad;
    }
    q.ticks = std::max(0, (int)std::min<long>(p.target, stream_positions(left, R, f.n_written)) - f.pos);
    return q;
}
}  // namespace vox_host

// ---- a peek's parts, common to a solo stream and a group ("Peek").
// A peek is ONE pass: a second would size its room from the advanced position and could overwrite samples the session still reads once it is taken back
namespace vox_host {
int32_t peek_second_pass(const char* who) { return fail(VOX_ERR_INVALID, "internal: %s: a peek needs a second pass", who); }
}  // namespace vox_host
// the most ticks a peek (a finish) of this session can have due: what is still to come is the backlog of a rate session -- 16 kHz samples of its unfinished block, at
// most fft_out + delay of them -- and the right pad, at most one token less a sample + the extra tokens; a tick takes stream_spp samples, and position p needs 40 beyond.
// `due` is checked against it.  `who`: what the message starts with ("", "member 3: ")
namespace vox_host {
int32_t peek_max_ticks(const FeedState& f, int R, int due, const char* who, int* T) {
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc);
    const long spt = (long)pad_spt(&pc), right_max = spt - 1 + (long)pc.extra_right_pad_tokens * spt, backlog = f.sr != 16000 ? f.rp.fft_out + f.rp.delay + 1 : 0;
    *T = (int)((backlog + right_max + 40) / stream_spp(R)) + 1;
    ARGCHK(due <= *T, "internal: %sa peek of %d ticks, %d at the most by the pad and the rate plan", who, due, *T);
    return VOX_OK;
}
}  // namespace vox_host
extern "C" int32_t vox_stream_peek_ids(size_t n_samples, uint32_t sample_rate, int32_t ids_out, int32_t* n) {
    ARGCHK(n, "null argument"); ARGCHK(ids_out >= 0, "ids_out %d", ids_out);
    int32_t positions, ids; size_t n16;
    VOXCHK(vox_stream_schedule_rate(n_samples, sample_rate, 1, &positions, &ids, &n16));
    ARGCHK(ids_out <= ids, "%d ids handed out of an utterance of %d", ids_out, ids);
    *n = ids - ids_out;
    return VOX_OK;
}
// ---- where a burst stream cuts a backlog ("Bursts"): the next burst of a pass with `due` ticks still to run, at position pos, of a stream
// created with burst_ticks = burst.  next_stop: the nearest position > pos at whose tick the host must act first (decoder cache growth, an endless session's wrap, list
// growth, the verification limit).  The smallest of the three, and at least 1: a burst never spans a stop, and a tick is always a burst of 1.
namespace vox_host {
int stream_burst_len(int64_t due, int burst, int64_t pos, int64_t next_stop) { return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(due, burst), next_stop - pos)); }
// ---- the rounds of a burst group's pass ("Bursts in stream groups"): from the members' ticks due in the pass, sorted descending, round k gives
// the first n_r = #{due_z > k B} members b_z = min(due_z - k B, B) ticks; returns n_r (0: the pass is over), b[0 .. n_r) descending.  ceil(max due / B) rounds.  A group's
// host never acts between the ticks of a pass (list growth, the RoPE refill, the pages and the position limits are settled in front of it): there is no next_stop cut.
int group_burst_rounds(const int* due, int n, int burst, int k, int* b) {
    int n_r = 0;
    for (int z = 0; z < n; z++) { const int64_t left = (int64_t)due[z] - (int64_t)k * burst; if (left <= 0) break; b[n_r++] = (int)std::min<int64_t>(left, burst); }
    return n_r;
}
}  // namespace vox_host
extern "C" int32_t vox_stream_group_burst_rounds(const int32_t* due, int32_t n, int32_t burst, int32_t* out, int32_t max_rounds, int32_t* n_rounds) {
    ARGCHK(due && n_rounds && (out || max_rounds == 0), "null argument"); ARGCHK(n >= 1 && n <= 16, "n %d out of range (1..16)", n);
    ARGCHK(burst >= 1 && burst <= VOX_STREAM_BURST_MAX, "burst_ticks %d out of range (1..%d)", burst, VOX_STREAM_BURST_MAX); ARGCHK(max_rounds >= 0, "max_rounds %d is negative", max_rounds);
    for (int z = 0; z < n; z++) {
        ARGCHK(due[z] >= 1 && due[z] <= 65536, "due[%d] = %d out of range (1..65536: a member of a pass has a tick due)", z, due[z]);
        ARGCHK(z == 0 || due[z] <= due[z - 1], "due[%d] = %d above due[%d] = %d: the pass's members are sorted by ticks due, descending", z, due[z], z - 1, due[z - 1]);
    }
    const int rounds = (due[0] + burst - 1) / burst;
    ARGCHK(rounds <= max_rounds, "%d rounds: the output buffer holds %d", rounds, max_rounds);
    for (int k = 0; k < rounds; k++) {
        int32_t* row = out + (size_t)17 * k; std::fill(row, row + 17, 0);
        row[0] = group_burst_rounds(due, n, burst, k, row + 1);
    }
    *n_rounds = rounds;
    return VOX_OK;
}
extern "C" int32_t vox_stream_burst_len(int64_t due, int32_t burst, int64_t pos, int64_t next_stop) { return stream_burst_len(due, burst, pos, next_stop); }
extern "C" int32_t vox_stream_group_pages_for(int64_t positions, int32_t page_rows, int32_t window, int32_t* first_page, int32_t* n_pages) {
    ARGCHK(first_page && n_pages, "null argument"); ARGCHK(positions >= 0 && positions <= ((int64_t)1 << 30), "positions %lld out of range", (long long)positions);
    ARGCHK(page_rows_ok(page_rows), "page_rows %d is not a power of two in %d..%d", page_rows, PAGE_ROWS_MIN, PAGE_ROWS_MAX); ARGCHK(window >= -1, "window %d: -1 is none", window);
    int first, n; pages_held(positions, page_rows, window, &first, &n); *first_page = first; *n_pages = n;
    return VOX_OK;
}

// ---- debug: the feed planner on its own (tests/test_stream_feed_cpu.py).  No device, no model: a fresh session at `sample_rate` (R = 4, the Voxtral left pad, no position
// limit to speak of) takes the calls (n_samples[c], finish[c]) through feed_plan and feed_pass as the drivers do, every due tick taken as run.  One row of 5 per pass:
// call index, input samples appended, 16 kHz samples that entered the 16 kHz ring (a 16 kHz session: the appended ones), pad zeros, ticks.  pass_cap: feed_pass's in_cap (0: none).
// the rounding of a bf16 K/V pool (vox_kv_bf16.h: the function the append, the seed and the restore call on the device), as host arithmetic
extern "C" int32_t vox_kv_round_bf16(const float* in, int64_t n, uint16_t* out) {
    ARGCHK(n >= 0, "n %lld is negative", (long long)n); ARGCHK(n == 0 || (in && out), "null argument");
    for (int64_t i = 0; i < n; i++) out[i] = vox::kv_bf16_round(in[i]);
    return VOX_OK;
}
extern "C" int32_t vox_debug_stream_feed_passes(uint32_t sample_rate, const size_t* n_samples, const int32_t* finish, int32_t n_calls, size_t pass_cap, int64_t* rows, int32_t max_rows,
                                                int32_t* n_rows) {
    ARGCHK(n_rows && (n_calls == 0 || (n_samples && finish)) && (rows || max_rows == 0), "null argument"); ARGCHK(sample_rate > 0, "bad sample rate 0");
    ARGCHK(n_calls >= 0 && max_rows >= 0, "bad count (%d calls, %d rows)", n_calls, max_rows);
    FeedState f; f.sr = sample_rate;
    if (sample_rate != 16000) { size_t bytes; VOXCHK(stream_rate_plan(sample_rate, &f.rp, &bytes, &f.in_ring_n)); }
    vox_pad_cfg pc; vox_pad_cfg_voxtral(&pc); const long left = (long)pad_left(&pc); const int R = 4;
    f.restart(VOX_PREFIX_TOKENS - 1);
    int k = 0;
    for (int c = 0; c < n_calls; c++) {
        ARGCHK(finish[c] >= 0 && finish[c] <= 2, "call %d: finish must be 0, 1 or 2 (a peek)", c); ARGCHK(n_samples[c] <= ((size_t)1 << 36), "call %d: push of %zu samples", c, n_samples[c]);
        const bool peek = finish[c] == 2; ARGCHK(!peek || n_samples[c] == 0, "call %d: finish = 2 (a peek) takes no samples", c);
        char who[32]; snprintf(who, sizeof who, "call %d: the session", c);
        FeedPlan plan; VOXCHK(feed_plan(f, R, left, INT32_MAX, n_samples[c], finish[c] != 0, INT32_MAX, who, &plan));
        f.n_pushed += (int64_t)plan.n;
        const FeedState::Mark was = f.mark();
        for (int pass = 0; feed_open(f, plan); pass++) {
            if (peek && pass > 0) { snprintf(who, sizeof who, "call %d", c); return peek_second_pass(who); }
            const FeedPass q = feed_pass(f, plan, R, left, pass_cap ? pass_cap : SIZE_MAX);
            if (q.idle()) return fail(VOX_ERR_INVALID, "internal: call %d stalled at position %d of %d", c, f.pos, plan.target);
            ARGCHK(k < max_rows, "more than %d passes: the output buffer is too small", max_rows);
            int64_t* r = rows + (size_t)5 * k++;
            r[0] = c; r[1] = (int64_t)q.n_in; r[2] = (int64_t)q.n16; r[3] = (int64_t)q.pad; r[4] = q.ticks;
            f.pos += q.ticks;
        }
        if (peek) { f.rewind(was); continue; }      // the session as it was: the drivers' rollback of the feed
        f.ids_out += plan.due; f.finished = plan.finish;
    }
    *n_rows = k;
    return VOX_OK;
}

// ---- debug: RoPE rows on their own (tests/test_stream_endless_cpu.py).  No device: rope_rows_fill (vox_host_base.h), the function behind every RoPE table, for rows
// first_pos .. first_pos + n - 1.  head_dim 128 is the decoder's geometry (its load-time table has 16 384 rows), any other the encoder's (the streaming encoder's
// table has 65 536): below that length a row has the table's bits, from there on the double-precision angle.
extern "C" int32_t vox_debug_rope_rows(int32_t head_dim, float theta, int64_t first_pos, int32_t n, float* inv_out, float* cos_out, float* sin_out) {
    ARGCHK(inv_out && cos_out && sin_out, "null argument");
    ARGCHK(head_dim >= 2 && head_dim <= 256 && head_dim % 2 == 0, "head_dim %d out of range (even, 2..256)", head_dim);
    ARGCHK(std::isfinite(theta) && theta > 1.0f, "theta %g must be finite and above 1", (double)theta);
    ARGCHK(n >= 0 && n <= (1 << 20), "%d rows out of range (0..%d)", n, 1 << 20);
    ARGCHK(first_pos >= 0 && first_pos + n <= ((int64_t)1 << 24), "rows %lld .. %lld: positions end at 2^24", (long long)first_pos, (long long)(first_pos + n));
    rope_rows_fill(head_dim, theta, first_pos, n, rope_debug_table_len(head_dim), inv_out, cos_out, sin_out);
    return VOX_OK;
}
