// vox_host_base.h -- what the host units share that needs no device: the error channel, the planners' structs, the resampler's plan, and the
// declarations of the device-free units' functions that another unit calls.  Includes no HIP header: the units built as plain C++ include this one only.
#pragma once
#include "../../include/voxtral_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace vox_host {
// ---- vox_ctx.cpp
int32_t fail(int32_t code, const char* fmt, ...);
}  // namespace vox_host

namespace vox_host {
#define VOXCHK(expr) do { int32_t _r = (expr); if (_r != VOX_OK) return _r; } while (0)
#define ARGCHK(cond, ...) do { if (!(cond)) return fail(VOX_ERR_INVALID, __VA_ARGS__); } while (0)

struct ResamplePlan { long fft_in = 0, fft_out = 0, new_len = 0, delay = 0; float cutoff = 0.f; };

// RoPE rows (models/layers/rope.rs:35-64), the ONE implementation (rope_row_fill, the row; rope_rows_fill, rows of it): the load-time tables (vox_model.cpp), the streaming encoder's table (vox_api.cpp) and
// vox_debug_rope_rows are filled here.  Rows first .. first + n - 1 of cos / sin [n][hd / 2] (either may be null); inv (hd / 2 floats, may be null): the f32 factors.
// Positions below table_len take the tables' formula -- the f32 product pos * inv, then f32 cos / sin: the bits every table has had.  From table_len on the angle is
// double(pos) * double(inv), cos / sin in double, rounded to f32: the f32 product loses the angle at large positions (its spacing is about 0.5 rad at 4 M).
inline const int ROPE_DEC_TABLE_LEN = 16384, ROPE_ENC_STREAM_TABLE_LEN = 1 << 16;
// the table length the debug entries take a head_dim for (vox_debug_rope_rows, vox_debug_stream_attn): 128 is the decoder's geometry, any other the streaming encoder's
inline int64_t rope_debug_table_len(int hd) { return hd == 128 ? ROPE_DEC_TABLE_LEN : ROPE_ENC_STREAM_TABLE_LEN; }
// one row: cos / sin [half] of position pos from the f32 factors inv [half] (rope_inv_fill) -- the row arithmetic of every caller: rope_rows_fill below, and the
// per-pass fill of an endless group's member rings (group_rope_refill, which computes inv once per group)
inline void rope_inv_fill(int hd, float theta, float* inv_out) { for (int j = 0; j < hd / 2; j++) inv_out[j] = 1.0f / std::pow(theta, (float)(2 * j) / (float)hd); }
inline void rope_row_fill(const float* inv, int half, int64_t pos, int64_t table_len, float* cos_out, float* sin_out) {
    for (int j = 0; j < half; j++) {
        float cv, sv;
        if (pos < table_len) { const float fr = (float)pos * inv[j]; cv = std::cos(fr); sv = std::sin(fr); }
        else { const double fr = (double)pos * (double)inv[j]; cv = (float)std::cos(fr); sv = (float)std::sin(fr); }
        if (cos_out) cos_out[j] = cv;
        if (sin_out) sin_out[j] = sv;
    }
}
inline void rope_rows_fill(int hd, float theta, int64_t first, int64_t n, int64_t table_len, float* inv_out, float* cos_out, float* sin_out) {
    const int half = hd / 2;
    std::vector<float> inv((size_t)half); rope_inv_fill(hd, theta, inv.data());      // (the factors once per call: the expression, and so the bits, of every table so far)
    if (inv_out) std::memcpy(inv_out, inv.data(), (size_t)half * sizeof(float));
    for (int64_t r = 0; r < n; r++) rope_row_fill(inv.data(), half, first + r, table_len, cos_out ? cos_out + (size_t)r * half : nullptr, sin_out ? sin_out + (size_t)r * half : nullptr);
}
}  // namespace vox_host

struct GTensor { std::string name; uint32_t ndims = 0; uint64_t dims[4] = {0, 0, 0, 0}; uint32_t dtype = 0; uint64_t offset = 0, nbytes = 0; };
struct vox_gguf {
    uint8_t* map = nullptr; size_t size = 0; uint32_t version = 0;
    int own = 1;                    // 1: mmap'ed file (munmap), 0: borrowed caller memory (from_bytes), 2: heap copy of shards (free)
    std::vector<GTensor> tensors; std::map<std::string, size_t> index; uint64_t data_off = 0;
    const GTensor* find(const std::string& n) const { auto it = index.find(n); return it == index.end() ? nullptr : &tensors[it->second]; }
    const uint8_t* data(const GTensor* t) const { return map + data_off + t->offset; }
};
namespace vox_host {
inline const int VOX_PREFIX_TOKENS = 38, VOX_TOK_BOS = 1, VOX_TOK_STREAMING_PAD = 32;      // the decoder's fixed prefix: BOS + 37 x STREAMING_PAD (gguf/model.rs:891-892)
inline const int kMaxGroups = 8;
struct SlotPlan { int G = 0; std::vector<std::vector<int>> queue; std::vector<int> steps_g; double cost_ms = 0.0; };
struct SlotSchedule {
    SlotPlan plan; int G = 1, Sl = 16, q_stride = 1, steps = 0; std::vector<int> h_queue; int run_g[kMaxGroups] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t active_at(int t) const { uint32_t a = 0; for (int gi = 0; gi < G; gi++) if (t < run_g[gi]) a |= 1u << gi; return a; }
};
inline const int STREAM_SAMPLE_RING = 1 << 16;      // samples held on the device (a tick reads 160 (4 R + 2) + 400 of them)
inline const int STREAM_FEED_CHUNK = 1 << 15;       // input-rate samples a rate stream's ring takes beyond two blocks; 16-bit samples of the host staging buffer
// The host mirror of ONE live session's feed -- a solo vox_stream's, a group member's: everything feed_plan and feed_pass (vox_feed_plan.cpp) read and advance.
struct FeedState {
    uint32_t sr = 16000; ResamplePlan rp; float* At = nullptr;      // the rate the caller feeds at; at any rate but 16000 a COPY of its plan and the block matrix in use
    float* in_ring = nullptr; int in_ring_n = 0;                    // ... and the session's own input-rate ring (a power of two: stream_rate_plan)
    int64_t n_pushed = 0, n_written = 0;      // samples the caller gave (at sr); samples in the 16 kHz ring (after finish: + the right pad)
    int64_t in_written = 0;                   // input-rate samples copied into the input ring so far
    int pos = 0, ids_out = 0; bool finished = false;      // decoder position of the next tick; ids handed to the caller; the utterance has ended (until a reset)
    void restart(int PC) { n_pushed = n_written = in_written = 0; pos = PC; ids_out = 0; finished = false; }      // create / reset: the session starts behind the prefix
    // what a peek takes back: its tail adds no input samples (in_written stays) and hands out no ids of the session's own (ids_out stays)
    struct Mark { int64_t n_written; int pos; };
    Mark mark() const { return Mark{n_written, pos}; } void rewind(const Mark& k) { n_written = k.n_written; pos = k.pos; finished = false; }
};
// what one call feeds a session: n samples at its rate, then `right` zeros (the right pad of a finishing session); `done` of the n + right written so far; goal16: the
// 16 kHz samples the session holds after the call, before the pad; the ticks up to position `target` run in this call and yield `due` ids
struct FeedPlan { size_t n = 0, right = 0, done = 0, goal16 = 0; int target = 0, due = 0; bool finish = false; };
// one pass: samples [at, at + n_in) of the call go to the session's FIRST ring at in_w0 (a rate session: its input ring; a 16 kHz session: the 16 kHz ring itself, and
// n16 == n_in, i0 == in_w0); the 16 kHz samples [i0, i0 + n16) exist after it (a rate session: to be resampled, the input ring holding in_written samples by then);
// `pad` zeros follow at pad_w0; `ticks` ticks became due
struct FeedPass {
    size_t at = 0, n_in = 0, n16 = 0, pad = 0; int64_t in_w0 = 0, i0 = 0, pad_w0 = 0; int ticks = 0;
    bool idle() const { return n_in == 0 && n16 == 0 && pad == 0 && ticks == 0; }      // an open call's pass is never idle: the callers' stall refusal
};
}  // namespace vox_host

namespace vox_host {
// ---- vox_audio_host.cpp
size_t pad_spt(const vox_pad_cfg* c);
size_t pad_left(const vox_pad_cfg* c);
size_t pad_right(const vox_pad_cfg* c, size_t total);
void build_filterbank(float* fb);
void build_hann(int len, float* w);
ResamplePlan resample_plan_make(uint32_t sr_in, uint32_t sr_out);
std::vector<float> resample_taps(const ResamplePlan& p);
int32_t resample_matrix_bytes(uint32_t sr_in, uint32_t sr_out, const ResamplePlan& p, size_t* bytes);
// ---- vox_batch_plan.cpp
void step_costs(const double* base, const double* meas, bool calib, bool shared, double* out);
SlotSchedule slot_schedule(const std::vector<std::pair<int, int>>& jobs, int force_G, const double* step_ms, int max_groups);
// ---- vox_feed_plan.cpp
int32_t stream_rate_plan(uint32_t sample_rate, ResamplePlan* rp, size_t* rs_bytes, int* in_ring_n);
int32_t feed_plan(const FeedState& f, int R, long left, int max_pos, size_t n, bool finish, int cap, const char* who, FeedPlan* out);
bool feed_open(const FeedState& f, const FeedPlan& p);
int feed_pass_max_ticks(int R);
FeedPass feed_pass(FeedState& f, FeedPlan& p, int R, long left, size_t in_cap);
int32_t peek_second_pass(const char* who);
int32_t peek_max_ticks(const FeedState& f, int R, int due, const char* who, int* T);
int stream_burst_len(int64_t due, int burst, int64_t pos, int64_t next_stop);
int group_burst_rounds(const int* due, int n, int burst, int k, int* b);
}  // namespace vox_host
