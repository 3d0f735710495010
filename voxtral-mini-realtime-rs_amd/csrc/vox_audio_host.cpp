// vox_audio_host.cpp -- audio front end, host arithmetic: peak, pad, chunk, mel tables, the resampler's plan and taps, time embedding (no device)
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the device-free host units: DESIGN.md, "Host units")
#include "vox_host_base.h"

using namespace vox_host;

// ------------------------------------------------------------------------------------------------
// audio front-end: host helpers (caller-side in the reference too)
// ------------------------------------------------------------------------------------------------
extern "C" int32_t vox_peak_normalize(float* s, size_t n, float target) {   // audio/io.rs:59-68
    ARGCHK(s || n == 0, "null samples");
    float mx = 0.f;
    for (size_t i = 0; i < n; i++) mx = std::fmax(mx, std::fabs(s[i]));
    if (mx < 1e-10f) return VOX_OK;
    const float scale = target / mx;
    for (size_t i = 0; i < n; i++) s[i] *= scale;
    return VOX_OK;
}
extern "C" int32_t vox_pad_cfg_voxtral(vox_pad_cfg* c) {                     // audio/pad.rs:32-52
    ARGCHK(c, "null cfg"); c->sample_rate = 16000; c->n_left_pad_tokens = 76; c->frame_rate = 12.5f; c->extra_right_pad_tokens = 17; return VOX_OK;
}
namespace vox_host {
size_t pad_spt(const vox_pad_cfg* c) { return (size_t)((float)c->sample_rate / c->frame_rate); }
size_t pad_left(const vox_pad_cfg* c) { return (size_t)c->n_left_pad_tokens * pad_spt(c); }
size_t pad_right(const vox_pad_cfg* c, size_t total) {                // audio/pad.rs:68-74
    const size_t spt = pad_spt(c), rem = total % spt;
    return (rem ? spt - rem : 0) + (size_t)c->extra_right_pad_tokens * spt;
}
}  // namespace vox_host
extern "C" int32_t vox_pad_len(size_t n, const vox_pad_cfg* c, size_t* out) {
    ARGCHK(c && out, "null argument"); ARGCHK(c->frame_rate > 0 && pad_spt(c) > 0, "bad pad config");
    *out = pad_left(c) + n + pad_right(c, n + pad_left(c)); return VOX_OK;
}
extern "C" int32_t vox_pad_audio(const float* in, size_t n, const vox_pad_cfg* c, float* out) {   // audio/pad.rs:89-103
    ARGCHK(c && out && (in || n == 0), "null argument");
    size_t total; VOXCHK(vox_pad_len(n, c, &total));
    std::memset(out, 0, total * sizeof(float));
    if (n) std::memcpy(out + pad_left(c), in, n * sizeof(float));
    return VOX_OK;
}
extern "C" int32_t vox_num_audio_tokens(size_t n, const vox_pad_cfg* c, size_t* out) { ARGCHK(c && out, "null argument"); *out = n / pad_spt(c); return VOX_OK; }

extern "C" int32_t vox_needs_chunking(size_t n, const vox_chunk_cfg* c, int32_t* out) {   // audio/chunk.rs:164-166
    ARGCHK(c && out, "null argument"); *out = n > (size_t)c->max_mel_frames * c->hop_length; return VOX_OK;
}
extern "C" int32_t vox_chunk_plan(size_t n, const vox_chunk_cfg* c, vox_chunk* out, size_t cap, size_t* n_chunks) {  // chunk.rs:120-161
    ARGCHK(c && n_chunks, "null argument");
    ARGCHK(c->max_mel_frames > c->overlap_frames && c->hop_length > 0, "overlap_frames must be < max_mel_frames");
    const size_t max_s = (size_t)c->max_mel_frames * c->hop_length, step = (size_t)(c->max_mel_frames - c->overlap_frames) * c->hop_length;
    size_t idx = 0;
    for (size_t pos = 0; pos < n; pos += step, idx++) {
        const size_t end = std::min(pos + max_s, n);
        if (out && idx < cap) { out[idx].start_sample = pos; out[idx].end_sample = end; out[idx].index = idx; out[idx].is_last = end >= n; }
    }
    *n_chunks = idx; return VOX_OK;
}

// mel tables (audio/mel.rs:260-349), computed on the host exactly as the reference does (f32 math)
static float hz_to_mel(float f) {
    const float F_SP = 200.0f / 3.0f, MIN_LOG_HZ = 1000.0f, MIN_LOG_MEL = MIN_LOG_HZ / F_SP, LOGSTEP = 0.06875174f;
    return f < MIN_LOG_HZ ? f / F_SP : MIN_LOG_MEL + std::log(f / MIN_LOG_HZ) / LOGSTEP;
}
static float mel_to_hz(float m) {
    const float F_SP = 200.0f / 3.0f, MIN_LOG_HZ = 1000.0f, MIN_LOG_MEL = MIN_LOG_HZ / F_SP, LOGSTEP = 0.06875174f;
    return m < MIN_LOG_MEL ? m * F_SP : MIN_LOG_HZ * std::exp((m - MIN_LOG_MEL) * LOGSTEP);
}
namespace vox_host {
void build_filterbank(float* fb) {
    const int n_mels = 128, n_freqs = 201;
    const float mel_min = hz_to_mel(0.0f), mel_max = hz_to_mel(8000.0f);
    float hz[130], fr[201];
    for (int i = 0; i <= n_mels + 1; i++) hz[i] = mel_to_hz(mel_min + (mel_max - mel_min) * (float)i / (float)(n_mels + 1));
    for (int j = 0; j < n_freqs; j++) fr[j] = (float)j * 16000.0f / 400.0f;
    std::memset(fb, 0, sizeof(float) * n_mels * n_freqs);
    for (int i = 0; i < n_mels; i++) {
        const float lo = hz[i], ce = hz[i + 1], up = hz[i + 2];
        for (int j = 0; j < n_freqs; j++) {
            if (fr[j] >= lo && fr[j] <= ce && ce > lo) fb[i * n_freqs + j] = (fr[j] - lo) / (ce - lo);
            else if (fr[j] > ce && fr[j] <= up && up > ce) fb[i * n_freqs + j] = (up - fr[j]) / (up - ce);
        }
        const float bw = hz[i + 2] - hz[i];
        if (bw > 0.0f) { const float en = 2.0f / bw; for (int j = 0; j < n_freqs; j++) fb[i * n_freqs + j] *= en; }
    }
}
void build_hann(int len, float* w) {
    const float PI = 3.14159265358979323846f;
    for (int i = 0; i < len; i++) w[i] = 0.5f * (1.0f - std::cos(2.0f * PI * (float)i / (float)len));
}
}  // namespace vox_host
extern "C" int32_t vox_mel_num_frames(size_t n, size_t* out) { ARGCHK(out, "null out"); *out = (n + 400 - 400) / 160; return VOX_OK; }   // mel.rs:175-182
extern "C" int32_t vox_mel_filterbank(float* out) { ARGCHK(out, "null out"); build_filterbank(out); return VOX_OK; }
extern "C" int32_t vox_hann_window(int32_t len, float* out) { ARGCHK(out && len > 0, "bad argument"); build_hann(len, out); return VOX_OK; }
// ---- sample-rate conversion (audio/resample.rs:16-52).  The reference's whole resampler is two calls into rubato 1.0 (Cargo.toml:41), a third-party crate
// that is not in the tree: Fft::<f32>::new(sr_in, sr_out, 1024, 2, 1, FixedSync::Input) and process_all_into_buffer.  What is implemented is that crate's
// published algorithm (synchronous FFT resampler; restated a second time, independently, by the test-side CPU checker; PARITY UNPINNED against the crate itself):
//   plan    gcd; fft_chunks = ceil(f32(1024) / f32(2) / f32(sr_in / gcd)); fft_in = fft_chunks * sr_in / gcd; fft_out = fft_chunks * sr_out / gcd
//   filter  fft_in taps, f32 arithmetic: (periodic 4-term Blackman-Harris window)^2 * sinc((x - fft_in / 2) * cutoff), unit sum, / (2 fft_in);
//           cutoff = 0.4^(16 / fft_in), times fft_out / fft_in when down-sampling
//   blocks  zero-pad to 2 fft_in, FFT, keep new_len bins (fft_out down, fft_in + 1 up) times the filter spectrum, inverse FFT of length 2 fft_out, overlap-add
//   output  drop output_delay = fft_out / 2 samples, keep ceil(n_in * (f64(sr_out) / f64(sr_in)))
// On the device the block pipeline is one fixed matrix (vox_kernels.hip resample_*_kernel), built once per rate pair and kept in the context.
static long gcd_l(long a, long b) { while (b) { long t = a % b; a = b; b = t; } return a; }
namespace vox_host {
ResamplePlan resample_plan_make(uint32_t sr_in, uint32_t sr_out) {
    ResamplePlan p; const long g = gcd_l(sr_in, sr_out), min_in = sr_in / g, min_out = sr_out / g;
    const long chunks = (long)std::ceil(1024.0f / 2.0f / (float)min_in);
    p.fft_in = chunks * min_in; p.fft_out = chunks * min_out;
    const float base = std::pow(0.4f, 16.0f / (float)p.fft_in);
    p.cutoff = p.fft_in > p.fft_out ? base * (float)p.fft_out / (float)p.fft_in : base;
    p.new_len = p.fft_in < p.fft_out ? p.fft_in + 1 : p.fft_out; p.delay = p.fft_out / 2;
    return p;
}
std::vector<float> resample_taps(const ResamplePlan& p) {
    const long n = p.fft_in; std::vector<float> h((size_t)n);
    const float npf = (float)n, pi = (float)M_PI, pi2 = 2.0f * pi, pi4 = 4.0f * pi, pi6 = 6.0f * pi;
    float sum = 0.f;
    for (long x = 0; x < n; x++) {
        const float xf = (float)x;
        const float bh = 0.35875f - 0.48829f * std::cos(pi2 * xf / npf) + 0.14128f * std::cos(pi4 * xf / npf) - 0.01168f * std::cos(pi6 * xf / npf);
        const float v = (xf - (float)(n / 2)) * p.cutoff;
        const float sinc = v == 0.f ? 1.0f : std::sin(v * pi) / (v * pi);
        h[(size_t)x] = bh * bh * sinc; sum += h[(size_t)x];
    }
    for (auto& v : h) v = v / sum / (float)(2 * n);
    return h;
}
}  // namespace vox_host
// largest block matrix kept on the device (2 fft_out x fft_in f32): every pair of standard audio rates needs <= 9 MB; co-prime rates would need FFTs of sr_in points
static constexpr size_t RESAMPLE_MATRIX_MAX = (size_t)64 << 20;
extern "C" int32_t vox_resample_len(size_t n_in, uint32_t sr_in, uint32_t sr_out, size_t* n_out) {
    ARGCHK(n_out && sr_in > 0 && sr_out > 0, "bad argument");
    *n_out = sr_in == sr_out ? n_in : (size_t)std::ceil(((double)sr_out / (double)sr_in) * (double)n_in); return VOX_OK;      // rubato: (resample_ratio() * len).ceil()
}
// the size of a plan's block matrix, or the refusal of a rate pair whose blocks are too large (shared by vox_resample and the streams fed at their capture rate)
namespace vox_host {
int32_t resample_matrix_bytes(uint32_t sr_in, uint32_t sr_out, const ResamplePlan& p, size_t* bytes) {
    *bytes = (size_t)p.fft_in * 2 * (size_t)p.fft_out * 4;
    if (*bytes > RESAMPLE_MATRIX_MAX) return fail(VOX_ERR_UNSUPPORTED, "resample %u -> %u Hz: FFT blocks of %ld -> %ld samples are not supported (rates must share a large common divisor)", sr_in, sr_out, p.fft_in, p.fft_out);
    return VOX_OK;
}
}  // namespace vox_host
// the plan and the filter taps (host; fft_in floats) -- lets the parity tests check the design independently of the kernels
extern "C" int32_t vox_resample_plan(uint32_t sr_in, uint32_t sr_out, int32_t* fft_in, int32_t* fft_out, int32_t* delay, float* cutoff, float* taps, size_t cap) {
    ARGCHK(fft_in && fft_out && delay && cutoff && sr_in > 0 && sr_out > 0, "bad argument");
    const ResamplePlan p = resample_plan_make(sr_in, sr_out);
    ARGCHK(p.fft_in <= INT32_MAX && p.fft_out <= INT32_MAX, "rates too far from a common divisor");
    *fft_in = (int32_t)p.fft_in; *fft_out = (int32_t)p.fft_out; *delay = (int32_t)p.delay; *cutoff = p.cutoff;
    if (taps) { ARGCHK(cap >= (size_t)p.fft_in, "taps buffer too small (%zu < %ld floats)", cap, p.fft_in); const std::vector<float> h = resample_taps(p); std::memcpy(taps, h.data(), h.size() * 4); }
    return VOX_OK;
}

extern "C" int32_t vox_time_embedding(float t, int32_t dim, float* out) {   // models/time_embedding.rs:41-71
    ARGCHK(out && dim > 0 && dim % 2 == 0, "bad argument");
    const int half = dim / 2; const float log_theta = std::log(10000.0f);
    for (int i = 0; i < half; i++) {
        const float freq = std::exp(-log_theta * (float)i / (float)half), ang = t * freq;
        out[i] = std::cos(ang); out[half + i] = std::sin(ang);
    }
    return VOX_OK;
}
