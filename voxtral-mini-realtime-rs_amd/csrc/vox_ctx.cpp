// vox_ctx.cpp -- the error channel, the context and its device memory, the mel tables, the resampler, the process-wide debug counters
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the host units: DESIGN.md, "Host units")
#include "vox_dev_base.h"

#include <dlfcn.h>

#include <chrono>

using namespace vox;
using namespace vox_host;

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
namespace vox_host {
int32_t fail(int32_t code, const char* fmt, ...) {
    char buf[1024];
    va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof buf, fmt, ap); va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace vox_host

extern "C" const char* vox_last_error(void) { return g_err.c_str(); }
extern "C" int32_t vox_abi_version(void) { return 1; }
extern "C" int32_t vox_device_count(int32_t* n) {
    ARGCHK(n, "null out pointer");
    int c = 0; hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; (void)hipGetLastError(); return VOX_OK; }
    *n = c; return VOX_OK;
}

// ---- roctx ranges with the reference's tracing span names (gguf/model.rs:784 "encode_audio", :878 "transcribe_streaming", :909 "prefill",
// :936-937 "decode"): librocprofiler-sdk-roctx is resolved lazily so the library has no hard dependency on the profiler; without it the
// calls are no-ops.  Under `rocprofv3 --marker-trace` the ranges attribute the kernel trace to the pipeline stages.
namespace {
struct Roctx {
    int (*push)(const char*) = nullptr; int (*pop)() = nullptr;
    Roctx() {
        if (knob_str("VOX_NO_ROCTX")) return;
        void* h = dlopen("librocprofiler-sdk-roctx.so", RTLD_LAZY | RTLD_LOCAL);
        if (!h) h = dlopen("librocprofiler-sdk-roctx.so.1", RTLD_LAZY | RTLD_LOCAL);
        if (!h) return;
        push = reinterpret_cast<int (*)(const char*)>(dlsym(h, "roctxRangePushA")); pop = reinterpret_cast<int (*)()>(dlsym(h, "roctxRangePop"));
        if (!push || !pop) { push = nullptr; pop = nullptr; }
    }
};
}  // namespace
static Roctx& roctx() { static Roctx r; return r; }
namespace vox_host {
void roctx_push(const char* name) { Roctx& r = roctx(); if (r.push) (void)r.push(name); }
void roctx_pop() { Roctx& r = roctx(); if (r.pop) (void)r.pop(); }

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace vox_host
// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------

extern "C" int32_t vox_ctx_create(int32_t device, vox_ctx** out) {
    ARGCHK(out, "null out pointer");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(VOX_ERR_HIP, "no HIP device available (libvoxtral_hip has no CPU fallback)"); }
    ARGCHK(device >= 0 && device < n, "device %d out of range (have %d)", device, n);
    HIPCHK(hipSetDevice(device));
    knobs_load_once();      // the VOX_* measurement knobs are snapshotted ONCE per process (std::call_once): no launch path calls getenv, and a second context created
                            // while another thread transcribes does not touch the table (vox_debug_reload_knobs replaces it: tests only)
    vox_ctx* c = new vox_ctx(); c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(VOX_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(e)); }
    *out = c; return VOX_OK;
}
extern "C" int32_t vox_debug_reload_knobs(void) { knobs_reload(); return VOX_OK; }
extern "C" int32_t vox_debug_attn_launches(uint64_t* out, int32_t cap) {
    ARGCHK(out && cap > 0, "bad argument");
    unsigned long long n[ATTN_FORM_COUNT]; attn_form_counts(n);
    for (int i = 0; i < cap; i++) out[i] = i < ATTN_FORM_COUNT ? (uint64_t)n[i] : 0;
    return VOX_OK;
}
extern "C" int32_t vox_debug_gemm_launches(uint64_t* out, int32_t cap) {
    ARGCHK(out && cap > 0, "bad argument");
    unsigned long long n[GEMM_FORM_COUNT]; gemm_form_counts(n);
    for (int i = 0; i < cap; i++) out[i] = i < GEMM_FORM_COUNT ? (uint64_t)n[i] : 0;
    return VOX_OK;
}
extern "C" int32_t vox_debug_occupy(vox_ctx* c, int32_t workgroups, int32_t micros) {
    ARGCHK(c && workgroups > 0 && workgroups <= 4096 && micros > 0 && micros <= 2000000, "bad argument"); VOXCHK(ctx_bind(c));
    if (!c->occupy_stream) HIPCHK(hipStreamCreateWithFlags(&c->occupy_stream, hipStreamNonBlocking));
    HIPCHK(launch_occupy(workgroups, micros, c->occupy_stream));
    return VOX_OK;
}
extern "C" int32_t vox_ctx_destroy(vox_ctx* c) {
    if (!c) return VOX_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    for (void* p : {(void*)c->d_window, (void*)c->d_cos, (void*)c->d_sin, (void*)c->d_fb, (void*)c->d_fb_lo, (void*)c->d_fb_hi, (void*)c->d_scale})
        if (p) (void)hipFree(p);
    for (auto& e : c->pool) (void)hipFree(e.p);
    if (c->xf_scratch) (void)hipFree(c->xf_scratch);
    if (c->kz_scratch) (void)hipFree(c->kz_scratch);
    if (c->rs_matrix) (void)hipFree(c->rs_matrix);
    if (c->occupy_stream) (void)hipStreamDestroy(c->occupy_stream);
    for (auto e : c->ev_seg) if (e) (void)hipEventDestroy(e);
    if (c->fe_stream) { (void)hipStreamSynchronize(c->fe_stream); (void)hipStreamDestroy(c->fe_stream); }
    for (auto e : c->ev_fe) if (e) (void)hipEventDestroy(e);
    for (auto e : c->ev_enc) if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(c->stream);
    delete c; return VOX_OK;
}
extern "C" int32_t vox_ctx_synchronize(vox_ctx* c) {
    ARGCHK(c, "null ctx"); VOXCHK(ctx_bind(c)); HIPCHK(hipStreamSynchronize(c->stream));
    if (c->pw_model) return pw_after_sync(c->pw_model);      // unverified decode-engine steps of the piecewise surface: their verdict is due at every synchronisation
    return VOX_OK;
}
extern "C" int32_t vox_ctx_set_shared(vox_ctx* c, int32_t shared) { ARGCHK(c, "null context"); c->shared = shared != 0; return VOX_OK; }
extern "C" int32_t vox_ctx_stream(vox_ctx* c, void** s) { ARGCHK(c && s, "null argument"); *s = (void*)c->stream; return VOX_OK; }
extern "C" int32_t vox_dev_alloc(vox_ctx* c, size_t nbytes, void** out) { ARGCHK(c && out, "null argument"); VOXCHK(ctx_bind(c)); HIPCHK(hipMalloc(out, nbytes ? nbytes : 1)); return VOX_OK; }
extern "C" int32_t vox_dev_free(vox_ctx* c, void* p) { ARGCHK(c, "null ctx"); VOXCHK(ctx_bind(c)); if (p) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(p)); } return VOX_OK; }
extern "C" int32_t vox_dev_upload(vox_ctx* c, void* dst, const void* src, size_t n) {
    ARGCHK(c && dst && src, "null argument"); VOXCHK(ctx_bind(c));
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return VOX_OK;
}
extern "C" int32_t vox_dev_download(vox_ctx* c, void* dst, const void* src, size_t n) {
    ARGCHK(c && dst && src, "null argument"); VOXCHK(ctx_bind(c));
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return VOX_OK;
}

extern "C" int32_t vox_dev_copy(vox_ctx* c, void* dst, const void* src, size_t n) {
    ARGCHK(c && dst && src, "null argument"); VOXCHK(ctx_bind(c));
    HIPCHK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); return VOX_OK;
}

namespace vox_host {
int32_t ctx_mel_tables(vox_ctx* c, MelTables* t) {
    if (!c->mel_ready) {
        std::vector<float> win(400), ct(400), st(400), fb(128 * 201);
        std::vector<int> lo(128), hi(128);
        build_hann(400, win.data()); build_filterbank(fb.data());
        for (int m = 0; m < 400; m++) { ct[m] = (float)std::cos(2.0 * M_PI * m / 400.0); st[m] = (float)std::sin(2.0 * M_PI * m / 400.0); }
        for (int i = 0; i < 128; i++) {
            int a = 201, b = 0;
            for (int j = 0; j < 201; j++) if (fb[i * 201 + j] != 0.0f) { a = std::min(a, j); b = std::max(b, j + 1); }
            if (a > b) { a = 0; b = 0; }
            lo[i] = a; hi[i] = b;
        }
        HIPCHK(hipMalloc((void**)&c->d_window, 400 * 4)); HIPCHK(hipMalloc((void**)&c->d_cos, 400 * 4)); HIPCHK(hipMalloc((void**)&c->d_sin, 400 * 4));
        HIPCHK(hipMalloc((void**)&c->d_fb, 128 * 201 * 4)); HIPCHK(hipMalloc((void**)&c->d_fb_lo, 128 * 4)); HIPCHK(hipMalloc((void**)&c->d_fb_hi, 128 * 4));
        HIPCHK(hipMalloc((void**)&c->d_scale, 16));
        HIPCHK(hipMemcpy(c->d_window, win.data(), 400 * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(c->d_cos, ct.data(), 400 * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_sin, st.data(), 400 * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(c->d_fb, fb.data(), 128 * 201 * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(c->d_fb_lo, lo.data(), 128 * 4, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(c->d_fb_hi, hi.data(), 128 * 4, hipMemcpyHostToDevice));
        c->mel_ready = true;
    }
    t->window = c->d_window; t->cos_t = c->d_cos; t->sin_t = c->d_sin; t->fb = c->d_fb; t->fb_lo = c->d_fb_lo; t->fb_hi = c->d_fb_hi;
    return VOX_OK;
}
}  // namespace vox_host

extern "C" int32_t vox_mel_compute_log(vox_ctx* c, const float* samples, size_t n, float* out, int32_t mem_kind) {
    ARGCHK(c && out && (samples || n == 0), "null argument"); VOXCHK(ctx_bind(c));
    const size_t T = n / 160;
    if (T == 0) return VOX_OK;
    MelTables t; VOXCHK(ctx_mel_tables(c, &t));
    if (mem_kind == VOX_MEM_DEVICE) {
        HIPCHK(launch_mel(samples, (long)n, 0, 0, nullptr, t, out, (int)T, 0, c->stream));
        return VOX_OK;
    }
    DevBuf din, dout; HIPCHK(din.alloc(n * 4)); HIPCHK(dout.alloc(T * 128 * 4));
    HIPCHK(hipMemcpyAsync(din.p, samples, n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_mel(din.as<float>(), (long)n, 0, 0, nullptr, t, dout.as<float>(), (int)T, 0, c->stream));
    HIPCHK(hipMemcpyAsync(out, dout.p, T * 128 * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VOX_OK;
}
// a plan's block matrix At[fft_in][2 fft_out] in a fresh device buffer the caller owns (the context's cache below, a vox_stream): the same taps, spectrum and kernel
// whoever asks, so the same bits.  Synchronises the context's stream.
namespace vox_host {
int32_t resample_matrix_build(vox_ctx* c, const ResamplePlan& p, size_t bytes, float** out) {
    const std::vector<float> h = resample_taps(p);
    const long Pi = 2 * p.fft_in; std::vector<double> ct((size_t)Pi), st((size_t)Pi), H((size_t)p.new_len * 2, 0.0);
    for (long j = 0; j < Pi; j++) { ct[(size_t)j] = std::cos(2.0 * M_PI * (double)j / (double)Pi); st[(size_t)j] = std::sin(2.0 * M_PI * (double)j / (double)Pi); }
    for (long k = 0; k < p.new_len; k++) {                                           // filter_f = FFT of the zero-padded taps (only the bins that are kept)
        double re = 0.0, im = 0.0;
        for (long n = 0; n < p.fft_in; n++) { const long j = (k * n) % Pi; re += (double)h[(size_t)n] * ct[(size_t)j]; im -= (double)h[(size_t)n] * st[(size_t)j]; }
        H[(size_t)2 * k] = re; H[(size_t)2 * k + 1] = im;
    }
    float* A = nullptr;
    DevBuf dH; HIPCHK(dH.alloc(H.size() * 8)); HIPCHK(hipMalloc((void**)&A, bytes));
    hipError_t e = hipMemcpyAsync(dH.p, H.data(), H.size() * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_resample_matrix(dH.as<double>(), (int)p.new_len, (int)p.fft_in, (int)p.fft_out, A, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { (void)hipFree(A); return fail(VOX_ERR_HIP, "resample matrix: %s", hipGetErrorString(e)); }
    *out = A;
    return VOX_OK;
}
}  // namespace vox_host
static int32_t resample_matrix_ensure(vox_ctx* c, uint32_t sr_in, uint32_t sr_out, const ResamplePlan& p) {
    if (c->rs_matrix && c->rs_in == sr_in && c->rs_out == sr_out) return VOX_OK;
    size_t bytes; VOXCHK(resample_matrix_bytes(sr_in, sr_out, p, &bytes));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->rs_matrix) { (void)hipFree(c->rs_matrix); c->rs_matrix = nullptr; }
    VOXCHK(resample_matrix_build(c, p, bytes, &c->rs_matrix));
    c->rs_in = sr_in; c->rs_out = sr_out;
    return VOX_OK;
}
extern "C" int32_t vox_resample(vox_ctx* c, const float* in, size_t n_in, uint32_t sr_in, uint32_t sr_out, float* out, size_t cap, size_t* n_out, int32_t mem_kind) {
    ARGCHK(c && out && n_out && (in || n_in == 0), "null argument"); ARGCHK(sr_in > 0 && sr_out > 0, "bad sample rate"); VOXCHK(ctx_bind(c));
    size_t no; VOXCHK(vox_resample_len(n_in, sr_in, sr_out, &no));
    ARGCHK(cap >= no, "output capacity %zu < %zu samples", cap, no);
    *n_out = no; if (no == 0) return VOX_OK;
    hipStream_t s = c->stream;
    if (sr_in == sr_out) {                                                     // resample.rs:17-19: same rate -> clone
        HIPCHK(hipMemcpyAsync(out, in, n_in * 4, mem_kind == VOX_MEM_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToHost, s)); HIPCHK(hipStreamSynchronize(s)); return VOX_OK;
    }
    const ResamplePlan p = resample_plan_make(sr_in, sr_out);
    VOXCHK(resample_matrix_ensure(c, sr_in, sr_out, p));
    DevBuf din, dout;
    const float* d_in = in; float* d_out = out;
    if (mem_kind != VOX_MEM_DEVICE) {
        HIPCHK(din.alloc(n_in * 4)); HIPCHK(dout.alloc(no * 4));
        HIPCHK(hipMemcpyAsync(din.p, in, n_in * 4, hipMemcpyHostToDevice, s)); d_in = din.as<float>(); d_out = dout.as<float>();
    }
    HIPCHK(launch_resample(d_in, (long)n_in, c->rs_matrix, (int)p.fft_in, (int)p.fft_out, (int)p.delay, d_out, (long)no, s));
    if (mem_kind != VOX_MEM_DEVICE) HIPCHK(hipMemcpyAsync(out, d_out, no * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
