// vox_model.cpp -- the model loader (GGUF / SafeTensors -> packed device arena), vox_model_free and the vox_model_* entries that size, replicate and configure a model
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the host units: DESIGN.md, "Host units")
#include "vox_dev_base.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace vox;
using namespace vox_host;

// ------------------------------------------------------------------------------------------------
// model
// ------------------------------------------------------------------------------------------------

// arena layout planner: pass 1 (base == nullptr) only sizes, pass 2 hands out pointers
struct Arena {
    uint8_t* base = nullptr; uint64_t off = 0;
    template <class T> T* take(size_t count) {
        off = (off + 255) / 256 * 256;
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += count * sizeof(T);
        return p;
    }
};

#define ENC_PFX "mm_streams_embeddings.embedding_module.whisper_encoder"       /* models/weights.rs:221 */
#define EMB_PFX "mm_streams_embeddings.embedding_module"
#define TOK_NAME EMB_PFX ".tok_embeddings.weight"                               /* models/weights.rs:225 */
#define ADP_PFX EMB_PFX ".audio_language_projection"                            /* models/weights.rs:227 */

// ---- tensor sources: GGUF (Q4 path) and SafeTensors (f32 path) behind one lookup ----------------------------
enum { DT_F32 = 0, DT_F16 = 1, DT_Q4_0 = 2, DT_BF16 = 3 };
struct TensorView { std::vector<uint64_t> shape; int dtype = 0; const uint8_t* data = nullptr; uint64_t nbytes = 0; };   // shape in PyTorch order
struct TensorSource {
    virtual ~TensorSource() {}
    virtual bool find(const std::string& name, TensorView* out) const = 0;
    virtual uint64_t max_q4_bytes() const { return 0; }
};
struct GgufSource : TensorSource {
    vox_gguf* g = nullptr;
    ~GgufSource() override { if (g) vox_gguf_close(g); }
    bool find(const std::string& name, TensorView* out) const override {
        const GTensor* t = g->find(name); if (!t) return false;
        out->shape.assign(t->dims, t->dims + t->ndims); std::reverse(out->shape.begin(), out->shape.end());   // gguf/loader.rs:497-499
        out->dtype = (int)t->dtype; out->data = g->data(t); out->nbytes = t->nbytes; return true;
    }
    uint64_t max_q4_bytes() const override { uint64_t m = 0; for (auto& t : g->tensors) if (t.dtype == 2) m = std::max<uint64_t>(m, t.nbytes); return m; }
};
// what a load looked up: (name -> shape, dtype) of every tensor the loader asked for.  Kept with the model so that a replica's arena can be laid out without the file.
struct RecordingSource : TensorSource {
    const TensorSource* in; mutable std::map<std::string, TensorMeta> seen;
    explicit RecordingSource(const TensorSource* s) : in(s) {}
    bool find(const std::string& name, TensorView* out) const override { if (!in->find(name, out)) return false; TensorMeta& t = seen[name]; t.shape = out->shape; t.dtype = out->dtype; t.nbytes = out->nbytes; return true; }
    uint64_t max_q4_bytes() const override { return in->max_q4_bytes(); }
};
struct ManifestSource : TensorSource {      // shapes only (data == nullptr): good for VOX_LOAD_LAYOUT_ONLY builds, which never touch tensor data
    const std::map<std::string, TensorMeta>* m;
    bool find(const std::string& name, TensorView* out) const override { auto it = m->find(name); if (it == m->end()) return false; out->shape = it->second.shape; out->dtype = it->second.dtype; out->data = nullptr; out->nbytes = it->second.nbytes; return true; }
};
// SafeTensors: u64 header length, JSON header {"name": {"dtype": "BF16", "shape": [..], "data_offsets": [a, b]}, ...}, raw data
// (models/weights.rs:16-66 load_tensor accepts F32 / F16 / BF16).
struct SafeTensorsSource : TensorSource {
    uint8_t* map = nullptr; size_t size = 0; std::map<std::string, TensorView> tensors;
    ~SafeTensorsSource() override { if (map) munmap(map, size); }
    bool find(const std::string& name, TensorView* out) const override { auto it = tensors.find(name); if (it == tensors.end()) return false; *out = it->second; return true; }
    static void skip_ws(const char*& p, const char* e) { while (p < e && (*p == ' ' || *p == '\n' || *p == '\t' || *p == '\r')) p++; }
    static bool parse_string(const char*& p, const char* e, std::string* out) {
        skip_ws(p, e); if (p >= e || *p != '"') return false; p++; out->clear();
        while (p < e && *p != '"') { if (*p == '\\' && p + 1 < e) { p++; } out->push_back(*p++); }
        if (p >= e) return false; p++; return true;
    }
    static bool skip_value(const char*& p, const char* e) {   // any JSON value (used for __metadata__)
        skip_ws(p, e); if (p >= e) return false;
        if (*p == '"') { std::string s; return parse_string(p, e, &s); }
        if (*p == '{' || *p == '[') {
            const char open = *p, close = open == '{' ? '}' : ']'; int depth = 0;
            while (p < e) {
                if (*p == '"') { std::string s; if (!parse_string(p, e, &s)) return false; continue; }
                if (*p == open) depth++; else if (*p == close) { depth--; if (depth == 0) { p++; return true; } }
                p++;
            }
            return false;
        }
        while (p < e && *p != ',' && *p != '}' && *p != ']') p++;
        return true;
    }
    int32_t open(const char* path) {
        int fd = ::open(path, O_RDONLY);
        if (fd < 0) return fail(VOX_ERR_IO, "cannot open %s: %s", path, strerror(errno));
        struct stat st;
        if (fstat(fd, &st) != 0 || st.st_size < 8) { close(fd); return fail(VOX_ERR_IO, "SafeTensors file too small"); }
        void* mp = mmap(nullptr, st.st_size, PROT_READ, MAP_PRIVATE, fd, 0); close(fd);
        if (mp == MAP_FAILED) return fail(VOX_ERR_IO, "mmap of %s failed", path);
        map = (uint8_t*)mp; size = st.st_size;
        if (size < 8) return fail(VOX_ERR_IO, "SafeTensors file too small");
        uint64_t hlen; std::memcpy(&hlen, map, 8);
        if (hlen > size - 8) return fail(VOX_ERR_IO, "SafeTensors header length out of range");
        const char* p = (const char*)map + 8; const char* e = p + hlen; const uint8_t* data0 = map + 8 + hlen; const uint64_t dsize = size - 8 - hlen;
        skip_ws(p, e); if (p >= e || *p != '{') return fail(VOX_ERR_IO, "SafeTensors header is not a JSON object"); p++;
        for (;;) {
            skip_ws(p, e); if (p < e && *p == '}') break;
            std::string name; if (!parse_string(p, e, &name)) return fail(VOX_ERR_IO, "bad SafeTensors header (key)");
            skip_ws(p, e); if (p >= e || *p != ':') return fail(VOX_ERR_IO, "bad SafeTensors header (colon)"); p++;
            if (name == "__metadata__") { if (!skip_value(p, e)) return fail(VOX_ERR_IO, "bad SafeTensors metadata"); }
            else {
                skip_ws(p, e); if (p >= e || *p != '{') return fail(VOX_ERR_IO, "bad SafeTensors entry for '%s'", name.c_str()); p++;
                TensorView tv; std::string dt; uint64_t off[2] = {0, 0}; bool have_dt = false, have_off = false, have_shape = false;
                for (;;) {
                    skip_ws(p, e); if (p < e && *p == '}') { p++; break; }
                    std::string key; if (!parse_string(p, e, &key)) return fail(VOX_ERR_IO, "bad SafeTensors entry key");
                    skip_ws(p, e); if (p >= e || *p != ':') return fail(VOX_ERR_IO, "bad SafeTensors entry"); p++;
                    if (key == "dtype") { if (!parse_string(p, e, &dt)) return fail(VOX_ERR_IO, "bad dtype"); have_dt = true; }
                    else if (key == "shape" || key == "data_offsets") {
                        skip_ws(p, e); if (p >= e || *p != '[') return fail(VOX_ERR_IO, "bad array"); p++;
                        std::vector<uint64_t> v;
                        for (;;) { skip_ws(p, e); if (p < e && *p == ']') { p++; break; } char* q; v.push_back(strtoull(p, &q, 10)); if (q == p) return fail(VOX_ERR_IO, "bad number"); p = q; skip_ws(p, e); if (p < e && *p == ',') p++; }
                        if (key == "shape") { tv.shape = v; have_shape = true; } else { if (v.size() != 2) return fail(VOX_ERR_IO, "bad data_offsets"); off[0] = v[0]; off[1] = v[1]; have_off = true; }
                    } else if (!skip_value(p, e)) return fail(VOX_ERR_IO, "bad SafeTensors value");
                    skip_ws(p, e); if (p < e && *p == ',') p++;
                }
                if (!have_dt || !have_off || !have_shape) return fail(VOX_ERR_IO, "incomplete SafeTensors entry '%s'", name.c_str());
                if (dt == "F32") tv.dtype = DT_F32; else if (dt == "F16") tv.dtype = DT_F16; else if (dt == "BF16") tv.dtype = DT_BF16;
                else return fail(VOX_ERR_UNSUPPORTED, "Unsupported dtype %s for tensor '%s'", dt.c_str(), name.c_str());   // weights.rs:60-64
                if (off[1] < off[0] || off[1] > dsize) return fail(VOX_ERR_IO, "tensor '%s' exceeds file size", name.c_str());
                uint64_t ne = 1; for (auto d : tv.shape) ne *= d;
                if (off[1] - off[0] != ne * (tv.dtype == DT_F32 ? 4 : 2)) return fail(VOX_ERR_IO, "tensor '%s' byte size does not match its shape", name.c_str());
                tv.data = data0 + off[0]; tv.nbytes = off[1] - off[0]; tensors[name] = tv;
            }
            skip_ws(p, e); if (p < e && *p == ',') p++;
        }
        return VOX_OK;
    }
};

static float half_bits_to_f32(uint16_t x) {
    const uint32_t sign = (uint32_t)(x & 0x8000u) << 16; uint32_t e = (x >> 10) & 0x1f, man = x & 0x3ffu, bits;
    if (e == 0) { if (!man) bits = sign; else { int k = -1; do { man <<= 1; k++; } while (!(man & 0x400u)); bits = sign | ((uint32_t)(112 - k) << 23) | ((man & 0x3ffu) << 13); } }
    else if (e == 31) bits = sign | 0x7f800000u | (man << 13); else bits = sign | ((e + 112) << 23) | (man << 13);
    float f; std::memcpy(&f, &bits, 4); return f;
}
static void to_f32(const TensorView& t, uint64_t ne, float* out) {     // weights.rs:16-66 / gguf/loader.rs:443-474
    if (t.dtype == DT_F32) std::memcpy(out, t.data, ne * 4);
    else if (t.dtype == DT_F16) { const uint16_t* h = (const uint16_t*)t.data; for (uint64_t i = 0; i < ne; i++) out[i] = half_bits_to_f32(h[i]); }
    else { const uint16_t* h = (const uint16_t*)t.data; for (uint64_t i = 0; i < ne; i++) { const uint32_t b = (uint32_t)h[i] << 16; std::memcpy(&out[i], &b, 4); } }
}

namespace {
struct Loader {
    vox_model* m; const TensorSource* src; Arena ar; bool fill; void* staging = nullptr; size_t staging_cap = 0;
    Arena ar2;      // DERIVED data (tile-ordered copies of the Q4 linears): laid out behind the primary planes so a multi-GPU start-up broadcasts only the primary part
    std::map<std::string, bool>* fmt_cache = nullptr;       // first tensor name of a dense linear -> all values bf16-representable (shared by both passes)
    std::string err;

    bool setfail(const std::string& e) { if (err.empty()) err = e; return false; }
    bool need(const std::string& name, TensorView* t) { if (!src->find(name, t)) return setfail("Tensor '" + name + "' not found"); return true; }
    static uint64_t numel(const TensorView& t) { uint64_t n = 1; for (auto d : t.shape) n *= d; return n; }

    const float* f32(const std::string& name, bool required = true) {
        TensorView t;
        if (!src->find(name, &t)) { if (required) setfail("Tensor '" + name + "' not found"); return nullptr; }
        if (t.dtype == DT_Q4_0) { setfail("Cannot load Q4_0 tensor '" + name + "' as f32"); return nullptr; }
        const uint64_t ne = numel(t);
        float* dst = ar.take<float>(ne);
        if (fill) {
            std::vector<float> tmp(ne); to_f32(t, ne, tmp.data());
            if (hipMemcpy(dst, tmp.data(), ne * 4, hipMemcpyHostToDevice) != hipSuccess) setfail("hipMemcpy failed for '" + name + "'");
        }
        return dst;
    }
    // conv weight [Cout][Cin][3] (f32 in the checkpoint) as the im2col GEMM operand W'[co][kk*Cin + ci] = w[co][ci][kk], held as two
    // dense bf16 planes hi + lo (w ~= hi + lo to 2^-17 relative): the conv stem then runs on the matrix cores (dense2_gemm_kernel)
    bool conv_planes(const std::string& name, Q4W* out) {
        TensorView t; if (!need(name, &t)) return false;
        if (t.dtype == DT_Q4_0 || t.shape.size() != 3 || t.shape[2] != 3) return setfail("conv weight '" + name + "' must be a dense [out][in][3] tensor");
        const int64_t Co = (int64_t)t.shape[0], Ci = (int64_t)t.shape[1], K = 3 * Ci;
        if (K % 128) return setfail("conv weight '" + name + "': 3*Cin must be a multiple of 128");
        uint16_t* hi = ar.take<uint16_t>((size_t)Co * K); uint16_t* lo = ar.take<uint16_t>((size_t)Co * K);
        *out = Q4W{(const uint4*)hi, lo, (int)Co, (int)K, (int)(K / 32), WFMT_BF16X2};
        if (fill) {
            const uint64_t ne = numel(t); std::vector<float> w(ne); to_f32(t, ne, w.data());
            std::vector<uint16_t> h((size_t)Co * K), l((size_t)Co * K);
            auto rne = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); };
            for (int64_t co = 0; co < Co; co++)
                for (int64_t ci = 0; ci < Ci; ci++)
                    for (int kk = 0; kk < 3; kk++) {
                        const float v = w[(size_t)(co * Ci + ci) * 3 + kk];
                        const uint16_t hb = rne(v); const uint32_t hu = (uint32_t)hb << 16; float hf; std::memcpy(&hf, &hu, 4);
                        const size_t d = (size_t)co * K + (size_t)kk * Ci + ci;
                        h[d] = hb; l[d] = rne(v - hf);
                    }
            if (hipMemcpy(hi, h.data(), h.size() * 2, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(lo, l.data(), l.size() * 2, hipMemcpyHostToDevice) != hipSuccess)
                return setfail("hipMemcpy failed for conv planes");
        }
        return true;
    }
    // linear made of `parts` source tensors [N_i][K]; rows concatenated (interleave=false) or interleaved (true).
    // Q4_0 sources -> re-packed Q4 planes; dense sources (BF16, or F16/F32 holding bf16-representable values) -> bf16 plane.
    bool lin(const std::vector<std::string>& parts, bool interleave, Lin* L, bool require_q4, bool tile = true) {
        int64_t K = -1, Ntot = 0; std::vector<TensorView> ts; int kind = -1;
        for (auto& n : parts) {
            TensorView t; if (!need(n, &t)) return false;
            if (require_q4 && t.dtype != DT_Q4_0) return setfail("Expected Q4_0 for '" + n + "'");                  // gguf/loader.rs:393-395
            if (t.shape.size() != 2) return setfail("Tensor '" + n + "' is not 2-D");
            const int64_t nn = (int64_t)t.shape[0], k = (int64_t)t.shape[1];
            if (k % 32) return setfail("tensor '" + n + "' has an inner dimension not divisible by 32");
            if (K < 0) K = k; else if (K != k) return setfail("fused tensors disagree on K");
            if (interleave && !ts.empty() && nn != (int64_t)ts[0].shape[0]) return setfail("interleaved tensors disagree on N");
            const int kd = t.dtype == DT_Q4_0 ? 0 : 1;
            if (kind < 0) kind = kd; else if (kind != kd) return setfail("fused tensors mix Q4_0 and dense dtypes");
            Ntot += nn; ts.push_back(t);
        }
        const int nb = (int)(K / 32);
        if (kind == 0) {
            uint4* qs = ar.take<uint4>((size_t)Ntot * nb); uint16_t* sc = ar.take<uint16_t>((size_t)Ntot * nb);
            L->w = Q4W{qs, sc, (int)Ntot, (int)K, nb, WFMT_Q4_0};
            if (fill) {
                int64_t row0 = 0;
                for (size_t i = 0; i < ts.size(); i++) {
                    const int64_t nn = (int64_t)ts[i].shape[0];
                    const int mul = interleave ? (int)ts.size() : 1, add = interleave ? (int)i : (int)row0;
                    if (upload_repack(m->ctx, ts[i].data, nn * nb, nb, qs, sc, mul, add, staging, staging_cap) != VOX_OK) return setfail(vox_last_error());
                    row0 += nn;
                }
            }
            if (tile && nb % 4 == 0) {   // second copy in MFMA tile order for the batched-decode (M <= 16) kernel
                const size_t n_tiles = (size_t)(Ntot + 15) / 16, nq = (size_t)nb / 4;
                uint4* qt = ar2.take<uint4>(n_tiles * nq * 64); uint16_t* st = ar2.take<uint16_t>(n_tiles * nq * 64);
                L->w.qt = qt; L->w.st = st;
                if (ar2.base) m->tiled.push_back(&L->w);      // (second pass only; the Lin objects live in the model and never move)
                if (fill) {
                    if (launch_q4_tile_build(L->w, qt, st, m->ctx->stream) != hipSuccess || hipStreamSynchronize(m->ctx->stream) != hipSuccess)
                        return setfail("q4_tile_build failed");
                }
            }
            return true;
        }
        // F32 / F16 sources whose values are not all bf16-representable keep their exact f32 values (WFMT_F32: f32 plane + bf16 hi / lo planes;
        // models/weights.rs:16-66 accepts any F32 / F16 / BF16 checkpoint).  The decision is made once per tensor set (both loader passes agree).
        bool exact_bf16 = true;
        {
            auto it = fmt_cache->find(parts[0]);
            if (it != fmt_cache->end()) exact_bf16 = it->second;
            else {
                for (size_t i = 0; i < ts.size() && exact_bf16; i++) {
                    if (ts[i].dtype == DT_BF16) continue;
                    const uint64_t ne = numel(ts[i]);
                    if (ts[i].dtype == DT_F32) { const uint32_t* b = (const uint32_t*)ts[i].data; for (uint64_t e = 0; e < ne; e++) if (b[e] & 0xFFFFu) { exact_bf16 = false; break; } }
                    else { const uint16_t* h = (const uint16_t*)ts[i].data; for (uint64_t e = 0; e < ne; e++) { const float f = half_bits_to_f32(h[e]); uint32_t b; std::memcpy(&b, &f, 4); if (b & 0xFFFFu) { exact_bf16 = false; break; } } }
                }
                (*fmt_cache)[parts[0]] = exact_bf16;
            }
        }
        if (!exact_bf16) {
            float* wf = ar.take<float>((size_t)Ntot * K); uint16_t* hi = ar.take<uint16_t>((size_t)Ntot * K); uint16_t* lo = ar.take<uint16_t>((size_t)Ntot * K);
            L->w = Q4W{(const uint4*)hi, lo, (int)Ntot, (int)K, nb, WFMT_F32}; L->w.qt = (const uint4*)wf;
            if (fill) {
                std::vector<float> host((size_t)Ntot * K); std::vector<uint16_t> h2((size_t)Ntot * K), l2((size_t)Ntot * K);
                auto rne = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); };
                int64_t row0 = 0;
                for (size_t i = 0; i < ts.size(); i++) {
                    const int64_t nn = (int64_t)ts[i].shape[0];
                    std::vector<float> src((size_t)nn * K); to_f32(ts[i], (uint64_t)nn * K, src.data());
                    for (int64_t r = 0; r < nn; r++)
                        std::memcpy(host.data() + (size_t)(interleave ? r * (int64_t)ts.size() + (int64_t)i : row0 + r) * K, src.data() + (size_t)r * K, (size_t)K * 4);
                    row0 += nn;
                }
                for (size_t e = 0; e < host.size(); e++) { const uint16_t hb = rne(host[e]); const uint32_t hu = (uint32_t)hb << 16; float hf; std::memcpy(&hf, &hu, 4); h2[e] = hb; l2[e] = rne(host[e] - hf); }
                if (hipMemcpy(wf, host.data(), host.size() * 4, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(hi, h2.data(), h2.size() * 2, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(lo, l2.data(), l2.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return setfail("hipMemcpy failed for dense f32 weight");
            }
            return true;
        }
        uint16_t* w = ar.take<uint16_t>((size_t)Ntot * K);
        L->w = Q4W{(const uint4*)w, nullptr, (int)Ntot, (int)K, nb, WFMT_BF16};
        if (fill) {
            std::vector<uint16_t> host((size_t)Ntot * K);
            int64_t row0 = 0;
            for (size_t i = 0; i < ts.size(); i++) {
                const int64_t nn = (int64_t)ts[i].shape[0];
                for (int64_t r = 0; r < nn; r++) {
                    uint16_t* dst = host.data() + (size_t)(interleave ? r * (int64_t)ts.size() + (int64_t)i : row0 + r) * K;
                    if (ts[i].dtype == DT_BF16) std::memcpy(dst, (const uint16_t*)ts[i].data + (size_t)r * K, (size_t)K * 2);
                    else {
                        for (int64_t k = 0; k < K; k++) {
                            float f = ts[i].dtype == DT_F32 ? ((const float*)ts[i].data)[(size_t)r * K + k] : half_bits_to_f32(((const uint16_t*)ts[i].data)[(size_t)r * K + k]);
                            uint32_t b; std::memcpy(&b, &f, 4);
                            if (b & 0xFFFFu) return setfail("internal: dense weight '" + parts[i] + "' was classified bf16-exact but is not");
                            dst[k] = (uint16_t)(b >> 16);
                        }
                    }
                }
                row0 += nn;
            }
            if (hipMemcpy(w, host.data(), host.size() * 2, hipMemcpyHostToDevice) != hipSuccess) return setfail("hipMemcpy failed for dense weight");
        }
        return true;
    }
    // concatenated f32 bias (missing parts -> zeros); returns nullptr if none of the parts exist
    const float* bias_cat(const std::vector<std::pair<std::string, int64_t>>& parts) {
        bool any = false; int64_t tot = 0; TensorView t;
        for (auto& p : parts) { if (!p.first.empty() && src->find(p.first, &t)) any = true; tot += p.second; }
        if (!any) return nullptr;
        float* dst = ar.take<float>(tot);
        if (fill) {
            std::vector<float> host(tot, 0.0f); int64_t o = 0;
            for (auto& p : parts) {
                if (!p.first.empty() && src->find(p.first, &t)) {
                    if (t.dtype == DT_Q4_0 || (int64_t)numel(t) != p.second) setfail("bias '" + p.first + "' has the wrong dtype or size");
                    else to_f32(t, (uint64_t)p.second, host.data() + o);
                }
                o += p.second;
            }
            if (hipMemcpy(dst, host.data(), (size_t)tot * 4, hipMemcpyHostToDevice) != hipSuccess) setfail("hipMemcpy failed for bias");
        }
        return dst;
    }
    const float* rope(int hd, int len, float theta, bool sine) {   // models/layers/rope.rs:35-64 (f32 powf / cos / sin)
        const int half = hd / 2; float* dst = ar.take<float>((size_t)len * half);
        if (fill) {
            std::vector<float> t((size_t)len * half);
            rope_rows_fill(hd, theta, 0, len, len, nullptr, sine ? nullptr : t.data(), sine ? t.data() : nullptr);      // (every row by the tables' f32 formula)
            if (hipMemcpy(dst, t.data(), t.size() * 4, hipMemcpyHostToDevice) != hipSuccess) setfail("hipMemcpy failed for rope table");
        }
        return dst;
    }

    // q4 == true: the GGUF path (gguf/loader.rs:109-491, linears must be Q4_0); false: the SafeTensors f32 path (models/loader.rs:49-300)
    bool run(bool q4) {
        vox_model_cfg& c = m->cfg; char a[320]; TensorView tv;
        // defaults not derivable from shapes: models/config.rs:441-493
        c.enc_head_dim = 64; c.dec_head_dim = 128; c.enc_window = 750; c.dec_window = 8192; c.rope_theta = 1e6f; c.norm_eps = 1e-5f; c.reshape_factor = 4;
        int ne = 0, nd = 0;
        for (;; ne++) { snprintf(a, sizeof a, ENC_PFX ".transformer.layers.%d.attention.wq.weight", ne); if (!src->find(a, &tv)) break; }
        for (;; nd++) { snprintf(a, sizeof a, "layers.%d.attention.wq.weight", nd); if (!src->find(a, &tv)) break; }
        if (ne == 0 || nd == 0) return setfail("model file has no encoder/decoder layers");
        c.enc_layers = ne; c.dec_layers = nd; m->enc.resize(ne); m->dec.resize(nd);
        TensorView cw; if (!need(ENC_PFX ".conv_layers.0.conv.weight", &cw)) return false;
        if (cw.shape.size() != 3 || cw.shape[2] != 3) return setfail("conv weight must be [out][in][3]");
        c.n_mels = (int)cw.shape[1]; c.enc_dim = (int)cw.shape[0];
        m->conv1_w = f32(ENC_PFX ".conv_layers.0.conv.weight"); m->conv1_b = f32(ENC_PFX ".conv_layers.0.conv.bias");
        m->conv2_w = f32(ENC_PFX ".conv_layers.1.conv.weight"); m->conv2_b = f32(ENC_PFX ".conv_layers.1.conv.bias");
        if ((3 * c.n_mels) % 128 == 0 && (3 * c.enc_dim) % 128 == 0) {      // MFMA conv stem (else the VALU conv kernel)
            if (!conv_planes(ENC_PFX ".conv_layers.0.conv.weight", &m->conv1_g) || !conv_planes(ENC_PFX ".conv_layers.1.conv.weight", &m->conv2_g)) return false;
        }
        for (int i = 0; i < ne; i++) {                                                      // gguf/loader.rs:215-260, models/loader.rs:84-196
            EncLayer& L = m->enc[i]; std::string p = std::string(ENC_PFX ".transformer.layers.") + std::to_string(i);
            L.attn_norm = f32(p + ".attention_norm.weight"); L.ffn_norm = f32(p + ".ffn_norm.weight");
            if (!lin({p + ".attention.wq.weight", p + ".attention.wk.weight", p + ".attention.wv.weight"}, false, &L.wqkv, q4)) return false;
            const int64_t hq = L.wqkv.w.N / 3;
            L.wqkv.bias = bias_cat({{p + ".attention.wq.bias", hq}, {"", hq}, {p + ".attention.wv.bias", hq}});   // wk has no bias (:228)
            if (!lin({p + ".attention.wo.weight"}, false, &L.wo, q4)) return false;
            L.wo.bias = bias_cat({{p + ".attention.wo.bias", L.wo.w.N}});
            if (!lin({p + ".feed_forward.w1.weight", p + ".feed_forward.w3.weight"}, true, &L.w13, q4)) return false;
            if (!lin({p + ".feed_forward.w2.weight"}, false, &L.w2, q4)) return false;
            L.w2.bias = bias_cat({{p + ".feed_forward.w2.bias", L.w2.w.N}});
        }
        m->enc_norm = f32(ENC_PFX ".transformer.norm.weight");
        if (!lin({ADP_PFX ".0.weight"}, false, &m->ad0, q4) || !lin({ADP_PFX ".2.weight"}, false, &m->ad2, q4)) return false;    // :378-383
        // tok_embeddings: Q4 (kept Q4 on device, the reference's WASM branch gguf/model.rs:689), or dense (F32/F16 accepted, loader.rs:305-326)
        if (!lin({TOK_NAME}, false, &m->tok, false, true)) return false;
        for (int i = 0; i < nd; i++) {                                                      // gguf/loader.rs:329-375
            DecLayer& L = m->dec[i]; std::string p = "layers." + std::to_string(i);
            if (!lin({p + ".ada_rms_norm_t_cond.0.weight"}, false, &L.ada0, q4) || !lin({p + ".ada_rms_norm_t_cond.2.weight"}, false, &L.ada2, q4)) return false;
            L.attn_norm = f32(p + ".attention_norm.weight"); L.ffn_norm = f32(p + ".ffn_norm.weight");
            if (!lin({p + ".attention.wq.weight", p + ".attention.wk.weight", p + ".attention.wv.weight"}, false, &L.wqkv, q4, true)) return false;
            if (!lin({p + ".attention.wo.weight"}, false, &L.wo, q4, true)) return false;
            if (!lin({p + ".feed_forward.w1.weight", p + ".feed_forward.w3.weight"}, true, &L.w13, q4, true)) return false;
            if (!lin({p + ".feed_forward.w2.weight"}, false, &L.w2, q4, true)) return false;
        }
        m->dec_norm = f32("norm.weight");
        if (!err.empty()) return false;
        // derived dims (PyTorch order [out, in])
        TensorView ewq, dwq, dwk;
        need(std::string(ENC_PFX ".transformer.layers.0.attention.wq.weight"), &ewq); need("layers.0.attention.wq.weight", &dwq); need("layers.0.attention.wk.weight", &dwk);
        c.enc_heads = (int)(ewq.shape[0] / c.enc_head_dim); c.enc_ffn = m->enc[0].w13.w.N / 2;
        c.dec_dim = (int)dwq.shape[1]; c.dec_heads = (int)(dwq.shape[0] / c.dec_head_dim); c.dec_kv_heads = (int)(dwk.shape[0] / c.dec_head_dim);
        c.dec_ffn = m->dec[0].w13.w.N / 2; c.vocab = m->tok.w.N; c.t_cond_dim = m->dec[0].ada0.w.N;
        if (ewq.shape[0] % c.enc_head_dim || dwq.shape[0] % c.dec_head_dim || dwk.shape[0] % c.dec_head_dim || c.dec_kv_heads == 0 || c.dec_heads % c.dec_kv_heads)
            return setfail("attention projection shapes are not multiples of head_dim");
        if ((int)ewq.shape[1] != c.enc_dim || m->ad0.w.K != c.enc_dim * c.reshape_factor || m->ad2.w.N != c.dec_dim || m->ad0.w.N != m->ad2.w.K || m->tok.w.K != c.dec_dim)
            return setfail("inconsistent encoder / adapter / embedding shapes");
        if (c.enc_dim % 32 || c.dec_dim % 32) return setfail("model dims must be multiples of 32");
        m->enc_cos = rope(c.enc_head_dim, m->enc_rope_len, c.rope_theta, false); m->enc_sin = rope(c.enc_head_dim, m->enc_rope_len, c.rope_theta, true);
        m->dec_cos = rope(c.dec_head_dim, m->dec_rope_len, c.rope_theta, false); m->dec_sin = rope(c.dec_head_dim, m->dec_rope_len, c.rope_theta, true);
        return err.empty();
    }
};
}  // namespace

namespace vox_host {
void model_release(vox_model* m) {
    if (!m) return;
    for (vox_model* t : m->twins) { vox_ctx* tc = t->ctx; model_release(t); (void)vox_ctx_destroy(tc); }
    m->twins.clear();
    (void)hipSetDevice(m->ctx->device); (void)hipStreamSynchronize(m->ctx->stream);
    graphs_destroy(m);
    cache_release(m->cache);
    if (m->ctx->pw_model == m) m->ctx->pw_model = nullptr;
    for (void* p : std::initializer_list<void*>{m->arena, m->ada_mul, m->ws, m->d_audio, m->d_mel, m->d_samples, m->d_tokens, m->d_pos, m->d_h, m->d_h2, m->d_wo_acc, m->d_q, m->d_att, m->d_act,
                    m->d_logits, m->d_part_val, m->d_part_idx, m->d_seq_len, m->d_seq_off, m->d_row_pos, m->d_prefix, m->enc_cos_s, m->enc_sin_s, m->eng_stream, m->eng_wob, m->eng_state,
                    m->engb_state[0], m->engb_state[1], m->engb_state[2], m->engb_state[3], m->engb_tab[0], m->engb_tab[1], m->engb_tab[2], m->engb_tab[3], m->pw_x, m->pw_hidden, m->pw_logits,
                    m->pw_ids, m->pw_zero, m->tap.out, m->tap.rows}) if (p) (void)hipFree(p);
    prefix_release(m);
    m->eng_offline.part_val = nullptr; m->eng_offline.part_idx = nullptr;      // the model's d_part_val / d_part_idx, freed above: that binding points at them and does not own them
    binding_release(m->eng_offline); binding_release(m->eng_pw);
    delete m;
}
}  // namespace vox_host
extern "C" int32_t vox_model_free(vox_model* m) { model_release(m); return VOX_OK; }

// shared tail of both loaders: plan the arena, fill it, allocate the decode-step buffers
static int32_t model_build(vox_ctx* ctx, const TensorSource* src_in, bool q4, bool layout_only, vox_model** out) {
    vox_model* m = new vox_model(); m->ctx = ctx;
    RecordingSource rec(src_in); const TensorSource* src = &rec;
    std::map<std::string, bool> fmt_cache;
    Loader plan{m, src, Arena{}, false}; plan.fmt_cache = &fmt_cache;
    if (!plan.run(q4)) { std::string e = plan.err; model_release(m); return fail(VOX_ERR_IO, "%s", e.c_str()); }
    m->arena_primary_bytes = (plan.ar.off + 255) / 256 * 256 + 256;
    m->arena_bytes = m->arena_primary_bytes + plan.ar2.off + 256;
    if (hipMalloc((void**)&m->arena, m->arena_bytes) != hipSuccess) { model_release(m); return fail(VOX_ERR_HIP, "hipMalloc of %.1f MB weight arena failed", m->arena_bytes / 1e6); }
    const size_t max_q4 = layout_only ? 16 : std::max<uint64_t>(src->max_q4_bytes(), 16);
    DevBuf staging; if (staging.alloc(max_q4) != hipSuccess) { model_release(m); return fail(VOX_ERR_HIP, "hipMalloc of staging buffer failed"); }
    Loader fillr{m, src, Arena{m->arena, 0}, !layout_only, staging.p, max_q4}; fillr.fmt_cache = &fmt_cache; fillr.ar2 = Arena{m->arena + m->arena_primary_bytes, 0};
    if (!fillr.run(q4)) { std::string e = fillr.err; model_release(m); return fail(VOX_ERR_IO, "%s", e.c_str()); }
    const vox_model_cfg& c = m->cfg;
    const int qdim = c.dec_heads * c.dec_head_dim;
    if (m->tok.w.fmt == WFMT_BF16 || m->tok.w.fmt == WFMT_F32) { m->argmax_R = 2; m->n_parts = dense_gemv_grid(c.vocab); }
    else { m->argmax_R = q4_gemv_default_R(c.vocab, c.dec_dim, EPI_ARGMAX); m->n_parts = m->argmax_R > 0 ? q4_gemv_grid(c.vocab, m->argmax_R) : 1; }
    hipError_t e = hipSuccess;
    auto A = [&](void** p, size_t n) { if (e == hipSuccess) e = hipMalloc(p, n); };
    A((void**)&m->ada_mul, (size_t)c.dec_layers * c.dec_dim * 4); A((void**)&m->d_pos, 64); A((void**)&m->d_h, (size_t)c.dec_dim * 4 * 4);
    A((void**)&m->d_q, (size_t)qdim * 4 * 4); A((void**)&m->d_att, (size_t)qdim * 4 * 4); A((void**)&m->d_act, (size_t)c.dec_ffn * 4 * 4);
    A((void**)&m->d_h2, (size_t)c.dec_dim * 4); A((void**)&m->d_wo_acc, (size_t)c.dec_layers * c.dec_dim * 8);
    A((void**)&m->d_logits, (size_t)c.vocab * 4); A((void**)&m->d_part_val, (size_t)m->n_parts * 4 * 4); A((void**)&m->d_part_idx, (size_t)m->n_parts * 4 * 4);
    if (e != hipSuccess) { model_release(m); return fail(VOX_ERR_HIP, "hipMalloc of decode buffers failed: %s", hipGetErrorString(e)); }
    m->eng_offline.part_val = m->d_part_val; m->eng_offline.part_idx = m->d_part_idx;      // the captured decode graphs and argmax_embed bake these pointers in: the binding points at them
    if (hipMemset(m->d_wo_acc, 0, (size_t)c.dec_layers * c.dec_dim * 8) != hipSuccess) { model_release(m); return fail(VOX_ERR_HIP, "hipMemset failed"); }
    for (int i = 0; i < c.dec_layers; i++) m->dec[i].ada_mul = m->ada_mul + (size_t)i * c.dec_dim;
    // decode engine eligibility: the real Voxtral decoder geometry, every decoder linear Q4_0 without bias, a 256-CU device.  VOX_ENGINE=0 keeps the per-operator launches.
    {
        const char* ev = knob_str("VOX_ENGINE"); bool ok = !(ev && ev[0] == '0') && c.dec_layers <= 32 && eng_geometry_ok(c.dec_dim, c.dec_heads, c.dec_kv_heads, c.dec_head_dim, c.dec_ffn, c.vocab, 256);
        hipDeviceProp_t prop; if (ok && (hipGetDeviceProperties(&prop, ctx->device) != hipSuccess || prop.multiProcessorCount != 256)) ok = false;
        for (int i = 0; ok && i < c.dec_layers; i++) { const DecLayer& L = m->dec[i]; for (const Lin* w : {&L.wqkv, &L.wo, &L.w13, &L.w2}) if (w->w.fmt != WFMT_Q4_0 || !w->w.qs || !w->w.sc || w->bias) ok = false; }
        if (ok && (m->tok.w.fmt != WFMT_Q4_0 || !m->tok.w.qs)) ok = false;
        // co-residency: the engine's 256 workgroups wait for each other; ask the runtime whether one workgroup (896 threads, 154 KB of LDS) fits per CU at all
        if (ok) { int occ = 0; if (eng_occupancy(&occ) != hipSuccess || occ < 1) { ok = false; (void)hipGetLastError(); } }
        m->eng_ok = ok; m->eng_on = ok;
        {   // the batched engine needs its 256 workgroups co-resident: ask the runtime (a CU mask or a debugger can take CUs away without changing multiProcessorCount)
            const char* bv = knob_str("VOX_BATCH_ENGINE"); int occ = 0;
            m->engb_ok = ok && !(bv && bv[0] == '0') && engb_occupancy(&occ) == hipSuccess && occ >= 1;
            (void)hipGetLastError();
            if (const char* f = knob_str("VOX_BATCH_ENGINE_FLAGS")) m->engb_flags = atoi(f);
            if (const char* f = knob_str("VOX_BATCH_ENGINE_FLAGS2")) m->engb_flags2 = atoi(f);
        }
        if (const char* f = knob_str("VOX_ENGINE_FLAGS")) m->eng_flags = atoi(f);      // measurement knobs of tools/micro/engine_bench (loader depth / probe / XCD-local edges)
        if (const char* f = knob_str("VOX_ENGINE_PACE")) m->eng_pace = atoi(f);
    }
    m->manifest = std::move(rec.seen); m->is_q4 = q4;
    *out = m; return VOX_OK;
}

extern "C" int32_t vox_q4_model_load(vox_ctx* ctx, const char* path, vox_model** out) { return vox_q4_model_load_ex(ctx, path, 0, out); }

// Q4ModelLoader::from_bytes / from_shards + load (gguf/loader.rs:92-128): build the model from an already-open GGUF reader (file,
// memory image or shards).  The reader is only read during the call; the caller closes it afterwards.
extern "C" int32_t vox_q4_model_load_gguf(vox_ctx* ctx, vox_gguf* g, uint32_t flags, vox_model** out) {
    ARGCHK(ctx && g && out, "null argument"); VOXCHK(ctx_bind(ctx));
    GgufSource src; src.g = g;
    const int32_t r = model_build(ctx, &src, true, (flags & VOX_LOAD_LAYOUT_ONLY) != 0, out);
    src.g = nullptr;      // borrowed
    return r;
}
extern "C" int32_t vox_q4_model_load_ex(vox_ctx* ctx, const char* path, uint32_t flags, vox_model** out) {
    ARGCHK(ctx && path && out, "null argument"); VOXCHK(ctx_bind(ctx));
    GgufSource src; VOXCHK(vox_gguf_open(path, &src.g));
    return model_build(ctx, &src, true, (flags & VOX_LOAD_LAYOUT_ONLY) != 0, out);
}

// VoxtralModelLoader::from_file(consolidated.safetensors).load(), models/loader.rs:35-78: the f32 path.  Linear weights are kept
// as bf16 on device (exact for the published BF16 checkpoint; F32/F16 inputs must hold bf16-representable values).
extern "C" int32_t vox_f32_model_load(vox_ctx* ctx, const char* path, vox_model** out) {
    ARGCHK(ctx && path && out, "null argument"); VOXCHK(ctx_bind(ctx));
    SafeTensorsSource src; VOXCHK(src.open(path));
    return model_build(ctx, &src, false, false, out);
}

extern "C" int32_t vox_model_config(const vox_model* m, vox_model_cfg* out) { ARGCHK(m && out, "null argument"); *out = m->cfg; return VOX_OK; }
extern "C" int32_t vox_model_weight_bytes(const vox_model* m, uint64_t* out) { ARGCHK(m && out, "null argument"); *out = m->arena_bytes; return VOX_OK; }
extern "C" int32_t vox_model_memory(const vox_model* m, uint64_t out[4]) {
    ARGCHK(m && out, "null argument");
    out[0] = m->arena_bytes; out[1] = m->arena_primary_bytes;
    out[2] = (m->eng_stream ? eng_stream_bytes(m->cfg.dec_layers, m->cfg.vocab) : 0) + (m->eng_wob ? engb_wo_stream_bytes(m->cfg.dec_layers) : 0);
    out[3] = m->eng_state ? eng_state_bytes() : 0;
    for (int gi = 0; gi < 4; gi++) if (m->engb_state[gi]) out[3] += engb_state_bytes();
    return VOX_OK;
}
extern "C" int32_t vox_model_arena(const vox_model* m, void** p, uint64_t* n) { ARGCHK(m && p && n, "null argument"); *p = m->arena; *n = m->arena_primary_bytes; return VOX_OK; }
// receiver side of a multi-GPU start-up: the primary part of the arena has been filled (vox_model_arena + a broadcast); rebuild everything derived from it on
// this GPU -- the tile-ordered copies of the Q4 linears (the decode engine's weight stream is built lazily at the first decode step either way)
extern "C" int32_t vox_model_arena_finalize(vox_model* m) {
    ARGCHK(m, "null argument"); VOXCHK(ctx_bind(m->ctx));
    for (Q4W* w : m->tiled) HIPCHK(launch_q4_tile_build(*w, const_cast<uint4*>(w->qt), const_cast<uint16_t*>(w->st), m->ctx->stream));
    HIPCHK(hipStreamSynchronize(m->ctx->stream));
    m->eng_ready = false; m->eng_offline.cache = nullptr;      // a stream packed from an earlier arena content is stale
    prefix_release(m);                                     // ... and so is a prefix state computed from it
    if (m->eng_wob) { HIPCHK(hipStreamSynchronize(m->ctx->stream)); (void)hipFree(m->eng_wob); m->eng_wob = nullptr; }
    graphs_destroy(m);
    return VOX_OK;
}

// One more replica of a loaded Q4 model on another context (another GPU, or the same one) WITHOUT the file and without a collective library: the destination arena is
// laid out from the source model's tensor manifest, the primary part (everything parsed from the file: 2.5 GB) is copied device to device -- hipMemcpyPeerAsync over
// xGMI between two GPUs -- and the derived copies are rebuilt on the destination GPU (vox_model_arena_finalize).  What a one-process, one-thread-per-GPU host
// (the shape a Rust `voxtral-transcribe`, bin/transcribe.rs:60-128, would take) needs instead of an RCCL broadcast.
extern "C" int32_t vox_model_replicate(const vox_model* src, vox_ctx* dst_ctx, vox_model** out) {
    ARGCHK(src && dst_ctx && out, "null argument");
    if (!src->is_q4 || src->manifest.empty()) return fail(VOX_ERR_UNSUPPORTED, "vox_model_replicate: Q4 (GGUF) models only");
    VOXCHK(ctx_bind(src->ctx)); HIPCHK(hipStreamSynchronize(src->ctx->stream));      // the source arena is complete (uploads / repack kernels of a fresh load)
    VOXCHK(ctx_bind(dst_ctx));
    ManifestSource ms; ms.m = &src->manifest;
    vox_model* d = nullptr;
    VOXCHK(model_build(dst_ctx, &ms, true, true, &d));
    if (d->arena_primary_bytes != src->arena_primary_bytes || d->arena_bytes != src->arena_bytes) { model_release(d); return fail(VOX_ERR_INVALID, "internal: replica arena layout differs from the source's"); }
    hipError_t e = src->ctx->device == dst_ctx->device ? hipMemcpyAsync(d->arena, src->arena, src->arena_primary_bytes, hipMemcpyDeviceToDevice, dst_ctx->stream)
                                                       : hipMemcpyPeerAsync(d->arena, dst_ctx->device, src->arena, src->ctx->device, src->arena_primary_bytes, dst_ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dst_ctx->stream);
    if (e != hipSuccess) { model_release(d); return fail(VOX_ERR_HIP, "vox_model_replicate: device copy failed: %s", hipGetErrorString(e)); }
    const int32_t r = vox_model_arena_finalize(d);
    if (r != VOX_OK) { model_release(d); return r; }
    *out = d; return VOX_OK;
}

// Ada scales: 1 + w2(gelu(w0 t_embed)) (gguf/model.rs:250-255) -- loop-invariant for a fixed delay, computed once.
extern "C" int32_t vox_model_set_t_embed(vox_model* m, const float* t_embed) {
    ARGCHK(m && t_embed, "null argument"); VOXCHK(ctx_bind(m->ctx));
    const vox_model_cfg& c = m->cfg; vox_ctx* cx = m->ctx;
    if (m->t_embed_set && m->t_embed_host.size() == (size_t)c.dec_dim && !std::memcmp(m->t_embed_host.data(), t_embed, (size_t)c.dec_dim * 4)) return VOX_OK;
    DevBuf dt, dh, ones; HIPCHK(dt.alloc((size_t)c.dec_dim * 4)); HIPCHK(dh.alloc((size_t)c.t_cond_dim * 4)); HIPCHK(ones.alloc((size_t)c.dec_dim * 4));
    std::vector<float> one(c.dec_dim, 1.0f);
    HIPCHK(hipMemcpyAsync(dt.p, t_embed, (size_t)c.dec_dim * 4, hipMemcpyHostToDevice, cx->stream));
    HIPCHK(hipMemcpyAsync(ones.p, one.data(), (size_t)c.dec_dim * 4, hipMemcpyHostToDevice, cx->stream));
    for (int i = 0; i < c.dec_layers; i++) {
        VOXCHK(q4_linear_dev(cx, m->dec[i].ada0.w, nullptr, dt.as<float>(), c.dec_dim, 1, dh.as<float>(), c.t_cond_dim, EPI_GELU));
        VOXCHK(q4_linear_dev(cx, m->dec[i].ada2.w, nullptr, dh.as<float>(), c.t_cond_dim, 1, m->dec[i].ada_mul, c.dec_dim, EPI_RESID, ones.as<float>(), c.dec_dim));
    }
    HIPCHK(hipStreamSynchronize(cx->stream));
    m->t_embed_host.assign(t_embed, t_embed + c.dec_dim); m->t_embed_set = true;
    m->pfx.dec_built = false;      // the decoder's prefix rows depend on the Ada scales (the encoder's do not): rebuilt at the next use
    return VOX_OK;
}
