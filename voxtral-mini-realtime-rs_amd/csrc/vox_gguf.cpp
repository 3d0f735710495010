// vox_gguf.cpp -- the GGUF reader (no device)
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the device-free host units: DESIGN.md, "Host units")
#include "vox_host_base.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

using namespace vox_host;

// ------------------------------------------------------------------------------------------------
// GGUF reader (gguf/reader.rs:13-223)
// ------------------------------------------------------------------------------------------------
namespace {
struct Cur {
    const uint8_t* p; size_t pos, size; bool bad = false;
    template <class T> T rd() { T v{}; if (pos + sizeof(T) > size) { bad = true; return v; } std::memcpy(&v, p + pos, sizeof(T)); pos += sizeof(T); return v; }
    std::string str() { uint64_t len = rd<uint64_t>(); if (bad || len > size - pos) { bad = true; return {}; } std::string s((const char*)p + pos, len); pos += len; return s; }
    void skip(size_t n) { if (n > size - pos) bad = true; else pos += n; }
    int skip_value(uint32_t ty) {   // gguf/reader.rs:327-376
        switch (ty) {
        case 0: case 1: case 7: skip(1); break;
        case 2: case 3: skip(2); break;
        case 4: case 5: case 6: skip(4); break;
        case 8: (void)str(); break;
        case 9: { uint32_t et = rd<uint32_t>(); uint64_t cnt = rd<uint64_t>(); for (uint64_t i = 0; i < cnt && !bad; i++) if (skip_value(et)) return 1; break; }
        case 10: case 11: case 12: skip(8); break;
        default: return 1;
        }
        return 0;
    }
};
}  // namespace

extern "C" int32_t vox_gguf_close(vox_gguf* g) {
    if (g) { if (g->map && g->own == 1) munmap(g->map, g->size); else if (g->map && g->own == 2) std::free(g->map); delete g; }
    return VOX_OK;
}
// parse the header of g->map / g->size (takes ownership of g: closes it on error)
static int32_t gguf_parse(vox_gguf* g, vox_gguf** out) {
    Cur c{g->map, 0, g->size};
    const uint32_t magic = c.rd<uint32_t>();
    if (c.bad || magic != 0x46554747u) { vox_gguf_close(g); return fail(VOX_ERR_IO, "Invalid GGUF magic: 0x%08X (expected 0x46554747)", magic); }
    g->version = c.rd<uint32_t>();
    if (g->version != 2 && g->version != 3) { uint32_t v = g->version; vox_gguf_close(g); return fail(VOX_ERR_IO, "Unsupported GGUF version: %u (expected 2 or 3)", v); }
    const uint64_t nt = c.rd<uint64_t>(), nkv = c.rd<uint64_t>();
    for (uint64_t i = 0; i < nkv && !c.bad; i++) {
        (void)c.str(); const uint32_t ty = c.rd<uint32_t>();
        if (c.skip_value(ty)) { vox_gguf_close(g); return fail(VOX_ERR_IO, "Unknown GGUF metadata value type"); }
    }
    if (c.bad || nt > (1u << 24)) { vox_gguf_close(g); return fail(VOX_ERR_IO, "Failed to parse GGUF metadata"); }
    g->tensors.resize(nt);
    for (uint64_t i = 0; i < nt; i++) {
        GTensor& t = g->tensors[i];
        t.name = c.str(); t.ndims = c.rd<uint32_t>();
        if (c.bad || t.ndims > 4) { vox_gguf_close(g); return fail(VOX_ERR_IO, "Failed to read tensor %llu", (unsigned long long)i); }
        uint64_t ne = 1; bool ovf = false;
        for (uint32_t d = 0; d < t.ndims; d++) { t.dims[d] = c.rd<uint64_t>(); if (__builtin_mul_overflow(ne, t.dims[d], &ne)) ovf = true; }
        t.dtype = c.rd<uint32_t>(); t.offset = c.rd<uint64_t>();
        if (c.bad) { vox_gguf_close(g); return fail(VOX_ERR_IO, "Failed to read tensor %llu", (unsigned long long)i); }
        if (ovf || ne > (1ull << 60)) { std::string n = t.name; vox_gguf_close(g); return fail(VOX_ERR_IO, "tensor '%s' has an element count that overflows", n.c_str()); }
        if (t.dtype > 2) { uint32_t d = t.dtype; vox_gguf_close(g); return fail(VOX_ERR_IO, "Unsupported GGML dtype code: %u", d); }
        t.nbytes = t.dtype == 0 ? ne * 4 : t.dtype == 1 ? ne * 2 : (ne / 32) * 18;     // reader.rs:37-48
        g->index[t.name] = i;
    }
    g->data_off = (c.pos + 31) / 32 * 32;                                                // reader.rs:177-179
    for (auto& t : g->tensors) {    // checked: a crafted offset / size must not wrap around the bounds test
        uint64_t end = 0;
        if (g->data_off > g->size || __builtin_add_overflow(g->data_off, t.offset, &end) || __builtin_add_overflow(end, t.nbytes, &end) || end > g->size) {
            std::string n = t.name; vox_gguf_close(g); return fail(VOX_ERR_IO, "tensor '%s' exceeds file size", n.c_str());
        }
    }
    *out = g; return VOX_OK;
}
extern "C" int32_t vox_gguf_open(const char* path, vox_gguf** out) {
    ARGCHK(path && out, "null argument");
    int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(VOX_ERR_IO, "cannot open %s: %s", path, strerror(errno));
    struct stat st;
    if (fstat(fd, &st) != 0 || st.st_size < 24) { close(fd); return fail(VOX_ERR_IO, "%s is not a GGUF file (stat failed or shorter than a header)", path); }
    void* mp = mmap(nullptr, st.st_size, PROT_READ, MAP_PRIVATE, fd, 0); close(fd);
    if (mp == MAP_FAILED) return fail(VOX_ERR_IO, "mmap of %s failed", path);
    vox_gguf* g = new vox_gguf(); g->map = (uint8_t*)mp; g->size = st.st_size; g->own = 1;
    return gguf_parse(g, out);
}
// GgufReader::from_bytes (gguf/reader.rs:98-103): parse a GGUF image that is already in host memory.  The memory is BORROWED: it
// must stay valid and unchanged until vox_gguf_close.
extern "C" int32_t vox_gguf_open_memory(const void* data, size_t size, vox_gguf** out) {
    ARGCHK(data && out, "null argument"); ARGCHK(size >= 24, "GGUF image too small (%zu bytes)", size);
    vox_gguf* g = new vox_gguf(); g->map = (uint8_t*)const_cast<void*>(data); g->size = size; g->own = 0;
    return gguf_parse(g, out);
}
// Q4ModelLoader::from_shards (gguf/loader.rs:101-107; the reference's ShardedCursor reads <= 512 MB pieces as one stream): the shards
// are the consecutive pieces of ONE GGUF image; they are concatenated into a private host copy.
extern "C" int32_t vox_gguf_open_shards(const void* const* shards, const size_t* sizes, int32_t n, vox_gguf** out) {
    ARGCHK(shards && sizes && out && n > 0, "bad shard list");
    size_t total = 0; for (int i = 0; i < n; i++) { ARGCHK(shards[i] || sizes[i] == 0, "null shard %d", i); total += sizes[i]; }
    ARGCHK(total >= 24, "GGUF image too small (%zu bytes)", total);
    uint8_t* buf = (uint8_t*)std::malloc(total); if (!buf) return fail(VOX_ERR_IO, "out of host memory for %zu bytes of shards", total);
    size_t o = 0; for (int i = 0; i < n; i++) { std::memcpy(buf + o, shards[i], sizes[i]); o += sizes[i]; }
    vox_gguf* g = new vox_gguf(); g->map = buf; g->size = total; g->own = 2;
    return gguf_parse(g, out);
}
extern "C" int32_t vox_gguf_version(const vox_gguf* g, uint32_t* out) { ARGCHK(g && out, "null argument"); *out = g->version; return VOX_OK; }
extern "C" int32_t vox_gguf_tensor_count(const vox_gguf* g, uint64_t* out) { ARGCHK(g && out, "null argument"); *out = g->tensors.size(); return VOX_OK; }
extern "C" int32_t vox_gguf_tensor_name(const vox_gguf* g, uint64_t i, const char** out) {
    ARGCHK(g && out, "null argument"); ARGCHK(i < g->tensors.size(), "tensor index out of range"); *out = g->tensors[i].name.c_str(); return VOX_OK;
}
extern "C" int32_t vox_gguf_tensor_info(const vox_gguf* g, const char* name, uint64_t dims[4], uint32_t* ndims, uint32_t* dtype, uint64_t* nbytes) {
    ARGCHK(g && name && dims && ndims && dtype && nbytes, "null argument");
    const GTensor* t = g->find(name);
    if (!t) return fail(VOX_ERR_NOTFOUND, "Tensor '%s' not found in GGUF", name);
    for (uint32_t d = 0; d < 4; d++) dims[d] = d < t->ndims ? t->dims[d] : 0;
    *ndims = t->ndims; *dtype = t->dtype; *nbytes = t->nbytes; return VOX_OK;
}
extern "C" int32_t vox_gguf_tensor_data(const vox_gguf* g, const char* name, void* dst, size_t cap) {
    ARGCHK(g && name && dst, "null argument");
    const GTensor* t = g->find(name);
    if (!t) return fail(VOX_ERR_NOTFOUND, "Tensor '%s' not found in GGUF", name);
    ARGCHK(cap >= t->nbytes, "destination too small for '%s' (%zu < %llu)", name, cap, (unsigned long long)t->nbytes);
    std::memcpy(dst, g->data(t), t->nbytes); return VOX_OK;
}
