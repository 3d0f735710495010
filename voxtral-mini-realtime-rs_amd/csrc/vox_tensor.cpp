// vox_tensor.cpp -- the Q4 tensor and the stand-alone operators (linear, conv stem, attention) on caller buffers
// (one unit of the C ABI of libvoxtral_hip.so, include/voxtral_hip.h; the host units: DESIGN.md, "Host units")
#include "vox_dev_base.h"

using namespace vox;
using namespace vox_host;

// ------------------------------------------------------------------------------------------------
// Q4 tensor + operator (gguf/tensor.rs, op.rs, linear.rs)
// ------------------------------------------------------------------------------------------------
struct vox_q4 { vox_ctx* ctx; Q4W w; void* qs_mem; void* sc_mem; void* qt_mem = nullptr; void* st_mem = nullptr; };

// upload raw 18-byte blocks and re-pack into (qs, sc) planes at [dst_row0 ..) of the destination planes
namespace vox_host {
int32_t upload_repack(vox_ctx* c, const uint8_t* raw, int64_t n_blocks, int nb, uint4* qs, uint16_t* sc, int row_mul, int row_add,
                             void* staging, size_t staging_cap) {
    const size_t bytes = (size_t)n_blocks * 18;
    DevBuf tmp; uint8_t* d_raw = (uint8_t*)staging;
    if (!staging || staging_cap < bytes) { HIPCHK(tmp.alloc(bytes)); d_raw = tmp.as<uint8_t>(); }
    HIPCHK(hipMemcpyAsync(d_raw, raw, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(launch_q4_repack(d_raw, qs, sc, n_blocks, nb, row_mul, row_add, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return VOX_OK;
}
}  // namespace vox_host

extern "C" int32_t vox_q4_tensor_from_bytes(vox_ctx* c, const uint8_t* raw, size_t nbytes, int64_t N, int64_t K, vox_q4** out) {
    ARGCHK(c && raw && out, "null argument"); ARGCHK(N > 0 && K > 0, "bad shape"); VOXCHK(ctx_bind(c));
    const int64_t ne = N * K;
    ARGCHK(ne % 32 == 0, "Q4_0 requires element count divisible by 32, got %lld", (long long)ne);           // tensor.rs:38-41
    const int64_t nblk = ne / 32;
    ARGCHK((int64_t)nbytes == nblk * 18, "Q4_0 byte count mismatch: expected %lld for %lld blocks, got %zu", (long long)(nblk * 18), (long long)nblk, nbytes);
    ARGCHK(K % 32 == 0, "Q4_0 rows must be a whole number of 32-element blocks (K=%lld)", (long long)K);
    vox_q4* q = new vox_q4(); q->ctx = c; q->qs_mem = q->sc_mem = nullptr;
    if (hipMalloc(&q->qs_mem, (size_t)nblk * 16) != hipSuccess || hipMalloc(&q->sc_mem, (size_t)nblk * 2) != hipSuccess) {
        if (q->qs_mem) (void)hipFree(q->qs_mem); delete q; return fail(VOX_ERR_HIP, "hipMalloc failed for Q4 tensor");
    }
    q->w = Q4W{(const uint4*)q->qs_mem, (const uint16_t*)q->sc_mem, (int)N, (int)K, (int)(K / 32)};
    int32_t r = upload_repack(c, raw, nblk, (int)(K / 32), (uint4*)q->qs_mem, (uint16_t*)q->sc_mem, 1, 0, nullptr, 0);
    if (r != VOX_OK) { (void)hipFree(q->qs_mem); (void)hipFree(q->sc_mem); delete q; return r; }
    if ((K / 32) % 4 == 0) {     // MFMA tile-order copy (skinny / large-M kernels); same bits, different order
        const size_t n_tiles = (size_t)(N + 15) / 16, nq = (size_t)(K / 128);
        if (hipMalloc(&q->qt_mem, n_tiles * nq * 64 * 16) == hipSuccess && hipMalloc(&q->st_mem, n_tiles * nq * 64 * 2) == hipSuccess &&
            launch_q4_tile_build(q->w, (uint4*)q->qt_mem, (uint16_t*)q->st_mem, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess) {
            q->w.qt = (const uint4*)q->qt_mem; q->w.st = (const uint16_t*)q->st_mem;
        } else { (void)hipFree(q->qt_mem); (void)hipFree(q->st_mem); (void)hipFree(q->qs_mem); (void)hipFree(q->sc_mem); delete q; return fail(VOX_ERR_HIP, "tile copy of Q4 tensor failed"); }
    }
    *out = q; return VOX_OK;
}
extern "C" int32_t vox_q4_tensor_shape(const vox_q4* q, int64_t* N, int64_t* K) { ARGCHK(q && N && K, "null argument"); *N = q->w.N; *K = q->w.K; return VOX_OK; }
extern "C" int32_t vox_q4_tensor_num_blocks(const vox_q4* q, int64_t* out) { ARGCHK(q && out, "null argument"); *out = (int64_t)q->w.N * q->w.nb; return VOX_OK; }
extern "C" int32_t vox_q4_tensor_free(vox_q4* q) {
    if (!q) return VOX_OK;
    (void)hipSetDevice(q->ctx->device); (void)hipStreamSynchronize(q->ctx->stream);
    (void)hipFree(q->qs_mem); (void)hipFree(q->sc_mem); (void)hipFree(q->qt_mem); (void)hipFree(q->st_mem); delete q; return VOX_OK;
}
extern "C" int32_t vox_q4_tensor_dequantize(vox_ctx* c, const vox_q4* q, float* out) {
    ARGCHK(c && q && out, "null argument"); VOXCHK(ctx_bind(c));
    const size_t ne = (size_t)q->w.N * q->w.K;
    DevBuf d; HIPCHK(d.alloc(ne * 4));
    HIPCHK(launch_q4_dequant(q->w, d.as<float>(), c->stream));
    HIPCHK(hipMemcpyAsync(out, d.p, ne * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
    return VOX_OK;
}

// out[rows][N] = x[rows][K] * W^T (+bias), device pointers.  rows <= 4 -> fused GEMV, else MFMA GEMM (op.rs:144-150)
namespace vox_host {
int32_t q4_linear_dev(vox_ctx* c, const Q4W& w, const float* bias, const float* x, int x_stride, int rows, float* out, int out_stride,
                             int epi, const float* resid, int resid_stride, int ksplit) {
    if (rows <= 4) {
        GemvParams p{}; p.w = w; p.x = x; p.x_stride = x_stride; p.out = out; p.out_stride = out_stride; p.bias = bias;
        p.resid = resid; p.resid_stride = resid_stride;
        HIPCHK(launch_q4_gemv(p, rows, PRO_NONE, epi, q4_gemv_default_R(w.N, w.K, epi), c->stream));
    } else {
        GemmParams p{}; p.w = w; p.x = x; p.x_stride = x_stride; p.M = rows; p.out = out; p.out_stride = out_stride; p.bias = bias;
        p.resid = resid; p.resid_stride = resid_stride; p.ksplit = ksplit;
        if (rows > 16 && rows <= 48 && w.fmt == WFMT_Q4_0 && w.K <= 16384) {      // the prefill GEMMs: rows -> XF tiles once (launch_q4_skinny_mt)
            c->want_scratch(true, true);
            p.xf_scratch = c->xf_scratch; p.xf_scratch_bytes = c->xf_scratch_bytes;
            p.kz_scratch = c->kz_scratch; p.kz_scratch_bytes = c->kz_scratch_bytes;
        }
        HIPCHK(launch_q4_gemm(p, epi, c->stream));
    }
    return VOX_OK;
}
}  // namespace vox_host

extern "C" int32_t vox_q4_linear_forward(vox_ctx* c, const vox_q4* w, const float* bias, const float* x, int32_t B, int32_t M, float* out, int32_t mem_kind) {
    ARGCHK(c && w && x && out, "null argument"); ARGCHK(B > 0 && M > 0, "bad batch/rows"); VOXCHK(ctx_bind(c));
    const int rows = B * M, K = w->w.K, N = w->w.N;
    if (mem_kind == VOX_MEM_DEVICE) return q4_linear_dev(c, w->w, bias, x, K, rows, out, N);
    DevBuf dx, dy, db; HIPCHK(dx.alloc((size_t)rows * K * 4)); HIPCHK(dy.alloc((size_t)rows * N * 4));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)rows * K * 4, hipMemcpyHostToDevice, c->stream));
    if (bias) { HIPCHK(db.alloc((size_t)N * 4)); HIPCHK(hipMemcpyAsync(db.p, bias, (size_t)N * 4, hipMemcpyHostToDevice, c->stream)); }
    VOXCHK(q4_linear_dev(c, w->w, bias ? db.as<float>() : nullptr, dx.as<float>(), K, rows, dy.as<float>(), N));
    HIPCHK(hipMemcpyAsync(out, dy.p, (size_t)rows * N * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
    return VOX_OK;
}
extern "C" int32_t vox_q4_matmul(vox_ctx* c, const vox_q4* w, const float* x, int32_t B, int32_t M, float* out, int32_t mem_kind) {
    return vox_q4_linear_forward(c, w, nullptr, x, B, M, out, mem_kind);
}

// ---- dense (f32-path) operators of models/layers on their own: what the f32 SafeTensors model runs, reachable per operator so that the reference's own
// per-component vectors (scripts/reference_forward.py; models/layers/swiglu.rs:101, conv.rs, rms_norm.rs tests) go through the HIP kernels, not only through the oracle
static uint16_t bf16_rne(float f) { uint32_t u; std::memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }
static void bf16_split(const float* w, size_t n, uint16_t* hi, uint16_t* lo) {
    for (size_t e = 0; e < n; e++) { const uint16_t hb = bf16_rne(w[e]); const uint32_t hu = (uint32_t)hb << 16; float hf; std::memcpy(&hf, &hu, 4); hi[e] = hb; lo[e] = bf16_rne(w[e] - hf); }
}
extern "C" int32_t vox_dense_tensor_from_f32(vox_ctx* c, const float* w, const float* w_other, int64_t N, int64_t K, vox_q4** out) {
    ARGCHK(c && w && out, "null argument"); ARGCHK(N > 0 && K > 0 && K % 32 == 0, "dense tensor [%lld][%lld]: K must be a positive multiple of 32", (long long)N, (long long)K);
    VOXCHK(ctx_bind(c));
    const int64_t Ntot = w_other ? 2 * N : N; const size_t ne = (size_t)Ntot * K;
    std::vector<float> host(ne);
    for (int64_t r = 0; r < N; r++) {
        std::memcpy(host.data() + (size_t)(w_other ? 2 * r : r) * K, w + (size_t)r * K, (size_t)K * 4);
        if (w_other) std::memcpy(host.data() + (size_t)(2 * r + 1) * K, w_other + (size_t)r * K, (size_t)K * 4);      // interleaved gate / up rows (the fused w1|w3 operand)
    }
    std::vector<uint16_t> h2(ne), l2(ne); bf16_split(host.data(), ne, h2.data(), l2.data());
    vox_q4* q = new vox_q4{c, Q4W{}, nullptr, nullptr};
    auto bail = [&](hipError_t e) { (void)hipGetLastError(); (void)hipFree(q->qs_mem); (void)hipFree(q->sc_mem); (void)hipFree(q->qt_mem); delete q; return fail(VOX_ERR_HIP, "dense tensor upload: %s", hipGetErrorString(e)); };
    hipError_t e = hipMalloc(&q->qs_mem, ne * 2); if (e == hipSuccess) e = hipMalloc(&q->sc_mem, ne * 2); if (e == hipSuccess) e = hipMalloc(&q->qt_mem, ne * 4);
    if (e == hipSuccess) e = hipMemcpy(q->qs_mem, h2.data(), ne * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(q->sc_mem, l2.data(), ne * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(q->qt_mem, host.data(), ne * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) return bail(e);
    q->w = Q4W{(const uint4*)q->qs_mem, (const uint16_t*)q->sc_mem, (int)Ntot, (int)K, (int)(K / 32), WFMT_F32}; q->w.qt = (const uint4*)q->qt_mem;      // the f32 model's WFMT_F32 operand (Loader::linear)
    *out = q; return VOX_OK;
}
extern "C" int32_t vox_linear_forward_ex(vox_ctx* c, const vox_q4* w, const float* bias, const float* x, int32_t B, int32_t M, float* out, int32_t epilogue, int32_t mem_kind) {
    ARGCHK(c && w && x && out, "null argument"); ARGCHK(B > 0 && M > 0, "bad batch/rows"); VOXCHK(ctx_bind(c));
    ARGCHK(epilogue == 0 || epilogue == 1 || epilogue == 2, "epilogue %d: 0 none, 1 GELU, 2 SwiGLU over interleaved gate / up rows", epilogue);
    const int epi = epilogue == 1 ? EPI_GELU : epilogue == 2 ? EPI_SWIGLU : EPI_STORE;
    const int rows = B * M, K = w->w.K, N = w->w.N, No = epilogue == 2 ? N / 2 : N;
    ARGCHK(epilogue != 2 || (N % 2 == 0 && !bias), "SwiGLU epilogue needs an even number of interleaved rows and no bias");
    if (mem_kind == VOX_MEM_DEVICE) return q4_linear_dev(c, w->w, bias, x, K, rows, out, No, epi);
    DevBuf dx, dy, db; HIPCHK(dx.alloc((size_t)rows * K * 4)); HIPCHK(dy.alloc((size_t)rows * No * 4));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)rows * K * 4, hipMemcpyHostToDevice, c->stream));
    if (bias) { HIPCHK(db.alloc((size_t)N * 4)); HIPCHK(hipMemcpyAsync(db.p, bias, (size_t)N * 4, hipMemcpyHostToDevice, c->stream)); }
    VOXCHK(q4_linear_dev(c, w->w, bias ? db.as<float>() : nullptr, dx.as<float>(), K, rows, dy.as<float>(), No, epi));
    HIPCHK(hipMemcpyAsync(out, dy.p, (size_t)rows * No * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream));
    return VOX_OK;
}
// ---- debug: ONE launch of the decode round's wo operator (tests): out = x W^T + resid as f32 rows, the XF planes of out * xf_w * scale and the per-tile sums of squares
// (launch_q4_gemm's EPI_RESID_XF on the XF tile of x).  order == null: the per-column form, every row multiplied by scale set d->set; order given: the per-row form
// (EPI_RESID_XF_ROWS), row m by scale set order[m].  Host pointers; xf_out holds 2 (N / 128) 256 8 16-bit values, ssq_out (N / 16) 16 floats; rows >= M stay 0.
extern "C" int32_t vox_debug_resid_xf(vox_ctx* c, const vox_q4* w, const vox_resid_xf_desc* d, const float* x, const float* resid, const float* xf_w, const float* scales,
                                      const int32_t* order, float* out, uint16_t* xf_out, float* ssq_out) {
    ARGCHK(c && w && d && x && resid && xf_w && scales && out && xf_out && ssq_out, "null argument");
    const int M = d->M, K = w->w.K, N = w->w.N, S = d->n_sets;
    ARGCHK(M >= 1 && M <= 16, "M %d out of range (1..16)", M); ARGCHK(S >= 1 && S <= 16, "n_sets %d out of range (1..16)", S);
    ARGCHK(w->w.fmt == WFMT_Q4_0 && w->w.qt && w->w.st && K % 128 == 0 && N % 128 == 0, "the XF step takes a tile-ordered Q4 weight with K and N multiples of 128 (K %d, N %d)", K, N);
    if (order) { for (int m = 0; m < M; m++) ARGCHK(order[m] >= 0 && order[m] < S, "order[%d] = %d names no scale set (0..%d)", m, order[m], S - 1); }
    else ARGCHK(d->set >= 0 && d->set < S, "set %d out of range (0..%d)", d->set, S - 1);
    VOXCHK(ctx_bind(c)); hipStream_t s = c->stream;
    const size_t xin_b = (size_t)2 * (K / 128) * 256 * 16, xout_b = (size_t)2 * (N / 128) * 256 * 16, ssq_b = (size_t)q4_skinny_resid_xf_parts(N) * 16 * 4;
    DevBuf dx, dxf, dres, dw1, dsc, dord, dout, dxo, dss;
    HIPCHK(dx.alloc((size_t)M * K * 4)); HIPCHK(dxf.alloc(xin_b)); HIPCHK(dres.alloc((size_t)M * N * 4)); HIPCHK(dw1.alloc((size_t)N * 4)); HIPCHK(dsc.alloc((size_t)S * N * 4));
    HIPCHK(dord.alloc(16 * 4)); HIPCHK(dout.alloc((size_t)M * N * 4)); HIPCHK(dxo.alloc(xout_b)); HIPCHK(dss.alloc(ssq_b));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)M * K * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dres.p, resid, (size_t)M * N * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dw1.p, xf_w, (size_t)N * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dsc.p, scales, (size_t)S * N * 4, hipMemcpyHostToDevice, s));
    if (order) HIPCHK(hipMemcpyAsync(dord.p, order, (size_t)M * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dxf.p, 0, xin_b, s)); HIPCHK(hipMemsetAsync(dxo.p, 0, xout_b, s)); HIPCHK(hipMemsetAsync(dss.p, 0, ssq_b, s));
    HIPCHK(launch_xf_rows(dx.as<float>(), K, M, K, dxf.as<uint16_t>(), s));
    GemmParams g{}; g.w = w->w; g.xf = (const uint4*)dxf.p; g.M = M; g.out = dout.as<float>(); g.out_stride = N; g.resid = dres.as<float>(); g.resid_stride = N;
    g.xf_out = dxo.as<uint16_t>(); g.xf_w = dw1.as<float>(); g.ssq_out = dss.as<float>();
    if (order) { g.xf_w2 = dsc.as<float>(); g.xf_w2_row = (const int*)dord.p; g.xf_w2_stride = N; } else g.xf_w2 = dsc.as<float>() + (size_t)d->set * N;
    HIPCHK(launch_q4_gemm(g, EPI_RESID_XF, s));
    HIPCHK(hipMemcpyAsync(out, dout.p, (size_t)M * N * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(xf_out, dxo.p, xout_b, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(ssq_out, dss.p, ssq_b, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
// ConvDownsampler::forward (models/layers/conv.rs:78-83): gelu(conv1d k3 s2 p1) twice, x [C][L] -> [O][L2], on the product's im2col MFMA path (conv_stem_dev)
extern "C" int32_t vox_conv_downsample(vox_ctx* c, const float* x, int32_t C, int32_t L, const float* w1, const float* b1, const float* w2, const float* b2, int32_t O, float* out) {
    ARGCHK(c && x && w1 && b1 && w2 && b2 && out && C > 0 && L > 0 && O > 0, "bad argument"); ARGCHK((3 * C) % 128 == 0 && (3 * O) % 128 == 0, "3 * channels must be a multiple of 128");
    VOXCHK(ctx_bind(c)); hipStream_t s = c->stream;
    const int T1 = (L + 2 - 3) / 2 + 1, S = (T1 + 2 - 3) / 2 + 1;      // models/layers/conv.rs:47-48
    auto planes = [&](const float* w, int Co, int Ci, DevBuf& hi, DevBuf& lo, Q4W* q) -> int32_t {      // W'[co][kk * Ci + ci] = w[co][ci][kk] as bf16 hi + lo (Loader::conv_planes)
        const size_t K = (size_t)3 * Ci; std::vector<float> r((size_t)Co * K);
        for (int co = 0; co < Co; co++) for (int ci = 0; ci < Ci; ci++) for (int kk = 0; kk < 3; kk++) r[(size_t)co * K + (size_t)kk * Ci + ci] = w[((size_t)co * Ci + ci) * 3 + kk];
        std::vector<uint16_t> h(r.size()), l(r.size()); bf16_split(r.data(), r.size(), h.data(), l.data());
        HIPCHK(hi.alloc(h.size() * 2)); HIPCHK(lo.alloc(l.size() * 2));
        HIPCHK(hipMemcpy(hi.p, h.data(), h.size() * 2, hipMemcpyHostToDevice)); HIPCHK(hipMemcpy(lo.p, l.data(), l.size() * 2, hipMemcpyHostToDevice));
        *q = Q4W{(const uint4*)hi.p, (const uint16_t*)lo.p, Co, (int)K, (int)(K / 32), WFMT_BF16X2}; return VOX_OK;
    };
    DevBuf h1, l1, h2, l2, dx, dm, d1, dy, dyt, db1, db2; Q4W g1{}, g2{};
    VOXCHK(planes(w1, O, C, h1, l1, &g1)); VOXCHK(planes(w2, O, O, h2, l2, &g2));
    HIPCHK(dx.alloc((size_t)C * L * 4)); HIPCHK(dm.alloc((size_t)(L + 2) * C * 4)); HIPCHK(d1.alloc((size_t)(T1 + 2) * O * 4)); HIPCHK(dy.alloc((size_t)S * O * 4)); HIPCHK(dyt.alloc((size_t)S * O * 4));
    HIPCHK(db1.alloc((size_t)O * 4)); HIPCHK(db2.alloc((size_t)O * 4));
    HIPCHK(hipMemcpyAsync(dx.p, x, (size_t)C * L * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(db1.p, b1, (size_t)O * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(db2.p, b2, (size_t)O * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(dm.p, 0, (size_t)(L + 2) * C * 4, s)); HIPCHK(hipMemsetAsync(d1.p, 0, (size_t)(T1 + 2) * O * 4, s));
    HIPCHK(launch_transpose(dx.as<float>(), C, L, dm.as<float>() + C, s));      // [C][L] -> token-major, one zero row either side
    { GemmParams g{}; g.w = g1; g.x = dm.as<float>(); g.x_stride = 2 * C; g.M = T1; g.out = d1.as<float>() + O; g.out_stride = O; g.bias = db1.as<float>(); HIPCHK(launch_dense2_gemm(g, EPI_GELU, s)); }
    { GemmParams g{}; g.w = g2; g.x = d1.as<float>(); g.x_stride = 2 * O; g.M = S; g.out = dy.as<float>(); g.out_stride = O; g.bias = db2.as<float>(); HIPCHK(launch_dense2_gemm(g, EPI_GELU, s)); }
    HIPCHK(launch_transpose(dy.as<float>(), S, O, dyt.as<float>(), s));      // token-major [S][O] -> the layer's [O][S]
    HIPCHK(hipMemcpyAsync(out, dyt.p, (size_t)S * O * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}

// causal (+ sliding-window) multi-head / grouped-query attention core on host or device buffers
// (gguf/model.rs:100-120,125-198; masking.rs:9-107).  q [M][n_heads*hd], k/v [kv_len][n_kv*hd] (token-major), query m at
// position offset+m sees keys j <= offset+m with offset+m-j <= window (window < 0: no window).  out [M][n_heads*hd].
extern "C" int32_t vox_attention(vox_ctx* c, const float* q, const float* k, const float* v, int32_t M, int32_t kv_len, int32_t n_heads,
                                 int32_t n_kv_heads, int32_t head_dim, int32_t offset, int32_t window, float* out, int32_t mem_kind) {
    ARGCHK(c && q && k && v && out, "null argument");
    ARGCHK(M > 0 && kv_len > 0 && n_heads > 0 && n_kv_heads > 0 && n_heads % n_kv_heads == 0, "bad attention shape");
    ARGCHK(head_dim == 64 || head_dim == 128, "head_dim must be 64 (encoder) or 128 (decoder)");
    ARGCHK(offset >= 0 && offset + M <= kv_len, "queries must lie inside the key range (offset + M <= kv_len)");
    VOXCHK(ctx_bind(c));
    const size_t qn = (size_t)M * n_heads * head_dim, kn = (size_t)kv_len * n_kv_heads * head_dim;
    DevBuf dq, dk, dv, dout;
    const float *pq = q, *pk = k, *pv = v; float* po = out;
    if (mem_kind != VOX_MEM_DEVICE) {
        HIPCHK(dq.alloc(qn * 4)); HIPCHK(dk.alloc(kn * 4)); HIPCHK(dv.alloc(kn * 4)); HIPCHK(dout.alloc(qn * 4));
        HIPCHK(hipMemcpyAsync(dq.p, q, qn * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dk.p, k, kn * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(dv.p, v, kn * 4, hipMemcpyHostToDevice, c->stream));
        pq = dq.as<float>(); pk = dk.as<float>(); pv = dv.as<float>(); po = dout.as<float>();
    }
    AttnParams ap{}; ap.q = pq; ap.q_stride = n_heads * head_dim; ap.k = pk; ap.v = pv; ap.kv_row_stride = n_kv_heads * head_dim; ap.kv_head_stride = head_dim;
    ap.out = po; ap.out_stride = n_heads * head_dim; ap.M = M; ap.kv_len = kv_len; ap.n_heads = n_heads; ap.n_kv_heads = n_kv_heads; ap.offset = offset; ap.window = window;
    HIPCHK(launch_attn_prefill(ap, head_dim, c->stream));
    if (mem_kind != VOX_MEM_DEVICE) { HIPCHK(hipMemcpyAsync(out, po, qn * 4, hipMemcpyDeviceToHost, c->stream)); HIPCHK(hipStreamSynchronize(c->stream)); }
    return VOX_OK;
}
