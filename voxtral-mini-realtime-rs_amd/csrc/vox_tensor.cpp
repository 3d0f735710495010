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
// ---- debug: ONE operator of the batched XF decode step (tests; include/voxtral_hip.h): the decode chain's launch for q|k|v, wo / w2, w1|w3 or the lm_head on caller data,
// through the chain's own parameter fill (xf_step_bind) -- launch_q4_gemm on one XF group, launch_q4_wide on 2..4; or (VOX_XF_MODE_ROWS) the encoder's EPI_ROPE_ROWS on f32 rows.
// Every argument is checked before a device is touched; the output buffers go up as the caller filled them and come back whole.
static_assert(sizeof(vox_xf_op_desc) == 112 && sizeof(vox_xf_op_bufs) == 17 * sizeof(void*), "vox_xf_op_desc / vox_xf_op_bufs: the layout tests/test_abi_cpu.py restates");
static int32_t xf_op_rows(vox_ctx* c, const vox_q4* w, vox_xf_op_desc* d, const vox_xf_op_bufs* b) {
    const int K = w->w.K, N = w->w.N, M = d->M, hd = d->hd;
    ARGCHK(b->x && b->out && b->rope_cos && b->rope_sin, "null argument");
    ARGCHK(M >= 1 && M <= 65536, "M %d out of range (1..65536)", M);
    ARGCHK((hd == 64 || hd == 128) && d->n_q >= hd && d->n_q <= N && d->n_q % hd == 0, "hd %d, n_q %d: hd is 64 or 128, n_q a multiple of it within N = %d", hd, d->n_q, N);
    ARGCHK(d->rope_rows >= 1 && d->rope_seq_rows >= 0, "rope_rows %d, rope_seq_rows %d", d->rope_rows, d->rope_seq_rows);
    if (b->pos) { for (int m = 0; m < M; m++) ARGCHK(b->pos[m] >= 0 && b->pos[m] < d->rope_rows, "pos[%d] = %d is outside the RoPE table (%d rows)", m, b->pos[m], d->rope_rows); }
    else ARGCHK((d->rope_seq_rows > 0 ? std::min(M, d->rope_seq_rows) : M) <= d->rope_rows, "the rows' positions run past the RoPE table (%d rows)", d->rope_rows);
    VOXCHK(ctx_bind(c)); hipStream_t s = c->stream;
    const size_t tab_b = (size_t)d->rope_rows * (hd / 2) * 4;
    DevBuf dx, dout, dcos, dsin, dpos;
    HIPCHK(dx.alloc((size_t)M * K * 4)); HIPCHK(dout.alloc((size_t)M * N * 4)); HIPCHK(dcos.alloc(tab_b)); HIPCHK(dsin.alloc(tab_b)); HIPCHK(dpos.alloc((size_t)M * 4));
    HIPCHK(hipMemcpyAsync(dx.p, b->x, (size_t)M * K * 4, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dout.p, b->out, (size_t)M * N * 4, hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(dcos.p, b->rope_cos, tab_b, hipMemcpyHostToDevice, s)); HIPCHK(hipMemcpyAsync(dsin.p, b->rope_sin, tab_b, hipMemcpyHostToDevice, s));
    if (b->pos) HIPCHK(hipMemcpyAsync(dpos.p, b->pos, (size_t)M * 4, hipMemcpyHostToDevice, s));
    GemmParams g{}; g.w = w->w; g.x = dx.as<float>(); g.x_stride = K; g.M = M; g.out = dout.as<float>(); g.out_stride = N; g.rope_cos = dcos.as<float>(); g.rope_sin = dsin.as<float>();
    g.hd = hd; g.n_q = d->n_q; g.pos = b->pos ? (const int*)dpos.p : nullptr; g.rope_seq_rows = d->rope_seq_rows;
    bool fused = false;
    HIPCHK(launch_q4_gemm(g, EPI_ROPE_ROWS, s, &fused));
    HIPCHK(hipMemcpyAsync(b->out, dout.p, (size_t)M * N * 4, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s));
    d->fused_rope = fused ? 1 : 0;
    return VOX_OK;
}
// VOX_XF_MODE_WIDE_ROWS: the decoder prefill's 17..48-row form -- rows -> XF tiles, q4_wide_kernel's row-major K-slice planes, the finishing kernel of `epi`
static int32_t xf_op_wide_rows(vox_ctx* c, const vox_q4* w, vox_xf_op_desc* d, const vox_xf_op_bufs* b) {
    const int K = w->w.K, N = w->w.N, M = d->M, hd = d->hd, mt = (M + 15) / 16, R = 16 * mt;
    ARGCHK(b->x, "null argument"); ARGCHK(M > 16 && M <= 48, "M %d out of range (17..48)", M);
    ARGCHK(d->n_part == 0 && !d->xf_in_gs && !d->xf_out_gs && !d->ssq_part_gs && !d->ssq_out_gs, "the row-major wide form takes no fused norm and no group strides");
    WidePlan pl; const int KZ = q4_skinny_mt2_plan(w->w, M);
    ARGCHK(N % 16 == 0 && q4_wide_plan(w->w, mt, EPI_ROPE_KV, &pl) && pl.kz == KZ, "the wide plan does not take this weight (N %d)", N);
    const int epi = d->epi;
    if (epi == VOX_XF_EPI_ROPE_KV) {
        ARGCHK(b->out && b->kc && b->vc && b->rope_cos && b->rope_sin && !b->bias, "null argument (or a bias)");
        ARGCHK((hd == 64 || hd == 128) && d->n_q >= hd && d->n_q % hd == 0 && d->n_kv >= 1 && (long)d->n_q + 2L * d->n_kv * hd == N, "hd %d, n_q %d, n_kv %d do not make N = %d", hd, d->n_q, d->n_kv, N);
        ARGCHK(d->kv_form == VOX_XF_KV_CONTIG && !d->kv_bf16 && d->kv_slices == 1 && d->kv_rows >= 1 && d->rope_rows >= 1 && (long)d->n_kv * d->kv_rows * hd < (1L << 28), "one f32 sequence: kv_form 0, kv_slices 1");
        ARGCHK(d->pos_off >= 0 && (long)d->pos_off + M <= d->kv_rows && (long)d->pos_off + M <= d->rope_rows, "pos_off %d + M %d runs past the cache (%d rows) or the RoPE table (%d rows)", d->pos_off, M, d->kv_rows, d->rope_rows);
    } else if (epi == VOX_XF_EPI_SWIGLU_XF) { ARGCHK(b->xf_out, "null argument"); ARGCHK(N % 256 == 0, "SWIGLU_XF takes N %% 256 == 0 (N %d)", N); }
    else if (epi == VOX_XF_EPI_RESID_XF) ARGCHK(b->out && !b->bias, "null argument (or a bias)");
    else return fail(VOX_ERR_INVALID, "epi %d: the row-major wide form finishes with 1 ROPE_KV, 2 SWIGLU_XF or 3 RESID_XF", epi);
    d->plan_ntw = pl.ntw; d->plan_ks = pl.kz; d->plan_steps = pl.sps;
    VOXCHK(ctx_bind(c)); hipStream_t s = c->stream;
    const size_t out_b = (size_t)R * N * 4, xin_b = (size_t)mt * K * 64, xo_b = (size_t)mt * (N / 2) * 64, planes_b = q4_wide_planes_bytes(w->w, mt, pl);      // (launch_q4_wide asks for room for 16 mt rows per slice; the kernel stores M)
    const size_t kv_b = epi == VOX_XF_EPI_ROPE_KV ? (size_t)d->n_kv * d->kv_rows * hd * 4 : 0, tab_b = epi == VOX_XF_EPI_ROPE_KV ? (size_t)d->rope_rows * (hd / 2) * 4 : 0;
    DevBuf dx, dxf, dpl, dout, dxo, dbias, dkc, dvc, dcos, dsin;
    auto up = [&](DevBuf& db, const void* src, size_t bytes) -> int32_t {
        if (!src || !bytes) return VOX_OK;
        HIPCHK(db.alloc(bytes)); HIPCHK(hipMemcpyAsync(db.p, src, bytes, hipMemcpyHostToDevice, s)); return VOX_OK;
    };
    VOXCHK(up(dx, b->x, (size_t)M * K * 4)); HIPCHK(dxf.alloc(xin_b)); HIPCHK(dpl.alloc(planes_b));
    if (epi != VOX_XF_EPI_SWIGLU_XF) VOXCHK(up(dout, b->out, out_b)); else { VOXCHK(up(dxo, b->xf_out, xo_b)); VOXCHK(up(dbias, b->bias, (size_t)N * 4)); }
    if (epi == VOX_XF_EPI_ROPE_KV) { VOXCHK(up(dkc, b->kc, kv_b)); VOXCHK(up(dvc, b->vc, kv_b)); VOXCHK(up(dcos, b->rope_cos, tab_b)); VOXCHK(up(dsin, b->rope_sin, tab_b)); }
    HIPCHK(launch_xf_rows(dx.as<float>(), K, M, K, dxf.as<uint16_t>(), s));
    GemmParams g{}; g.w = w->w; g.xf = (const uint4*)dxf.p; g.M = M; g.kz_scratch = dpl.as<float>(); g.kz_scratch_bytes = planes_b;      // (the prefill's gemm_xf)
    HIPCHK(launch_q4_skinny_mt2_planes(g, KZ, s));
    if (epi == VOX_XF_EPI_ROPE_KV)
        HIPCHK(launch_splitk_finish_rope_kv(dpl.as<float>(), KZ, M, N, dout.as<float>(), N, d->n_q, d->n_kv, hd, d->pos_off, dcos.as<float>(), dsin.as<float>(), dkc.as<float>(), dvc.as<float>(), d->kv_rows * hd, s));
    else if (epi == VOX_XF_EPI_SWIGLU_XF) HIPCHK(launch_splitk_finish_swiglu_xf(dpl.as<float>(), KZ, M, N, dbias.as<float>(), dxo.as<uint16_t>(), s));
    else HIPCHK(launch_splitk_finish_resid(dpl.as<float>(), KZ, M, N, dout.as<float>(), N, s));
    if (epi != VOX_XF_EPI_SWIGLU_XF) HIPCHK(hipMemcpyAsync(b->out, dout.p, out_b, hipMemcpyDeviceToHost, s)); else HIPCHK(hipMemcpyAsync(b->xf_out, dxo.p, xo_b, hipMemcpyDeviceToHost, s));
    if (epi == VOX_XF_EPI_ROPE_KV) { HIPCHK(hipMemcpyAsync(b->kc, dkc.p, kv_b, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(b->vc, dvc.p, kv_b, hipMemcpyDeviceToHost, s)); }
    HIPCHK(hipStreamSynchronize(s));
    return VOX_OK;
}
extern "C" int32_t vox_debug_xf_op(vox_ctx* c, const vox_q4* w, vox_xf_op_desc* d, const vox_xf_op_bufs* b) {
    ARGCHK(c && w && d && b, "null argument");
    ARGCHK(!d->reserved[0] && !d->reserved[1], "reserved words must be 0");
    const int K = w->w.K, N = w->w.N, G = d->groups, hd = d->hd, n_part = d->n_part;
    ARGCHK(w->w.fmt == WFMT_Q4_0 && w->w.qt && w->w.st && K % 128 == 0, "the XF step takes a tile-ordered Q4 weight with K a multiple of 128 (K %d)", K);
    d->plan_ntw = d->plan_ks = d->plan_steps = d->plan_straight = d->fused_rope = 0;
    if (d->mode == VOX_XF_MODE_ROWS) return xf_op_rows(c, w, d, b);
    if (d->mode == VOX_XF_MODE_WIDE_ROWS) return xf_op_wide_rows(c, w, d, b);
    ARGCHK(d->mode == VOX_XF_MODE_STEP, "mode %d: 0 the XF step, 1 the encoder's RoPE rows, 2 the prefill's row-major wide form", d->mode);
    ARGCHK(G >= 1 && G <= 4, "groups %d out of range (1..4)", G);
    ARGCHK(G == 1 ? (d->M >= 1 && d->M <= 16) : d->M == 16 * G, "M %d: 1..16 for one group, 16 * groups for the wide step", d->M);
    const int M = d->M, R = 16 * G, mtw = G == 1 ? 0 : G;
    ARGCHK(b->x, "null argument"); ARGCHK(n_part >= 0, "n_part %d is negative", n_part); ARGCHK(n_part == 0 || b->ssq_part, "n_part without ssq_part");
    ARGCHK(d->norm_eps >= 0.f && d->norm_eps == d->norm_eps, "norm_eps must be a non-negative number");
    int epi; size_t xout_cols = 0;
    switch (d->epi) {
    case VOX_XF_EPI_STORE: epi = EPI_STORE;
        ARGCHK(b->out, "null argument"); ARGCHK(!b->bias || G == 1, "a bias: the one-group STORE alone takes it"); ARGCHK(G == 1 || (N % 16 == 0 && n_part >= 1), "the wide STORE takes N %% 16 == 0 and the fused norm");
        break;
    case VOX_XF_EPI_ROPE_KV: epi = EPI_ROPE_KV;
        ARGCHK(b->out && b->kc && b->vc && b->pos && b->rope_cos && !b->bias, "null argument (or a bias)"); ARGCHK(n_part >= 1, "ROPE_KV runs with the fused norm (n_part >= 1)");
        ARGCHK((hd == 64 || hd == 128) && d->n_q >= hd && d->n_q % hd == 0 && d->n_kv >= 1 && (long)d->n_q + 2L * d->n_kv * hd == N, "hd %d, n_q %d, n_kv %d do not make N = %d", hd, d->n_q, d->n_kv, N);
        ARGCHK(d->kv_form >= VOX_XF_KV_CONTIG && d->kv_form <= VOX_XF_KV_PAGED_RING && (G == 1 || d->kv_form <= VOX_XF_KV_SLOTS), "kv_form %d (the wide step: contiguous or slots)", d->kv_form);
        ARGCHK(d->kv_bf16 == 0 || (d->kv_bf16 == 1 && d->kv_form >= VOX_XF_KV_PAGED), "kv_bf16 %d: a paged form's, 0 or 1", d->kv_bf16);
        ARGCHK(d->kv_slices >= 1 && d->kv_rows >= 1 && d->rope_rows >= 1 && (long)d->kv_slices * d->n_kv * d->kv_rows * hd < (1L << 28), "kv_slices %d, kv_rows %d, rope_rows %d", d->kv_slices, d->kv_rows, d->rope_rows);
        ARGCHK(d->kv_form == VOX_XF_KV_CONTIG || b->kv_row, "kv_row is null"); ARGCHK(d->kv_form < VOX_XF_KV_PAGED || b->kv_pos, "kv_pos is null");
        if (d->kv_form == VOX_XF_KV_PAGED_RING) {
            ARGCHK(b->rope_member && d->rope_mask >= 0 && !(d->rope_mask & (d->rope_mask + 1)) && d->rope_rows % (d->rope_mask + 1) == 0, "a RoPE ring: rope_member, rope_mask + 1 a power of two that divides rope_rows");
        } else ARGCHK(b->rope_sin, "rope_sin is null");
        for (int r = 0; r < M; r++) {
            const int ps = b->pos[r], slice = d->kv_form == VOX_XF_KV_CONTIG ? r : b->kv_row[r], row = d->kv_form >= VOX_XF_KV_PAGED ? b->kv_pos[r] : ps;
            ARGCHK(ps >= 0 && slice >= 0 && slice < d->kv_slices && row >= 0 && row < d->kv_rows, "row %d: position %d, slice %d of %d, cache row %d of %d", r, ps, slice, d->kv_slices, row, d->kv_rows);
            if (d->kv_form == VOX_XF_KV_PAGED_RING) ARGCHK(b->rope_member[r] >= 0 && b->rope_member[r] < d->rope_rows / (d->rope_mask + 1), "rope_member[%d] = %d names no ring member", r, b->rope_member[r]);
            else ARGCHK(ps < d->rope_rows, "pos[%d] = %d is outside the RoPE table (%d rows)", r, ps, d->rope_rows);
        }
        break;
    case VOX_XF_EPI_SWIGLU_XF: epi = EPI_SWIGLU_XF; xout_cols = (size_t)N / 2;
        ARGCHK(b->xf_out && !b->bias, "null argument (or a bias)"); ARGCHK(N % 256 == 0, "SWIGLU_XF takes N %% 256 == 0 (N %d)", N); ARGCHK(G == 1 || n_part >= 1, "the wide SWIGLU_XF runs with the fused norm");
        break;
    case VOX_XF_EPI_RESID_XF: epi = EPI_RESID_XF; xout_cols = (size_t)N;
        ARGCHK(b->out && b->resid && b->xf_w && b->xf_out && b->ssq_out && !b->bias, "null argument (or a bias)"); ARGCHK(N % 128 == 0, "RESID_XF takes N %% 128 == 0 (N %d)", N);
        ARGCHK(n_part == 0, "RESID_XF takes no fused norm");
        break;
    default: return fail(VOX_ERR_INVALID, "epi %d: 0 STORE, 1 ROPE_KV, 2 SWIGLU_XF, 3 RESID_XF", d->epi);
    }
    // group strides (0: packed), in the elements the kernels count them in
    const long xin_pk = (long)K * 32, xout_pk = (long)xout_cols * 32, sp_pk = (long)n_part * 16, so_pk = (long)q4_skinny_resid_xf_parts(N) * 16;
    const long xin_gs = d->xf_in_gs ? d->xf_in_gs : xin_pk, xout_gs = d->xf_out_gs ? d->xf_out_gs : xout_pk, sp_gs = d->ssq_part_gs ? d->ssq_part_gs : sp_pk, so_gs = d->ssq_out_gs ? d->ssq_out_gs : so_pk;
    ARGCHK(xin_gs >= xin_pk && xin_gs % 8 == 0 && xout_gs >= xout_pk && xout_gs % 8 == 0 && sp_gs >= sp_pk && so_gs >= so_pk, "a group stride is smaller than its block (or the planes' is no multiple of 8)");
    // the plan, before anything is allocated: the one-group launcher refuses more partial sums than its threads take (12 each)
    size_t planes_b = 0;
    if (mtw) {
        WidePlan pl; ARGCHK(q4_wide_plan(w->w, mtw, epi, &pl), "the wide step does not take this weight (N %d)", N);
        d->plan_ntw = pl.ntw; d->plan_ks = pl.kz; d->plan_steps = pl.sps; if (epi != EPI_STORE) planes_b = q4_wide_planes_bytes(w->w, mtw, pl);
    } else {
        const bool paged = epi == EPI_ROPE_KV && d->kv_form >= VOX_XF_KV_PAGED;
        SkinnyPlan pl; q4_skinny_plan(w->w, q4_skinny_epi(epi, paged, paged && d->kv_bf16, paged && d->kv_form == VOX_XF_KV_PAGED_RING, false), true, n_part > 0, &pl);
        ARGCHK(n_part <= 12 * (64 * pl.ks / 16), "n_part %d: a launch of %d waves takes at most %d", n_part, pl.ks, 12 * (64 * pl.ks / 16));
        d->plan_ntw = pl.ntw; d->plan_ks = pl.ks; d->plan_steps = pl.steps; d->plan_straight = pl.straight;
    }
    VOXCHK(ctx_bind(c)); hipStream_t s = c->stream;
    const size_t out_b = (size_t)R * N * 4, kv_b = epi == EPI_ROPE_KV ? (size_t)d->kv_slices * d->n_kv * d->kv_rows * hd * (d->kv_bf16 ? 2 : 4) : 0;
    const bool ring = epi == EPI_ROPE_KV && d->kv_form == VOX_XF_KV_PAGED_RING;
    const size_t tab_b = epi == EPI_ROPE_KV ? (size_t)d->rope_rows * (ring ? hd : hd / 2) * 4 : 0;
    DevBuf dx, dxf, dsp, dbias, dres, dw1, dw2, dout, dkc, dvc, dxo, dso, dcos, dsin, dpos, drow, dkp, dmem, dpl;
    auto up = [&](DevBuf& db, const void* src, size_t bytes) -> int32_t {
        if (!src || !bytes) return VOX_OK;
        HIPCHK(db.alloc(bytes)); HIPCHK(hipMemcpyAsync(db.p, src, bytes, hipMemcpyHostToDevice, s)); return VOX_OK;
    };
    VOXCHK(up(dx, b->x, (size_t)R * K * 4));
    HIPCHK(dxf.alloc((size_t)G * xin_gs * 2)); HIPCHK(hipMemsetAsync(dxf.p, 0xFF, (size_t)G * xin_gs * 2, s));      // (the gaps between the groups' planes: NaN)
    for (int gi = 0; gi < G; gi++) HIPCHK(launch_xf_rows(dx.as<float>() + (size_t)gi * 16 * K, K, 16, K, dxf.as<uint16_t>() + (size_t)gi * xin_gs, s));      // all 16 rows of a group: rows >= M hold data too
    if (n_part) {
        HIPCHK(dsp.alloc((size_t)G * sp_gs * 4)); HIPCHK(hipMemsetAsync(dsp.p, 0xFF, (size_t)G * sp_gs * 4, s));
        for (int gi = 0; gi < G; gi++) HIPCHK(hipMemcpyAsync(dsp.as<float>() + (size_t)gi * sp_gs, b->ssq_part + (size_t)gi * sp_pk, (size_t)sp_pk * 4, hipMemcpyHostToDevice, s));
    }
    VOXCHK(up(dbias, b->bias, (size_t)N * 4));
    if (epi != EPI_SWIGLU_XF) VOXCHK(up(dout, b->out, out_b));
    if (epi == EPI_RESID_XF) { VOXCHK(up(dres, b->resid, out_b)); VOXCHK(up(dw1, b->xf_w, (size_t)N * 4)); VOXCHK(up(dw2, b->xf_w2, (size_t)N * 4)); VOXCHK(up(dso, b->ssq_out, (size_t)G * so_gs * 4)); }
    if (xout_cols) VOXCHK(up(dxo, b->xf_out, (size_t)G * xout_gs * 2));
    if (epi == EPI_ROPE_KV) {
        VOXCHK(up(dkc, b->kc, kv_b)); VOXCHK(up(dvc, b->vc, kv_b)); VOXCHK(up(dcos, b->rope_cos, tab_b)); if (!ring) VOXCHK(up(dsin, b->rope_sin, tab_b));
        VOXCHK(up(dpos, b->pos, (size_t)M * 4)); if (d->kv_form != VOX_XF_KV_CONTIG) VOXCHK(up(drow, b->kv_row, (size_t)M * 4));
        if (d->kv_form >= VOX_XF_KV_PAGED) VOXCHK(up(dkp, b->kv_pos, (size_t)M * 4)); if (ring) VOXCHK(up(dmem, b->rope_member, (size_t)M * 4));
    }
    if (planes_b) HIPCHK(dpl.alloc(planes_b));
    // the operator's epilogue fields, through the decode chain's own fill helpers
    GemmParams g{}; const float* sp = n_part ? dsp.as<float>() : nullptr;
    if (epi == EPI_STORE) { xf_fill_store(g, dout.as<float>(), N, sp, n_part); g.bias = dbias.as<float>(); }
    if (epi == EPI_ROPE_KV) {
        xf_fill_rope_kv(g, dout.as<float>(), N, sp, n_part, (const int*)dpos.p, dcos.as<float>(), dsin.as<float>(), hd, d->n_q, d->n_kv, dkc.as<float>(), dvc.as<float>(),
                        (long)d->n_kv * d->kv_rows * hd, d->kv_rows, d->kv_form == VOX_XF_KV_SLOTS ? (const int*)drow.p : nullptr);
        if (d->kv_form >= VOX_XF_KV_PAGED) xf_fill_rope_kv_paged(g, (long)d->n_kv * d->kv_rows * hd, d->kv_rows, (const int*)drow.p, (const int*)dkp.p, d->kv_bf16);
        if (ring) xf_fill_rope_ring(g, dcos.as<float>(), (const int*)dmem.p, d->rope_mask);
    }
    if (epi == EPI_SWIGLU_XF) xf_fill_swiglu_xf(g, dxo.as<uint16_t>(), N / 2, sp, n_part);
    if (epi == EPI_RESID_XF) xf_fill_resid_xf(g, dout.as<float>(), dres.as<float>(), N, dxo.as<uint16_t>(), dw1.as<float>(), dw2.as<float>(), dso.as<float>());
    xf_step_bind(g, w->w, dxf.as<uint16_t>(), M, epi, d->norm_eps, mtw, dpl.as<float>(), planes_b, xin_gs, xout_gs, sp_gs, so_gs);
    HIPCHK(xf_step_launch(g, epi, s));
    if (epi != EPI_SWIGLU_XF) HIPCHK(hipMemcpyAsync(b->out, dout.p, out_b, hipMemcpyDeviceToHost, s));
    if (xout_cols) HIPCHK(hipMemcpyAsync(b->xf_out, dxo.p, (size_t)G * xout_gs * 2, hipMemcpyDeviceToHost, s));
    if (epi == EPI_RESID_XF) HIPCHK(hipMemcpyAsync(b->ssq_out, dso.p, (size_t)G * so_gs * 4, hipMemcpyDeviceToHost, s));
    if (epi == EPI_ROPE_KV) { HIPCHK(hipMemcpyAsync(b->kc, dkc.p, kv_b, hipMemcpyDeviceToHost, s)); HIPCHK(hipMemcpyAsync(b->vc, dvc.p, kv_b, hipMemcpyDeviceToHost, s)); }
    HIPCHK(hipStreamSynchronize(s));
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
