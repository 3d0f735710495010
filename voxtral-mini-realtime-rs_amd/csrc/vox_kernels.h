// vox_kernels.h -- host-side launch interface of the gfx950 kernels (vox_kernels.hip).
// Everything here is internal to libvoxtral_hip.so; the public boundary is include/voxtral_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <atomic>
// "done once per DEVICE" flag for per-kernel attributes (hipFuncSetAttribute applies to the current device: one vox_ctx per GPU in one process)
struct DevOnce {
    std::atomic<uint64_t> mask{0};
    bool done(int dev) const { return (mask.load(std::memory_order_acquire) >> (dev & 63)) & 1ull; }
    void set(int dev) { mask.fetch_or(1ull << (dev & 63), std::memory_order_release); }
};
static inline int vox_current_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; } return d; }
#include <stdint.h>

namespace vox {

// Q4_0 weight [N][K] re-packed at load (bit-lossless) from the 18-byte AoS GGUF blocks
// (gguf/tensor.rs:98-109) into two 16-byte-aligned planes so a wavefront streams coalesced
// global_load_dwordx4:  qs[n][b] = the block's 16 nibble bytes (element i <-> low nibble of
// byte i, element i+16 <-> high nibble), sc[n][b] = the block's f16 scale.
struct Q4W {
    const uint4* qs;     // fmt 0: nibble chunks [N][nb]; fmt 1: dense bf16 weights [N][K] viewed as uint4 (8 bf16 each)
    const uint16_t* sc;  // fmt 0: IEEE f16 scale bits [N][nb]; fmt 1: unused (nullptr)
    int N, K, nb;        // nb = K / 32
    int fmt;             // WFMT_Q4_0 or WFMT_BF16 (the f32 SafeTensors path: the checkpoint is BF16 on disk, exact in bf16)
    // optional second copy in MFMA tile order (q4_tile_build_kernel): [N/16 tiles][nb/4][64 lanes] uint4 + scales; used by the
    // skinny (M <= 16) and the large-M MFMA kernels, whose B fragments then are single coalesced dwordx4 loads
    const uint4* qt = nullptr; const uint16_t* st = nullptr;
};
enum WFmt { WFMT_Q4_0 = 0, WFMT_BF16 = 1, WFMT_BF16X2 = 2, WFMT_F32 = 3 };
// WFMT_F32: a dense F32 / F16 checkpoint tensor whose values are NOT bf16-representable (models/weights.rs:16-66 accepts any): qt = the exact f32
// plane [N][K] (decode GEMV, embedding lookup), qs / sc = bf16 hi / lo planes (w ~= hi + lo to 2^-17; the MFMA GEMMs for > 4 rows).   // BF16X2: f32 weights as two dense bf16 planes, qs = hi [N][K], sc = lo [N][K] (conv stem)

enum Epi { EPI_STORE = 0, EPI_RESID = 1, EPI_SWIGLU = 2, EPI_ROPE_KV = 3, EPI_ARGMAX = 4, EPI_GELU = 5, EPI_SWIGLU_XF = 6, EPI_RESID_XF = 7,
           EPI_ROPE_ROWS = 8,        // launch_q4_gemm only: store, with RoPE (interleaved pairs, rope.rs:77-141) on the first n_q columns, row m at position pos[m] (or m % rope_seq_rows, or m) -- the encoder's q|k|v operator
           EPI_ROPE_KV_PAGED = 9,    // inside launch_q4_skinny only: EPI_ROPE_KV with GemmParams::kv_pos set runs as this instantiation
           EPI_ROPE_KV_RING = 10,    // launch_q4_gemv only (Q4 weights): EPI_ROPE_KV on a cache used as a RING of cache_head_stride / hd rows per KV head -- k / v go to cache row
                                     // pos % that -- with the RoPE row read from a session's RoPE ring: row pos & rope_mask of [rope_mask + 1][cos hd/2 | sin hd/2] (rope_cos = the ring,
                                     // rope_sin = the ring + hd / 2: rows are hd floats apart, not hd / 2).  An epilogue instantiation of its own: EPI_ROPE_KV compiles as it did
           EPI_ROPE_KV_PAGED_BF16 = 12, EPI_ROPE_KV_PAGED_RING_BF16 = 13,      // inside launch_q4_skinny only: the two paged epilogues on a bf16 pool (GemmParams::kv_bf16) -- RoPE in f32 as
                                     // below, then K and V rounded by kv_bf16_round (vox_kv_bf16.h) and stored as 16-bit values; q is untouched.  Instantiations of their own
           EPI_RESID_XF_ROWS = 14,   // inside launch_q4_skinny only: EPI_RESID_XF with GemmParams::xf_w2_row set (a stream group with a delay per member) -- row m's second scale is read
                                     // from scale set xf_w2_row[m]: xw = xf_w[n] * xf_w2[xf_w2_row[m] * xf_w2_stride + n], the per-column form's product.  An instantiation of its own
           EPI_ROPE_KV_PAGED_RING = 11 };  // inside launch_q4_skinny only: EPI_ROPE_KV_PAGED with GemmParams::rope_member set (an endless paged group) -- the RoPE row is read from the
                                     // group's member-strided RoPE ring: row rope_member[m] * (rope_mask + 1) + (pos[m] & rope_mask) of [members][rope_mask + 1][cos hd/2 | sin hd/2]
                                     // (rope_cos = the ring, rope_sin = the ring + hd / 2).  An epilogue instantiation of its own: the other two compile as they did
// (M <= 16 only) _SWIGLU_XF: SwiGLU written as XF planes; _RESID_XF: out = acc + resid as f32 AND as XF planes of out * xf_w (* xf_w2) plus
// per-workgroup partial sums of squares -- the next RMSNorm is folded into its producer and its consumer (GemmParams::ssq_part)
enum Pro { PRO_NONE = 0, PRO_RMS = 1, PRO_RMS_MUL = 2,      // RMS_MUL: RMSNorm then * mul (the cached Ada scale)
           PRO_RMS_MUL_SUM = 3 };   // RMS_MUL on x + xacc * 2^-32 (the fixed-point wo product accumulated by attn_wo_kernel); the sum is also written to x_out

// ---- fused Q4 GEMV (decode, rows of x <= 4): out[y][n] = epi( sum_k pro(x[y])[k] * W[n][k] )
struct GemvParams {
    Q4W w;
    const float* x; int x_stride;        // gridDim.y input rows
    float* out; int out_stride;          // may be null for EPI_ARGMAX / EPI_ROPE_KV (q goes to out)
    const float* bias;                   // [N] or null
    const float* resid; int resid_stride;// EPI_RESID: out = resid + acc (+ bias)
    const float* gamma; const float* mul; float eps;   // PRO_RMS: x <- (x / rms(x)) * gamma (* mul)
    long long* zero_acc; int zero_n;     // any launch: workgroup b clears its share of zero_acc[0, zero_n) (the layer's attn_wo accumulators, already consumed by w1|w3)
    const long long* xacc; float* x_out;   // PRO_RMS_MUL_SUM: int64 fixed-point (2^-32) accumulators xacc[k]; x_out[k] = x[k] + xacc[k] * 2^-32 (one workgroup per piece writes it)
    const int* pos_ptr; int pos_off;     // position = (pos_ptr ? *pos_ptr : 0) + pos_off
    const float* rope_cos; const float* rope_sin; int hd;   // tables [max_pos][hd/2]
    int n_q, n_k;                        // EPI_ROPE_KV: rows [0,n_q) q, [n_q,n_q+n_k) k, then v
    float* kcache; float* vcache; int cache_head_stride;    // [kv_head][max_seq][hd]
    float* part_val; int* part_idx;      // EPI_ARGMAX: per-workgroup (max, argmax)
    int tl_slot;                         // timeline slot (measurement builds, -DVOX_TIMELINE; assigned by the launcher, -1 = off)
    int rope_mask;                       // EPI_ROPE_KV_RING: rows of the RoPE ring - 1 (a power of two - 1)
};
// rows_per_wave R in {1,2,4,8}; K tiles of 2048 chosen from K. Returns hipError_t.
hipError_t launch_q4_gemv(const GemvParams& p, int n_rows_x, int pro, int epi, int R, hipStream_t s);
const char* q4_gemv_kernel_name(int K, int pro, int epi, int R);
int q4_gemv_default_R(int N, int K, int epi);
int q4_gemv_grid(int N, int R);
int q4_gemv_nwv(int K, int epi);        // waves per workgroup the launcher will use for this shape (4 / 6 / 12)
int q4_gemv_grid_k(int N, int K, int R, int epi);
int dense_gemv_grid(int N);        // same, for WFMT_BF16 weights   // workgroups launched for N rows at R rows per wave (== number of argmax partials)

// ---- Q4 GEMM on MFMA (prefill / encoder, rows of x > 4): out[M][N'] = epi( x[M][K] * W^T )
struct GemmParams {
    Q4W w;
    const float* x; int x_stride; int M;
    float* out; int out_stride;
    const float* bias;
    const float* resid; int resid_stride;
    const uint4* xf;      // optional (M <= 16): the input as XF fragment planes (see xf_store4) instead of f32 rows x
    uint16_t* xf_scratch; size_t xf_scratch_bytes;   // 17..48 rows (the 38-token prefill): room for ceil(M/16) XF tiles of K columns (64 B per column and tile);
                          // the launcher converts the f32 rows ONCE (xf_rows_kernel) instead of every wave of every workgroup splitting them again
    // fused RMSNorm, consumer side: the XF input holds x * gamma UNnormalised; row m's accumulators are scaled by
    // rstd[m] = 1/sqrt(sum_i ssq_part[i][m] / K + norm_eps) (a per-row scalar commutes with the GEMM); n_part partials of 16 rows
    const float* ssq_part; int n_part; float norm_eps;
    // EPI_RESID_XF, producer side
    uint16_t* xf_out; const float* xf_w; const float* xf_w2; float* ssq_out;
    // EPI_ROPE_KV (M <= 16, one row per sequence): columns [0, n_q) -> RoPE -> out; [n_q, n_q + n_kv*hd) -> RoPE -> K cache; rest -> V cache,
    // all at position pos[m] of sequence m's cache slice
    const int* pos; const float* rope_cos; const float* rope_sin; int hd, n_q, n_kv; float* kc; float* vc; union { long kv_seq_stride; long xf_w2_stride; }; int kv_head_stride;
    // EPI_RESID_XF, optional (the <= 16-row XF form alone, an epilogue instantiation of its own): xf_w2 holds scale SETS xf_w2_stride floats apart and row m multiplies
    // by set xf_w2_row[m] (a stream group's row -> member map: every member's Ada scales); null: xf_w2 is one [N] vector for all rows.  The two words share the storage
    // of kv_row and kv_seq_stride, which only EPI_ROPE_KV reads: the argument block keeps its size and layout, and every other instantiation the code it had
    union { const int* xf_w2_row; const int* kv_row; };    // kv_row: EPI_ROPE_KV, optional: row m writes into cache slice kv_row[m] instead of slice m (continuous batching: a SLOT of the step decodes whichever utterance it currently holds)
    const int* kv_pos;    // EPI_ROPE_KV, optional (the <= 16-row XF form alone, an epilogue instantiation of its own): row m's row INSIDE its slice; null: pos[m], the address of every contiguous cache.  A paged cache
                          // (a paged stream group) passes kv_row[m] = the physical page, kv_seq_stride = the floats of a page, kv_head_stride = page_rows * hd, kv_pos[m] = pos[m] % page_rows
    const int* rope_member; int rope_mask;      // EPI_ROPE_KV with kv_pos, optional (EPI_ROPE_KV_PAGED_RING): row m's member of a member-strided RoPE ring of rope_mask + 1 rows (a power of two) per member
    int tl_slot;          // timeline slot (measurement builds, -DVOX_TIMELINE)
    // split-K (q4_gemm_kernel only, EPI_STORE): blockIdx.z = K slice; slice z writes its partial product to out + z * M * out_stride (bias in slice 0).
    // The consumer (launch_rms_norm_sumk) adds the slices in a fixed order -- for few-column GEMMs (the encoder's N = 1280 w2: 40 K-steps per workgroup)
    int ksplit;
    float* kz_scratch; size_t kz_scratch_bytes;      // 17..48 rows: room for the K-slice planes of q4_skinny_mt2_kernel ([ksplit][M][N] f32); null: the one-dimensional kernel
    // wide decode step (launch_q4_wide): M = 16 * wide_mt rows = wide_mt slot groups of 16; rows of consecutive groups are consecutive in out / resid / pos / kv_row,
    // the XF planes and the partial sums of squares of group g start g * (the group stride) after group 0's
    int rope_seq_rows;    // EPI_ROPE_ROWS without a position table: stacked sequences of this many rows restart at position 0 (0: row m sits at position m)
    int wide_mt; long xf_gstride /* uint4 */, xf_out_gstride /* uint16 */, ssq_part_gstride, ssq_out_gstride /* floats */;
    int wide_rows;        // > 0: q4_wide_kernel stores its K-slice planes ROW-MAJOR, [slice][wide_rows][N] f32 (rows < wide_rows only): the layout the 38-token prefill's finishing kernels read
    int kv_bf16;          // EPI_ROPE_KV with kv_pos (a bf16 paged group): kc / vc point at uint16_t pools, every K / V stride counts 16-bit elements, the values are rounded by kv_bf16_round
};
// ---- wide decode step (round 6): 32 / 48 / 64 rows (2..4 slot groups of a continuous batch) through ONE weight fetch and ONE nibble -> bf16 conversion per K step.
// GEMM (q4_wide_kernel: the groups' XF planes staged through LDS once per workgroup, K split over workgroups into planes) + a finishing launch that sums the planes in a
// fixed order and applies the batched step's epilogues (EPI_ROPE_KV / EPI_RESID_XF / EPI_SWIGLU_XF); EPI_STORE with one K slice (the lm_head) stores directly.
struct WidePlan { int kz, sps, ntw; };      // K slices, K steps (128 columns) per slice, n-tiles per wave
bool q4_wide_plan(const Q4W& w, int mt, int epi, WidePlan* pl);
size_t q4_wide_planes_bytes(const Q4W& w, int mt, const WidePlan& pl);
hipError_t launch_q4_wide(const GemmParams& p, int epi, hipStream_t s);      // p.xf (+ xf_gstride), p.wide_mt, p.kz_scratch (planes); epilogue fields as launch_q4_gemm's XF step
hipError_t launch_q4_tile_build(Q4W w, uint4* qt, uint16_t* st, hipStream_t s);
hipError_t launch_q4_gemm(const GemmParams& p, int epi, hipStream_t s, bool* fused_rope = nullptr);      // EPI_ROPE_ROWS: *fused_rope (if given) = the RoPE ran in the GEMM's epilogue
// dense f32-class GEMM on two bf16 weight planes (w.fmt == WFMT_BF16X2; the conv stem as an im2col GEMM); epi: EPI_STORE / EPI_GELU
hipError_t launch_dense2_gemm(const GemmParams& p, int epi, hipStream_t s);
hipError_t launch_transpose(const float* in, int R, int C, float* out, hipStream_t s);   // [R][C] -> [C][R]
int q4_skinny_resid_xf_parts(int N);   // number of [16]-row partial sums of squares an EPI_RESID_XF launch writes to ssq_out
// the plan of one <= 16-row launch (q4_skinny_kernel): n-tiles per wave, split-K waves, tile-ordered weights, K steps per wave (the last waves may own fewer),
// `even`: the steps of EVERY wave when K / 128 divides by ks (else 0), `straight`: a straight-line instantiation runs (XF input only), else the loop
struct SkinnyPlan { int ntw, ks, tiled, steps, even, straight; };
int q4_skinny_epi(int epi, bool kv_pos, bool kv_bf16, bool rope_member, bool xf_w2_row);      // the epilogue instantiation of a <= 16-row launch: EPI_ROPE_KV's paged / ring / bf16 forms, EPI_RESID_XF's per-row form
void q4_skinny_plan(const Q4W& w, int epi_inst, bool xf, bool pro, SkinnyPlan* pl);      // epi_inst: q4_skinny_epi's; xf: XF input; pro: the fused norm
// The epilogue fields of the batched XF decode step's operators: the decode chain and the tests' operator hook fill them through these alone.
//  q|k|v: f32 rows out (columns < n_q), the folded norm's partial sums, positions, the RoPE table, the cache (slice stride, head stride; kv_row: slots or null)
inline void xf_fill_rope_kv(GemmParams& g, float* out, int out_stride, const float* ssq_part, int n_part, const int* pos, const float* cos_t, const float* sin_t,
                            int hd, int n_q, int n_kv, float* kc, float* vc, long kv_seq_stride, int kv_rows, const int* kv_row) {
    g.out = out; g.out_stride = out_stride; g.ssq_part = ssq_part; g.n_part = n_part; g.pos = pos; g.rope_cos = cos_t; g.rope_sin = sin_t;
    g.hd = hd; g.n_q = n_q; g.n_kv = n_kv; g.kc = kc; g.vc = vc; g.kv_seq_stride = kv_seq_stride; g.kv_head_stride = kv_rows * hd; g.kv_row = kv_row;
}
//  ... on a paged cache: the page's elements, rows per page = 1 << page_shift, the rows' physical pages and rows inside them; kv_bf16: 16-bit pools
inline void xf_fill_rope_kv_paged(GemmParams& g, long page_elems, int page_rows, const int* kv_page, const int* kv_in, int kv_bf16) {
    g.kv_seq_stride = page_elems; g.kv_head_stride = g.hd * page_rows; g.kv_row = kv_page; g.kv_pos = kv_in; g.kv_bf16 = kv_bf16;
}
//  ... with the RoPE rows in a member-strided ring [members][rope_mask + 1][cos | sin]
inline void xf_fill_rope_ring(GemmParams& g, const float* ring, const int* member, int rope_mask) {
    g.rope_cos = ring; g.rope_sin = ring + g.hd / 2; g.rope_member = member; g.rope_mask = rope_mask;
}
//  wo / w2: out = x W^T + resid as f32 rows, the XF planes of out * xf_w * xf_w2 (xf_w2 may be null), the per-tile sums of squares
inline void xf_fill_resid_xf(GemmParams& g, float* out, const float* resid, int stride, uint16_t* xf_out, const float* xf_w, const float* xf_w2, float* ssq_out) {
    g.out = out; g.out_stride = stride; g.resid = resid; g.resid_stride = stride; g.xf_out = xf_out; g.xf_w = xf_w; g.xf_w2 = xf_w2; g.ssq_out = ssq_out;
}
//  w1|w3: the XF planes of F = N / 2 columns (passed as `out`)
inline void xf_fill_swiglu_xf(GemmParams& g, uint16_t* xf_out, int F, const float* ssq_part, int n_part) { g.out = (float*)xf_out; g.out_stride = F; g.ssq_part = ssq_part; g.n_part = n_part; }
//  the lm_head
inline void xf_fill_store(GemmParams& g, float* out, int out_stride, const float* ssq_part, int n_part) { g.out = out; g.out_stride = out_stride; g.ssq_part = ssq_part; g.n_part = n_part; }
// One operator of the batched XF decode step (the decode chain and the tests' operator hook): the fields that do not depend on the epilogue.  g holds the operator's
// epilogue fields; xin: the input XF planes of K columns, M rows.  mtw == 0: one <= 16-row group through launch_q4_gemm.  mtw = 2..4: the wide step's slot groups
// through launch_q4_wide -- planes: its K-split scratch; the groups' input planes xf_in_gs, output planes xf_out_gs (16-bit elements), partial sums ssq_part_gs and
// output sums ssq_out_gs (floats) apart.
inline void xf_step_bind(GemmParams& g, const Q4W& w, const uint16_t* xin, int M, int epi, float norm_eps, int mtw, float* planes, size_t planes_bytes,
                         long xf_in_gs, long xf_out_gs, long ssq_part_gs, long ssq_out_gs) {
    g.w = w; g.xf = (const uint4*)xin; g.M = M; if (mtw || epi != EPI_RESID_XF) g.norm_eps = norm_eps;
    if (!mtw) return;
    g.wide_mt = mtw; g.xf_gstride = xf_in_gs / 8; g.kz_scratch = planes; g.kz_scratch_bytes = planes_bytes;
    if (g.ssq_part) g.ssq_part_gstride = ssq_part_gs;
    if (epi == EPI_RESID_XF) { g.xf_out_gstride = xf_out_gs; g.ssq_out_gstride = ssq_out_gs; } else if (epi == EPI_SWIGLU_XF) g.xf_out_gstride = xf_out_gs;
}
inline hipError_t xf_step_launch(const GemmParams& g, int epi, hipStream_t s) { return g.wide_mt ? launch_q4_wide(g, epi, s) : launch_q4_gemm(g, epi, s); }

// ---- small fused ops
hipError_t launch_q4_repack(const uint8_t* raw, uint4* qs, uint16_t* sc, int64_t n_blocks, int nb, int row_mul, int row_add, hipStream_t s);
hipError_t launch_q4_dequant(Q4W w, float* out, hipStream_t s);                 // diagnostics (tensor.rs:88-113)
hipError_t launch_rms_norm(const float* x, int x_stride, int rows, int dim, const float* gamma, const float* mul,
                           float eps, float* out, int out_stride, hipStream_t s);
// x[row] += sum of ksplit partial planes (fixed order; plane stride = part_stride floats), written back, then RMSNorm -> out (dim <= 4096, dim % 4 == 0)
hipError_t launch_rms_norm_sumk(float* x, int x_stride, int rows, int dim, const float* part, size_t part_stride, int ksplit, const float* gamma, float eps, float* out, int out_stride, hipStream_t s);
// pieces of the two-dimensional 17..48-row GEMM (q4_skinny_mt2_kernel) for callers that fold the finishing sum of the K-slice planes into their next kernel
int q4_skinny_mt2_plan(const Q4W& w, int M);                                                                  // K slices, 0 = not applicable
hipError_t launch_xf_rows(const float* x, int x_stride, int M, int K, uint16_t* xf, hipStream_t s);        // f32 rows -> XF tiles
hipError_t launch_q4_skinny_mt2_planes(const GemmParams& p, int KZ, hipStream_t s);                         // p.xf in, planes [KZ][M][N] -> p.kz_scratch
hipError_t launch_splitk_finish_resid(const float* planes, int KZ, int M, int N, float* x, int x_stride, hipStream_t s);
hipError_t launch_splitk_finish_swiglu_xf(const float* planes, int KZ, int M, int N, const float* bias, uint16_t* xf, hipStream_t s);      // planes -> SwiGLU -> XF tiles (K' = N / 2)
hipError_t launch_splitk_finish_rope_kv(const float* planes, int KZ, int M, int N, float* q_out, int q_stride, int n_q, int n_kv, int hd, int pos_off,
                                        const float* cos_t, const float* sin_t, float* kc, float* vc, int head_stride, hipStream_t s);           // planes -> RoPE -> q rows + KV cache
hipError_t launch_rms_norm_xf_sumk(float* x, int x_stride, int rows, int dim, const float* planes, int kz, const float* gamma, const float* mul, float eps, uint16_t* xf, hipStream_t s);
hipError_t launch_rms_norm_xf(const float* x, int x_stride, int rows, int dim, const float* gamma, const float* mul,
                              float eps, uint16_t* xf, hipStream_t s);   // rows <= 16 -> XF fragment planes
// interleaved-pair RoPE in place on columns [0, n_rot) of buf[M][stride]; row m has position pos_off + m
// (seq_rows > 0: stacked sequences of seq_rows rows each, positions restart per sequence)
// (row_pos != nullptr: ragged sequences packed back to back, row m has position pos_off + row_pos[m])
hipError_t launch_rope(float* buf, int M, int stride, int n_rot, int hd, int pos_off, const float* cos_t,
                       const float* sin_t, hipStream_t s, int seq_rows = 0, const int* row_pos = nullptr);
// copy k (columns [k_col, k_col+n_kv*hd)) and v (next n_kv*hd columns) of buf rows into the cache at pos_off+m
hipError_t launch_kv_store(const float* buf, int M, int stride, int k_col, int n_kv, int hd, int pos_off,
                           float* kcache, float* vcache, int cache_head_stride, hipStream_t s, int seq_rows = 0, long kv_seq_stride = 0);

struct AttnParams {
    const float* q; int q_stride;            // q[m][h*hd + d]
    const float* k; const float* v;          // k[kvh*kv_head_stride + j*kv_row_stride + d]
    int kv_row_stride, kv_head_stride;
    float* out; int out_stride;              // out[m][h*hd + d]
    int M, kv_len, n_heads, n_kv_heads, offset, window;   // query m at position offset+m; window<0: none
    const int* pos_ptr;                      // decode: position = *pos_ptr + offset, kv_len = position+1
    // batched decode (gridDim.y = sequences): sequence s reads pos_ptr[s] and its own q / out rows and KV-cache slice
    int pos_per_seq; int q_seq_stride, out_seq_stride; long kv_seq_stride;
    const int* kv_row;    // batched decode, optional: sequence s reads cache slice kv_row[s] instead of slice s (attn_decode_kernel and attn_decode_gqa_kernel alike; the paged forms: table row kv_row[s])
    // stacked prefill (gridDim.z = sequences): sequence z has seq_len[z] query rows (kv_len = offset + seq_len[z]); p.M = the maximum;
    // q / out / k / v of sequence z start q_seq_stride / out_seq_stride / kv_seq_stride floats after those of z-1
    const int* seq_len;
    const int* seq_row_off;   // stacked prefill, optional (MFMA kernel only): sequence z starts seq_row_off[z] ROWS into q / k / v / out (ragged sequences packed back to back) instead of z * the sequence strides
    uint16_t* out_xf_tiles; long out_xf_tile_stride;      // attn_prefill_small_kernel, optional: the output rows as XF tiles (tile = row / 16; stride in uint16 units) instead of `out`
    uint16_t* out_xf;     // batched decode: write the output rows (row = sequence) as XF fragment planes instead of out
    long out_xf_gstride;  // ... more than 16 sequences in one launch (attn_decode_gqa_kernel): sequence s is row s % 16 of the planes out_xf + (s / 16) * out_xf_gstride (uint16 units)
    int prefer_gqa;       // batched decode: one workgroup per (KV head, sequence) serving its 4 query heads (wide batches)
    int no_xcd_remap;     // measurement knob: keep the linear (head, sequence) workgroup order in attn_decode_kernel
    int tl_slot;          // timeline slot (measurement builds, -DVOX_TIMELINE)
    int spec_zero;        // always 0 (see attn_decode_kernel: keeps the position load a vector load)
    int spec_rows;        // decode (head-major cache, kv_row_stride == hd): rows per KV head in the cache; > 0 lets the kernel request the first
                          // 160 rows before the position word has arrived (attn_decode_core SPEC).  0: indices derived from the position.
    // prefill, one sequence, MFMA kernel only (attn_prefill_prefix_ok): a second K / V segment in FRONT of k / v.  Key index j < prefix_len is row j of prefix_k / prefix_v
    // ([kvh * prefix_head_stride + j * prefix_row_stride + d]); j >= prefix_len is row j - prefix_len of k / v.  offset = prefix_len, kv_len = prefix_len + M.
    const float* prefix_k; const float* prefix_v; int prefix_len, prefix_row_stride, prefix_head_stride;
    // paged decode (launch_attn_decode_paged): k / v = the layer's page pool [page][kv head][page_rows][hd] (kv_head_stride = page_rows * hd, kv_row_stride = hd,
    // page_floats per page); page_tab[kv_row[s] * page_tab_stride + q] = the physical page of logical page q (rows q << page_shift ..) of sequence s, read only for the
    // pages of the window; score_rows: LDS score rows per query head, >= the most keys a query attends (min(max positions, window + 1))
    const int* page_tab; int page_tab_stride, page_shift, score_rows; long page_floats;
    // 0: the table row is flat, entry q = logical page q.  L > 0 (an endless paged group): the row is a RING of L entries, logical page q at entry q % L -- a sequence
    // holds at most L pages at a time, so the window's pages never collide; L <= page_tab_stride, any L >= 1 (no power of two)
    int page_tab_len;
    // paged decode on a bf16 pool (a bf16 paged group, VOX_KV_BF16): k / v point at uint16_t pools of the same layout, every K / V stride above counts 16-bit elements;
    // the kernels widen the rows in registers (kv_bf16_widen) and run the f32 forms' arithmetic in their order
    int kv_bf16;
};
hipError_t launch_attn_prefill(const AttnParams& p, int hd, hipStream_t s, int n_seq = 1);     // M > 1, causal (+window)
bool attn_prefill_prefix_ok(const AttnParams& p, int hd, int n_seq);     // may launch_attn_prefill take p's two K / V segments (prefix_len > 0)?
bool attn_prefill_small_ok(const AttnParams& p, int hd, int n_seq);      // will launch_attn_prefill take the short-sequence kernel (<= 48 rows from position 0, f32; may write XF tiles: p.out_xf_tiles)?
hipError_t launch_attn_decode(const AttnParams& p, int hd, int max_seq, hipStream_t s, int n_seq = 1);  // M == 1 per sequence; hipErrorInvalidValue, nothing launched: the GQA form with max_seq above attn_decode_gqa_max_seq
// does launch_attn_decode take the GQA form for this geometry when AttnParams::prefer_gqa is set (one workgroup per KV head and sequence, 4 query heads each)?
bool attn_decode_takes_gqa(int hd, int n_heads, int n_kv_heads);
// the most cache rows per KV head (max_seq) that form can serve: the dynamic LDS a workgroup of the current device may ask for (160 KB less the kernel's static LDS,
// as launch_attn_decode raises the limit) / 16 bytes of scores per row.  The per-head form and the paged forms (score_rows <= window + 1) are not bound by it.
hipError_t attn_decode_gqa_max_seq(int* out);
// the same attention with K / V read through a page table: the GQA form where n_heads == 4 n_kv_heads and hd == 128, else the per-head form; a row has launch_attn_decode's bits
hipError_t launch_attn_decode_paged(const AttnParams& p, int hd, hipStream_t s, int n_seq);
// the same attention on a cache used as a RING of `cap` rows per KV head ([kv head][cap][hd]; kv_head_stride = cap * hd, kv_row_stride = hd): row j of a sequence lives
// at ring row j % cap, positions are not bound by cap; window >= 0 and window + 1 <= cap (hipErrorInvalidValue otherwise, nothing launched).  The per-head kernel with
// the ring row policy: a row has launch_attn_decode's bits
hipError_t launch_attn_decode_ring(const AttnParams& p, int hd, int cap, hipStream_t s, int n_seq = 1);
// single sequence: attention + the wo linear in one launch; acc[wo.N] (int64, zero on entry) receives the product in 2^-32 fixed point (consumer: PRO_RMS_MUL_SUM)
bool attn_wo_supported(const AttnParams& p, const Q4W& wo, int hd, int max_seq);
hipError_t launch_attn_wo(const AttnParams& p, const Q4W& wo, long long* acc, int max_seq, hipStream_t s);
// host-side launch counts of the attention kernels and of the single-stream decode engine, by form (vox_debug_attn_launches: tests assert which path a call took);
// behind them, in slots of their own, the two resampling ingest kernels of the live sessions (a group's pass-wide one, a solo stream's)
enum AttnForm { ATTN_FORM_PREFILL_SMALL, ATTN_FORM_PREFILL_MFMA, ATTN_FORM_PREFILL_F32, ATTN_FORM_DECODE, ATTN_FORM_DECODE_SPEC, ATTN_FORM_DECODE_GQA, ATTN_FORM_WO,
                ATTN_FORM_ENGINE, ATTN_FORM_STREAM_RING, ATTN_FORM_GROUP_RESAMPLE, ATTN_FORM_STREAM_RESAMPLE,
                ATTN_FORM_DECODE_PAGED, ATTN_FORM_DECODE_GQA_PAGED,      // the paged decode forms (launch_attn_decode_paged), behind every earlier slot
                ATTN_FORM_DECODE_RING,                                   // the ring decode form (launch_attn_decode_ring)
                ATTN_FORM_DECODE_PAGED_RING, ATTN_FORM_DECODE_GQA_PAGED_RING,      // the paged decode forms on a ring table (AttnParams::page_tab_len > 0)
                ATTN_FORM_DECODE_PAGED_BF16, ATTN_FORM_DECODE_GQA_PAGED_BF16,      // the paged decode forms on a bf16 pool (AttnParams::kv_bf16): counted here and in no slot above
                ATTN_FORM_DECODE_PAGED_RING_BF16, ATTN_FORM_DECODE_GQA_PAGED_RING_BF16,      // ... on a ring table
                ATTN_FORM_COUNT };
void attn_form_note(AttnForm f);
void attn_form_counts(unsigned long long out[ATTN_FORM_COUNT]);
// host-side launch counts of the linear kernels, by form (vox_debug_gemm_launches: tests assert which kernel a shape ran; counters only, nothing is dispatched by them).
// TILE_mn = q4_gemm_kernel<MT m, NT n>, _TB its tile-ordered form; XF_ROWS / SPLITK_FINISH are the helper launches of the 17..48-row forms
enum GemmForm { GEMM_FORM_GEMV_R1, GEMM_FORM_GEMV_R2, GEMM_FORM_GEMV_R4, GEMM_FORM_DENSE_GEMV, GEMM_FORM_SKINNY, GEMM_FORM_SKINNY_MT, GEMM_FORM_SKINNY_MT2, GEMM_FORM_XF_ROWS,
                GEMM_FORM_SPLITK_FINISH, GEMM_FORM_TILE_11, GEMM_FORM_TILE_12, GEMM_FORM_TILE_21, GEMM_FORM_TILE_22, GEMM_FORM_TILE_21_TB, GEMM_FORM_TILE_22_TB, GEMM_FORM_K32,
                GEMM_FORM_BIG, GEMM_FORM_BIG_ROPE, GEMM_FORM_DENSE2, GEMM_FORM_WIDE, GEMM_FORM_COUNT };
void gemm_form_counts(unsigned long long out[GEMM_FORM_COUNT]);

// gelu(conv1d k3 s2 p1): in [Cin][L] -> out; out_token_major: out[t][co] else out[co][t]
hipError_t launch_conv1d_gelu(const float* in, int Cin, int L, const float* w, const float* b, int Cout, float* out,
                              int out_token_major, hipStream_t s);

// log-mel: frames of the (virtually) padded signal zeros(left)+scale*audio+zeros(right); out layout
// [T][128] (transposed=0) or [128][T] (transposed=1). scale_ptr may be null (scale 1).
struct MelTables { const float* window; const float* cos_t; const float* sin_t; const float* fb; const int* fb_lo; const int* fb_hi; };
hipError_t launch_mel(const float* audio, long n, long left, long right, const float* scale_ptr, MelTables t,
                      float* out, int T, int transposed, hipStream_t s);
// sample-rate conversion (rubato `Fft` algorithm as one block matrix, vox_kernels.hip): the matrix builder (once per rate pair) and the block product + overlap-add
hipError_t launch_resample_matrix(const double* H, int new_len, int fft_in, int fft_out, float* At, hipStream_t s);      // H: new_len (re, im) pairs; At: [fft_in][2 fft_out]
hipError_t launch_resample(const float* x, long n_in, const float* At, int fft_in, int fft_out, int delay, float* out, long n_out, hipStream_t s);
hipError_t launch_absmax(const float* x, long n, float target_peak, float* scale_out, hipStream_t s);
// group peaks: every unit folds max|x| into its group's cell (zeroed by the caller); unit_scale[i] = target / peak of unit i's group (1 for a silent group or group < 0)
hipError_t launch_absmax_group(const float* x, long n, unsigned* group_max_cell, hipStream_t s);
hipError_t launch_group_scale(const unsigned* group_max, const int* unit_group, int n, float target, float* unit_scale, hipStream_t s);

// h[i][:] = (audio ? audio[(a_base+i)][:] : 0) + dequant(tok[ids[id_base+i]]) ; bases add *pos_ptr if given
hipError_t launch_embed(Q4W tok, const int* ids, int n, const float* audio, int D, const int* pos_ptr, int id_off,
                        int a_off, float* out, hipStream_t s);
// ---- greedy argmax, the rule of every decode form: the largest logit wins, the lowest index wins among equal values (+0.0 == -0.0), and a NaN never wins.  Value
// descending, index ascending is a strict total order over the non-NaN candidates, so every reduction tree yields the same (value, index) pair.  When nothing wins (a row
// of NaN and -inf only) the index is the sentinel 0x7fffffff: the kernels that embed the token read row 0 for it and store it as it is, launch_argmax_rows stores 0.  The launches below
// and the EPI_ARGMAX epilogues share one device implementation (argmax_take and block_argmax, vox_kernels.hip); the persistent engines keep their in-launch copies of the
// same rule (comm_next_input and the per-CU partial, vox_engine.hip and vox_engine_b16.hip).
// final argmax over per-workgroup partials; writes tokens[*pos_ptr+tok_off], then *pos_ptr += inc
hipError_t launch_argmax_final(const float* part_val, const int* part_idx, int n_parts, int* tokens, int* pos_ptr,
                               int tok_off, int inc, hipStream_t s);
// fused decode-step tail: tokens[*pos+1] = argmax(partials); *pos += 1; h = audio[*pos] + dequant(tok[tokens[*pos]])
hipError_t launch_argmax_embed(const float* part_val, const int* part_idx, int n_parts, int* tokens, int* pos_ptr, Q4W tok,
                               const float* audio, int D, float* h, hipStream_t s);
// batched decode step helpers (n sequences, per-sequence positions pos[s], caches [seq][kv_head][max_seq][hd] per layer)
hipError_t launch_rope_kv_batch(float* qkv, int n, int stride, int n_q, int n_kv, int hd, const int* pos, const float* cos_t, const float* sin_t,
                                float* kcache, float* vcache, long seq_stride, int head_stride, hipStream_t s);
hipError_t launch_argmax_embed_batch(const float* logits, int n, int vocab, int* tokens, int tok_stride, int* pos, const int* seq_len, Q4W tok,
                                     const float* audio, long audio_seq_stride, int D, float* h, hipStream_t s,
                                     uint16_t* xf = nullptr, const float* xf_w = nullptr, float* ssq_out = nullptr,     // xf: also h * xf_w as XF planes + sum of squares,
                                     long xf_group_stride = 0, int ssq_group_stride = 0,                                  // per group of 16 sequences (strides in elements)
                                     const long* audio_off = nullptr);      // optional: sequence s reads its audio rows at audio + audio_off[s] (floats) instead of audio + s * audio_seq_stride
// continuous batching: the argmax / next-input launch of a decode step over SLOTS (argmax_embed_slots_kernel)
struct SlotStepParams {
    const float* logits; int vocab;                    // [n_slots][vocab] (unused when init)
    int* tokens; int tok_stride; const int* clip_len;  // per utterance: token rows [n_clips][tok_stride], sequence lengths
    int* slot_clip; int* slot_qpos; const int* queue; int q_stride;      // per slot: current utterance (-1: none), index into its queue, queue [n_slots][q_stride] (-1 terminated)
    int* pos; int* kv_row; int n_clips; int first_pos; // per slot: position of the last token written, cache slice (n_clips = the scratch slice of idle slots); first_pos = prefix length
    Q4W tok; const float* audio; const long* audio_off; int D;           // audio rows of utterance c start at audio + audio_off[c] (floats), row stride D
    const float* h0;                                   // [n_clips][D]: first decode input of every utterance
    float* h;                                          // [n_slots][D]: the step's input rows
    uint16_t* xf; const float* xf_w; float* ssq_out; long xf_group_stride; int ssq_group_stride;      // as launch_argmax_embed_batch
    int init;                                          // 1: no argmax, every slot takes the head of its queue
};
hipError_t launch_argmax_embed_slots(const SlotStepParams& p, int n_slots, hipStream_t s);
// debug (vox_debug_batch_tap_*): copy the logits rows the next argmax launch of a batched decode takes its tokens from.  Row r belongs to utterance slot_clip[r]
// (slot_clip null: clip0 + r; < 0: an idle slot, nothing written) and yields that utterance's token at position pos[r] + 1 -- when seq_len is given, only if
// pos[r] + 1 < seq_len[r], as argmax_embed_batch_kernel -- which is id k = pos[r] + 1 - first_pos of its output.  Utterances with clip_unit[c] = j >= 0 are tapped:
// the row goes to out[j][k] (k < max_rows; a later row is dropped) and rows[j] = max(rows[j], k + 1), so rows[j] > max_rows tells how many were dropped.
struct BatchTapParams {
    const float* logits; int vocab;                    // [n_rows][vocab]
    const int* slot_clip; int clip0; const int* pos; const int* seq_len;      // per row (seq_len may be null)
    const int* clip_unit; int n_clips;                 // per utterance of the driver call: tap index or -1
    float* out; int* rows; int n_units, max_rows, first_pos;      // out [n_units][max_rows][vocab]
};
hipError_t launch_batch_tap(const BatchTapParams& p, int n_rows, hipStream_t s);
hipError_t launch_occupy(int workgroups, int micros, hipStream_t s);      // test hook: spin `workgroups` x 1024 threads for `micros` us
hipError_t launch_add_rows(const float* a, const float* b, float* out, long n, hipStream_t s);
hipError_t launch_gelu(float* x, long n, hipStream_t s);
hipError_t launch_argmax_rows(const float* x, int rows, int V, int* out, hipStream_t s);      // out[r] = argmax of row r (0 when nothing wins)

// ---- persistent decode-step engine (vox_engine.hip): the whole single-stream decode step -- 26 layers + final norm + tied lm_head + argmax
// partials -- as ONE launch of 256 workgroups (one per CU) x 8 waves: wave 0 streams this CU's slice of every Q4 operator, in consumption order,
// from a per-CU contiguous copy of the weights into an LDS ring with LDS-DMA (global_load_lds ... nt) and runs ahead of every dependency edge;
// wave 1 moves activations between CUs as 8-byte {value, tag} write-through granules; waves 2..7 consume the ring (VALU dot products, x in registers).
// Replaces gguf/model.rs:938-960 (one decode step) for the real Voxtral decoder geometry; everything else keeps the per-operator launches.
struct EngLayerTab { const float* attn_norm; const float* ffn_norm; const float* ada_mul; float* kc; float* vc; };   // per decoder layer; kc / vc: [n_kv][max_seq][hd]
struct EngParams {
    const unsigned char* stream; size_t cu_stride;   // per-CU weight stream (eng_stream_bytes / 256 bytes each)
    const EngLayerTab* layers; int n_layers;          // device array
    const float* h_in;                                // [D] the step's input embedding
    const float* final_norm;                          // [D]
    const int* pos_ptr; int pos_off;                  // position = *pos_ptr + pos_off
    const float* rope_cos; const float* rope_sin;     // [max_pos][hd/2]
    int max_seq, window; float eps;
    unsigned long long *H0, *H1, *G, *PW, *A, *P2;    // granule buffers: [3072] [3072] [6144] [32][3072] [9216] [24][3072]
    unsigned long long *SS0, *SS1;                    // [256] per-CU partial sums of squares of H0 / H1's raw rows
    unsigned long long* XC;                           // [256] XCC id of every workgroup (start-up exchange)
    unsigned* serial; unsigned* err;                  // launch serial (tags never repeat), first failure code (0 = ok)
    float* part_val; int* part_idx;                   // [256] per-CU argmax partials
    // flags 65536 (the product's graph-replayed steps): the launch BEGINS with the argmax over the previous launch's 256 partials (read back from part_val / part_idx),
    // writes tokens[*pos_rw + 1], runs at that position on its own input rows audio[position] + embed(token) (h_in is not read) and leaves *pos_rw = its position
    int* tokens; int* pos_rw; const uint4* tok_qs; const uint16_t* tok_sc; int tok_nb; const float* audio;
    float* logits_out;                                // optional [vocab]
    int vocab;
    unsigned long long* tl; int tl_layer;             // timeline stamps [256][32] of layer tl_layer (null: off)
    int flags;                                        // product default 641 = 1 | 128 | 512.  1: one LDS-DMA packet in flight while the CU polls memory; 128: XCD-local
                                                      // edges as plain stores through the shared L2 (placement verified per launch); 512: all-gathers swept ag_delay_ticks
                                                      // after the CU's own publish instead of probe-then-sweep.  Measurement / diagnostic: 2 loader re-reads one packet,
                                                      // 4 probe before small sweeps, 32 no LDS-DMA (wrong results), 64 loader pauses while polling, 1024 / 2048 loader depth
                                                      // 2 / 1, 4096 nt polls on XCD-local edges, 16384 FAULT INJECTION (workgroup 7 loses a publish: the timeout test); 65536: see tokens / pos_rw above
    int ag_delay_ticks;                               // flags 512: 10-ns ticks between the CU's own publish and the all-gather sweep
    int pace_ticks;                                   // loader: minimum 10-ns ticks between two packet issues inside the layers (0: none)
};
bool eng_geometry_ok(int D, int n_heads, int n_kv, int hd, int ffn, int vocab, int max_seq);
size_t eng_stream_bytes(int n_layers, int vocab);     // total bytes of the engine weight copy (all 256 CU streams)
size_t eng_state_bytes();                             // granule buffers + serial + err
// op: 0 q|k|v (fused [6144][3072]), 1 wo, 2 w1|w3 (row-interleaved), 3 w2, 4 tied lm_head; layer ignored for op 4; 5: wo for the batched engine into ITS stream (EngBParams::stream_wo)
hipError_t launch_eng_pack(const Q4W& w, int op, int layer, int n_layers, unsigned char* stream, int vocab, hipStream_t s);
void eng_state_carve(unsigned char* state, EngParams* p);      // point p's granule buffers / serial / err into a zero-initialised state block
hipError_t launch_decode_engine(const EngParams& p, hipStream_t s);
// after a launch without flags 65536 has ended: the final norm's OUTPUT of that step (what forward_hidden_with_cache returns, gguf/model.rs:676) from the launch's own last
// all-gather (H0 = h * final_norm * 512 granules, SS0 = 256 partial sums of squares) -> out[3072]
hipError_t launch_eng_hidden(const EngParams& p, float* out, hipStream_t s);
hipError_t eng_occupancy(int* blocks_per_cu);      // resident workgroups per CU the runtime grants decode_engine_kernel
int eng_lds_bytes();

// ---- persistent decode-layer engine for a group of <= 16 sequences (vox_engine_b16.hip): the 26 decoder layers of one batched decode step as ONE launch of 256 workgroups
// (one per CU) x 14 waves on the single-stream engine's packet stream.  Replaces the 26 x 5 launches of the batched step (gguf/model.rs:938-960 for B > 1); the step's tail
// (16-row lm_head GEMM, argmax / next embedding) stays launch-based and reads xf_out / ssq_out.
struct EngBParams {
    const unsigned char* stream;                      // the packet stream built by launch_eng_pack (layer part)
    const unsigned char* stream_wo;                   // wo in the XCD-group K split (launch_eng_pack op 5 per layer; engb_wo_stream_bytes): [layer][packet 2][CU][13824]
    const EngLayerTab* layers; int n_layers;          // device array; kc / vc: the GROUP's first sequence, [sequence][n_kv][max_seq][hd]
    long kv_seq_stride;                               // floats between two sequences' cache slices
    const float* h_in; int h_stride; int n_rows;      // [n_rows][D] the step's input rows (sequences n_rows..15 of the tile are zeros)
    const float* final_norm;                          // [D]
    const int* pos;                                   // [n_rows] position of every sequence
    const int* kv_row;                                // null: sequence m's cache slice is slice m of kc / vc; else slice kv_row[m] (device-resident: the wide batch's slots change utterances between launches)
    const float* rope_cos; const float* rope_sin;     // [max_pos][hd/2]
    int max_seq, window; float eps;
    unsigned char *XH0, *XH1;                         // all-gathered streams as MFMA A fragments: [96 blocks][hi, lo][64 lanes] x 16 B
    float *SS0, *SS1;                                 // [256 CUs][16] partial sums of squares
    unsigned long long* G;                            // [16][6144] q|k|v granules {value, tag}
    unsigned char* XO;                                // [32 heads][4 blocks][hi, lo][64] x 16 B attention outputs
    float* PW;                                        // [8 planes][3072][16] wo partial products (one plane per XCD group)
    unsigned char* XA;                                // [8 groups][36 blocks][hi, lo][64] x 16 B SwiGLU outputs
    float* P2;                                        // [8 planes][3072][16] w2 partial products
    unsigned *F0, *F1, *FO, *FW, *FA, *F2;            // flag words: F0 / F1 [256 CUs], 16 bytes apart (same-line write-through stores serialise); FO [32 heads][16 sequences], FA [256 CUs] (XCD-local); FW / F2: unused
                                                      // since the partial planes carry their own validity (empty = all ones)
    unsigned long long* XC; unsigned* serial; unsigned* err;
    uint16_t* xf_out; float* ssq_out;                 // the layer stack's output: XF planes of h * final_norm (xf_store4 layout) + [256][16] partial sums of squares
    unsigned long long* tl; int tl_layer;             // timeline stamps [256][32] of layer tl_layer (null: off)
    int flags;                                        // product default 2241 = 1 | 64 | 128 | 2048.  1: one LDS-DMA packet in flight while the CU's COMM wave polls; 64: none issued meanwhile (bounded 3 us); 128: plain stores on XCD-local
                                                      // edges (placement verified per launch); 1024 / 2048: loader depth 2 / 1; 32: no LDS-DMA (diagnostic, wrong results); 16384: fault injection
};
size_t engb_state_bytes();
size_t engb_wo_stream_bytes(int n_layers);            // bytes of the batched engine's wo stream (all 256 CUs)
void engb_state_carve(unsigned char* state, EngBParams* p);      // point p's edge buffers / flags / serial / err into a state block prepared by engb_state_init
hipError_t engb_state_init(unsigned char* state, hipStream_t s);      // zeros + the partial planes marked empty: before the first launch and after a failed one
hipError_t launch_decode_engine_b16(const EngBParams& p, hipStream_t s);
// TWO groups (2 x <= 16 sequences) through ONE launch, phase by phase: group B computes while group A's hand-off resolves.  Same weights / layer table / RoPE tables / flags,
// kv_row set in both, one state block (engb_state_bytes) per group; a timeout is reported in group A's err word.
hipError_t launch_decode_engine_b16x2(const EngBParams& a, const EngBParams& b, hipStream_t s);
hipError_t engb_occupancy(int* blocks_per_cu);
hipError_t engb_prepare_kernels();                    // the dynamic-LDS limits of the three launch forms (once; never inside a stream capture)
hipError_t launch_engb_ssq_fold(const float* ssq256, float* ssq16, hipStream_t s);      // [256][16] -> [16][16] partial sums of squares (fixed order)
int engb_lds_bytes();
int engb_lds_bytes2();                                // ... of the two-group launch

// ---- knobs: VOX_* environment snapshot (taken at vox_ctx_create / vox_debug_reload_knobs); launch paths never call getenv
void knobs_load_once();      // vox_ctx_create: build the snapshot if it does not exist yet (thread-safe)
void knobs_reload();         // vox_debug_reload_knobs (tests): replace the snapshot
// MI355X behaviour found in round 6 (tools/repro/pk_fp32_corun.cpp, profiles/r06_pk_fp32_corun.txt): a packed-FP32 VALU instruction (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32)
// whose op_sel takes the HIGH dword of SRC1 for the LOW lane returns a wrong low lane while ANOTHER wave on the CU executes MFMAs (another stream's GEMM: two contexts on
// one GPU, forked launch chains); so does v_pk_mov_b32 op_sel:[1,0] (low <- src0.high, high <- src1.low).  Straight lanes, src0 / src2 swaps and low-dword broadcasts are
// fine.  hipcc forms these encodings on its own (SLP-vectorised pair arithmetic: rope_kernel's rotation, dense_gemv_kernel's horizontal add, rms_norm_sumk_kernel's sum of
// squares, a swapped 8-byte LDS store in the batched engine), so: kernels where they appeared are compiled without packed FP32 (this attribute) or re-worded, and
// tests/test_abi_cpu.py::test_no_packed_fp32_src1_swap scans every shipped code object for them (tools/kernel_resources.py).  (Only rope_kernel's instance was ever seen to
// fail in the product -- two sessions on one GPU; the others are removed because the stand-alone reproducer fails on their encoding.)
#define VOX_NO_PK_F32 __attribute__((target("no-packed-fp32-ops")))
const char* knob_str(const char* name);      // nullptr when unset

// ---- timeline instrumentation (measurement builds only, -DVOX_TIMELINE): every q4_gemv / attn_decode launch gets the next slot and its
// waves stamp s_memrealtime (100 MHz) at 4 points into buf[slot][wave][4]; under graph replay the captured slot is rewritten per replay.
// Returns hipErrorNotSupported in product builds.
hipError_t tl_configure(unsigned long long* buf, int n_slots, int n_waves);   // buf == nullptr: off
int tl_slots_used();
void tl_slot_meta(int slot, int out[4]);    // {0 gemv / 1 attention, epi, N, K} of the launch that took `slot`

// ---- live streaming session (vox_stream, vox_stream_group): a session advances in TICKS of one decoder position (16 mel frames -> 4 encoder rows ->
// 1 adapter row -> 1 decode step).  The integers a tick depends on live in one device block per session, advanced by the tick's last kernel, so a tick's launch arguments
// never change.  A ROUND runs one tick of n sessions at once (n = 1: a solo vox_stream): slot z of the round serves session order[z], whose pointers the kernels read from
// a device array of StreamMember descriptors.
enum StreamWord { STRM_POS = 0,         // decoder position of the next tick (= its adapter row, its decoder cache row; the step yields tokens[position + 1])
                  STRM_ENC_POS = 1,     // encoder stream position of the tick's first row (RoPE position, ring row before the modulo)
                  STRM_FRAME = 2,       // first NEW mel frame of the tick (the halo starts halo_back frames before it)
                  STRM_HEAD = 3,        // STRM_ENC_POS modulo the ring capacity
                  STRM_TICKS = 4,       // ticks run since create / reset
                  STRM_TAP_ROWS = 5,    // group members: logits rows offered to the member's tap since it was armed
                  STRM_WORDS = 16 };    // block size in ints (a group of N sessions holds N such blocks back to back)
struct TokenScore { float logprob, margin; int runner_up, id; };      // vox_token_score (voxtral_hip.h)
static const int VOX_ALTS_MAX = 8;                                     // VOX_MAX_ALTERNATIVES
struct TokenAlt { int id; float logprob; };
struct TokenAlts { float entropy; int n; TokenAlt alt[VOX_ALTS_MAX]; };      // vox_token_alts (voxtral_hip.h)
struct TickLevel { float peak, mean_square; };                         // vox_tick_level (voxtral_hip.h)
struct StreamMember {
    const float* samples; float gain;   // the session's 16 kHz sample ring; every sample is multiplied by gain before the mel
    int* state;                         // its StreamWord block
    float *kring, *vring;               // its encoder K / V ring, [enc_layers][n_heads][cap][hd]
    int* tokens;                        // its token row
    float* tap; int tap_max;            // group members: [tap_max][vocab] logits rows (null: not armed)
    struct TokenScore* scores; int scores_cap;      // the session's score records, one per id of the utterance (null: scores off, launch_stream_score skips the slot)
    struct TokenAlts* alts; int alts_cap, alts_k;   // its alternatives records, one per id, and its k (null: alternatives off, launch_stream_alts skips the slot)
    struct TickLevel* levels; int levels_cap;       // its level records, one per id (null: levels off, launch_stream_level skips the slot)
};
// front end: for every slot z < n the log-mel frames STRM_FRAME - halo_back .. + n_frames - 1 of the virtually padded signal zeros(left) + gain * samples of session
// order[z], token-major into out + z * slot_stride ([n_frames][128]: the layout the conv stem's im2col GEMM reads).  Sample i of a session lives at ring[i & ring_mask];
// every sample a frame reads has been written (the host runs a tick only then), the reflections of mel_kernel never apply (left >= 200, and the right end of a finished
// session is its zero pad).
hipError_t launch_stream_mel(const StreamMember* mem, const int* order, int n, int ring_mask, long left, MelTables t, int halo_back, int n_frames, float* out, long slot_stride,
                             hipStream_t s);
// ingest at the capture rate: the 16 kHz samples [i0, i0 + count) of the stream from its input-rate ring, through the device function resample_apply_kernel computes a sample
// with (vox_kernels.hip resample_sample; At, fft_in, fft_out, delay: launch_resample's) -- bit for bit vox_resample's samples for the concatenated input.  Input sample k lives at in_ring[k & in_mask], output sample i goes to
// out_ring[i & out_mask]; n_in: the input samples that exist (written so far, or the utterance's length at its end): blocks are clipped there.  The caller launches it only
// for samples whose blocks are complete or clipped, and while block (i0 + delay) / fft_out - 1 is still in the input ring.  count <= out_mask + 1.
hipError_t launch_stream_resample(const float* in_ring, int in_mask, long n_in, const float* At, int fft_in, int fft_out, int delay, float* out_ring, int out_mask, long i0, int count,
                                  hipStream_t s);
// 16-bit PCM into a stream's f32 ring: ring[(w0 + k) & mask] = float(src[k]) / 32768 for k < count <= mask + 1 (src: device memory)
hipError_t launch_stream_s16(const short* src, int count, float* ring, int mask, long w0, hipStream_t s);
// ---- the ingest of a stream group's pass: both kernels above with a slot dimension, ONE launch for every fed member.  Slot z reads desc[z] (device array; `host`: the
// same n <= 16 descriptors on the host, which the launch validates with the checks of the solo launches: power-of-two masks, counts within the ring, no null pointer);
// slots may have count 0, a launch whose counts are all 0 is skipped.
struct StreamIngest {                     // launch_stream_resample's arguments for one member; the 16 kHz ring mask is the launch's
    const float* in_ring; int in_mask;    // the member's input-rate ring
    long n_in;                            // input samples that exist (blocks are clipped there)
    const float* At; int fft_in, fft_out, delay;      // its rate's block matrix and plan
    float* out_ring;                      // its 16 kHz ring
    long i0; int count;                   // 16 kHz samples [i0, i0 + count)
};
hipError_t launch_stream_group_resample(const StreamIngest* desc, const StreamIngest* host, int n, int out_mask, hipStream_t s);
struct StreamS16 { const short* src; int count; float* ring; int mask; long w0; };      // launch_stream_s16's arguments for one member
hipError_t launch_stream_group_s16(const StreamS16* desc, const StreamS16* host, int n, hipStream_t s);
// one encoder layer's attention for the round's n x M rows (M <= 8 per session, slot z's rows at z * M) against each session's own K / V ring: RoPE on q and k at the
// session's absolute stream position, k / v appended at position % cap, query m attends the keys j <= position_m, position_m - j <= window in ascending order of j (the
// ring changes addresses, not the order).  cap > window + M.
struct StreamAttnParams {
    const float* qkv; int qkv_stride;        // [n M][q | k | v], each n_heads * hd wide, not rotated
    const StreamMember* mem; const int* order; int n;
    size_t ring_off; int cap;                // this layer's ring inside a session's kring / vring (floats), [n_heads][cap][hd]
    const float* cos_t; const float* sin_t;  // [positions][hd / 2]
    float* out; int out_stride;              // [n M][n_heads * hd]
    int M, n_heads, window;
    int rope_mask;                           // 0 (the default): cos_t / sin_t are tables, row = the position.  > 0 (an endless session past its wrap): cos_t is a RoPE ring of
                                             // rope_mask + 1 rows [cos hd/2 | sin hd/2] (sin_t = cos_t + hd / 2), row = position & rope_mask, refilled by the host for the tick's positions
    int rope_stride;                         // with rope_mask > 0: 0 (the default) one ring for every slot; > 0 (an endless group): a ring per session, rope_stride rows apart --
                                             // slot z reads row order[z] * rope_stride + (position & rope_mask)
};
hipError_t launch_stream_attn(const StreamAttnParams& p, int hd, hipStream_t s);
// the same attention for a burst of ticks: 1 <= M <= 64 rows per session (b ticks' 4 b rows, all at STRM_ENC_POS + m), cap > window + M, and with a RoPE ring
// rope_mask + 1 >= M.  One workgroup per (head, tile of 4 query rows, slot) reads every ring row once for its tile.  One launch with M = 4 b leaves the bits in `out`
// and in every ring word that b launches of launch_stream_attn with M = 4 leave when STRM_ENC_POS moves by 4 between them (stream_attn_burst_kernel, vox_kernels.hip).
hipError_t launch_stream_attn_burst(const StreamAttnParams& p, int hd, hipStream_t s);
// launches enqueued by launch_stream_attn_burst (vox_debug_stream_attn_burst_launches); attn_form_counts does not count them
unsigned long long stream_attn_burst_launches();
// ---- a BURST ROUND of a stream group ("Bursts in stream groups"): slot z of the round runs b[z] ticks (1 .. 16, descending over z), its rows
// packed behind the slots before it -- its first tick is tick0[z] = b[0] + .. + b[z - 1], its encoder rows start at row rpt * tick0[z].  One descriptor per round,
// uploaded once; the kernels below read it on the device.
struct StreamBurstDesc { int tick0[16]; int b[16]; };
// the RAGGED burst attention: launch_stream_attn_burst with a row count per slot.  Slot z's M_z = rpt * b[z] rows of qkv and out start at row rpt * tick0[z]; grid
// (heads, ceil(max M_z / 4), n), tiles at or beyond M_z leave at once.  For every slot the launch leaves in `out` and in every word of that session's rings the bits
// b[z] launches of launch_stream_attn with M = 4 leave; sessions outside `order[0 .. n)` keep every ring word.  a.M is unread.  host: the descriptor's host copy, checked
// before the launch (b 1 .. 16, tick0 the running sum, rpt * b <= 64, cap > window + max M_z, a RoPE ring of at least max M_z rows): a refused call launches nothing.
// Counted by stream_attn_burst_launches.
struct StreamAttnGroupParams : StreamAttnParams { const StreamBurstDesc* desc; int rpt; };
hipError_t launch_stream_attn_group_burst(const StreamAttnParams& a, const StreamBurstDesc* desc, const StreamBurstDesc& host, int rpt, int hd, hipStream_t s);
// the pack of a burst round's conv rows: slot z's first rpt * b[z] rows of src (slots src_slot_rows rows apart, D floats per row, D % 4 == 0) to rows rpt * tick0[z] ..
// of dst -- the encoder input, slot after slot.  max_b: the largest b of the round (the grid)
hipError_t launch_stream_burst_pack(const float* src, int src_slot_rows, const StreamBurstDesc* desc, int n, int rpt, int max_b, int D, float* dst, hipStream_t s);
// rows 0 .. rows-1 of every layer's ring from token-major k | v rows (the model's prefix state: [layers][rows][k row | v row])
hipError_t launch_stream_ring_init(const float* kv, int layers, int rows, int n_heads, int hd, int cap, float* kring, float* vring, hipStream_t s);
// h = audio_row + embed(tokens[STRM_POS]); the adapter row is also kept in audio_keep[STRM_POS % keep_rows] (an engine hand-off timeout re-runs the decode steps from there)
hipError_t launch_stream_embed(Q4W tok, const int* tokens, const float* audio_row, float* audio_keep, int keep_rows, int D, const int* state, float* h, hipStream_t s);
// the same input from the kept row (the re-run)
hipError_t launch_stream_embed_kept(Q4W tok, const int* tokens, const float* audio_keep, int keep_rows, int D, const int* state, float* h, hipStream_t s);
// tokens[STRM_POS + 1] = argmax over the lm_head partials, then the state advances by one tick (enc_rows encoder rows, frames mel frames;
// enc_rows = 0: a decode-only re-run moves STRM_POS alone)
hipError_t launch_stream_advance(const float* part_val, const int* part_idx, int n_parts, int* tokens, int* state, int enc_rows, int frames, int cap, hipStream_t s);
// ---- the decode half of a group round (vox_stream_group): n <= 16 rows, row r = session order[r], through xf_chain.
// input rows: h[r] = audio[r] + embed(tokens[STRM_POS]) as f32, as layer 0's XF planes of h * xf_w with the row's sum of squares (what launch_argmax_embed_batch forms),
// pos[r] = STRM_POS and kv_row[r] = order[r]: the positions and cache slices xf_chain reads
// pages (a paged group): also page_out[r] = the table entry of the row's position (tab[order[r] * tab_stride + pos >> shift]) and in_page_out[r] = pos % page_rows
// tab_len > 0 (an endless group): the table row is a ring of tab_len entries, the entry is (pos >> shift) % tab_len (AttnParams::page_tab_len)
struct StreamPages { const int* tab; int tab_stride, shift; int* page_out; int* in_page_out; int tab_len; };
hipError_t launch_stream_group_embed(Q4W tok, const StreamMember* mem, const int* order, int n, const float* audio, int D, float* h, uint16_t* xf, const float* xf_w,
                                     float* ssq_out, int* pos, int* kv_row, hipStream_t s, const StreamPages* pages = nullptr);
// launch_stream_group_embed for decode round t of a burst round: row r's audio row is row desc->tick0[r] + t of `audio` (tick t of slot r); everything else as above
hipError_t launch_stream_group_embed_burst(Q4W tok, const StreamMember* mem, const int* order, int n, const float* audio, const StreamBurstDesc* desc, int t, int D, float* h, uint16_t* xf,
                                           const float* xf_w, float* ssq_out, int* pos, int* kv_row, hipStream_t s, const StreamPages* pages = nullptr);
// a paged member's seed: rows 0 .. rows-1 of src_k / src_v [layers][kv_heads][rows][hd] into the pages tab[0 ..] of the pool (layers layer_stride floats apart)
// kv_bf16: pool_k / pool_v point at uint16_t pools (layer_stride in 16-bit elements), the rows are rounded by kv_bf16_round
hipError_t launch_stream_pages_seed(const float* src_k, const float* src_v, int layers, int kv_heads, int rows, int hd, const int* tab, int page_shift, size_t layer_stride,
                                    float* pool_k, float* pool_v, hipStream_t s, bool kv_bf16 = false);
// tokens[STRM_POS + 1] = argmax of logits row r (argmax_take / block_argmax: the rule of every decode form), the row copied to the session's tap when one is armed,
// then the session's state advances by one tick as launch_stream_advance moves it
hipError_t launch_stream_group_advance(const float* logits, int vocab, const StreamMember* mem, const int* order, int n, int enc_rows, int frames, int cap, hipStream_t s);
// ---- scores of emitted ids (vox_token_score): for a logits row L[V] and an id t, logprob = L[t] - (m + log sum_v exp(L[v] - m)), m = max L (f32, expf / logf),
// runner_up = the argmax over v != t by the rule above launch_argmax_final (-1 when no such column can win), margin = L[t] - L[runner_up] (L[t] + inf without one).
// A row with a NaN or a maximum that is not finite: logprob = NaN.  The record is a function of the row's values and V alone (one scan order for aligned and
// misaligned rows, a fixed reduction tree): score_row, vox_kernels.hip.
// out[r] = the record of ids[r] on row r of x [rows][V] (device pointers; ids null: the row's argmax, 0 when nothing wins)
hipError_t launch_score_rows(const float* x, int rows, int V, const int* ids, TokenScore* out, hipStream_t s);
// behind launch_stream_advance / launch_stream_group_advance: slot z < n scores the id session order[z] just emitted (tokens[STRM_POS]) on row z of logits [n][vocab],
// into mem[order[z]].scores[STRM_POS - first_pos]; sessions whose scores pointer is null are skipped
hipError_t launch_stream_score(const float* logits, int vocab, const StreamMember* mem, const int* order, int n, int first_pos, hipStream_t s);
// ---- alternatives of emitted ids (vox_token_alts): for a logits row L[V] and k in 1 .. 8, alt[j] = the argmax by the rule over the columns not yet taken (n = how many
// could win, at most k; the entries behind are {-1, NaN}) with logprob = (L[id] - m) - logf(S), and entropy = max(0, logf(S) - T / S), S = sum exp(L - m) as score_row sums
// it, T = sum exp(L - m) (L - m) over the columns above -inf.  A row with a NaN or a maximum that is not finite: entropy and every logprob NaN.  A function of the row's
// values, V and k alone; the list for k is the list for 8 cut short: alts_row, vox_kernels.hip.
// out[r] = the record of row r of x [rows][V] (device pointers)
hipError_t launch_alts_rows(const float* x, int rows, int V, int k, TokenAlts* out, hipStream_t s);
// behind launch_stream_score's place in the tick: slot z < n writes the record of the id session order[z] just emitted from row z of logits [n][vocab] into
// mem[order[z]].alts[STRM_POS - first_pos] at that session's alts_k; sessions whose alts pointer is null are skipped
hipError_t launch_stream_alts(const float* logits, int vocab, const StreamMember* mem, const int* order, int n, int first_pos, hipStream_t s);
// ---- both records in one launch (the offline and batch paths: records_row, vox_kernels.hip).  The scored id is the row's own argmax by the rule (0 when nothing wins).
// k == 0: scores[r] alone (alts null), launch_score_rows' arithmetic.  k in 1 .. 8: alts[r] and, when scores is given, scores[r] from the same two scans of the row.
// Bit for bit the records of launch_score_rows(ids = null) and launch_alts_rows on the same row.
hipError_t launch_records_rows(const float* x, int rows, int V, int k, TokenScore* scores, TokenAlts* alts, hipStream_t s);
// the batch drivers' form, in front of the argmax launch of a step (which moves pos, slot_clip and the queues).  Rows are addressed as BatchTapParams addresses them;
// utterance c's id j = pos[r] + 1 - first_pos goes to record rec_off[c] + j of scores / alts (rec_off [n_clips + 1]: the prefix sum of the utterances' id counts,
// n_records = rec_off[n_clips]; a j outside the utterance's count writes nothing).  scores / alts / k as launch_records_rows.
struct BatchRecordsParams {
    const float* logits; int vocab;                    // [n_rows][vocab]
    const int* slot_clip; int clip0; const int* pos; const int* seq_len;      // per row (slot_clip, seq_len may be null)
    const int* rec_off; int n_clips, n_records, first_pos;
    TokenScore* scores; TokenAlts* alts; int k;
};
hipError_t launch_batch_records(const BatchRecordsParams& p, int n_rows, hipStream_t s);
// ---- levels of the audio behind emitted ids (vox_tick_level; DESIGN.md section 8, "Levels"): record k of a session describes the LEVEL_TICK = 2560 samples that are new
// to the tick that chooses id k -- the window [2560 (k - 1), 2560 k) of the session's own 16 kHz sample index -- each taken as stream_mel_kernel takes it:
// v = ring[i & ring_mask]; v *= gain (f32), 0 for i < 0 (the silent left pad).  peak = max |v| (exact); mean_square = (sum v * v) / 2560 in f32 by ONE scan order and ONE
// reduction tree (level_window, vox_kernels.hip): thread t of 256 squares (one rounding each) and adds its samples t, t + 256, .., t + 2304 in that order (10 additions
// from 0), 6 butterfly levels add the 64 partials of each wave (__shfl_xor, o = 32 .. 1), the four waves' sums are added as (w0 + w1) + (w2 + w3), one division by
// 2560 -- 18 additions on every path from a sample to the root, so without underflow the result is within (1 + 2^-24)^20 - 1 < 2^-19 relative of the exact sum of the exact squares; a square below 2^-126 rounds on the
// subnormal grid, which adds at most 2^-149 absolute to the record.  A non-finite sample makes mean_square non-finite; nothing else is promised then.
// The record is a function of the window's samples and the gain alone: every launch form below runs the one device function.
// launch_stream_level, in front of the round's mel launch (the state block is the one the round's first tick finds; the samples the two launches read are the same ones):
// grid (ticks, n); slot z < n works for session order[z], block (t, z) writes mem[order[z]].levels[STRM_POS - first_pos + t] from the window starting at
// 160 STRM_FRAME - left + 2560 t.  first_pos: the position whose tick chooses id 0 (VOX_PREFIX_TOKENS - 1).  ticks = 1: a tick / a plain round; ticks = b, desc null: a
// solo burst of b ticks; desc (device; host: its host copy, checked here): a burst round, slot z runs desc->b[z] <= ticks ticks, blocks beyond leave at once.
// Sessions whose levels pointer is null are skipped; a record index outside 0 .. levels_cap - 1 writes nothing.
static const int LEVEL_TICK = 2560;
hipError_t launch_stream_level(const StreamMember* mem, const int* order, int n, int ring_mask, long left, int first_pos, int ticks, const StreamBurstDesc* desc,
                               const StreamBurstDesc* host, hipStream_t s);
// ---- the ring keep of a peek (vox_stream_peek, vox_stream_group_peek): around ticks that are taken back.  Slot z < n works for session order[z] on its own area
// keep + z * slot_stride (floats, a multiple of 4): [STRM_WORDS ints: the state block][K: layers x n_heads x rows x hd][V: the same].
// restore = 0 (save, in front of the ticks): the state block, and of every (layer, head) of K and V the `rows` ring rows from STRM_HEAD on, modulo cap -- the slots the
// next rows / 4 ticks write.  restore = 1 (behind them): the same rows back from where the SAVED block's STRM_HEAD points, then the block itself.  16-byte accesses, no
// arithmetic on the values; the launch arguments of the two directions of a call are the same.  rows <= cap, hd % 4 == 0.
struct StreamKeepParams {
    const StreamMember* mem; const int* order; int n;
    int layers, n_heads, hd, cap, rows;
    float* keep; size_t slot_stride;
};
size_t stream_keep_floats(int layers, int n_heads, int hd, int rows);      // one slot's area
hipError_t launch_stream_keep(const StreamKeepParams& p, int restore, hipStream_t s);
// ---- a session blob's K / V sections (vox_stream_snapshot / vox_stream_restore; DESIGN.md section 8, "Snapshot and resume"): ONE launch moves the logical rows
// lo .. hi - 1 of the planes plane0 .. plane0 + n_planes - 1 (plane = layer * heads + head) of K and of V between the blob's dense layout -- blob_k / blob_v
// [n_planes][hi - lo][hd], the first plane of the launch at the pointer -- and a cache addressed in one of the project's four layouts.  Row r of (layer, head) lives at
//   SNAP_FLAT        cache + layer * layer_stride + head * head_stride + r * hd                          (a solo cache, a slab slice: head_stride = rows * hd)
//   SNAP_RING        ... + (r % cap) * hd                                                                  (the encoder ring, an endless session's decoder ring; any cap)
//   SNAP_PAGED       cache + layer * layer_stride + tab[r >> shift] * page_floats + head * head_stride + (r & (page_rows - 1)) * hd     (head_stride = page_rows * hd)
//   SNAP_PAGED_RING  the same with tab[(r >> shift) % tab_len]
// restore = 0 packs (cache -> blob), 1 unpacks (blob -> cache), on the same arguments.  16-byte accesses, no arithmetic on the values; cache rows outside lo .. hi - 1
// keep their bits.  hd 64 | 128; a ring holds the range (hi - lo <= cap; the range's pages <= tab_len), so no slot is named twice.  lo == hi launches nothing.  The
// table entries are the CALLER's to validate against the pool (snapshot_kv_pages_ok): the kernel reads tab[] as it is.
enum SnapLayout { SNAP_FLAT = 0, SNAP_RING = 1, SNAP_PAGED = 2, SNAP_PAGED_RING = 3 };
struct SnapshotKvParams {
    float *cache_k, *cache_v; float *blob_k, *blob_v;
    int layers, heads, hd, lo, hi;
    int plane0, n_planes;                   // the launch's planes (a host blob passes through staging in pieces of whole planes); n_planes 0: all of them
    int layout;                             // SnapLayout
    size_t layer_stride, head_stride;       // floats
    int cap;                                // SNAP_RING
    const int* tab; int shift, tab_len;     // SNAP_PAGED / SNAP_PAGED_RING: device table of the session, log2(page_rows); tab_len: SNAP_PAGED the entries the table has, SNAP_PAGED_RING the ring's
    size_t page_floats;                     // floats between two pages of one layer
    // SNAP_PAGED / SNAP_PAGED_RING on a bf16 pool: cache_k / cache_v point at uint16_t pools, the three strides count 16-bit elements.  Pack widens (exact), restore
    // rounds by kv_bf16_round (exact for a blob packed from a bf16 pool); the blob holds f32 rows either way
    int kv_bf16;
};
// host: every table entry the range lo .. hi - 1 touches lies in 0 .. pool_pages - 1 (tab: the HOST copy of the table); *bad_page: the first logical page that does not
bool snapshot_kv_pages_ok(const int* tab, int layout, int shift, int tab_len, int lo, int hi, int pool_pages, int* bad_page);
hipError_t launch_snapshot_kv(const SnapshotKvParams& p, int restore, hipStream_t s);

}  // namespace vox
