// vox_q8.hip -- linear operators on Q8_0 weights (gfx950): out[m][n] = epi(x[m] . W[n] + bias[n]) for a WFMT_Q8_0 matrix, behind ONE entry, launch_q8_linear,
// which picks a kernel by the row count.  Also the tensor's load-time split (q8_repack_kernel) and its diagnostic dequantisation.
//
// Device form of a Q8_0 tensor (Q4W with fmt WFMT_Q8_0): the file's 34-byte blocks {f16 d; int8 q[32]} are split at creation into qs = the int8 plane [N][K]
// (32 bytes per block, rows 16-byte aligned) and sc = the f16 scales [N][K / 32].  The 32 bytes of a block are stored in the element order of to_digits' planes
// (vox_digits.h): bytes [0, 8) = elements 0..7, [8, 16) = 16..23, [16, 24) = 8..15, [24, 32) = 24..31 -- half h (16 bytes) is one lane's B operand of the int8 MFMA.
//
// (a) q8_rows_kernel, M <= 4 and K <= 8192 (decode, tick): the four-row operator's design (vox_rows4.hip) on Q8 bytes.  A workgroup of 8 waves stages the rows once in
// LDS as four 7-bit digit planes plus block info (to_digits).  One v_mfma_i32_16x16x64_i8 takes, as its 16 A rows, the 4 digits x 4 rows of ONE block (the K columns
// of the step's other block are zero) and, as B, 16 weight rows x that block's int8 values: one 16-byte load per lane, no unpack, no offset.  D[4 r + c][n] is the
// exact digit sum (|D| <= 32 * 127 * 128 < 2^20); lane (n, g) forms D0 + 2^7 D1 + 2^14 D2 + 2^21 D3 -- up to 39 bits -- exactly in f64, rounds it to f32 ONCE and
// applies one FMA with f32(d) * 2^-shift into its accumulator, blocks ascending.  (rows4's digits_finish converts a 2^26 `lo` term to f32: exact for nibbles, not for
// bytes.)  Waves split K by a rule that depends on K alone (wave w: steps [w spw, (w + 1) spw), spw = ceil(steps / 8)); the eight partials meet in LDS and are added in
// one fixed order by wave 0, which runs the epilogue.  The grid is min(N / 16, 512) workgroups walking the 16-row output tiles; the next step's (or the next tile's
// first) loads are issued before the current step is consumed.  A row's bits depend on that row, the matrix and K alone: not on M, the grid or the run.
//
// (M <= 4 with K > 8192 goes to the K-slice operator of vox_q8_slices.hip: launch_q8_linear hands it the caller's planes.)
//
// (b) q8_gemm_kernel, M >= 5 (prefill, bursts, groups): v_mfma_f32_16x16x32_bf16, one MFMA K-step == one Q8_0 block.  A 4-wave workgroup
// owns 64 output columns (wave w: n-tile w) for up to 64 rows (1..4 m-tiles: a workgroup runs only the m-tiles that hold rows); M > 64 tiles over grid.y, the weights
// of a tile re-read from L2.  The activation rows are the A operand, split into bf16 hi + lo ONCE per workgroup and held in LDS in fragment order, K in double-buffered
// chunks of 64 columns (one barrier per chunk; the next chunk's rows and weights are requested before the current chunk runs).  The weights are the B operand: lane
// (n, g) loads stored bytes [8 g, 8 g + 8) of its weight row's block and widens them to bf16 exactly (|q| <= 128); the A fragments follow the stored element order.
// Per block t = mfma(lo, B, mfma(hi, B, 0)), acc = fma(t, d[n], acc): the scale belongs to the lane's own output column.  K ascending, no atomics.
#include "vox_kernels.h"

#include <hip/hip_fp16.h>

namespace vox {
namespace {

#include "vox_engine_common.h"
#include "vox_digits.h"
#include "vox_q8_common.h"      // WB8, f16_bits_f32, q8_digits_finish: shared with vox_q8_slices.hip

typedef __attribute__((__vector_size__(8 * sizeof(__bf16)))) __bf16 bf16x8;
typedef __attribute__((__vector_size__(4 * sizeof(float)))) float f32x4;
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float gelu_q8(float x) { return x * 0.5f * (1.0f + erff(x / 1.41421356237309504880f)); }      // gelu_f's form (vox_kernels.hip)
__device__ __forceinline__ float sbyte_f32(unsigned w, int n) { return (float)(int)(signed char)(w >> (8 * n)); }

// ------------------------------------------------------------------------------------------------
// load-time split and diagnostics
// ------------------------------------------------------------------------------------------------
__global__ void q8_repack_kernel(const uint8_t* __restrict__ raw, uint4* __restrict__ qs, uint16_t* __restrict__ sc, int64_t n_blocks) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const uint8_t* p = raw + b * 34;
    sc[b] = (uint16_t)(p[0] | (p[1] << 8));
    uint32_t w[8];      // w[i] = elements 4 i .. 4 i + 3
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)p[2 + 4 * i] | ((uint32_t)p[3 + 4 * i] << 8) | ((uint32_t)p[4 + 4 * i] << 16) | ((uint32_t)p[5 + 4 * i] << 24);
    qs[2 * b] = make_uint4(w[0], w[1], w[4], w[5]);          // half 0: elements 0..7, 16..23
    qs[2 * b + 1] = make_uint4(w[2], w[3], w[6], w[7]);      // half 1: elements 8..15, 24..31
}

__global__ void q8_dequant_kernel(Q4W w, float* __restrict__ out) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= (int64_t)w.N * w.nb) return;
    const uint4 h0 = w.qs[2 * b], h1 = w.qs[2 * b + 1];
    const float d = f16_bits_f32(w.sc[b]);
    const uint32_t ww[8] = {h0.x, h0.y, h1.x, h1.y, h0.z, h0.w, h1.z, h1.w};      // back in element order
    float* o = out + b * 32;
#pragma unroll
    for (int i = 0; i < 32; i++) o[i] = d * sbyte_f32(ww[i >> 2], i & 3);
}

// ------------------------------------------------------------------------------------------------
// (a) M <= 4 rows on the int8 matrix core
// ------------------------------------------------------------------------------------------------
constexpr int Q8R_WAVES = 8, Q8R_THREADS = 64 * Q8R_WAVES, Q8R_MAX_GRID = 512, Q8R_MAX_K = 8192;
__host__ __device__ inline int q8r_nbp(int nb) { return (nb + 1) & ~1; }      // blocks per row in LDS: a whole number of K steps (the pad block is zeros)
__host__ __device__ inline size_t q8r_lds_bytes(int nb) { return (size_t)4 * q8r_nbp(nb) * (128 + 8) + 2 * Q8R_WAVES * 64 * 4; }
static_assert(4 * (Q8R_MAX_K / 32) * (128 + 8) + 2 * Q8R_WAVES * 64 * 4 <= 160 * 1024, "the largest K must fit a workgroup's LDS");

template <int EPI>
__global__ __launch_bounds__(Q8R_THREADS, 1) void q8_rows_kernel(const Q8LinearParams p) {
    extern __shared__ __align__(16) unsigned char q8_lds[];
    const int nb = p.w.nb, nbp = q8r_nbp(nb), M = p.M, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* planes = q8_lds;                                                   // [4 rows][nbp][4 digits][2 halves][16]
    float2* binfo = reinterpret_cast<float2*>(q8_lds + (size_t)4 * nbp * 128);        // [4 rows][nbp]: {unused here (the Q4 offset), 2^-shift}
    float* red = reinterpret_cast<float*>(binfo + 4 * nbp);                           // [2][waves][64]

    // (1) stage the rows: piece i = 4 consecutive elements; 8 consecutive lanes hold one block (to_digits' DPP steps stay inside them), rows M..3 and the pad
    // block are zeros -> zero planes
    const int npp = nbp * 8, npieces = nb * 8;
    for (int i = tid; i < 4 * npp; i += Q8R_THREADS) {
        const int r = i / npp, pc = i - r * npp;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < M && pc < npieces) v = *reinterpret_cast<const float4*>(p.x + (size_t)r * p.x_stride + 4 * pc);
        const float vv[4] = {v.x, v.y, v.z, v.w};
        to_digits(vv, lane, planes + ((size_t)r * nbp + (pc >> 3)) * 128, binfo + r * nbp + (pc >> 3));
    }
    __syncthreads();

    // (2) the product.  Lane (n, g): weight row n of the tile, half g & 1 of block 2 s + (g >> 1) as B; A row n = digit n & 3 of activation row n >> 2
    const int n = lane & 15, g = lane >> 4, pb = g >> 1, h = g & 1, tiles = p.w.N >> 4, nsteps = nbp >> 1;
    const int spw = (nsteps + Q8R_WAVES - 1) / Q8R_WAVES, s_lo = min(wave * spw, nsteps), s_hi = min(s_lo + spw, nsteps);
    const auto wload = [&](int t, int s) {
        const size_t b0 = (size_t)(16 * t + n) * nb + 2 * s;
        WB8 w; w.q = u32x4{0u, 0u, 0u, 0u}; w.s1 = 0;
        if (2 * s + pb < nb) w.q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.w.qs + (b0 + pb) * 2 + h));
        w.s0 = __builtin_nontemporal_load(p.w.sc + b0);
        if (2 * s + 1 < nb) w.s1 = __builtin_nontemporal_load(p.w.sc + b0 + 1);
        return w;
    };
    const unsigned char* a_base = planes + (size_t)(n >> 2) * nbp * 128 + ((n & 3) * 2 + h) * 16;
    const float2* bi_base = binfo + g * nbp;
    WB8 cur; cur.q = u32x4{0u, 0u, 0u, 0u}; cur.s0 = cur.s1 = 0;
    int t = blockIdx.x, par = 0;
    if (t < tiles && s_lo < s_hi) cur = wload(t, s_lo);
    for (; t < tiles; t += gridDim.x) {
        float acc = 0.f;
        for (int s = s_lo; s < s_hi; s++) {
            WB8 nxt = cur;
            if (s + 1 < s_hi) nxt = wload(t, s + 1);
            else if (t + (int)gridDim.x < tiles) nxt = wload(t + gridDim.x, s_lo);
            const i4v X = *reinterpret_cast<const i4v*>(a_base + (size_t)(2 * s + pb) * 128);
            const i4v z = i4v{0, 0, 0, 0}, A0 = g < 2 ? X : z, A1 = g < 2 ? z : X;
            const i4v B = i4v{(int)cur.q.x, (int)cur.q.y, (int)cur.q.z, (int)cur.q.w};
            const i4v D0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0, B, z, 0, 0, 0), D1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B, z, 0, 0, 0);
            const float sx0 = bi_base[2 * s].y, sx1 = bi_base[2 * s + 1].y;
            acc = q8_digits_finish(D0, f16_bits_f32(cur.s0), sx0, acc);      // fixed order: the wave's blocks ascending
            acc = q8_digits_finish(D1, f16_bits_f32(cur.s1), sx1, acc);
            cur = nxt;
        }
        float* rd = red + par * (Q8R_WAVES * 64);
        rd[wave * 64 + lane] = acc;
        __syncthreads();      // (the other area is free again: wave 0 read it before it arrived here)
        par ^= 1;
        if (wave != 0) continue;
        // (3) epilogue, wave 0: lane (n, g) = output row g, weight row 16 t + n
        float v = ((rd[lane] + rd[64 + lane]) + (rd[128 + lane] + rd[192 + lane])) + ((rd[256 + lane] + rd[320 + lane]) + (rd[384 + lane] + rd[448 + lane]));
        const int col = 16 * t + n;
        if (p.bias) v += p.bias[col];
        if (EPI == EPI_SWIGLU) {      // interleaved rows: 2 i gate, 2 i + 1 up -- the partner is the neighbouring lane (all 64 lanes active for the DPP move)
            const float up = dppf<0xB1>(v);
            if (g < M && !(n & 1)) p.out[(size_t)g * p.out_stride + (col >> 1)] = silu_e(v) * up;
        } else if (g < M) {
            if (EPI == EPI_GELU) v = gelu_q8(v);
            p.out[(size_t)g * p.out_stride + col] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// (b) M >= 5 rows (and K > 8192) on the bf16 matrix core
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cvt_pk_bf16(float a, float b) {      // v_cvt_pk_bf16_f32: round to nearest even
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {a, b};
    union { bf16x2_t b; uint32_t u; } c; c.b = __builtin_convertvector(v, bf16x2_t); return c.u;
}
__device__ __forceinline__ void split_pair(float a, float b, uint32_t& hi, uint32_t& lo) {      // x ~= hi + lo, |err| <= 2^-17 |x|
    hi = cvt_pk_bf16(a, b);
    lo = cvt_pk_bf16(a - __uint_as_float(hi << 16), b - __uint_as_float(hi & 0xFFFF0000u));
}
__device__ __forceinline__ uint32_t pack_bf16_exact(float a, float b) { return (__float_as_uint(a) >> 16) | (__float_as_uint(b) & 0xFFFF0000u); }      // integers |q| <= 128: exact in bf16
__device__ __forceinline__ bf16x8 as_bf16x8(uint4 v) { union { uint4 u; bf16x8 b; } c; c.u = v; return c.b; }
__device__ __forceinline__ bf16x8 q8_widen(uint2 q) {      // 8 int8 -> 8 bf16, slot i = byte i
    return as_bf16x8(make_uint4(pack_bf16_exact(sbyte_f32(q.x, 0), sbyte_f32(q.x, 1)), pack_bf16_exact(sbyte_f32(q.x, 2), sbyte_f32(q.x, 3)),
                                pack_bf16_exact(sbyte_f32(q.y, 0), sbyte_f32(q.y, 1)), pack_bf16_exact(sbyte_f32(q.y, 2), sbyte_f32(q.y, 3))));
}

struct WG8 { uint2 q0, q1; unsigned short s0, s1; };      // one lane's share of a chunk: 8 int8 values and the f16 scale of each of the chunk's two blocks

template <int EPI>
__global__ __launch_bounds__(256) void q8_gemm_kernel(const Q8LinearParams p) {
    __shared__ __attribute__((aligned(16))) uint4 lds[2][2][2][256];      // [buffer][hi / lo][block of the chunk][mt * 64 + lane]: 32 KiB
    const int nb = p.w.nb, N = p.w.N, M = p.M, nch = (nb + 1) >> 1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4;
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int mts = min(4, (M - m0 + 15) >> 4);      // m-tiles of this workgroup that hold rows
    // MFMA role: weight row wn; N % 16 == 0, so an n-tile lies inside the matrix or outside it (then the wave computes on tile 0 and stores nothing)
    const bool wave_ok = n0 + 16 * wave < N;
    const int wn = (wave_ok ? n0 + 16 * wave : 0) + (lane & 15);
    const uint2* wq = reinterpret_cast<const uint2*>(p.w.qs) + (size_t)wn * nb * 4 + g;
    const uint16_t* ws = p.w.sc + (size_t)wn * nb;
    // staging role: fragment f = tid + 256 i -> (row f >> 3, block (f >> 2) & 1 of the chunk, group f & 3): 8 consecutive threads read 256 contiguous bytes of a row.
    // Group sg of the A fragments holds the elements of stored bytes [8 sg, 8 sg + 8): 0..7, 16..23, 8..15, 24..31
    const int sj = (tid >> 2) & 1, sg = tid & 3, xcol = 32 * sj + 8 * ((sg >> 1) | ((sg & 1) << 1));
    float4 xr[2][2];
    const auto xload = [&](int c) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int sm = (tid >> 3) + 32 * i;
            xr[i][0] = xr[i][1] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (m0 + sm < M && 2 * c + sj < nb) {
                const float* src = p.x + (size_t)(m0 + sm) * p.x_stride + 64 * c + xcol;
                xr[i][0] = *reinterpret_cast<const float4*>(src); xr[i][1] = *reinterpret_cast<const float4*>(src + 4);
            }
        }
    };
    const auto xstage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int sm = (tid >> 3) + 32 * i, slot = (sm >> 4) * 64 + sg * 16 + (sm & 15);
            if (sm >= 16 * mts) continue;
            uint4 hi, lo;
            split_pair(xr[i][0].x, xr[i][0].y, hi.x, lo.x); split_pair(xr[i][0].z, xr[i][0].w, hi.y, lo.y);
            split_pair(xr[i][1].x, xr[i][1].y, hi.z, lo.z); split_pair(xr[i][1].z, xr[i][1].w, hi.w, lo.w);
            lds[buf][0][sj][slot] = hi; lds[buf][1][sj][slot] = lo;
        }
    };
    const auto wload = [&](int c) {      // the second block of an odd tail: clamped (read again, never used)
        const int b0 = 2 * c, b1 = min(2 * c + 1, nb - 1);
        WG8 w; w.q0 = wq[(size_t)b0 * 4]; w.q1 = wq[(size_t)b1 * 4]; w.s0 = ws[b0]; w.s1 = ws[b1];
        return w;
    };

    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    xload(0); xstage(0);
    WG8 cur = wload(0);
    __syncthreads();
    for (int c = 0; c < nch; c++) {
        const int buf = c & 1;
        WG8 nxt = cur;
        if (c + 1 < nch) { xload(c + 1); nxt = wload(c + 1); }      // in flight while this chunk is on the MFMAs
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (2 * c + j >= nb) continue;
            const bf16x8 bw = q8_widen(j ? cur.q1 : cur.q0);
            const float d = f16_bits_f32(j ? cur.s1 : cur.s0);
#pragma unroll
            for (int mt = 0; mt < 4; mt++) {
                if (mt >= mts) continue;
                const bf16x8 ah = as_bf16x8(lds[buf][0][j][mt * 64 + lane]), al = as_bf16x8(lds[buf][1][j][mt * 64 + lane]);
                f32x4 t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bw, (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
                t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bw, t, 0, 0, 0);
                acc[mt][0] = fmaf(t[0], d, acc[mt][0]); acc[mt][1] = fmaf(t[1], d, acc[mt][1]);
                acc[mt][2] = fmaf(t[2], d, acc[mt][2]); acc[mt][3] = fmaf(t[3], d, acc[mt][3]);
            }
        }
        if (c + 1 < nch) { xstage(buf ^ 1); cur = nxt; }      // (every wave left buffer buf ^ 1 behind at the last barrier)
        __syncthreads();
    }
    // epilogue: lane holds D[m = m0 + 16 mt + 4 g + r][n = wn]
    const float bias = p.bias ? p.bias[wn] : 0.f;
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
        if (mt >= mts) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int m = m0 + mt * 16 + 4 * g + r;
            float v = acc[mt][r] + bias;
            if (EPI == EPI_SWIGLU) {      // interleaved rows: even n = gate, odd n = up, the neighbouring lane's (all 64 lanes active for the DPP move)
                const float up = dppf<0xB1>(v);
                if (m < M && wave_ok && !(wn & 1)) p.out[(size_t)m * p.out_stride + (wn >> 1)] = silu_e(v) * up;
            } else if (m < M && wave_ok) {
                if (EPI == EPI_GELU) v = gelu_q8(v);
                p.out[(size_t)m * p.out_stride + wn] = v;
            }
        }
    }
}

template <int EPI>
hipError_t q8_rows_launch_t(const Q8LinearParams& p, hipStream_t s) {
    static DevOnce once;
    auto kern = q8_rows_kernel<EPI>;
    const int dev = vox_current_device();
    if (!once.done(dev)) {      // more than the default 64 KiB of dynamic LDS: raised once per device to the largest K's
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)q8r_lds_bytes(Q8R_MAX_K / 32));
        if (e != hipSuccess) return e;
        once.set(dev);
    }
    const int tiles = p.w.N / 16;
    kern<<<dim3(tiles < Q8R_MAX_GRID ? tiles : Q8R_MAX_GRID), dim3(Q8R_THREADS), q8r_lds_bytes(p.w.nb), s>>>(p);
    return hipGetLastError();
}

template <int EPI>
hipError_t q8_gemm_launch_t(const Q8LinearParams& p, hipStream_t s) {
    q8_gemm_kernel<EPI><<<dim3((p.w.N + 63) / 64, (p.M + 63) / 64), dim3(256), 0, s>>>(p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_q8_repack(const uint8_t* raw, Q4W w, hipStream_t s) {
    if (!raw || !w.qs || !w.sc || w.fmt != WFMT_Q8_0) return hipErrorInvalidValue;
    const int64_t n_blocks = (int64_t)w.N * w.nb;
    q8_repack_kernel<<<dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, s>>>(raw, const_cast<uint4*>(w.qs), const_cast<uint16_t*>(w.sc), n_blocks);
    return hipGetLastError();
}

hipError_t launch_q8_dequant(Q4W w, float* out, hipStream_t s) {
    if (!out || !w.qs || !w.sc || w.fmt != WFMT_Q8_0) return hipErrorInvalidValue;
    const int64_t n_blocks = (int64_t)w.N * w.nb;
    q8_dequant_kernel<<<dim3((unsigned)((n_blocks + 255) / 256)), dim3(256), 0, s>>>(w, out);
    return hipGetLastError();
}

hipError_t launch_q8_linear(const Q8LinearParams& p, int epi, hipStream_t s, float* planes, size_t planes_bytes) {
    const Q4W& w = p.w;
    if (w.fmt != WFMT_Q8_0 || !w.qs || !w.sc || p.M < 1 || p.M > 64 * 65535 || w.K < 32 || w.K % 32 || w.nb != w.K / 32 || w.N < 16 || w.N % 16) return hipErrorInvalidValue;
    if (!p.x || !p.out || (p.x_stride & 3) || ((uintptr_t)p.x & 15) || p.x_stride < w.K) return hipErrorInvalidValue;      // the rows are read as float4
    if (epi != EPI_STORE && epi != EPI_GELU && epi != EPI_SWIGLU) return hipErrorInvalidValue;
    if (p.M <= 4 && w.K > Q8R_MAX_K) {      // decode rows past the rows kernel's LDS: the K-slice operator (vox_q8_slices.hip), which needs the caller's planes
        Q8SliceParams q{}; q.w = w; q.x = p.x; q.x_stride = p.x_stride; q.M = p.M; q.out = p.out; q.out_stride = p.out_stride; q.bias = p.bias;
        return launch_q8_slices(q, PRO_NONE, epi, planes, planes_bytes, s);
    }
    const bool rows = p.M <= 4 && w.K <= Q8R_MAX_K;      // the digit planes of four rows in a workgroup's LDS; beyond, the GEMM
#define VOX_Q8(E_) if (epi == E_) return rows ? q8_rows_launch_t<E_>(p, s) : q8_gemm_launch_t<E_>(p, s);
    VOX_Q8(EPI_STORE) VOX_Q8(EPI_GELU) VOX_Q8(EPI_SWIGLU)
#undef VOX_Q8
    return hipErrorInvalidValue;
}

}  // namespace vox
