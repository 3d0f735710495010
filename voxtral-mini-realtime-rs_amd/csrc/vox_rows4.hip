// vox_rows4.hip -- the four-row Q4 operator of a live session's tick (gfx950): out[m][n] = epi(pro(x[m]) . W[n] + bias[n]) for M <= 4 rows of a WFMT_Q4_0
// matrix in ONE pass over the weights, with the RMSNorm fused in front (PRO_RMS) and the tick's three epilogues behind (store, residual, SwiGLU).
//
// What it replaces: q4_gemv_kernel with grid.y = rows -- a one-row kernel whose every y slice streams the whole matrix again -- and the norm launch in front of it.
//
// Arithmetic: the decode engine's exact integer product (vox_digits.h).  Every 32-element block of every row is held in LDS as four 7-bit digit planes plus the
// block info {-8 sum(x_int), 2^-shift}.  One v_mfma_i32_16x16x64_i8 takes, as its 16 A rows, the 4 digits of the 4 activation rows of ONE block (A row 4 r + c =
// digit c of row r; the K columns of the step's other block are zero) and, as B, the step's 16 weight rows x 64 nibbles as int8.  D[4 r + c][n] is then the exact
// digit sum of that block: lane (n = lane & 15, g = lane >> 4) holds the four digits of activation row g for weight row n and finishes them itself -- Horner in
// int32, one f32 FMA, the -8 offset, the f16 block scale times 2^-shift -- into ONE f32 accumulator per lane.  One weight fetch and one nibble unpack serve all
// four rows; no cross-lane sum exists inside a wave.
//
// Work split: a workgroup of 8 waves stages the rows once, then walks the 16-row output tiles t = blockIdx.x, + gridDim.x, ...; the grid is min(tiles, 512).  Within
// a workgroup the waves split K: wave w owns the K steps (64 columns) [w spw, (w + 1) spw), spw = ceil(steps / 8) -- a function of K alone, so a value's bits do not
// depend on the grid.  The eight partials meet in LDS and are added in one fixed order by wave 0, which runs the epilogue.  (Splitting the TILES over the waves
// would need no sum, but the encoder's wo / w2 have 80 tiles: 20 workgroups of serial 80-step chains.  K split: 80 workgroups, 10 steps per wave.)
// B operand: the plain [N][nb] chunks (Q4W::qs / sc), lane (n, g) reads bytes [8 (g & 1), +8) of block 2 s + (g >> 1) of row 16 t + n, non-temporal; the next
// step's (or the next tile's first) loads are issued before the current step is consumed.  No weight request before the rows are staged (q4_gemv_kernel, step (3)).
// LDS: 4 bytes per element and row (planes) + 8 bytes per block and row (info) + 4 KiB (two reduction areas, so one barrier per tile) + 128 bytes (sums of squares).
#include "vox_kernels.h"

#include <hip/hip_fp16.h>

namespace vox {
namespace {

#include "vox_engine_common.h"
#include "vox_digits.h"

constexpr int R4_WAVES = 8, R4_THREADS = 64 * R4_WAVES, R4_MAX_GRID = 512, R4_MAX_K = 8192;
__host__ __device__ inline int r4_nbp(int nb) { return (nb + 1) & ~1; }      // blocks per row in LDS: a whole number of K steps (the pad block is zeros)
__host__ __device__ inline size_t r4_lds_bytes(int nb) { return (size_t)4 * r4_nbp(nb) * (128 + 8) + 2 * R4_WAVES * 64 * 4 + R4_WAVES * 4 * 4; }
static_assert(4 * (R4_MAX_K / 32) * (128 + 8) + 2 * R4_WAVES * 64 * 4 + R4_WAVES * 4 * 4 <= 160 * 1024, "the largest K must fit a workgroup's LDS");

struct WB { uint2 q; unsigned short s0, s1; };      // one lane's share of a K step: 8 bytes of nibbles, the f16 scales of the step's two blocks of its weight row

template <int PRO, int EPI>
__global__ __launch_bounds__(R4_THREADS, 1) void q4_rows4_kernel(const Rows4Params p) {
    extern __shared__ __align__(16) unsigned char r4_lds[];
    const int nb = p.w.nb, nbp = r4_nbp(nb), M = p.M, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char* planes = r4_lds;                                                   // [4 rows][nbp][4 digits][2 halves][16]
    float2* binfo = reinterpret_cast<float2*>(r4_lds + (size_t)4 * nbp * 128);        // [4 rows][nbp]
    float* red = reinterpret_cast<float*>(binfo + 4 * nbp);                           // [2][waves][64]
    float* ssq_s = red + 2 * R4_WAVES * 64;                                           // [waves][4 rows]

    // (1) stage the rows: piece i = 4 consecutive elements; 8 consecutive lanes hold one block (to_digits' DPP steps stay inside them), rows M..3 and the pad
    // block are zeros -> zero planes, info {-0, 2^-26}
    const int npp = nbp * 8, npieces = nb * 8;
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < 4 * npp; i += R4_THREADS) {
        const int r = i / npp, pc = i - r * npp;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < M && pc < npieces) v = *reinterpret_cast<const float4*>(p.x + (size_t)r * p.x_stride + 4 * pc);
        if (PRO == PRO_RMS) {
            const float q = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
#pragma unroll
            for (int rr = 0; rr < 4; rr++) ss[rr] += r == rr ? q : 0.f;
            if (pc < npieces) { const float4 gm = *reinterpret_cast<const float4*>(p.gamma + 4 * pc); v.x *= gm.x; v.y *= gm.y; v.z *= gm.z; v.w *= gm.w; }
        }
        const float vv[4] = {v.x, v.y, v.z, v.w};
        to_digits(vv, lane, planes + ((size_t)r * nbp + (pc >> 3)) * 128, binfo + r * nbp + (pc >> 3));
    }
    if (PRO == PRO_RMS) {      // each row's sum of squares in a fixed order: the thread's pieces ascending, the wave's DPP tree, the waves ascending (below)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) { const float w = wave_sum_e(ss[rr]); if (lane == 0) ssq_s[wave * 4 + rr] = w; }
    }
    __syncthreads();

    // (2) the product.  Lane (n, g): weight row n of the tile, half g & 1 of block 2 s + (g >> 1) as B; A row n = digit n & 3 of activation row n >> 2
    const int n = lane & 15, g = lane >> 4, pb = g >> 1, h = g & 1, tiles = p.w.N >> 4, nsteps = nbp >> 1;
    const int spw = (nsteps + R4_WAVES - 1) / R4_WAVES, s_lo = min(wave * spw, nsteps), s_hi = min(s_lo + spw, nsteps);
    const uint2* qs2 = reinterpret_cast<const uint2*>(p.w.qs);
    const auto wload = [&](int t, int s) {
        const size_t b0 = (size_t)(16 * t + n) * nb + 2 * s;
        WB w; w.q = make_uint2(0u, 0u); w.s1 = 0;
        if (2 * s + pb < nb) { const v2u_t q = __builtin_nontemporal_load(reinterpret_cast<const v2u_t*>(qs2 + (b0 + pb) * 2 + h)); w.q = make_uint2(q.x, q.y); }
        w.s0 = __builtin_nontemporal_load(p.w.sc + b0);
        if (2 * s + 1 < nb) w.s1 = __builtin_nontemporal_load(p.w.sc + b0 + 1);
        return w;
    };
    const unsigned char* a_base = planes + (size_t)(n >> 2) * nbp * 128 + ((n & 3) * 2 + h) * 16;
    const float2* bi_base = binfo + g * nbp;
    float rstd = 1.0f;
    if (PRO == PRO_RMS) {
        float a = 0.f;
#pragma unroll
        for (int w = 0; w < R4_WAVES; w++) a += ssq_s[w * 4 + g];
        rstd = 1.0f / sqrtf(a / (float)p.w.K + p.eps);
    }
    WB cur; cur.q = make_uint2(0u, 0u); cur.s0 = cur.s1 = 0;
    int t = blockIdx.x, par = 0;
    if (t < tiles && s_lo < s_hi) cur = wload(t, s_lo);
    for (; t < tiles; t += gridDim.x) {
        float acc = 0.f;
        for (int s = s_lo; s < s_hi; s++) {
            WB nxt = cur;
            if (s + 1 < s_hi) nxt = wload(t, s + 1);
            else if (t + (int)gridDim.x < tiles) nxt = wload(t + gridDim.x, s_lo);
            const i4v X = *reinterpret_cast<const i4v*>(a_base + (size_t)(2 * s + pb) * 128);
            const i4v z = i4v{0, 0, 0, 0}, A0 = g < 2 ? X : z, A1 = g < 2 ? z : X;
            i4v B;
            B[0] = (int)(cur.q.x & 0x0F0F0F0Fu); B[1] = (int)(cur.q.y & 0x0F0F0F0Fu); B[2] = (int)((cur.q.x >> 4) & 0x0F0F0F0Fu); B[3] = (int)((cur.q.y >> 4) & 0x0F0F0F0Fu);
            const i4v D0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0, B, z, 0, 0, 0), D1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B, z, 0, 0, 0);
            const float2 i0 = bi_base[2 * s], i1 = bi_base[2 * s + 1];
            acc = digits_finish(D0, i0.x, __half2float(__ushort_as_half(cur.s0)), i0.y, acc);      // fixed order: the wave's blocks ascending
            acc = digits_finish(D1, i1.x, __half2float(__ushort_as_half(cur.s1)), i1.y, acc);
            cur = nxt;
        }
        float* rd = red + par * (R4_WAVES * 64);
        rd[wave * 64 + lane] = acc;
        __syncthreads();      // (the other area is free again: wave 0 read it before it arrived here)
        par ^= 1;
        if (wave != 0) continue;
        // (3) epilogue, wave 0: lane (n, g) = output row g, weight row 16 t + n
        float v = ((rd[lane] + rd[64 + lane]) + (rd[128 + lane] + rd[192 + lane])) + ((rd[256 + lane] + rd[320 + lane]) + (rd[384 + lane] + rd[448 + lane]));
        const int col = 16 * t + n;
        if (PRO == PRO_RMS) v *= rstd;
        if (p.bias) v += p.bias[col];
        if (EPI == EPI_SWIGLU) {      // interleaved rows: 2 i gate, 2 i + 1 up -- the partner is the neighbouring lane (all 64 lanes active for the DPP move)
            const float up = dppf<0xB1>(v);
            if (g < M && !(n & 1)) p.out[(size_t)g * p.out_stride + (col >> 1)] = silu_e(v) * up;
        } else if (g < M) {
            if (EPI == EPI_RESID) v = v + p.resid[(size_t)g * p.resid_stride + col];
            p.out[(size_t)g * p.out_stride + col] = v;
        }
    }
}

std::atomic<unsigned long long> g_rows4_launches{0};

template <int PRO, int EPI>
hipError_t rows4_launch_t(const Rows4Params& p, hipStream_t s) {
    static DevOnce once;
    auto kern = q4_rows4_kernel<PRO, EPI>;
    const int dev = vox_current_device();
    if (!once.done(dev)) {      // more than the default 64 KiB of dynamic LDS: raised once per device to the largest K's
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)r4_lds_bytes(R4_MAX_K / 32));
        if (e != hipSuccess) return e;
        once.set(dev);
    }
    const int tiles = p.w.N / 16;
    kern<<<dim3(tiles < R4_MAX_GRID ? tiles : R4_MAX_GRID), dim3(R4_THREADS), r4_lds_bytes(p.w.nb), s>>>(p);
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) g_rows4_launches.fetch_add(1, std::memory_order_relaxed);      // launches so far: one that failed is not counted
    return e;
}

}  // namespace

bool q4_rows4_serves(const Q4W& w, int M, int pro, int epi) {
    return w.fmt == WFMT_Q4_0 && w.qs && w.sc && M >= 1 && M <= 4 && w.K >= 32 && w.K % 32 == 0 && w.K <= R4_MAX_K && w.nb == w.K / 32 && w.N >= 16 && w.N % 16 == 0 &&
           (pro == PRO_NONE || pro == PRO_RMS) && (epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SWIGLU);
}
unsigned long long q4_rows4_launches() { return g_rows4_launches.load(std::memory_order_relaxed); }

hipError_t launch_q4_rows4(const Rows4Params& p, int pro, int epi, hipStream_t s) {
    if (!q4_rows4_serves(p.w, p.M, pro, epi) || !p.x || !p.out) return hipErrorInvalidValue;
    if ((p.x_stride & 3) || ((uintptr_t)p.x & 15) || p.x_stride < p.w.K) return hipErrorInvalidValue;      // the rows are read as float4
    if (pro == PRO_RMS && (!p.gamma || ((uintptr_t)p.gamma & 15))) return hipErrorInvalidValue;
    if (epi == EPI_RESID && !p.resid) return hipErrorInvalidValue;
#define VOX_R4(P_, E_) if (pro == P_ && epi == E_) return rows4_launch_t<P_, E_>(p, s);
    VOX_R4(PRO_NONE, EPI_STORE) VOX_R4(PRO_NONE, EPI_RESID) VOX_R4(PRO_NONE, EPI_SWIGLU) VOX_R4(PRO_RMS, EPI_STORE) VOX_R4(PRO_RMS, EPI_RESID) VOX_R4(PRO_RMS, EPI_SWIGLU)
#undef VOX_R4
    return hipErrorInvalidValue;
}

}  // namespace vox
