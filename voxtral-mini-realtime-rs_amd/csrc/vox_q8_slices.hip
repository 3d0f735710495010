// vox_q8_slices.hip -- M <= 4 rows of a Q8_0 matrix at ANY K (gfx950), split over K slices, RMSNorm in front and the residual behind fused:
//     out[m][n] = epi( pro(x[m]) . W[n] + bias[n] ),  pro: none / RMSNorm,  epi: store / residual / SwiGLU / GELU
// on a WFMT_Q8_0 tensor as vox_q8.hip stores it (the int8 plane in to_digits' element order + f16 scales; no second copy).  Two launches, always:
//
// (1) q8_slice_kernel<PRO>, grid (workgroups per slice, slices): the product of ONE K slice.  K is cut into slices of Q8S_COLS = 3072 columns (96 blocks),
// ceil(K / 3072) of them, the last one short (down to one block) -- a rule of K alone.  Why 3072: a workgroup holds its slice of the four rows as digit planes,
// 4 rows x 96 blocks x (128 B of planes + 8 B of block info) = 51 KiB, plus 4 KiB of reduction areas and 144 B of sums of squares = 56464 B.  Two such workgroups
// fit a CU's 160 KiB (three would need 165 KiB), the allocation stays under the 64 KiB a kernel gets without asking, and the decoder's w2 (K = 9216) is three equal
// slices.  A workgroup of 8 waves stages its slice of the rows (to_digits, vox_digits.h; rows >= M and the pad block are zero planes; with PRO_RMS the rows are staged
// as x * gamma, unnormalised, and the slice's sum of squares per row is formed next to it) and then walks 16-row output tiles t = blockIdx.x, + gridDim.x, ...
// Inside the slice the arithmetic is q8_rows_kernel's: the waves split the slice's K steps (64 columns) by a rule of the slice length alone (wave w: steps
// [w spw, (w + 1) spw), spw = ceil(steps / 8)); one v_mfma_i32_16x16x64_i8 per block (A = 4 digits x 4 rows of the block, the step's other block's K columns zero; B =
// 16 weight rows x the block's 32 bytes); the 39-bit block sum exactly in f64, rounded once, one FMA with f32(d) * 2^-shift (q8_digits_finish), blocks ascending; the
// eight partials meet in LDS and are added in one fixed order (a wave without steps contributes +0) by a NINTH wave, which owns every global store of the kernel:
// on gfx9 loads and stores share vmcnt, so the product waves' loop is kept to loads alone and never waits behind a store.
// Memory side: every product wave keeps a register ring of Q8S_DEPTH = 4 K steps of weight loads in flight (16 B of int8 + two f16 scales per lane and step; a
// step's loads go into the registers it was consumed from).  The ring is filled BEFORE the rows are staged -- the weights do not depend on them, so the staging
// waits together with the first loads, not in front of them -- and runs on across the boundary to the workgroup's next tile.  Depth: a CU's share of the memory
// system is ~31 B/ns (8 TB/s over 256 CUs); at 1-2 us of loaded latency that is 31-62 KiB to keep in flight per CU, and 2 workgroups x 8 waves x 4 steps x 1 KiB =
// 64 KiB.  Two workgroups per CU are 18 waves, 5 on a SIMD, 102 VGPRs each: the kernel takes about 50, the ring 20 of them.  (As compiled today the waits
// of the unrolled loop come out as one wait for the whole ring per four steps, not one per step: four steps are requested and awaited together.)
// Workgroups per slice, a rule of N and K alone: with tiles = N / 16 and 512 = 256 CUs x 2 resident workgroups, one workgroup per tile while tiles x slices <= 512;
// beyond that every workgroup walks L = ceil(tiles x slices / 512) tiles, grid.x = ceil(tiles / L) -- so all of them are resident at once and carry the same work
// (w2: 192 tiles x 3 slices -> L = 2, 96 x 3 workgroups of two tiles each).  Staging costs 4 x slice floats per workgroup (re-read from L2) against 16 x slice weight
// bytes per tile from memory: equal at one tile per workgroup, which is why the walk grows before the grid exceeds what is resident.
// Output: plane [slice][4][N] f32 (rows < M) and, with the norm, [slice][4] partial sums of squares (workgroup 0 of the slice), plain vector stores.  No atomics, no
// arrival counters, no spinning.
//
// (2) q8_slice_finish_kernel<PRO, EPI>: one thread per output element adds the slice planes SLICE-ASCENDING, forms rstd[m] = 1 / sqrt(sum of the partials / K + eps)
// in the same order and scales the row, adds the bias and applies the epilogue.
//
// Properties: a row's bits depend on that row, the matrix and K alone -- not on M (the other rows' planes never meet it), the grid (the tile walk only says WHO
// computes a tile) or the run.  An all-zero row gives exact zeros (+ bias, residual), also under the norm (eps > 0: rstd is finite, 0 * rstd = 0).  No scratch, no
// spills; the unit is compiled without packed-f32 instructions, as vox_q8.hip is (build.py).
#include "vox_kernels.h"

#include <hip/hip_fp16.h>

namespace vox {
namespace {

#include "vox_engine_common.h"
#include "vox_digits.h"
#include "vox_q8_common.h"

constexpr int Q8S_COLS = 3072, Q8S_BLOCKS = Q8S_COLS / 32, Q8S_WAVES = 8, Q8S_THREADS = 64 * (Q8S_WAVES + 1), Q8S_DEPTH = 4, Q8S_RESIDENT = 2 * 256, Q8S_MAX_K = 65536;
__host__ __device__ inline int q8s_nbp(int nbs) { return (nbs + 1) & ~1; }      // blocks per row in LDS: a whole number of K steps (the pad block is zeros)
__host__ __device__ inline size_t q8s_lds_bytes(int nbs) { return (size_t)4 * q8s_nbp(nbs) * (128 + 8) + 2 * Q8S_WAVES * 64 * 4 + (Q8S_WAVES + 1) * 4 * 4; }
static_assert(Q8S_BLOCKS % 2 == 0, "a slice is a whole number of K steps, so the steps of a slice pair the blocks the matrix pairs");
static_assert(2 * (4 * Q8S_BLOCKS * (128 + 8) + 2 * Q8S_WAVES * 64 * 4 + (Q8S_WAVES + 1) * 4 * 4) <= 160 * 1024, "two workgroups fit a CU's LDS");
static_assert(4 * Q8S_BLOCKS * (128 + 8) + 2 * Q8S_WAVES * 64 * 4 + (Q8S_WAVES + 1) * 4 * 4 <= 64 * 1024, "within the dynamic LDS a kernel gets without an attribute");
inline int q8s_slices(int K) { return (K + Q8S_COLS - 1) / Q8S_COLS; }
inline int q8s_grid_x(int N, int K) {      // workgroups per slice (header: a rule of N and K alone)
    const long tiles = N / 16, walk = (tiles * q8s_slices(K) + Q8S_RESIDENT - 1) / Q8S_RESIDENT;
    return (int)((tiles + walk - 1) / walk);
}

__device__ __forceinline__ float gelu_q8s(float x) { return x * 0.5f * (1.0f + erff(x / 1.41421356237309504880f)); }      // gelu_f's form (vox_kernels.hip)

template <int PRO>
__global__ __launch_bounds__(Q8S_THREADS, 5) void q8_slice_kernel(const Q8SliceParams p, float* __restrict__ planes_out, float* __restrict__ ssq_out) {
    extern __shared__ __align__(16) unsigned char q8s_lds[];
    const int nb = p.w.nb, N = p.w.N, M = p.M, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int z = blockIdx.y, zb0 = z * Q8S_BLOCKS, nbs = min(nb - zb0, Q8S_BLOCKS), nbp = q8s_nbp(nbs), G = gridDim.x;      // this slice: blocks [zb0, zb0 + nbs)
    unsigned char* planes = q8s_lds;                                                   // [4 rows][nbp][4 digits][2 halves][16]
    float2* binfo = reinterpret_cast<float2*>(q8s_lds + (size_t)4 * nbp * 128);        // [4 rows][nbp]: {unused here (the Q4 offset), 2^-shift}
    float* red = reinterpret_cast<float*>(binfo + 4 * nbp);                            // [2][waves][64]
    float* ssq_s = red + 2 * Q8S_WAVES * 64;                                           // [waves + 1][4 rows]

    // roles of the product.  Lane (n, g): weight row n of the tile, half g & 1 of block 2 s + (g >> 1) of the slice as B; A row n = digit n & 3 of activation row n >> 2
    const int n = lane & 15, g = lane >> 4, pb = g >> 1, h = g & 1, tiles = N >> 4, nsteps = nbp >> 1;
    const int spw = (nsteps + Q8S_WAVES - 1) / Q8S_WAVES, s_lo = min(wave * spw, nsteps), s_hi = min(s_lo + spw, nsteps), nst = s_hi - s_lo;      // (the ninth wave: none)
    const int my_tiles = (tiles - (int)blockIdx.x + G - 1) / G;      // grid.x <= tiles: at least one
    // step s of the slice, tile t (t < tiles).  ALWAYS three loads, no branch around any of them: an odd slice's missing last block is read as the step's first
    // block again -- the same lines, no more traffic -- and its scale is dropped where the step is consumed (its digit planes are zeros as well)
    const auto wload = [&](int t, int s) {
        const size_t b0 = (size_t)(16 * t + n) * nb + zb0 + 2 * s;
        const int second = 2 * s + 1 < nbs ? 1 : 0;
        WB8 w;
        w.q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p.w.qs + (b0 + (pb & second)) * 2 + h));
        w.s0 = __builtin_nontemporal_load(p.w.sc + b0);
        w.s1 = __builtin_nontemporal_load(p.w.sc + b0 + second);
        return w;
    };

    // (1) the ring: the wave's first Q8S_DEPTH steps are requested before the rows are staged.  The wave's steps in order: its steps of tile blockIdx.x, then of the
    // next tile of the walk, ...; (lt, ls) = the next step to request, n_load = steps not requested yet
    WB8 ring[Q8S_DEPTH];
    int lt = blockIdx.x, ls = s_lo, n_load = my_tiles * nst, n_left = n_load;
    const auto request = [&](WB8& slot) { slot = wload(lt, ls); if (++ls == s_hi) { ls = s_lo; lt += G; } n_load--; };
#pragma unroll
    for (int u = 0; u < Q8S_DEPTH; u++) { ring[u].q = u32x4{0u, 0u, 0u, 0u}; ring[u].s0 = ring[u].s1 = 0; if (u < n_left) request(ring[u]); }

    // (2) stage the slice of the rows: piece i = 4 consecutive elements; 8 consecutive lanes hold one block (to_digits' DPP steps stay inside them; 4 npp is a
    // multiple of 64, so whole waves run the loop), rows M..3 and the pad block are zeros -> zero planes
    const int npp = nbp * 8, npieces = nbs * 8;
    float ss[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < 4 * npp; i += Q8S_THREADS) {
        const int r = i / npp, pc = i - r * npp;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < M && pc < npieces) v = *reinterpret_cast<const float4*>(p.x + (size_t)r * p.x_stride + 32 * zb0 + 4 * pc);
        if (PRO == PRO_RMS) {
            const float q = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
#pragma unroll
            for (int rr = 0; rr < 4; rr++) ss[rr] += r == rr ? q : 0.f;
            if (pc < npieces) { const float4 gm = *reinterpret_cast<const float4*>(p.gamma + 32 * zb0 + 4 * pc); v.x *= gm.x; v.y *= gm.y; v.z *= gm.z; v.w *= gm.w; }
        }
        const float vv[4] = {v.x, v.y, v.z, v.w};
        to_digits(vv, lane, planes + ((size_t)r * nbp + (pc >> 3)) * 128, binfo + r * nbp + (pc >> 3));
    }
    if (PRO == PRO_RMS) {      // the slice's sum of squares per row in a fixed order: the thread's pieces ascending, the wave's DPP tree, the waves ascending (below)
#pragma unroll
        for (int rr = 0; rr < 4; rr++) { const float w = wave_sum_e(ss[rr]); if (lane == 0) ssq_s[wave * 4 + rr] = w; }
    }
    __syncthreads();

    // (3) the product
    int par = 0;
    if (wave == Q8S_WAVES) {      // the storing wave: per tile, the eight partials added in one fixed order -> the slice's plane.  Lane (n, g) = row g, column 16 t + n
        if (PRO == PRO_RMS && blockIdx.x == 0 && lane < M) {      // every workgroup of the slice holds the same sums of squares: the first one stores them
            float a = 0.f;
#pragma unroll
            for (int w = 0; w <= Q8S_WAVES; w++) a += ssq_s[w * 4 + lane];
            ssq_out[z * 4 + lane] = a;
        }
        for (int t = blockIdx.x; t < tiles; t += G) {
            __syncthreads();      // (the other area is free again: this wave read it before it arrived here)
            const float* rd = red + par * (Q8S_WAVES * 64);
            par ^= 1;
            if (g < M)
                planes_out[((size_t)z * 4 + g) * N + 16 * t + n] = ((rd[lane] + rd[64 + lane]) + (rd[128 + lane] + rd[192 + lane])) + ((rd[256 + lane] + rd[320 + lane]) + (rd[384 + lane] + rd[448 + lane]));
        }
        return;
    }
    if (nst == 0) {      // a wave without steps (a short slice): +0 into every tile's sum, the same barriers as the others
        for (int j = 0; j < my_tiles; j++) { red[par * (Q8S_WAVES * 64) + wave * 64 + lane] = 0.f; __syncthreads(); par ^= 1; }
        return;
    }
    const unsigned char* a_base = planes + (size_t)(n >> 2) * nbp * 128 + ((n & 3) * 2 + h) * 16;
    const float2* bi_base = binfo + g * nbp;
    int cs = s_lo;      // the step being consumed
    float acc = 0.f;
    const auto consume = [&](const WB8& cur) {
        const i4v X = *reinterpret_cast<const i4v*>(a_base + (size_t)(2 * cs + pb) * 128);
        const i4v zz = i4v{0, 0, 0, 0}, A0 = g < 2 ? X : zz, A1 = g < 2 ? zz : X;
        const i4v B = i4v{(int)cur.q.x, (int)cur.q.y, (int)cur.q.z, (int)cur.q.w};
        const i4v D0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A0, B, zz, 0, 0, 0), D1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B, zz, 0, 0, 0);
        const float sx0 = bi_base[2 * cs].y, sx1 = bi_base[2 * cs + 1].y;
        acc = q8_digits_finish(D0, f16_bits_f32(cur.s0), sx0, acc);      // fixed order: the wave's blocks ascending
        acc = q8_digits_finish(D1, 2 * cs + 1 < nbs ? f16_bits_f32(cur.s1) : 0.f, sx1, acc);      // (the pad block: zero planes, D1 = 0, and no scale)
        if (++cs < s_hi) return;
        red[par * (Q8S_WAVES * 64) + wave * 64 + lane] = acc;      // the wave's last step of the tile: its partial meets the others', the storing wave takes them
        __syncthreads();
        par ^= 1;
        acc = 0.f; cs = s_lo;
    };
    // steady state: every step consumed puts the step Q8S_DEPTH ahead in flight, INTO the registers it was consumed from (requested first, the new value would
    // need registers of its own and the compiler would move it, freshly loaded, at the loop's end: a wait for the whole ring)
    while (n_load >= Q8S_DEPTH) {
#pragma unroll
        for (int u = 0; u < Q8S_DEPTH; u++) { consume(ring[u]); request(ring[u]); }
        n_left -= Q8S_DEPTH;
    }
    // drain: n_left <= 2 Q8S_DEPTH - 1 steps, n_load < Q8S_DEPTH of them not requested yet
#pragma unroll
    for (int u = 0; u < Q8S_DEPTH; u++) {
        if (u < n_left) { consume(ring[u]); if (n_load > 0) request(ring[u]); }
    }
    n_left -= Q8S_DEPTH;
#pragma unroll
    for (int u = 0; u < Q8S_DEPTH; u++) {
        if (u < n_left) consume(ring[u]);
    }
}

template <int PRO, int EPI>
__global__ __launch_bounds__(256) void q8_slice_finish_kernel(const Q8SliceParams p, const float* __restrict__ planes, const float* __restrict__ ssq, int slices) {
    const int N = p.w.N, No = EPI == EPI_SWIGLU ? N >> 1 : N;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)p.M * No) return;
    const int m = (int)(i / No), c = (int)(i - (long)m * No);
    float rstd = 1.0f;
    if (PRO == PRO_RMS) {
        float a = ssq[m];
        for (int z = 1; z < slices; z++) a += ssq[z * 4 + m];
        rstd = 1.0f / sqrtf(a / (float)p.w.K + p.eps);
    }
    const auto column = [&](int col) {      // the slices ascending, then rstd, then the bias
        const float* pl = planes + (size_t)m * N + col;
        float v = pl[0];
        for (int z = 1; z < slices; z++) v += pl[(size_t)z * 4 * N];
        if (PRO == PRO_RMS) v *= rstd;
        if (p.bias) v += p.bias[col];
        return v;
    };
    if (EPI == EPI_SWIGLU) {      // interleaved rows: 2 c gate, 2 c + 1 up
        const float gate = column(2 * c), up = column(2 * c + 1);
        p.out[(size_t)m * p.out_stride + c] = silu_e(gate) * up;
    } else {
        float v = column(c);
        if (EPI == EPI_GELU) v = gelu_q8s(v);
        if (EPI == EPI_RESID) v = v + p.resid[(size_t)m * p.resid_stride + c];
        p.out[(size_t)m * p.out_stride + c] = v;
    }
}

std::atomic<unsigned long long> g_q8_slices_launches{0};

template <int PRO, int EPI>
hipError_t q8_slices_launch_t(const Q8SliceParams& p, float* planes, hipStream_t s) {
    const int slices = q8s_slices(p.w.K), No = EPI == EPI_SWIGLU ? p.w.N / 2 : p.w.N;
    float* ssq = planes + (size_t)slices * 4 * p.w.N;
    q8_slice_kernel<PRO><<<dim3(q8s_grid_x(p.w.N, p.w.K), slices), dim3(Q8S_THREADS), q8s_lds_bytes(p.w.nb < Q8S_BLOCKS ? p.w.nb : Q8S_BLOCKS), s>>>(p, planes, ssq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    q8_slice_finish_kernel<PRO, EPI><<<dim3((unsigned)(((long)p.M * No + 255) / 256)), dim3(256), 0, s>>>(p, planes, ssq, slices);
    e = hipGetLastError();
    if (e == hipSuccess) g_q8_slices_launches.fetch_add(1, std::memory_order_relaxed);      // operator calls so far: one that failed is not counted
    return e;
}

}  // namespace

bool q8_slices_serves(const Q4W& w, int M, int pro, int epi) {
    return w.fmt == WFMT_Q8_0 && w.qs && w.sc && M >= 1 && M <= 4 && w.K >= 32 && w.K % 32 == 0 && w.K <= Q8S_MAX_K && w.nb == w.K / 32 && w.N >= 16 && w.N % 16 == 0 &&
           (pro == PRO_NONE || pro == PRO_RMS) && (epi == EPI_STORE || epi == EPI_RESID || epi == EPI_SWIGLU || epi == EPI_GELU);
}
size_t q8_slices_planes_bytes(const Q4W& w) { const size_t slices = (size_t)q8s_slices(w.K); return slices * 4 * (size_t)w.N * 4 + slices * 4 * 4; }
unsigned long long q8_slices_launches() { return g_q8_slices_launches.load(std::memory_order_relaxed); }

hipError_t launch_q8_slices(const Q8SliceParams& p, int pro, int epi, float* planes, size_t planes_bytes, hipStream_t s) {
    if (!q8_slices_serves(p.w, p.M, pro, epi) || !p.x || !p.out) return hipErrorInvalidValue;
    if ((p.x_stride & 3) || ((uintptr_t)p.x & 15) || p.x_stride < p.w.K) return hipErrorInvalidValue;      // the rows are read as float4
    if (pro == PRO_RMS && (!p.gamma || ((uintptr_t)p.gamma & 15) || !(p.eps > 0.f))) return hipErrorInvalidValue;
    if (epi == EPI_RESID && !p.resid) return hipErrorInvalidValue;
    if (!planes || ((uintptr_t)planes & 3) || planes_bytes < q8_slices_planes_bytes(p.w)) return hipErrorInvalidValue;
#define VOX_Q8S(P_, E_) if (pro == P_ && epi == E_) return q8_slices_launch_t<P_, E_>(p, planes, s);
    VOX_Q8S(PRO_NONE, EPI_STORE) VOX_Q8S(PRO_NONE, EPI_RESID) VOX_Q8S(PRO_NONE, EPI_SWIGLU) VOX_Q8S(PRO_NONE, EPI_GELU)
    VOX_Q8S(PRO_RMS, EPI_STORE) VOX_Q8S(PRO_RMS, EPI_RESID) VOX_Q8S(PRO_RMS, EPI_SWIGLU) VOX_Q8S(PRO_RMS, EPI_GELU)
#undef VOX_Q8S
    return hipErrorInvalidValue;
}

}  // namespace vox
