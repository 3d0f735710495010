// Microbenchmark (not product code), round 3: Q4_0 x f32 dot products on v_mfma_i32_16x16x64_i8 -- EXACT integer products and sums.
// (The fp8 form, tools/micro/mfma_fp8_dot.hip, is fast but its K = 32 accumulation truncates small products next to a large one: 1e-3 errors
// on heavy-tailed activations.)
//   B = the Q4 nibbles as int8 0..15 (and / shift / and: 3 VALU per 8 weights), 16 rows x 64 columns = two Q4_0 blocks per row;
//   A = the activation in FIXED POINT, one power-of-two scale per 32-element block, split into four digits (7 + 7 + 7 + 6 bits, top digit signed):
//       row m = 4 p + c holds digit c of block p (zero in the other block's columns), so D[4 p + c][n] = sum_k digit_c(x_k) * q[n][k] over block p, exactly;
//   epilogue per lane (lane group g = p): Horner over the four digits in f32, minus 8 * sum(x_int), times (block scale of the row) x (2^-shift of the x block).
// Checks the fragment layouts and the accuracy against double precision next to the f32 FMA chain; then the issue rate of the whole per-step stream.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)
typedef int i4 __attribute__((ext_vector_type(4)));

// layout probe: A[m][k] = m + 1 at k = 17 * (m % 4) only... simpler: A[m][k] = (k == m * 4 + 1) ? (m + 1) : 0;  B[k][n] = (k % 16 == n) ? k / 16 + 1 : 0  ->  D[m][n] = sum_k A[m][k] B[k][n]
__global__ void layout_probe(int* out) {
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    i4 A, B;
    for (int w = 0; w < 4; w++) {
        unsigned a = 0, b = 0;
        for (int by = 0; by < 4; by++) {
            const int k = 16 * g + 4 * w + by;
            const int av = (k == n * 4 + 1) ? n + 1 : 0;              // row m = n of A
            const int bv = (k % 16 == n) ? k / 16 + 1 : 0;            // column n of B
            a |= (unsigned)(av & 0xFF) << (8 * by); b |= (unsigned)(bv & 0xFF) << (8 * by);
        }
        A[w] = (int)a; B[w] = (int)b;
    }
    i4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc, 0, 0, 0);
    for (int r = 0; r < 4; r++) out[lane * 4 + r] = acc[r];
}

// one wave: 16 rows x 64 columns.  qs [16 rows][2 blocks][4 dwords], sc [16][2] f16 scales, x [64] floats.  out[row] = sum_p d[row][p] * sum_k x[32 p + k] * (q - 8)
__global__ void mfma_dot(const unsigned* __restrict__ qs, const unsigned short* __restrict__ sc, const float* __restrict__ x, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char planes[2 * 4 * 2 * 16];      // [block p][digit c][half h][16 B]
    __shared__ float sxinv[2]; __shared__ int sxsum[2];
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    // ---- staging (what the all-gather does): lane l < 16 holds elements [4 l, +4): block p = l / 8 ----
    if (lane < 16) {
        const int p = lane >> 3, e0 = 4 * (lane & 7);
        float v[4]; float mx = 0.f;
        for (int i = 0; i < 4; i++) { v[i] = x[32 * p + e0 + i]; mx = fmaxf(mx, fabsf(v[i])); }
        for (int o = 1; o < 8; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));      // block max over its 8 lanes
        int e = 0; (void)frexpf(mx, &e);                                          // mx < 2^e
        e = max(e, -100);
        const float f = ldexpf(1.0f, 26 - e);
        int xi[4], s = 0;
        for (int i = 0; i < 4; i++) { xi[i] = (int)rintf(v[i] * f); s += xi[i]; }
        for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o);
        if ((lane & 7) == 0) { sxinv[p] = ldexpf(1.0f, e - 26); sxsum[p] = s; }
        const int h = (e0 >> 3) & 1, off = (e0 & 4) + 8 * (e0 >> 4);
        for (int c = 0; c < 4; c++) {
            unsigned d = 0;
            for (int i = 0; i < 4; i++) { const int dv = c < 3 ? (xi[i] >> (7 * c)) & 127 : xi[i] >> 21; d |= (unsigned)(dv & 0xFF) << (8 * i); }
            *reinterpret_cast<unsigned*>(planes + ((p * 4 + c) * 2 + h) * 16 + off) = d;
        }
    }
    __syncthreads();
    // ---- A: row m = n: digit c = m & 3 of block p = m >> 2 (m < 8); this lane group covers block g >> 1, half g & 1 ----
    i4 A = {0, 0, 0, 0};
    if (n < 8 && (g >> 1) == (n >> 2)) A = *reinterpret_cast<const i4*>(planes + (((n >> 2) * 4 + (n & 3)) * 2 + (g & 1)) * 16);
    // ---- B: row n, block g >> 1, half g & 1: dwords 2 h, 2 h + 1 -> k-slots [lo(w0) lo(w1) hi(w0) hi(w1)] = elements 8 h .. 8 h + 7, 16 + 8 h .. ----
    const unsigned w0 = qs[(n * 2 + (g >> 1)) * 4 + 2 * (g & 1)], w1 = qs[(n * 2 + (g >> 1)) * 4 + 2 * (g & 1) + 1];
    i4 B; B[0] = (int)(w0 & 0x0F0F0F0Fu); B[1] = (int)(w1 & 0x0F0F0F0Fu); B[2] = (int)((w0 >> 4) & 0x0F0F0F0Fu); B[3] = (int)((w1 >> 4) & 0x0F0F0F0Fu);
    i4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc, 0, 0, 0);      // D[m = 4 g + r][n]: lane group g < 2 holds the four digits of block g
    float v = 0.f;
    if (g < 2) {
        float t = fmaf((float)acc[3], 128.f, (float)acc[2]);
        t = fmaf(t, 128.f, (float)acc[1]);
        t = fmaf(t, 128.f, (float)acc[0]);
        t = fmaf(-8.f, (float)sxsum[g], t);
        v = t * (__half2float(__ushort_as_half(sc[n * 2 + g])) * sxinv[g]);
    }
    v += __shfl(v, lane + 16);      // block 0 + block 1 (lanes g = 0)
    if (g == 0) out[n] = v;
}

// paired form: the same D takes a second MFMA whose A fragment lives in rows 8..15 (zeros in rows 0..7), so rows 0..7 keep the first product and rows 8..15 take the
// second.  Probe: A1[m][k] as above for m < 8, A2[m][k] likewise for m >= 8; B1 as above, B2[k][n] = (k % 16 == n) ? 7 - k / 16 : 0.
__global__ void layout_probe2(int* out) {
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    i4 A1, A2, B1, B2;
    for (int w = 0; w < 4; w++) {
        unsigned a = 0, b1 = 0, b2 = 0;
        for (int by = 0; by < 4; by++) {
            const int k = 16 * g + 4 * w + by;
            const int av = (k == n * 4 + 1) ? n + 1 : 0;
            const int bv1 = (k % 16 == n) ? k / 16 + 1 : 0, bv2 = (k % 16 == n) ? 7 - k / 16 : 0;
            a |= (unsigned)(av & 0xFF) << (8 * by); b1 |= (unsigned)(bv1 & 0xFF) << (8 * by); b2 |= (unsigned)(bv2 & 0xFF) << (8 * by);
        }
        A1[w] = n < 8 ? (int)a : 0; A2[w] = n >= 8 ? (int)a : 0; B1[w] = (int)b1; B2[w] = (int)b2;
    }
    i4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A1, B1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A2, B2, acc, 0, 0, 0);
    for (int r = 0; r < 4; r++) out[lane * 4 + r] = acc[r];
}

// sum over the four lane groups in ONE fixed order, (g0 + g2) + (g1 + g3), valid in lanes 0..15: v_permlane32_swap, v_permlane16_swap and two adds
__device__ __forceinline__ float g4_sum(float v) {
    const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    const float w = __uint_as_float(a[0]) + __uint_as_float(a[1]);
    const auto b = __builtin_amdgcn_permlane16_swap(__float_as_uint(w), __float_as_uint(w), false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// one wave: 16 rows x 128 columns = two K-steps.  qs [16 rows][4 blocks][4 dwords], sc [16][4] f16 scales, x [128] floats.
// PAIRED = false: two single steps chained through acc, block 0 + block 1 by ds_bpermute.  PAIRED = true: both steps in one D, one epilogue, four-group sum.
template <bool PAIRED>
__global__ void mfma_dot2(const unsigned* __restrict__ qs, const unsigned short* __restrict__ sc, const float* __restrict__ x, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned char planes[4 * 4 * 2 * 16];      // [block][digit c][half h][16 B]
    __shared__ float sxinv[4]; __shared__ int sxsum[4];
    const int lane = threadIdx.x, n = lane & 15, g = lane >> 4;
    if (lane < 32) {
        const int p = lane >> 3, e0 = 4 * (lane & 7);
        float v[4]; float mx = 0.f;
        for (int i = 0; i < 4; i++) { v[i] = x[32 * p + e0 + i]; mx = fmaxf(mx, fabsf(v[i])); }
        for (int o = 1; o < 8; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        int e = 0; (void)frexpf(mx, &e);
        e = max(e, -100);
        const float f = ldexpf(1.0f, 26 - e);
        int xi[4], s = 0;
        for (int i = 0; i < 4; i++) { xi[i] = (int)rintf(v[i] * f); s += xi[i]; }
        for (int o = 1; o < 8; o <<= 1) s += __shfl_xor(s, o);
        if ((lane & 7) == 0) { sxinv[p] = ldexpf(1.0f, e - 26); sxsum[p] = s; }
        const int h = (e0 >> 3) & 1, off = (e0 & 4) + 8 * (e0 >> 4);
        for (int c = 0; c < 4; c++) {
            unsigned d = 0;
            for (int i = 0; i < 4; i++) { const int dv = c < 3 ? (xi[i] >> (7 * c)) & 127 : xi[i] >> 21; d |= (unsigned)(dv & 0xFF) << (8 * i); }
            *reinterpret_cast<unsigned*>(planes + ((p * 4 + c) * 2 + h) * 16 + off) = d;
        }
    }
    __syncthreads();
    // B of step s: row n, block 2 s + (g >> 1), half g & 1
    i4 B[2];
    for (int s = 0; s < 2; s++) {
        const unsigned w0 = qs[(n * 4 + 2 * s + (g >> 1)) * 4 + 2 * (g & 1)], w1 = qs[(n * 4 + 2 * s + (g >> 1)) * 4 + 2 * (g & 1) + 1];
        B[s][0] = (int)(w0 & 0x0F0F0F0Fu); B[s][1] = (int)(w1 & 0x0F0F0F0Fu); B[s][2] = (int)((w0 >> 4) & 0x0F0F0F0Fu); B[s][3] = (int)((w1 >> 4) & 0x0F0F0F0Fu);
    }
    float v = 0.f;
    if (!PAIRED) {
        for (int s = 0; s < 2; s++) {
            i4 A = {0, 0, 0, 0};
            if (n < 8 && (g >> 1) == (n >> 2)) A = *reinterpret_cast<const i4*>(planes + (((2 * s + (n >> 2)) * 4 + (n & 3)) * 2 + (g & 1)) * 16);
            i4 acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B[s], acc, 0, 0, 0);
            if (g < 2) {
                const int lo = (int)((unsigned)acc[0] + ((unsigned)acc[1] << 7)), hi = (int)((unsigned)acc[2] + ((unsigned)acc[3] << 7));
                float t = fmaf((float)hi, 16384.0f, (float)lo);
                t += -8.f * (float)sxsum[2 * s + g];
                v = fmaf(t, __half2float(__ushort_as_half(sc[n * 4 + 2 * s + g])) * sxinv[2 * s + g], v);
            }
        }
        v += __shfl(v, (lane + 16) & 63);
    } else {
        // A_lo: rows 0..7 = step 0's digit planes (as above); A_hi: rows 8..15 = step 1's: lanes n >= 8, block p = (n - 8) >> 2, digit n & 3, the same k-group test
        i4 Alo = {0, 0, 0, 0}, Ahi = {0, 0, 0, 0};
        if (n < 8 && (g >> 1) == (n >> 2)) Alo = *reinterpret_cast<const i4*>(planes + (((n >> 2) * 4 + (n & 3)) * 2 + (g & 1)) * 16);
        if (n >= 8 && (g >> 1) == ((n - 8) >> 2)) Ahi = *reinterpret_cast<const i4*>(planes + (((2 + ((n - 8) >> 2)) * 4 + (n & 3)) * 2 + (g & 1)) * 16);
        i4 acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Alo, B[0], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(Ahi, B[1], acc, 0, 0, 0);      // D rows 4 g + r: lane group g holds the four digit sums of block g (of the 128 columns)
        const int lo = (int)((unsigned)acc[0] + ((unsigned)acc[1] << 7)), hi = (int)((unsigned)acc[2] + ((unsigned)acc[3] << 7));
        float t = fmaf((float)hi, 16384.0f, (float)lo);
        t += -8.f * (float)sxsum[g];
        v = g4_sum(t * (__half2float(__ushort_as_half(sc[n * 4 + g])) * sxinv[g]));
    }
    if (g == 0) out[n] = v;
}

// rate: per step = [2 ds_read-free: unpack 6 VALU + MFMA + epilogue 11 VALU], W waves per SIMD
__global__ __launch_bounds__(1024) void mfma_rate(const unsigned* __restrict__ qs, float* __restrict__ out, int iters) {
    const int lane = threadIdx.x & 63;
    unsigned w0 = qs[lane], w1 = qs[(lane + 7) & 63];
    i4 A = {0x01020304, 0x05060708, 0x090a0b0c, 0x0d0e0f10};
    float sum = 0.f, sc = 1.0f + lane * 1e-6f, sx = 3.0f;
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            i4 B; B[0] = (int)(w0 & 0x0F0F0F0Fu); B[1] = (int)(w1 & 0x0F0F0F0Fu); B[2] = (int)((w0 >> 4) & 0x0F0F0F0Fu); B[3] = (int)((w1 >> 4) & 0x0F0F0F0Fu);
            i4 acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc, 0, 0, 0);
            float t = fmaf((float)acc[3], 128.f, (float)acc[2]);
            t = fmaf(t, 128.f, (float)acc[1]);
            t = fmaf(t, 128.f, (float)acc[0]);
            t = fmaf(-8.f, sx, t);
            sum = fmaf(t, sc, sum);
            w0 = w0 * 1664525u + 1013904223u; w1 ^= w0;
        }
    }
    if (sum == 12345.f) out[0] = 1.f;
}

// rate of the paired form: per TWO steps = [2 x unpack 6 VALU + 2 MFMA (the second accumulates into the first's D) + ONE epilogue]
__global__ __launch_bounds__(1024) void mfma_rate2(const unsigned* __restrict__ qs, float* __restrict__ out, int iters) {
    const int lane = threadIdx.x & 63;
    unsigned w0 = qs[lane], w1 = qs[(lane + 7) & 63];
    i4 A = {0x01020304, 0x05060708, 0x090a0b0c, 0x0d0e0f10}, A2 = {0x0d0e0f10, 0x090a0b0c, 0x05060708, 0x01020304};
    float sum = 0.f, sc = 1.0f + lane * 1e-6f, sx = 3.0f;
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 4; u++) {
            i4 B; B[0] = (int)(w0 & 0x0F0F0F0Fu); B[1] = (int)(w1 & 0x0F0F0F0Fu); B[2] = (int)((w0 >> 4) & 0x0F0F0F0Fu); B[3] = (int)((w1 >> 4) & 0x0F0F0F0Fu);
            w0 = w0 * 1664525u + 1013904223u; w1 ^= w0;
            i4 B2; B2[0] = (int)(w0 & 0x0F0F0F0Fu); B2[1] = (int)(w1 & 0x0F0F0F0Fu); B2[2] = (int)((w0 >> 4) & 0x0F0F0F0Fu); B2[3] = (int)((w1 >> 4) & 0x0F0F0F0Fu);
            w0 = w0 * 1664525u + 1013904223u; w1 ^= w0;
            i4 acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A, B, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(A2, B2, acc, 0, 0, 0);
            float t = fmaf((float)acc[3], 128.f, (float)acc[2]);
            t = fmaf(t, 128.f, (float)acc[1]);
            t = fmaf(t, 128.f, (float)acc[0]);
            t = fmaf(-8.f, sx, t);
            sum = fmaf(t, sc, sum);
        }
    }
    if (sum == 12345.f) out[0] = 1.f;
}

int main() {
    {
        int* dp; CHK(hipMalloc(&dp, 1024)); layout_probe<<<1, 64>>>(dp); CHK(hipDeviceSynchronize());
        std::vector<int> o(256); CHK(hipMemcpy(o.data(), dp, 1024, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int l = 0; l < 64; l++) for (int r = 0; r < 4; r++) {
            const int m = 4 * (l >> 4) + r, n = l & 15;
            int want = 0; for (int k = 0; k < 64; k++) want += ((k == m * 4 + 1) ? m + 1 : 0) * ((k % 16 == n) ? k / 16 + 1 : 0);
            bad += o[l * 4 + r] != want;
        }
        printf("i8 16x16x64 layout (A: row lane & 15, k = 16 (lane >> 4) + byte; B likewise by column; D row = 4 (lane >> 4) + reg, col = lane & 15): %s (%d of 256 differ)\n", bad ? "DIFFERENT" : "as assumed", bad);
    }
    {
        int* dp; CHK(hipMalloc(&dp, 1024)); layout_probe2<<<1, 64>>>(dp); CHK(hipDeviceSynchronize());
        std::vector<int> o(256); CHK(hipMemcpy(o.data(), dp, 1024, hipMemcpyDeviceToHost));
        int bad = 0;
        for (int l = 0; l < 64; l++) for (int r = 0; r < 4; r++) {
            const int m = 4 * (l >> 4) + r, n = l & 15;
            int want = 0; for (int k = 0; k < 64; k++) want += ((k == m * 4 + 1) ? m + 1 : 0) * ((k % 16 == n) ? (m < 8 ? k / 16 + 1 : 7 - k / 16) : 0);
            bad += o[l * 4 + r] != want;
        }
        printf("paired: D = mfma(A rows 0..7, B1, 0); D = mfma(A rows 8..15, B2, D): rows 0..7 = A B1, rows 8..15 = A B2: %s (%d of 256 differ)\n", bad ? "DIFFERENT" : "as assumed", bad);
    }
    unsigned* dq; unsigned short* dsc; float* dx; float* dout;
    CHK(hipMalloc(&dq, 16 * 2 * 4 * 4)); CHK(hipMalloc(&dsc, 64)); CHK(hipMalloc(&dx, 256)); CHK(hipMalloc(&dout, 64));
    std::mt19937 rng(7);
    double worst[4] = {0, 0, 0, 0}, mean[4] = {0, 0, 0, 0}, worst_chain = 0, mean_chain = 0; const int trials = 400;
    for (int t = 0; t < trials; t++) {
        std::vector<unsigned> q(128); std::vector<unsigned short> sc(32); std::vector<float> x(64);
        for (auto& v : q) v = rng();
        std::normal_distribution<float> nd(0.f, 1.f);
        for (auto& v : sc) { const __half hh = __float2half(0.01f + 0.02f * std::fabs(nd(rng))); v = *reinterpret_cast<const unsigned short*>(&hh); }
        const int mode = t % 4;      // 0: N(0,1)  1: heavy tail (one 100x outlier)  2: wide dynamic range  3: tiny values next to a big one
        for (int k = 0; k < 64; k++) { float v = nd(rng); if (mode == 2) v *= std::exp2f((float)(rng() % 24) - 12.f); if (mode == 3) v *= 1e-4f; x[k] = v; }
        if (mode == 1 || mode == 3) x[rng() % 64] = 100.f * nd(rng);
        CHK(hipMemcpy(dq, q.data(), 512, hipMemcpyHostToDevice)); CHK(hipMemcpy(dsc, sc.data(), 64, hipMemcpyHostToDevice)); CHK(hipMemcpy(dx, x.data(), 256, hipMemcpyHostToDevice));
        mfma_dot<<<1, 64>>>(dq, dsc, dx, dout);
        CHK(hipDeviceSynchronize());
        std::vector<float> o(16); CHK(hipMemcpy(o.data(), dout, 64, hipMemcpyDeviceToHost));
        for (int n = 0; n < 16; n++) {
            double ex = 0, mag = 0; float ch = 0.f;
            for (int p = 0; p < 2; p++) {
                const __half hh = *reinterpret_cast<const __half*>(&sc[n * 2 + p]); const float d = __half2float(hh);
                float cb = 0.f;
                for (int k = 0; k < 32; k++) {
                    const int dd = (k & 15) >> 2, b = k & 3; const unsigned w = q[(n * 2 + p) * 4 + dd];
                    const int qv = (k < 16 ? (w >> (8 * b)) & 15 : (w >> (8 * b + 4)) & 15) - 8;
                    ex += (double)d * x[32 * p + k] * qv; mag += std::fabs((double)d * x[32 * p + k] * qv); cb = fmaf(x[32 * p + k], (float)qv, cb);
                }
                ch = fmaf(d, cb, ch);
            }
            const double em = std::fabs(o[n] - ex) / mag, ec = std::fabs(ch - ex) / mag;
            worst[mode] = std::max(worst[mode], em); mean[mode] += em / (trials / 4 * 16); worst_chain = std::max(worst_chain, ec); mean_chain += ec / (trials * 16);
        }
    }
    printf("error / sum |d x (q - 8)|, max (mean) per input mode: N(0,1) %.2e (%.2e) | outlier %.2e (%.2e) | wide range %.2e (%.2e) | tiny+big %.2e (%.2e)   [f32 FMA chain: max %.2e mean %.2e]\n",
           worst[0], mean[0], worst[1], mean[1], worst[2], mean[2], worst[3], mean[3], worst_chain, mean_chain);
    for (int wps : {1, 2, 3, 4}) {
        hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
        const int iters = 2000;
        mfma_rate<<<256, 256 * wps>>>(dq, dout, 10);
        CHK(hipEventRecord(e0)); mfma_rate<<<256, 256 * wps>>>(dq, dout, iters); CHK(hipEventRecord(e1)); CHK(hipDeviceSynchronize());
        float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
        const double ns = ms * 1e6 / (iters * 8.0 * wps);
        printf("rate: %d waves/SIMD: %.2f ns per step per SIMD (MFMA 16x16x64 i8 + 6 unpack + 9 epilogue + 3 LCG VALU); 1024 weights per step -> %.1f TB/s of Q4 bytes chip-wide\n", wps, ns, 1024.0 * 1024 * 0.5625 / ns / 1e3);
    }
    {   // 16 rows x 128 columns: two single steps against one paired step, both against double
        unsigned* dq2; unsigned short* dsc2; float* dx2;
        CHK(hipMalloc(&dq2, 16 * 4 * 4 * 4)); CHK(hipMalloc(&dsc2, 128)); CHK(hipMalloc(&dx2, 512));
        std::mt19937 rng2(11);
        double w2[2][4] = {{0}}, m2[2][4] = {{0}}; int differ = 0;
        for (int t = 0; t < trials; t++) {
            std::vector<unsigned> q(256); std::vector<unsigned short> sc(64); std::vector<float> x(128);
            for (auto& v : q) v = rng2();
            std::normal_distribution<float> nd(0.f, 1.f);
            const int mode = t % 4;
            for (int i = 0; i < 64; i++) {
                float d = 0.01f + 0.02f * std::fabs(nd(rng2));
                if (mode == 1 && rng2() % 8 == 0) d *= 30.f;      // outlier block scales: a scale taken from the wrong lane group's block shows at once
                const __half hh = __float2half(d); sc[i] = *reinterpret_cast<const unsigned short*>(&hh);
            }
            for (int k = 0; k < 128; k++) { float v = nd(rng2); if (mode == 2) v *= std::exp2f((float)(rng2() % 24) - 12.f); if (mode == 3) v *= 1e-4f; x[k] = v; }
            if (mode == 1 || mode == 3) x[rng2() % 128] = 100.f * nd(rng2);
            CHK(hipMemcpy(dq2, q.data(), 1024, hipMemcpyHostToDevice)); CHK(hipMemcpy(dsc2, sc.data(), 128, hipMemcpyHostToDevice)); CHK(hipMemcpy(dx2, x.data(), 512, hipMemcpyHostToDevice));
            std::vector<float> o[2] = {std::vector<float>(16), std::vector<float>(16)};
            mfma_dot2<false><<<1, 64>>>(dq2, dsc2, dx2, dout); CHK(hipDeviceSynchronize()); CHK(hipMemcpy(o[0].data(), dout, 64, hipMemcpyDeviceToHost));
            mfma_dot2<true><<<1, 64>>>(dq2, dsc2, dx2, dout); CHK(hipDeviceSynchronize()); CHK(hipMemcpy(o[1].data(), dout, 64, hipMemcpyDeviceToHost));
            for (int n = 0; n < 16; n++) {
                double ex = 0, mag = 0;
                for (int p = 0; p < 4; p++) {
                    const __half hh = *reinterpret_cast<const __half*>(&sc[n * 4 + p]); const float d = __half2float(hh);
                    for (int k = 0; k < 32; k++) {
                        const int dd = (k & 15) >> 2, b = k & 3; const unsigned w = q[(n * 4 + p) * 4 + dd];
                        const int qv = (k < 16 ? (w >> (8 * b)) & 15 : (w >> (8 * b + 4)) & 15) - 8;
                        ex += (double)d * x[32 * p + k] * qv; mag += std::fabs((double)d * x[32 * p + k] * qv);
                    }
                }
                for (int f = 0; f < 2; f++) { const double em = std::fabs(o[f][n] - ex) / mag; w2[f][mode] = std::max(w2[f][mode], em); m2[f][mode] += em / (trials / 4 * 16); }
                differ += o[0][n] != o[1][n];
            }
        }
        for (int f = 0; f < 2; f++)
            printf("128 columns, %s: error / sum |d x (q - 8)|, max (mean): N(0,1) %.2e (%.2e) | outlier x and block scales %.2e (%.2e) | wide range %.2e (%.2e) | tiny+big %.2e (%.2e)\n",
                   f ? "ONE PAIRED step (four-group sum)" : "two single steps (chained)      ", w2[f][0], m2[f][0], w2[f][1], m2[f][1], w2[f][2], m2[f][2], w2[f][3], m2[f][3]);
        printf("paired and single results differ in the last bits (f32 summation order only) in %d of %d rows\n", differ, trials * 16);
    }
    for (int wps : {1, 2, 3, 4}) {
        hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
        const int iters = 2000;
        mfma_rate2<<<256, 256 * wps>>>(dq, dout, 10);
        CHK(hipEventRecord(e0)); mfma_rate2<<<256, 256 * wps>>>(dq, dout, iters); CHK(hipEventRecord(e1)); CHK(hipDeviceSynchronize());
        float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
        const double ns = ms * 1e6 / (iters * 8.0 * wps);
        printf("rate, PAIRED: %d waves/SIMD: %.2f ns per step per SIMD (per two steps: 2 MFMA chained on one D + 2 x 6 unpack + 9 epilogue + 2 x 3 LCG VALU)\n", wps, ns);
    }
    return 0;
}
