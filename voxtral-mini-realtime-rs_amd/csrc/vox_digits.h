// vox_digits.h -- the fixed-point digit arithmetic of the int8 matrix core, shared by the decode engine (vox_engine.hip) and the four-row operator (vox_rows4.hip).
// An activation block of 32 elements is held as a power-of-two scale 2^shift (block maximum < 2^26 after scaling), x_int = rint(x * 2^shift) =
// d0 + 128 d1 + 128^2 d2 + 128^3 d3 (d0..d2 in 0..127, d3 signed) and the block info {-8 * sum(x_int), 2^-shift}.  A v_mfma_i32_16x16x64_i8 whose A rows are the
// digit planes of a block and whose B columns are Q4 nibbles as int8 then yields the four digit sums of the block EXACTLY (int32); digits_finish turns them
// into scale * sum_k x[k] * (q[k] - 8).  Included behind vox_engine_common.h (dppf / dppi) inside `namespace vox { namespace {` of each translation unit.
#pragma once

typedef int i4v __attribute__((ext_vector_type(4)));

// Four consecutive elements of a 32-element block (8 consecutive lanes = one block, this lane: elements [4 (lane & 7), +4)) -> digit planes + block info.
// Plane layout of a block (128 bytes): [digit 4][half 2][16 bytes]; half h holds elements 8 h .. 8 h + 7 and 16 + 8 h .. 16 + 8 h + 7, the order of the int8 values
// a lane unpacks from bytes 8 h .. 8 h + 7 of the block's nibbles (low nibbles of the two dwords, then the high ones).
__device__ __forceinline__ void to_digits(const float (&v)[4], int lane, unsigned char* plane_blk, float2* binfo_blk) {
    float mx = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
    mx = fmaxf(mx, dppf<0xB1>(mx)); mx = fmaxf(mx, dppf<0x4E>(mx)); mx = fmaxf(mx, dppf<0x141>(mx));      // over the block's 8 lanes
    int e = __builtin_amdgcn_frexp_expf(mx);          // mx < 2^e (0 for mx == 0)
    e = max(e, -100);
    const float f = ldexpf(1.0f, 26 - e);
    int xi[4];
#pragma unroll
    for (int i = 0; i < 4; i++) xi[i] = (int)rintf(v[i] * f);
    int s = (xi[0] + xi[1]) + (xi[2] + xi[3]);
    s += dppi<0xB1>(s); s += dppi<0x4E>(s); s += dppi<0x141>(s);      // exact: |x_int| <= 2^26, 32 of them
    if ((lane & 7) == 0) *binfo_blk = make_float2(-8.0f * (float)s, ldexpf(1.0f, e - 26));
    const int e0 = 4 * (lane & 7), h = (e0 >> 3) & 1, off = (e0 & 4) + 8 * (e0 >> 4);
#pragma unroll
    for (int cdig = 0; cdig < 4; cdig++) {
        unsigned d = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) { const int dv = cdig < 3 ? (xi[i] >> (7 * cdig)) & 127 : xi[i] >> 21; d |= (unsigned)(dv & 0xFF) << (8 * i); }
        *reinterpret_cast<unsigned*>(plane_blk + (cdig * 2 + h) * 16 + off) = d;
    }
}

// digits -> value: (D0 + 128 D1) and (D2 + 128 D3) exactly in int32 (v_lshl_add_u32; |D| <= 32 * 15 * 128), then one f32 FMA (one rounding), the -8 offset
// (m8sx = -8 * sum(x_int)) and the product of the weight block's scale sc and the activation block's 2^-shift sxinv
__device__ __forceinline__ float digits_finish(const i4v D, float m8sx, float sc, float sxinv, float acc) {
    const int lo = (int)((unsigned)D[0] + ((unsigned)D[1] << 7)), hi = (int)((unsigned)D[2] + ((unsigned)D[3] << 7));
    float t = fmaf((float)hi, 16384.0f, (float)lo);
    t += m8sx;
    return fmaf(t, sc * sxinv, acc);
}
