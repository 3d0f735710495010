// vox_q8_common.h -- what the Q8_0 units on the int8 matrix core share (vox_q8.hip: q8_rows_kernel; vox_q8_slices.hip: q8_slice_kernel): one lane's share of a K step,
// the f16 scale widening and the exact finish of a block's digit sums.  Included behind vox_engine_common.h and vox_digits.h (u32x4, i4v) and <hip/hip_fp16.h>,
// inside `namespace vox { namespace {` of each translation unit.
#pragma once

__device__ __forceinline__ float f16_bits_f32(unsigned short h) { return __half2float(__ushort_as_half(h)); }

struct WB8 { u32x4 q; unsigned short s0, s1; };      // one lane's share of a K step: 16 int8 values, the f16 scales of the step's two blocks of its weight row

// digit sums of one block -> value: D0 + 2^7 D1 and D2 + 2^7 D3 in int32 (|D| < 2^20), their 39-bit combination in f64 (exact), ONE rounding to f32, one FMA
// with the product of the weight block's scale and the activation block's 2^-shift
__device__ __forceinline__ float q8_digits_finish(const i4v D, float sc, float sxinv, float acc) {
    const int lo = (int)((unsigned)D[0] + ((unsigned)D[1] << 7)), hi = (int)((unsigned)D[2] + ((unsigned)D[3] << 7));
    const float t = (float)fma((double)hi, 16384.0, (double)lo);
    return fmaf(t, sc * sxinv, acc);
}
