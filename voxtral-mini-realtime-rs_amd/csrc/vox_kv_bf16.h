// The K / V pool element of a bf16 paged stream group (vox_stream_group_create_kv, VOX_KV_BF16; DESIGN.md section 8, "A bf16 K/V pool"): the ONE f32 -> bf16
// rounding of the project's caches and its inverse.  The q|k|v epilogue's append, the seed of a member's first pages, the restore of a session blob and the host
// entry vox_kv_round_bf16 all call kv_bf16_round: the bits below are the contract, whatever instruction the compiler picks for them.
//   finite      round to nearest, ties to even, on the upper 16 bits: (u + 0x7fff + ((u >> 16) & 1)) >> 16.  A value that rounds past the largest finite becomes inf
//               (the carry runs into the exponent); the sign of zero and denormals are kept (a denormal rounds like any other value, possibly to zero or to the
//               smallest normal)
//   inf         itself
//   NaN         a quiet NaN: the upper 16 bits with the quiet bit set (the payload's low bits could otherwise round it into inf)
// Widening is u << 16: exact, every bf16 value is an f32 value.
#pragma once
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VOX_KV_HD __host__ __device__ __forceinline__
#else
#define VOX_KV_HD inline
#endif

namespace vox {

VOX_KV_HD uint16_t kv_bf16_round_bits(uint32_t u) {
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x0040u);      // NaN stays NaN, quiet
    return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
VOX_KV_HD uint16_t kv_bf16_round(float x) {
    uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(x);
#else
    memcpy(&u, &x, 4);
#endif
    return kv_bf16_round_bits(u);
}
VOX_KV_HD float kv_bf16_widen(uint16_t h) {
    const uint32_t u = (uint32_t)h << 16;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float x; memcpy(&x, &u, 4); return x;
#endif
}

}  // namespace vox
