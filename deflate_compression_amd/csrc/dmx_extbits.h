// First mismatch of W word pairs (ext_len2's rounds in dmx_kernels.hip), as host and device
// code: the device takes v_ffbl_b32 as the hardware defines it, the host a plain ctz, so the
// arithmetic can be checked against a byte loop in a stand-alone host program
// (tests/c/ext_rounds_model.cpp).
#ifndef DMX_EXTBITS_H
#define DMX_EXTBITS_H
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_HD __host__ __device__ __forceinline__
#else
#define DMX_HD static inline
#endif

// lowest set bit, ~0 for 0.  On the device the instruction is opaque to the optimizer, so it
// does not re-derive the zero case with compares and selects.
DMX_HD uint32_t dmx_ffbl(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
#else
    return x ? (uint32_t)__builtin_ctz(x) : 0xFFFFFFFFu;
#endif
}
DMX_HD uint32_t dmx_add_sat(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_elementwise_add_sat(a, b);   // v_add_u32 clamp
#else
    const uint32_t s = a + b;
    return s < a ? 0xFFFFFFFFu : s;
#endif
}
DMX_HD uint32_t dmx_minu(uint32_t a, uint32_t b) { return a < b ? a : b; }

// x[t] = xor of word t of the two sides.  Returns the bit index of the first differing bit of
// the 4 W bytes (so >> 3 is the count of equal leading bytes: 4 t0 + ctz(x[t0]) / 8 for the
// first non-zero word t0), or ~0 when all W words are equal: ffbl(0) = ~0 and the saturating
// add keeps it there.  W ffbl, W - 1 adds, the mins pair into v_min3_u32.
template <int W>
DMX_HD uint32_t dmx_first_diff_bit(const uint32_t (&x)[W]) {
    uint32_t m = dmx_ffbl(x[0]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 1; t < W; t++) m = dmx_minu(m, dmx_add_sat(dmx_ffbl(x[t]), 32u * (uint32_t)t));
    return m;
}
#endif
