/* dmx_crc.h -- CRC-32 (IEEE 802.3 / RFC 1952 §8) arithmetic shared by the host code and the
 * CRC kernels (dmx_crc.hip).  Reflected representation: bit 31 of a word is the coefficient
 * of x^0, bit 0 that of x^31; P = 0xEDB88320 (x^32 left implicit).
 *
 * The raw remainder R(M) = M(x) x^32 mod P (register started at 0, no final xor) is linear:
 *     R(A || B) = R(A) x^(8 |B|)  xor  R(B),         R(0...0 || M) = R(M),
 * and the check value of an n-byte message is the affine map
 *     crc(M) = R(M)  xor  0xFFFFFFFF x^(8 n)  xor  0xFFFFFFFF.
 * Internal (C, C++ and HIP). */
#ifndef DMX_CRC_H
#define DMX_CRC_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define DMX_CRC_HD __host__ __device__
#else
#define DMX_CRC_HD
#endif

#define DMX_CRC_POLY 0xEDB88320u
#define DMX_CRC_ONE 0x80000000u /* x^0 */

/* a(x) b(x) mod P: 32 shift/xor steps, branch-free */
static inline DMX_CRC_HD uint32_t dmx_gf2_mulmod(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= (0u - ((a >> i) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & DMX_CRC_POLY);
    }
    return p;
}

/* x^(n 2^k) mod P by square-and-multiply (k = 3: x^(8 n), the shift of n bytes) */
static inline DMX_CRC_HD uint32_t dmx_gf2_xpow(uint64_t n, unsigned k) {
    uint32_t base = DMX_CRC_ONE >> 1; /* x^1 */
    while (k--) base = dmx_gf2_mulmod(base, base);
    uint32_t p = DMX_CRC_ONE;
    while (n) {
        if (n & 1) p = dmx_gf2_mulmod(p, base);
        n >>= 1;
        if (n) base = dmx_gf2_mulmod(base, base);
    }
    return p;
}

/* x^(-8 n) mod P: x has order 2^32 - 1 in GF(2)[x] / P (P is primitive) */
static inline DMX_CRC_HD uint32_t dmx_gf2_xpow_neg_bytes(uint64_t n) {
    const uint64_t ord = 0xFFFFFFFFull;
    const uint64_t e = ((n % ord) * 8) % ord;
    return dmx_gf2_xpow(e ? ord - e : 0, 0);
}

/* the affine term of an n-byte message: 0xFFFFFFFF x^(8 n) xor 0xFFFFFFFF */
static inline DMX_CRC_HD uint32_t dmx_crc32_affine(uint64_t n) {
    return dmx_gf2_mulmod(0xFFFFFFFFu, dmx_gf2_xpow(n, 3)) ^ 0xFFFFFFFFu;
}

#ifdef __cplusplus
extern "C" {
#endif
/* host CRC-32 of a buffer, continuing from crc (0 to start), as zlib's crc32() (dmx_inflate.c) */
uint32_t dmx_crc32_host(uint32_t crc, const uint8_t* d, uint64_t n);
#ifdef __cplusplus
}
#endif

#endif
