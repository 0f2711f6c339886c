// dmx_crc.hip -- CRC-32 (RFC 1952 §8) of a device buffer, the check value of the gzip
// container (DMX_F_GZIP) and of PNG chunks.  Two launches, no allocation, no host
// synchronisation (graph-capturable, as the encode):
//
//   dmx_crc_span_kernel   the input, extended by zero bytes in front down to a 16-byte
//                         boundary and behind up to a whole span, is cut into spans of CRC_S
//                         bytes.  A workgroup stages a span in LDS with coalesced 16-byte
//                         loads; lane j then runs a slice-by-16 table CRC (tables in LDS) over
//                         its own CRC_L contiguous bytes, multiplies its raw remainder by the
//                         fixed x^(8 CRC_L (CRC_T - 1 - j)) and the workgroup xors the
//                         products: the span's raw remainder, 4 bytes per span.  Workgroups
//                         stride over the spans so the tables are loaded once per workgroup.
//   dmx_crc_fold_kernel   one workgroup: Horner over the span remainders with x^(8 CRC_S), then
//                         the padding behind is divided out (x^-(8 Z): x is invertible mod P)
//                         and the affine term of init / final xor is added (dmx_crc.h).
//
// Zero bytes in front leave a raw remainder unchanged, so an unaligned base needs no special
// case; the constants that depend on n (x^-(8 Z), the affine term, the fold's chunk shift) are
// computed on the host at launch, by square-and-multiply.
// Included by dmx_kernels.hip (its host section): not a translation unit of its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dmx_crc.h"
#include "dmx_ctx.h"

#define CRC_T 256                 // lanes per workgroup
#define CRC_L 128                 // bytes per lane slice
#define CRC_S (CRC_T * CRC_L)     // bytes per span (32 KiB)
#define CRC_NS 16                 // slice-by-16: 16 independent lookups per 16 input bytes
#define CRC_ROW (CRC_L / 4 + 4)   // LDS words per staged slice: +4 skews the lanes' ds_read_b128
                                  // over all 64 banks (36 j mod 64 is distinct for 16 lanes)
#define CRC_Q (CRC_S / 16 / CRC_T)   // 16-byte loads per thread and span
#define CRC_FT 1024               // fold kernel threads
static_assert(CRC_S == DMX_BLK, "the context reserves one remainder per DMX_BLK bytes");
static_assert(CRC_L % 16 == 0 && (CRC_ROW * 4) % 16 == 0, "16-byte staging stores");

struct CrcTables {
    uint32_t t[CRC_NS][256];   // t[k][b]: byte b followed by k zero bytes, raw remainder
    uint32_t lane[CRC_T];      // x^(8 CRC_L (CRC_T - 1 - j))
};
static constexpr uint32_t crc_cmul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 31; i >= 0; i--) {
        p ^= (0u - ((a >> i) & 1u)) & b;
        b = (b >> 1) ^ ((0u - (b & 1u)) & DMX_CRC_POLY);
    }
    return p;
}
static constexpr CrcTables crc_make_tables() {
    CrcTables T = {};
    for (uint32_t b = 0; b < 256; b++) {
        uint32_t c = b;
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ ((0u - (c & 1u)) & DMX_CRC_POLY);
        T.t[0][b] = c;
    }
    for (int k = 1; k < CRC_NS; k++)
        for (uint32_t b = 0; b < 256; b++) T.t[k][b] = (T.t[k - 1][b] >> 8) ^ T.t[0][T.t[k - 1][b] & 0xFFu];
    uint32_t xl = DMX_CRC_ONE >> 1;   // x -> x^(8 CRC_L) by squaring (CRC_L is a power of two)
    for (uint32_t e = 1; e < 8u * CRC_L; e <<= 1) xl = crc_cmul(xl, xl);
    static_assert((CRC_L & (CRC_L - 1)) == 0, "CRC_L: a power of two");
    uint32_t p = DMX_CRC_ONE;
    for (int j = CRC_T - 1; j >= 0; j--) { T.lane[j] = p; p = crc_cmul(p, xl); }
    return T;
}
__device__ const CrcTables g_crc = crc_make_tables();
static constexpr uint32_t crc_xspan() {   // x^(8 CRC_S)
    uint32_t x = DMX_CRC_ONE >> 1;
    for (uint64_t e = 1; e < 8ull * CRC_S; e <<= 1) x = crc_cmul(x, x);
    return x;
}
static_assert((CRC_S & (CRC_S - 1)) == 0, "CRC_S: a power of two");

// the 16 bytes at byte offset g of the padded message [0, lo) zeros, [lo, hi) data, zeros after
__device__ __forceinline__ uint4 crc_load16(const uint8_t* __restrict__ base, uint64_t g, uint64_t lo, uint64_t hi) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (g + 16 <= lo || g >= hi) return v;   // no byte of the input: nothing is read
    v = *reinterpret_cast<const uint4*>(base + g);   // 16-byte aligned, shares a byte with the input
    if (g < lo || g + 16 > hi) {
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            uint32_t m = 0;
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint64_t q = g + 4 * i + k;
                if (q >= lo && q < hi) m |= 0xFFu << (8 * k);
            }
            w[i] &= m;
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

__global__ __launch_bounds__(CRC_T) void dmx_crc_span_kernel(const uint8_t* __restrict__ base, uint64_t lo, uint64_t hi,
                                                             uint32_t nspan, uint32_t* __restrict__ rem) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[CRC_NS * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage[CRC_T * CRC_ROW];
    __shared__ uint32_t wred[CRC_T / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < CRC_NS * 256; i += CRC_T) tab[i] = (&g_crc.t[0][0])[i];
    const uint32_t klane = g_crc.lane[tid];
    uint4 v[CRC_Q];
    uint32_t s = blockIdx.x;
    if (s < nspan) {
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++)
            v[i] = crc_load16(base, (uint64_t)s * CRC_S + 16ull * (tid + CRC_T * i), lo, hi);
    }
    for (; s < nspan; s += gridDim.x) {
        // chunk q = tid + CRC_T i of the span belongs to slice q / (CRC_L / 16)
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) {
            const uint32_t q = tid + CRC_T * i;
            *reinterpret_cast<uint4*>(&stage[(q / (CRC_L / 16)) * CRC_ROW + 4 * (q % (CRC_L / 16))]) = v[i];
        }
        __syncthreads();   // (and the tables, the first time)
        const uint32_t sn = s + gridDim.x;
        if (sn < nspan) {   // the next span's loads fly during this one's lookups
#pragma unroll
            for (uint32_t i = 0; i < CRC_Q; i++)
                v[i] = crc_load16(base, (uint64_t)sn * CRC_S + 16ull * (tid + CRC_T * i), lo, hi);
        }
        uint32_t c = 0;
        const uint4* p = reinterpret_cast<const uint4*>(&stage[tid * CRC_ROW]);
#pragma unroll
        for (uint32_t k = 0; k < CRC_L / 16; k++) {
            const uint4 d = p[k];
            const uint32_t x = d.x ^ c;
            c = tab[15 * 256 + (x & 0xFFu)] ^ tab[14 * 256 + ((x >> 8) & 0xFFu)] ^ tab[13 * 256 + ((x >> 16) & 0xFFu)] ^
                tab[12 * 256 + (x >> 24)] ^
                tab[11 * 256 + (d.y & 0xFFu)] ^ tab[10 * 256 + ((d.y >> 8) & 0xFFu)] ^ tab[9 * 256 + ((d.y >> 16) & 0xFFu)] ^
                tab[8 * 256 + (d.y >> 24)] ^
                tab[7 * 256 + (d.z & 0xFFu)] ^ tab[6 * 256 + ((d.z >> 8) & 0xFFu)] ^ tab[5 * 256 + ((d.z >> 16) & 0xFFu)] ^
                tab[4 * 256 + (d.z >> 24)] ^
                tab[3 * 256 + (d.w & 0xFFu)] ^ tab[2 * 256 + ((d.w >> 8) & 0xFFu)] ^ tab[1 * 256 + ((d.w >> 16) & 0xFFu)] ^
                tab[0 * 256 + (d.w >> 24)];
        }
        uint32_t r = dmx_gf2_mulmod(c, klane);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) r ^= __shfl_xor(r, o);
        if ((tid & 63) == 0) wred[tid >> 6] = r;
        __syncthreads();   // (also: every lane has read its slice before the next staging)
        if (tid == 0) {
            uint32_t t = 0;
#pragma unroll
            for (uint32_t w = 0; w < CRC_T / 64; w++) t ^= wred[w];
            rem[s] = t;
        }
    }
}

// rem[0 .. nspan): the spans' raw remainders.  Thread t takes the C spans [t C - z, t C - z + C)
// (z = CRC_FT C - nspan virtual zero remainders in front, so every thread's chunk is whole and
// the shift after thread t is the fixed x^(8 CRC_S C (CRC_FT - 1 - t))); xc = x^(8 CRC_S C).
// *crc = total x^-(8 Z) xor affine.
__global__ __launch_bounds__(CRC_FT) void dmx_crc_fold_kernel(const uint32_t* __restrict__ rem, uint32_t nspan, uint32_t C,
                                                              uint32_t xc, uint32_t unshift, uint32_t affine,
                                                              uint32_t* __restrict__ crc) {
    __shared__ uint32_t wv[CRC_FT / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    constexpr uint32_t XS = crc_xspan();
    const uint64_t z = (uint64_t)CRC_FT * C - nspan;
    uint32_t acc = 0;
    for (uint32_t i = 0; i < C; i++) {
        const uint64_t vi = (uint64_t)tid * C + i;
        if (vi < z) continue;   // (a zero remainder: acc stays 0)
        acc = dmx_gf2_mulmod(acc, XS) ^ rem[vi - z];
    }
    // inclusive scan in the wave: lane 63 ends with sum_j acc_j xc^(63 - j)
    uint32_t xk = xc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(acc, o);
        if (lane >= (uint32_t)o) acc ^= dmx_gf2_mulmod(y, xk);
        xk = dmx_gf2_mulmod(xk, xk);
    }
    if (lane == 63) wv[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;   // xk = xc^64 now
        for (uint32_t w = 0; w < CRC_FT / 64; w++) t = dmx_gf2_mulmod(t, xk) ^ wv[w];
        *crc = dmx_gf2_mulmod(t, unshift) ^ affine;
    }
}

extern "C" void dmx_crc32_geometry(uint32_t* span, uint32_t* lane_slice) {
    if (span) *span = CRC_S;
    if (lane_slice) *lane_slice = CRC_L;
}

// spans of d_in[0..n): the input after the zero bytes down to a 16-byte boundary
static uint64_t dmx_crc32_spans(const void* d_in, uint64_t n) {
    const uint64_t pad = n ? (reinterpret_cast<uintptr_t>(d_in) & 15) : 0;
    return (pad + n + CRC_S - 1) / CRC_S;
}

// the launches of dmx_crc32_async on stream s (dmx_encode_async shares them); the caller has
// checked dmx_crc32_spans(d_in, n) <= c->crc_cap and d_crc.  No span: only the fold kernel, which
// then reads no remainder (c->crc_rem may be NULL).
static int dmx_crc32_launch(dmx_ctx* c, const void* d_in, uint64_t n, uint32_t* d_crc, hipStream_t s) {
    const uint64_t pad = n ? (reinterpret_cast<uintptr_t>(d_in) & 15) : 0;
    const uint64_t nspan64 = dmx_crc32_spans(d_in, n);
    if (nspan64 > c->crc_cap || !d_crc) return -(int)E_SZ;
    const uint32_t nspan = (uint32_t)nspan64;
    if (nspan) {
        const uint32_t gmax = 3 * c->ncu;   // 3 workgroups of 52 KiB LDS per CU
        hipLaunchKernelGGL(dmx_crc_span_kernel, dim3(nspan < gmax ? nspan : gmax), dim3(CRC_T), 0, s,
                           (const uint8_t*)d_in - pad, pad, pad + n, nspan, c->crc_rem);
    }
    const uint32_t C = nspan ? (nspan + CRC_FT - 1) / CRC_FT : 0;
    const uint64_t Z = nspan64 * CRC_S - (pad + n);
    hipLaunchKernelGGL(dmx_crc_fold_kernel, dim3(1), dim3(CRC_FT), 0, s, (const uint32_t*)c->crc_rem, nspan, C,
                       dmx_gf2_xpow((uint64_t)C * CRC_S, 3), dmx_gf2_xpow_neg_bytes(Z), dmx_crc32_affine(n), d_crc);
    return 0;
}

extern "C" int dmx_crc32_async(dmx_ctx* c, const void* d_in, uint64_t n, uint32_t* d_crc, void* stream) {
    if (!c || !d_crc || (!d_in && n)) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_crc) & 3) != 0) return -(int)E_INVAL;
    HIPCHK(hipSetDevice(c->device));
    const int r = dmx_crc32_launch(c, d_in, n, d_crc, stream ? (hipStream_t)stream : c->stream);
    if (r) return r;
    HIPCHK(hipGetLastError());
    return 0;
}
