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

// ---- per-block CRC-32 (DMX_F_BGZF: every member's own check value) ----
//
//   dmx_crc_blocks_kernel  the finished CRC-32 of every sw-byte block of the input (the last one
//                          may be short), one launch.  A workgroup stages one block as the span
//                          kernel stages a span -- from the 16-byte group that holds the block's
//                          first byte, zeros in front of the data and behind it up to CRC_S bytes
//                          -- and runs the same slice-by-16 lookups and lane fold.  What differs
//                          is the padding, which is no per-launch constant here:
//                            front   0..15 zero bytes, per block: free (R(0..0 || M) = R(M));
//                            behind  Z_b = CRC_S - (front + length) zero bytes, per block: divided
//                                    out with x^-(8 Z_b), the product of two table entries
//                                    (x^-(8 v) and x^-(8 256 v), Z_b < 2^15), computed by wave 0
//                                    while the block's loads are in flight;
//                            a block of more than CRC_S - front bytes (sw near 32 KiB at an
//                            unaligned address) spills into one more 16-byte group, which thread 0
//                            runs through one lookup step: R = R(span) x^128 xor R(group), and Z_b
//                            counts from the end of that group (Z_b < 16).
//                          The affine term has two values, for a full block and for the short last
//                          one, computed on the host at launch.  Workgroups stride over the blocks;
//                          lanes whose slice lies behind the data skip their lookups, so a small sw
//                          costs loads and lookups for its own bytes only.
struct CrcUnshift {
    uint32_t lo[256];   // x^-(8 v)
    uint32_t hi[128];   // x^-(8 256 v)
};
static constexpr CrcUnshift crc_make_unshift() {
    CrcUnshift U = {};
    uint32_t x8 = 0xDB710641u;   // x^-1: (P + 1) / x
    for (int k = 0; k < 3; k++) x8 = crc_cmul(x8, x8);   // x^-8
    uint32_t p = DMX_CRC_ONE;
    for (int v = 0; v < 256; v++) { U.lo[v] = p; p = crc_cmul(p, x8); }
    const uint32_t x2048 = p;    // x^-(8 256)
    p = DMX_CRC_ONE;
    for (int v = 0; v < 128; v++) { U.hi[v] = p; p = crc_cmul(p, x2048); }
    return U;
}
static_assert(crc_cmul(0xDB710641u, DMX_CRC_ONE >> 1) == DMX_CRC_ONE, "x^-1 x = 1");
static_assert(CRC_S <= 128 * 256, "Z_b < 2^15: two table entries");
__device__ const CrcUnshift g_crc_unshift = crc_make_unshift();
static constexpr uint32_t crc_x128() {   // x^(8 16): the shift of one 16-byte group
    uint32_t x = DMX_CRC_ONE >> 1;
    for (int e = 1; e < 128; e <<= 1) x = crc_cmul(x, x);
    return x;
}

// crc_load16 for a block: offsets from the block's aligned base fit 32 bits (g <= CRC_S, lo < 16,
// hi <= CRC_S + 15), and a word's mask is two shifts: its bytes [a, e) are data
__device__ __forceinline__ uint4 crc_load16_blk(const uint8_t* __restrict__ base, uint32_t g, uint32_t lo, uint32_t hi) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (g + 16 <= lo || g >= hi) return v;   // no byte of the block: nothing is read
    v = *reinterpret_cast<const uint4*>(base + g);   // 16-byte aligned, shares a byte with the block
    if (g < lo || g + 16 > hi) {
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t i = 0; i < 4; i++) {
            const int32_t q0 = (int32_t)(g + 4 * i);
            const int32_t a = min(max((int32_t)lo - q0, 0), 4), e = min(max((int32_t)hi - q0, 0), 4);
            const uint32_t below_e = (uint32_t)((1ull << (8 * e)) - 1ull), below_a = (uint32_t)((1ull << (8 * a)) - 1ull);
            w[i] &= below_e & ~below_a;
        }
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    return v;
}

// one slice-by-16 step: the remainder c extended by the 16 bytes d
#define CRC_STEP16(c, d, tab)                                                                                          \
    do {                                                                                                               \
        const uint32_t x_ = (d).x ^ (c);                                                                               \
        (c) = tab[15 * 256 + (x_ & 0xFFu)] ^ tab[14 * 256 + ((x_ >> 8) & 0xFFu)] ^ tab[13 * 256 + ((x_ >> 16) & 0xFFu)] ^ \
              tab[12 * 256 + (x_ >> 24)] ^ tab[11 * 256 + ((d).y & 0xFFu)] ^ tab[10 * 256 + (((d).y >> 8) & 0xFFu)] ^     \
              tab[9 * 256 + (((d).y >> 16) & 0xFFu)] ^ tab[8 * 256 + ((d).y >> 24)] ^ tab[7 * 256 + ((d).z & 0xFFu)] ^    \
              tab[6 * 256 + (((d).z >> 8) & 0xFFu)] ^ tab[5 * 256 + (((d).z >> 16) & 0xFFu)] ^ tab[4 * 256 + ((d).z >> 24)] ^ \
              tab[3 * 256 + ((d).w & 0xFFu)] ^ tab[2 * 256 + (((d).w >> 8) & 0xFFu)] ^                                    \
              tab[1 * 256 + (((d).w >> 16) & 0xFFu)] ^ tab[0 * 256 + ((d).w >> 24)];                                      \
    } while (0)

__global__ __launch_bounds__(CRC_T) void dmx_crc_blocks_kernel(const uint8_t* __restrict__ in, uint64_t n, uint32_t sw,
                                                               uint32_t nblk, uint32_t aff_full, uint32_t aff_tail,
                                                               uint32_t* __restrict__ crc) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[CRC_NS * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage[CRC_T * CRC_ROW];
    __shared__ uint32_t wred[CRC_T / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < CRC_NS * 256; i += CRC_T) tab[i] = (&g_crc.t[0][0])[i];
    const uint32_t klane = g_crc.lane[tid];
    constexpr uint32_t X128 = crc_x128();
    // block b: its aligned base, the data's bytes [lo, hi) from there
    auto geom = [&](uint32_t b, const uint8_t*& base, uint32_t& lo, uint32_t& hi) {
        const uint64_t off = (uint64_t)b * sw;
        const uint32_t len = (n - off) < sw ? (uint32_t)(n - off) : sw;
        const uint8_t* p = in + off;
        lo = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15);
        base = p - lo;
        hi = lo + len;
    };
    uint4 v[CRC_Q], vx = make_uint4(0u, 0u, 0u, 0u);   // vx: the group behind the span (thread 0)
    auto load = [&](uint32_t b) {
        const uint8_t* base;
        uint32_t lo, hi;
        geom(b, base, lo, hi);
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) v[i] = crc_load16_blk(base, 16u * (tid + CRC_T * i), lo, hi);
        if (tid == 0) vx = crc_load16_blk(base, CRC_S, lo, hi);   // (nothing is read unless hi > CRC_S)
    };
    uint32_t b = blockIdx.x;
    if (b < nblk) load(b);
    for (; b < nblk; b += gridDim.x) {
        const uint8_t* base;
        uint32_t lo, hi;
        geom(b, base, lo, hi);
        const bool spill = hi > CRC_S;
        // x^-(8 Z_b), by wave 0 while the loads fly (thread 0 uses it)
        uint32_t unshift = 0;
        if (tid < 64) {
            const uint32_t Z = (spill ? CRC_S + 16u : (uint32_t)CRC_S) - hi;
            unshift = dmx_gf2_mulmod(g_crc_unshift.lo[Z & 255u], g_crc_unshift.hi[Z >> 8]);
        }
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) {
            const uint32_t q = tid + CRC_T * i, sl = q / (CRC_L / 16);
            if (sl * CRC_L < hi)   // (a slice behind the data is never read)
                *reinterpret_cast<uint4*>(&stage[sl * CRC_ROW + 4 * (q % (CRC_L / 16))]) = v[i];
        }
        const uint4 gx = vx;
        __syncthreads();   // (and the tables, the first time)
        const uint32_t bn = b + gridDim.x;
        if (bn < nblk) load(bn);   // the next block's loads fly during this one's lookups
        uint32_t c = 0;
        if (tid * CRC_L < hi) {
            const uint4* p = reinterpret_cast<const uint4*>(&stage[tid * CRC_ROW]);
#pragma unroll
            for (uint32_t k = 0; k < CRC_L / 16; k++) {
                const uint4 d = p[k];
                CRC_STEP16(c, d, tab);
            }
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
            if (spill) {
                uint32_t cg = 0;
                CRC_STEP16(cg, gx, tab);
                t = dmx_gf2_mulmod(t, X128) ^ cg;
            }
            crc[b] = dmx_gf2_mulmod(t, unshift) ^ ((hi - lo) == sw ? aff_full : aff_tail);
        }
    }
}

// the launch of dmx_crc32_blocks_async on stream s (dmx_encode_async shares it: DMX_F_BGZF).  No
// scratch: every workgroup writes finished values.
static int dmx_crc32_blocks_launch(dmx_ctx* c, const void* d_in, uint64_t n, uint32_t sw, uint32_t* d_crc,
                                   hipStream_t s) {
    const uint64_t nblk64 = (n + sw - 1) / sw;
    if (nblk64 > 0x7FFFFFFFull) return -(int)E_SZ;
    if (!nblk64) return 0;
    const uint32_t nblk = (uint32_t)nblk64;
    const uint64_t tail = n - (nblk64 - 1) * sw;
    const uint32_t gmax = 3 * c->ncu;   // 3 workgroups of 52 KiB LDS per CU
    hipLaunchKernelGGL(dmx_crc_blocks_kernel, dim3(nblk < gmax ? nblk : gmax), dim3(CRC_T), 0, s, (const uint8_t*)d_in,
                       n, sw, nblk, dmx_crc32_affine(sw), dmx_crc32_affine(tail), d_crc);
    return 0;
}

extern "C" int dmx_crc32_blocks_async(dmx_ctx* c, const void* d_in, uint64_t n, int32_t sw, uint32_t* d_crc,
                                      void* stream) {
    if (!c || !d_crc || (!d_in && n)) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_crc) & 3) != 0) return -(int)E_INVAL;
    if (sw == 0) sw = DMX_BLK;
    if (sw < 1 || sw > DMX_BLK) return -(int)E_RANGE;
    HIPCHK(hipSetDevice(c->device));
    const int r = dmx_crc32_blocks_launch(c, d_in, n, (uint32_t)sw, d_crc, stream ? (hipStream_t)stream : c->stream);
    if (r) return r;
    HIPCHK(hipGetLastError());
    return 0;
}

// ---- CRC-32 over index ranges (the members of a BGZF file: any offset, 0..65536 bytes each) ----
//
//   dmx_crc_ranges_kernel  the blocks kernel with the block's geometry read from an index entry
//                          {out_off, out_len} instead of computed from b and sw.  A workgroup takes
//                          an entry and stages it in pieces of at most CRC_S bytes, from the 16-byte
//                          group that holds its first byte: a range of 65 536 bytes at an odd address
//                          is two whole pieces and one of 1..15 bytes.  Every piece is staged, looked
//                          up and lane-folded as a block is (in piece-local 32-bit offsets, through
//                          crc_load16_blk), and thread 0 folds piece by piece, R = R x^(8 CRC_S) xor
//                          R(piece).  Only the last piece has zeros behind its data, Z < CRC_S of
//                          them, divided out with the g_crc_unshift tables as in the blocks kernel.
//                          The affine term depends on the entry's length, so the host cannot pass
//                          it: 0xFFFFFFFF x^(8 len) is the product of two more table entries
//                          (g_crc_shift: len <= 65 536 = 256 x 256), computed with x^-(8 Z) by wave 0
//                          while the piece's loads fly.  (dmx_crc32_affine itself is host and device
//                          code, but its square-and-multiply is about 37 dependent multiplications,
//                          more than the lookups of a whole piece: the tables make it one.)
//                          The flat sequence of pieces of a workgroup's entries is pipelined as the
//                          blocks are: the next piece's loads fly during this one's lookups.
//                          An empty entry is one piece without data (no load, no lookup, value 0); an
//                          entry out of range is the same and writes nothing.
//                          want == NULL: crc[k] receives entry k's value.  want != NULL (the check of
//                          dmx_inflate_members_async): the value is compared with want[k], a
//                          difference sets -E_CRC unless a status is there -- and a status that is
//                          there at the start ends the kernel at once: the decode before it failed,
//                          and its index may be unsound.
struct CrcShift {
    uint32_t lo[256];   // 0xFFFFFFFF x^(8 v)
    uint32_t hi[257];   // x^(8 256 v)
};
static constexpr CrcShift crc_make_shift() {
    CrcShift U = {};
    uint32_t x8 = DMX_CRC_ONE >> 1;
    for (int k = 0; k < 3; k++) x8 = crc_cmul(x8, x8);   // x^8
    uint32_t p = 0xFFFFFFFFu, q = DMX_CRC_ONE;
    for (int v = 0; v < 256; v++) { U.lo[v] = p; p = crc_cmul(p, x8); q = crc_cmul(q, x8); }
    const uint32_t x2048 = q;    // x^(8 256)
    p = DMX_CRC_ONE;
    for (int v = 0; v < 257; v++) { U.hi[v] = p; p = crc_cmul(p, x2048); }
    return U;
}
static_assert(DMX_BGZF_MAX_ISIZE == 256 * 256, "a length is lo + 256 hi with hi <= 256");
static_assert(2 * CRC_S == DMX_BGZF_MAX_ISIZE, "a range is at most two spans and one 16-byte group");
__device__ const CrcShift g_crc_shift = crc_make_shift();

__global__ __launch_bounds__(CRC_T) void dmx_crc_ranges_kernel(const uint8_t* __restrict__ in, uint64_t n,
                                                               const dmx_iblock* __restrict__ index, uint32_t nblk,
                                                               uint32_t* __restrict__ crc, const uint32_t* __restrict__ want,
                                                               dmx_inflate_status* st) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[CRC_NS * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage[CRC_T * CRC_ROW];
    __shared__ uint32_t wred[CRC_T / 64];
    __shared__ int32_t st0;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) st0 = want ? st->status : 0;   // one read: the whole workgroup stays or leaves
    __syncthreads();
    if (st0 != 0) return;
    for (uint32_t i = tid; i < CRC_NS * 256; i += CRC_T) tab[i] = (&g_crc.t[0][0])[i];
    const uint32_t klane = g_crc.lane[tid];
    constexpr uint32_t XS = crc_xspan();
    // piece j of entry k: its aligned base, the data's bytes [lo, hi) from there (hi <= CRC_S),
    // the entry's pieces and length; false: the entry is out of range (then one piece, no data)
    auto geom = [&](uint32_t k, uint32_t j, const uint8_t*& base, uint32_t& lo, uint32_t& hi, uint32_t& np, uint32_t& len) {
        const uint64_t off = index[k].out_off;
        len = index[k].out_len;
        const bool ok = len <= DMX_BGZF_MAX_ISIZE && off <= n && len <= n - off;
        uint32_t elo = 0, ehi = 0;   // the whole entry from its aligned base: ehi <= 15 + 65 536
        base = in;
        if (ok && len) {
            const uint8_t* p = in + off;
            elo = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15);
            base = p - elo;
            ehi = elo + len;
        }
        np = ehi > CRC_S ? (ehi + CRC_S - 1) / CRC_S : 1u;
        base += (size_t)j * CRC_S;
        lo = j ? 0u : elo;
        hi = ehi - j * CRC_S < CRC_S ? ehi - j * CRC_S : (uint32_t)CRC_S;   // (j < np: ehi > j CRC_S, or both are 0)
        return ok;
    };
    uint4 v[CRC_Q];
    auto load = [&](uint32_t k, uint32_t j) {
        const uint8_t* base;
        uint32_t lo, hi, np, len;
        geom(k, j, base, lo, hi, np, len);
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) v[i] = crc_load16_blk(base, 16u * (tid + CRC_T * i), lo, hi);
    };
    uint32_t k = blockIdx.x, j = 0, acc = 0;   // acc (thread 0): the raw remainder of the entry's pieces so far
    if (k < nblk) load(k, 0);
    while (k < nblk) {
        const uint8_t* base;
        uint32_t lo, hi, np, len;
        const bool ok = geom(k, j, base, lo, hi, np, len);
        const bool last = j + 1 == np;
        // x^-(8 Z) and the affine term, by wave 0 while the loads fly (thread 0 uses them)
        uint32_t unshift = 0, affine = 0;
        if (last && tid < 64) {
            const uint32_t Z = (CRC_S - hi) & (CRC_S - 1u), l = ok ? len : 0u;   // (no data: R = 0, any factor)
            unshift = dmx_gf2_mulmod(g_crc_unshift.lo[Z & 255u], g_crc_unshift.hi[Z >> 8]);
            affine = dmx_gf2_mulmod(g_crc_shift.lo[l & 255u], g_crc_shift.hi[l >> 8]) ^ 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) {
            const uint32_t q = tid + CRC_T * i, sl = q / (CRC_L / 16);
            if (sl * CRC_L < hi)   // (a slice behind the data is never read)
                *reinterpret_cast<uint4*>(&stage[sl * CRC_ROW + 4 * (q % (CRC_L / 16))]) = v[i];
        }
        __syncthreads();   // (and the tables, the first time)
        const uint32_t kn = last ? k + gridDim.x : k, jn = last ? 0u : j + 1;
        if (kn < nblk) load(kn, jn);   // the next piece's loads fly during this one's lookups
        uint32_t c = 0;
        if (tid * CRC_L < hi) {
            const uint4* p = reinterpret_cast<const uint4*>(&stage[tid * CRC_ROW]);
#pragma unroll
            for (uint32_t s = 0; s < CRC_L / 16; s++) {
                const uint4 d = p[s];
                CRC_STEP16(c, d, tab);
            }
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
            acc = j ? dmx_gf2_mulmod(acc, XS) ^ t : t;
            if (last) {
                const uint32_t val = dmx_gf2_mulmod(acc, unshift) ^ affine;
                if (!ok) {
                    if (st) atomicCAS(&st->status, 0, -(int32_t)E_RANGE);
                } else if (!want) {
                    crc[k] = val;
                } else if (val != want[k]) {
                    atomicCAS(&st->status, 0, -(int32_t)E_CRC);
                }
            }
        }
        k = kn;
        j = jn;
    }
}

// compute units of the current device (the grid of the ranges kernel, which has no context)
static uint32_t crc_device_ncu(void) {
    static uint32_t ncu[64];
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256u;
    if (!ncu[dev])
        ncu[dev] = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0
                       ? (uint32_t)v : 256u;
    return ncu[dev];
}

// the launch of dmx_crc32_ranges_async on stream s, and with d_want the check of
// dmx_inflate_members_async (dmx_inflate_dev.hip).  No scratch: every workgroup writes (or
// compares) finished values.
int dmx_crc32_ranges_launch(const void* d_in, uint64_t n, const dmx_iblock* d_index, uint32_t nblk, uint32_t* d_crc,
                            const uint32_t* d_want, dmx_inflate_status* d_status, hipStream_t s) {
    if (!nblk) return 0;
    const uint32_t gmax = 3 * crc_device_ncu();   // 3 workgroups of 52 KiB LDS per CU
    hipLaunchKernelGGL(dmx_crc_ranges_kernel, dim3(nblk < gmax ? nblk : gmax), dim3(CRC_T), 0, s, (const uint8_t*)d_in,
                       n, d_index, nblk, d_crc, d_want, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

extern "C" int dmx_crc32_ranges_async(const void* d_in, uint64_t n, const dmx_iblock* d_index, uint32_t nblk,
                                      uint32_t* d_crc, dmx_inflate_status* d_status, void* stream) {
    if ((!d_in && n) || (nblk && (!d_index || !d_crc))) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_crc) & 3) != 0) return -(int)E_INVAL;
    return dmx_crc32_ranges_launch(d_in, n, d_index, nblk, d_crc, NULL, d_status, (hipStream_t)stream);
}

// ---- CRC-32 of the gzip members of a batch (dmx_inflate_batch_async: any offset, any length) ----
//
//   dmx_crc_batch_kernel   the ranges kernel with an entry's geometry read from the batch's records
//                          -- out_off of stream k's descriptor, out_len of its result -- and a
//                          length without a bound: an entry is a loop over pieces of at most CRC_S
//                          bytes with the ranges kernel's per-piece arithmetic, folded by thread 0
//                          with the constant x^(8 CRC_S).  The affine term's x^(8 len) is the product
//                          of the two g_crc_shift entries for len mod 65 536 and, above that, of
//                          x^(8 65 536 (len >> 16)) by square-and-multiply -- by wave 0 while the
//                          last piece's loads fly.
//                          Only an entry with status 0 and format gzip has data; any other is one
//                          piece without data and is left alone.  The value is compared with the
//                          stored CRC-32 (check) and the member is finished: -E_CRC, else -E_LEN
//                          where the decode noted a wrong ISIZE (reserved), else 0; the note is
//                          cleared, a failed member's out_len / in_used / check become 0, and the
//                          summary counts the member (integer sums and a minimum).
__global__ __launch_bounds__(CRC_T) void dmx_crc_batch_kernel(const uint8_t* __restrict__ in, uint64_t n,
                                                              const dmx_bstream* __restrict__ streams, uint32_t nstreams,
                                                              dmx_bresult* res, dmx_batch_status* __restrict__ st) {
    __shared__ __attribute__((aligned(16))) uint32_t tab[CRC_NS * 256];
    __shared__ __attribute__((aligned(16))) uint32_t stage[CRC_T * CRC_ROW];
    __shared__ uint32_t wred[CRC_T / 64];
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < CRC_NS * 256; i += CRC_T) tab[i] = (&g_crc.t[0][0])[i];
    const uint32_t klane = g_crc.lane[tid];
    constexpr uint32_t XS = crc_xspan();
    // piece j of entry k: its aligned base, the data's bytes [lo, hi) from there (hi <= CRC_S), the
    // entry's pieces and length; false: not a gzip member that decoded (then one piece, no data)
    auto geom = [&](uint32_t k, uint64_t j, const uint8_t*& base, uint32_t& lo, uint32_t& hi, uint64_t& np, uint64_t& len) {
        const uint64_t off = streams[k].out_off;
        len = res[k].out_len;
        const bool ok = res[k].status == 0 && res[k].format == DMX_BATCH_GZIP && off <= n && len <= n - off;
        uint64_t elo = 0, ehi = 0;   // the whole entry from its aligned base
        base = in;
        if (ok && len) {
            const uint8_t* p = in + off;
            elo = reinterpret_cast<uintptr_t>(p) & 15;
            base = p - elo;
            ehi = elo + len;
        }
        np = ehi > CRC_S ? (ehi + CRC_S - 1) / CRC_S : 1u;
        base += j * CRC_S;
        lo = j ? 0u : (uint32_t)elo;
        const uint64_t left = ehi - j * CRC_S;   // (j < np: ehi > j CRC_S, or both are 0)
        hi = left < CRC_S ? (uint32_t)left : (uint32_t)CRC_S;
        return ok;
    };
    uint4 v[CRC_Q];
    auto load = [&](uint32_t k, uint64_t j) {
        const uint8_t* base;
        uint32_t lo, hi;
        uint64_t np, len;
        geom(k, j, base, lo, hi, np, len);
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) v[i] = crc_load16_blk(base, 16u * (tid + CRC_T * i), lo, hi);
    };
    uint32_t k = blockIdx.x, acc = 0;   // acc (thread 0): the raw remainder of the entry's pieces so far
    uint64_t j = 0;
    if (k < nstreams) load(k, 0);
    while (k < nstreams) {
        const uint8_t* base;
        uint32_t lo, hi;
        uint64_t np, len;
        const bool ok = geom(k, j, base, lo, hi, np, len);
        const bool last = j + 1 == np;
        // x^-(8 Z) and the affine term, by wave 0 while the loads fly (thread 0 uses them)
        uint32_t unshift = 0, affine = 0;
        if (last && tid < 64) {
            const uint32_t Z = (CRC_S - hi) & (CRC_S - 1u);   // (no data: R = 0, any factor)
            const uint64_t l = ok ? len : 0u;
            unshift = dmx_gf2_mulmod(g_crc_unshift.lo[Z & 255u], g_crc_unshift.hi[Z >> 8]);
            affine = dmx_gf2_mulmod(g_crc_shift.lo[l & 255u], g_crc_shift.hi[(l >> 8) & 255u]);
            if (l >> 16) affine = dmx_gf2_mulmod(affine, dmx_gf2_xpow(l >> 16, 19));   // x^(8 65 536 (l >> 16))
            affine ^= 0xFFFFFFFFu;
        }
#pragma unroll
        for (uint32_t i = 0; i < CRC_Q; i++) {
            const uint32_t q = tid + CRC_T * i, sl = q / (CRC_L / 16);
            if (sl * CRC_L < hi)   // (a slice behind the data is never read)
                *reinterpret_cast<uint4*>(&stage[sl * CRC_ROW + 4 * (q % (CRC_L / 16))]) = v[i];
        }
        __syncthreads();   // (and the tables, the first time)
        const uint32_t kn = last ? k + gridDim.x : k;
        const uint64_t jn = last ? 0u : j + 1;
        if (kn < nstreams) load(kn, jn);   // the next piece's loads fly during this one's lookups
        uint32_t c = 0;
        if (tid * CRC_L < hi) {
            const uint4* p = reinterpret_cast<const uint4*>(&stage[tid * CRC_ROW]);
#pragma unroll
            for (uint32_t s = 0; s < CRC_L / 16; s++) {
                const uint4 d = p[s];
                CRC_STEP16(c, d, tab);
            }
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
            acc = j ? dmx_gf2_mulmod(acc, XS) ^ t : t;
            if (last && ok) {
                const uint32_t val = dmx_gf2_mulmod(acc, unshift) ^ affine;
                const int32_t fin = val != res[k].check ? -(int32_t)E_CRC : res[k].reserved ? -(int32_t)E_LEN : 0;
                res[k].reserved = 0;
                if (fin) {
                    res[k].status = fin;
                    res[k].out_len = 0;
                    res[k].in_used = 0;
                    res[k].check = 0;
                    atomicAdd(&st->nfailed, 1u);
                    atomicMin(&st->first_bad, k);
                } else {
                    atomicAdd((unsigned long long*)&st->total_out, (unsigned long long)len);
                }
            }
        }
        k = kn;
        j = jn;
    }
}

int dmx_crc32_batch_launch(const void* d_out, uint64_t out_bytes, const dmx_bstream* d_streams, uint32_t nstreams,
                           dmx_bresult* d_results, dmx_batch_status* d_status, hipStream_t s) {
    if (!nstreams) return 0;
    const uint32_t gmax = 3 * crc_device_ncu();   // 3 workgroups of 52 KiB LDS per CU
    hipLaunchKernelGGL(dmx_crc_batch_kernel, dim3(nstreams < gmax ? nstreams : gmax), dim3(CRC_T), 0, s,
                       (const uint8_t*)d_out, out_bytes, d_streams, nstreams, d_results, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
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
