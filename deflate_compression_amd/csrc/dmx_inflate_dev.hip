// dmx_inflate_dev.hip -- RFC 1950/1951 inflate on the MI355X.
//
// Two kernels over one decoder:
//   * indexed (dmx_inflate_index_kernel): one single-wave workgroup per sw block listed in a
//     block index {start bit, output offset, output length}; it decodes DEFLATE blocks until
//     the sw block's output is complete (one, or up to four with DMX_F_SPLIT).  Blocks of a dmx stream
//     never reference earlier blocks (every sw-sized block is its own window),
//     so all blocks decode in parallel; the encoder exports the index (dmx_block_index).
//   * stream (dmx_inflate_stream_kernel): one workgroup decodes a whole zlib stream
//     (header, blocks until BFINAL, Adler-32 check) -- any RFC 1950 stream, e.g. PNG IDAT.
//
// The decoder is wave-uniform: the 64-bit bit buffer, the stream word index and the output
// position are SGPRs; the compressed stream is staged in two VGPRs (one dword per lane, the
// next 256 bytes prefetched), so a refill is a v_readlane.  The common path of the symbol loop
// is hand-scheduled (isym_run): the literal/length and distance tables live in VGPRs during it
// (a v_readlane under the VGPR index mode per lookup, no LDS round trip), each entry carries its base
// and is the s_bfe control of its own extra bits, a literal is one LDS byte store, and a match
// is copied by the whole wave, 64 bytes a round (periodic sources by residue; sources older
// than the ring from the output already flushed to HBM).  Output is assembled in an LDS ring
// and written to HBM in 16-byte-per-lane coalesced stores every half ring (indexed mode: an
// 8 KiB ring; stream mode: the 32 KiB window, folding the Adler-32 sums into the same pass).
// Tables: 10-bit first level, built lane-parallel (ballot counts and ranks) into a per-
// workgroup area of HBM and loaded into VGPRs by the symbol loop, so that LDS holds only the
// ring (12 workgroups per CU); longer codes take a canonical slow path (first code / count /
// offset per length, in LDS).
#include <hip/hip_runtime.h>
#include <pthread.h>
#include <stdint.h>
#include <type_traits>
#include <stdio.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_ctx.h"   // dmx_crc32_ranges_launch, dmx_crc32_batch_launch
#include "dmx_gz_head.h"
#include "dmx_pfind.h"   // the plan of one foreign stream: search, landing, walk, sizes
#include "dmx_ptail.h"   // its decode: the tail and pack rules
#include "dmx_crc.h"

#define IW 32768          // window = LDS ring (stream mode; the indexed mode's ring is IWX)
#ifndef DMX_IWX
#define DMX_IWX 8192      // indexed mode: an 8 KiB ring, older sources read back from HBM
#endif
#define IWX DMX_IWX
#define IWC 4096          // chained decode: a ring of 4 096 cells (8 KiB)
#define IFB 10            // first-level table bits
#define ITAB_WORDS 2048   // a workgroup's first-level tables in HBM: literal/length, then distance
#define IFLUSH 16384      // stream mode: flush to HBM every IFLUSH bytes (half the ring)

// The first-level entries (1 << IFB words per table, format "Table entries" below) live in
// HBM, ITAB_WORDS per workgroup: the symbol loop holds them in VGPRs and reloads them at each
// entry (agent-scope loads, L2), so LDS keeps only the ring and these small arrays -- 10 KB
// a workgroup, and all 3 052 blocks of 100 MB resident at once (12 per CU, the VGPR limit)
// instead of 2 048 (8 per CU with the tables in LDS).
struct ITable {
    uint16_t first[16];        // first canonical code of each length
    uint16_t cnt[16];
    uint16_t offs[16];         // index into sym[] of the first symbol of each length
    uint16_t sym[288];         // symbols sorted by (length, symbol)
};

// T = uint8_t: the output bytes; T = uint16_t: cells of the chained decode (a byte value, or
// 0x100 + b - 1 for the byte b positions before the sw block's first output byte, resolved
// afterwards: dmx_inflate_chained_async)
template <uint32_t W, typename T = uint8_t>
struct InfLDS {
    T win[W];
    ITable lt, dt;
    uint8_t len[320];
    uint8_t seq[320];
};

__device__ __forceinline__ uint32_t rfl(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t rfl64(uint64_t v) {
    return ((uint64_t)rfl((uint32_t)(v >> 32)) << 32) | rfl((uint32_t)v);
}

// ---------------------------------------------------------------------------------------
// Bit reader.  Coordinates are relative to the dword-aligned address at or below z.  The
// stream is staged in two VGPRs, one dword per lane: vcur holds words wb + lane, vnxt words
// wb + 64 + lane, so a refill is one v_readlane; when the reader passes into vnxt the pair
// advances and the load of the next 256 bytes is issued, 64 refills before it is needed.
// Words that are not wholly inside the stream are assembled from bytes (zeros past the end).
// ---------------------------------------------------------------------------------------
// global-space views: plain loads, not flat ones (a flat load counts in lgkmcnt too, so every
// LDS wait would also wait for the stream prefetch)
typedef __attribute__((address_space(1))) const uint8_t gu8;
typedef __attribute__((address_space(1))) const uint32_t gu32;

struct IBits {
    gu8* zb;               // aligned base as bytes
    uint32_t lo, hi;       // valid byte range [lo, hi) relative to zb
    uint32_t wfast;        // words < wfast are wholly inside the stream
    uint32_t wb;           // word index of vcur's lane 0 (a multiple of 64)
    uint32_t vcur, vnxt;   // per lane: word wb + lane, word wb + 64 + lane
    uint32_t wi;           // next word
    uint32_t bc;
    uint64_t bb;
};

__device__ __forceinline__ uint32_t ib_vload(const IBits& r, uint32_t w0) {   // word w0 + lane
    const uint32_t wi = w0 + __lane_id();
    if (wi < r.wfast) return reinterpret_cast<gu32*>(r.zb)[wi];
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; j++) {
        const uint32_t b = wi * 4 + j;
        if (b >= r.lo && b < r.hi) v |= (uint32_t)r.zb[b] << (8 * j);
    }
    return v;
}
__device__ __forceinline__ uint32_t ib_word(IBits& r, uint32_t wi) {   // wi: sequential from the seek
    uint32_t k = wi - r.wb;
    if (k >= 64) {
        r.vcur = r.vnxt;
        r.wb += 64;
        r.vnxt = ib_vload(r, r.wb + 64);
        k -= 64;
    }
    return __builtin_amdgcn_readlane(r.vcur, k);
}
__device__ __forceinline__ void ib_refill(IBits& r) {   // afterwards bc >= 32
    if (r.bc <= 32) {
        r.bb |= (uint64_t)ib_word(r, r.wi) << r.bc;
        r.wi++;
        r.bc += 32;
    }
}
// Bits consumed so far and bits the stream has (both from zb).  The reader hands out zeros past
// the end, so a decode that ran out of input is seen afterwards, exactly: used > have.
__device__ __forceinline__ uint64_t ib_used(const IBits& r) { return (uint64_t)r.wi * 32 - r.bc; }
__device__ __forceinline__ uint64_t ib_have(const IBits& r) { return (uint64_t)r.hi * 8; }
__device__ __forceinline__ bool ib_past(const IBits& r) { return ib_used(r) > ib_have(r); }
// The status of a block that returned err (0 or -E_*), as the host decoder reports it
// (dmx_inflate.c; the table in include/dmx.h): input that ended before the block did is -E_LEN
// whatever the zeros behind it decoded to, and a bit pattern that is no code is -E_HUFINV only
// where the 15 bits that show it are all there (the pattern itself is not consumed).
__device__ __forceinline__ int ib_status(const IBits& r, int err) {
    if (ib_past(r)) return -(int)E_LEN;
    if (err == -(int)E_HUFINV && ib_used(r) + 15 > ib_have(r)) return -(int)E_LEN;
    return err;
}
__device__ __forceinline__ void ib_seek(IBits& r, uint64_t bit) {   // bit: relative to z
    const uint64_t ab = bit + (uint64_t)r.lo * 8;
    r.wi = (uint32_t)(ab >> 5);
    r.wb = r.wi & ~63u;
    r.vcur = ib_vload(r, r.wb);
    r.vnxt = ib_vload(r, r.wb + 64);
    r.bb = (uint64_t)ib_word(r, r.wi) >> (ab & 31);
    r.bc = 32 - (uint32_t)(ab & 31);
    r.wi++;
}
__device__ __forceinline__ void ib_init(IBits& r, const uint8_t* z, uint64_t zbytes) {
    const uintptr_t a = (uintptr_t)z;
    r.zb = (gu8*)(a & ~(uintptr_t)3);
    r.lo = (uint32_t)(a & 3);
    r.hi = r.lo + (uint32_t)zbytes;
    r.wfast = r.hi >> 2;
    r.wi = r.wb = 0;
    r.vcur = r.vnxt = 0;
    r.bb = 0;
    r.bc = 0;
}
__device__ __forceinline__ uint32_t ib_peek(const IBits& r, uint32_t n) { return (uint32_t)r.bb & ((1u << n) - 1); }
__device__ __forceinline__ void ib_drop(IBits& r, uint32_t n) {
    r.bb >>= n;
    r.bc -= n;
}
__device__ __forceinline__ uint32_t ib_bits(IBits& r, uint32_t n) {   // n <= 32
    ib_refill(r);
    const uint32_t v = n ? ib_peek(r, n) : 0;
    ib_drop(r, n);
    return v;
}
__device__ __forceinline__ uint64_t ib_bytepos(const IBits& r) {   // after ib_align; relative to z
    return (uint64_t)r.wi * 4 - r.bc / 8 - r.lo;
}

#define ISLOW 0xFFFFu

// DEFLATE length / distance bases by arithmetic (RFC 1951 3.2.5), no table loads.
__device__ __forceinline__ uint32_t len_extra(uint32_t li) { return li < 8 || li == 28 ? 0 : (li - 4) >> 2; }
__device__ __forceinline__ uint32_t len_base(uint32_t li) {
    return li < 8 ? li + 3 : li == 28 ? 258 : ((4 + (li & 3)) << ((li - 4) >> 2)) + 3;
}
__device__ __forceinline__ uint32_t dist_extra(uint32_t d) { return d < 4 ? 0 : (d - 2) >> 1; }
__device__ __forceinline__ uint32_t dist_base(uint32_t d) { return d < 4 ? d + 1 : ((2 + (d & 1)) << ((d - 2) >> 1)) + 1; }

// Table entries (32-bit).  The symbol loop looks its codes up in 1024-entry tables held in 16
// VGPRs (entry x in lane x & 63 of register x >> 6: a v_readlane under the index mode, no LDS round
// trip).  A length or distance entry is laid out so that it is itself the s_bfe control that
// extracts its extra bits from the bit buffer: bits [4:0] the code length (the field's offset),
// [22:16] the extra-bit count (its width); [12:8] code + extra bits (the bits to drop).
//   literal/length: literal  sym << 16 | clen                      (bit 15 clear)
//                   length   base << 23 | extra << 16 | 0x8000 | (clen + extra) << 8 | clen
//                   EOB      0xC000 | clen;  invalid (286, 287) 0xE000 | clen  (bit 14 set)
//   distance:       m << 28 | extra << 16 | (clen + extra) << 8 | clen, where base - 1 = m << extra
//                   (m = code for codes 0..3, 2 + (code & 1) above);  IVBAD invalid (30, 31)
//   both:           IVSLOW: a code longer than IFB bits (or none) -- the canonical slow path
#define IVSLOW 0xFFFFFFFFu
#define IVBAD 0xFFFFFFFEu
__device__ __forceinline__ uint32_t iv_ll(uint32_t e) {   // from a sym << 4 | clen entry
    if (e == ISLOW) return IVSLOW;
    const uint32_t sym = e >> 4, l = e & 15u;
    if (sym < 256) return (sym << 16) | l;
    if (sym == 256) return 0xC000u | l;
    const uint32_t li = sym - 257;
    if (li >= 29) return 0xE000u | l;
    const uint32_t x = len_extra(li);
    return (len_base(li) << 23) | (x << 16) | 0x8000u | ((l + x) << 8) | l;
}
__device__ __forceinline__ uint32_t iv_d(uint32_t e) {
    if (e == ISLOW) return IVSLOW;
    const uint32_t ds = e >> 4, l = e & 15u;
    if (ds >= 30) return IVBAD;
    const uint32_t x = dist_extra(ds), m = ds < 4 ? ds : 2 + (ds & 1);
    return (m << 28) | (x << 16) | ((l + x) << 8) | l;
}
// the value of a length / distance entry's field (its extra bits at the reader) and its base
__device__ __forceinline__ uint32_t iv_extra(uint64_t bb, uint32_t e) {
    return (uint32_t)(bb >> (e & 31u)) & ((1u << ((e >> 16) & 15u)) - 1);
}
__device__ __forceinline__ uint32_t iv_dbase(uint32_t e) { return ((e >> 28) << ((e >> 16) & 15u)) + 1; }

// ---------------------------------------------------------------------------------------
// Huffman tables, lane-parallel over symbols (lane t holds symbols t, t + 64, ...): counts per
// code length by ballots, the canonical first codes and offsets (uniform), then each symbol's
// rank among the symbols of its length (mbcnt of the same ballots) gives its code and its slot
// in the length-sorted list; every lane then fills its symbol's first-level entries at once,
// in the 32-bit format above (DIST: a distance table; otherwise literal/length, which also
// serves the code length code: its symbols 0..18 take the literal form).  IVSLOW marks a code
// longer than IFB bits (or no code).  Returns 0 complete, 1 incomplete, -1 over-subscribed.
// ---------------------------------------------------------------------------------------
// agent-scope load of a table word (to L2, past the vector L1, which may hold the words of the
// previous block's table)
__device__ __forceinline__ uint32_t gtab_ld(const uint32_t* p) {
    return __hip_atomic_load((const __attribute__((address_space(1))) uint32_t*)p, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
}

template <bool DIST, uint32_t W, typename TW>
__device__ __forceinline__ int itable_build(InfLDS<W, TW>& S, ITable& T, uint32_t* __restrict__ fast, int n,
                                            uint32_t lane) {
    const int nc = (n + 63) >> 6;   // symbol chunks, <= 5
    uint32_t lc[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        const int s = c * 64 + (int)lane;
        lc[c] = (c < nc && s < n) ? S.len[s] : 0u;
    }
    for (int k = (int)lane; k < (1 << IFB); k += 64) fast[k] = IVSLOW;
    uint32_t cnt[16], first[16], offs[16];
#pragma unroll
    for (int l = 1; l < 16; l++) {
        uint32_t t = 0;
#pragma unroll
        for (int c = 0; c < 5; c++)
            if (c < nc) t += (uint32_t)__popcll(__ballot(lc[c] == (uint32_t)l));
        cnt[l] = t;
    }
    // Kraft check, first codes and offsets (uniform)
    int left = 1, res = 0;
    uint32_t code = 0, off = 0, cprev = 0;
#pragma unroll
    for (int l = 1; l < 16; l++) {
        left = 2 * left - (int)cnt[l];
        if (left < 0) res = -1;
        code = (code + cprev) << 1;
        first[l] = code;
        offs[l] = off;
        if (lane == 0) {
            T.first[l] = (uint16_t)code;
            T.cnt[l] = (uint16_t)cnt[l];
            T.offs[l] = (uint16_t)off;
        }
        off += cnt[l];
        cprev = cnt[l];
    }
    if (res == 0 && left > 0) res = 1;
    if (off == 0) res = 1;   // no codes at all
    if (res >= 0) {
        uint32_t run[16];
#pragma unroll
        for (int l = 1; l < 16; l++) run[l] = 0;
#pragma unroll
        for (int c = 0; c < 5; c++) {
            if (c >= nc) break;
            const uint32_t l0 = lc[c];
            uint32_t mycode = 0, myoff = 0;
#pragma unroll
            for (int l = 1; l < 16; l++) {
                const uint64_t m = __ballot(l0 == (uint32_t)l);
                const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                if (l0 == (uint32_t)l) {
                    mycode = first[l] + run[l] + below;
                    myoff = offs[l] + run[l] + below;
                }
                run[l] += (uint32_t)__popcll(m);
            }
            if (l0) {
                const uint32_t s = c * 64 + lane;
                T.sym[myoff] = (uint16_t)s;
                if (l0 <= IFB) {
                    const uint32_t rv = __brev(mycode) >> (32 - l0);
                    const uint32_t e16 = (s << 4) | l0;
                    const uint32_t e = DIST ? iv_d(e16) : iv_ll(e16);
                    for (uint32_t j = 0; j < (1u << (IFB - l0)); j++) fast[rv | (j << l0)] = e;
                }
            }
        }
    }
    __builtin_amdgcn_s_waitcnt(0);   // the table stores are done before anyone loads them
    __syncthreads();
    return res;
}

// Entry for the code at the reader (caller refilled: bc >= 15): the first-level entry, or
// for longer codes the canonical decode; ISLOW = no valid code.
__device__ __forceinline__ uint32_t ientry_slow(const IBits& r, const ITable& T) {
    const uint32_t cr = __brev((uint32_t)r.bb);   // next bits, first bit in the MSB
    for (uint32_t l = IFB + 1; l < 16; l++) {
        const uint32_t code = cr >> (32 - l);
        const uint32_t d = code - rfl(T.first[l]);
        if (d < rfl(T.cnt[l])) return (rfl(T.sym[rfl(T.offs[l]) + d]) << 4) | l;
    }
    return ISLOW;
}
// the code length code (symbols 0..18, in the literal form): sym << 4 | len, or ISLOW
__device__ __forceinline__ uint32_t ientry_cl(const IBits& r, const ITable& T, const uint32_t* fast) {
    const uint32_t e = rfl(gtab_ld(fast + ib_peek(r, IFB)));
    return e != IVSLOW ? (((e >> 16) & 0xFFu) << 4) | (e & 15u) : ientry_slow(r, T);
}

__constant__ uint8_t c_iclorder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---------------------------------------------------------------------------------------
// Output.  Positions are 32-bit and relative to ob (a multiple of IW, so the window index
// of a position is pos & IM); stream mode moves ob forward as it flushes.
// ---------------------------------------------------------------------------------------
// DMX_INF_STAMPS (diagnostic builds only): per-workgroup cycle totals of the decode phases
#ifdef DMX_INF_STAMPS
#define INF_NST 16
__device__ unsigned long long dmx_inf_st[1 << 16][INF_NST];
#define IST_NOW() __builtin_amdgcn_s_memtime()
#define IST_ADD(o, k, v) ((o).st[k] += (v))
#else
#define IST_NOW() 0ull
#define IST_ADD(o, k, v) ((void)0)
#endif

struct IOut {
#ifdef DMX_INF_STAMPS
    unsigned long long st[INF_NST];   // 0 header + tables, 1 symbol loop, 2 flushes, 3 matches, 4 far matches, 5 asm runs,
                                      // 6 blocks, 7 code length table, 8 code lengths, 9 literal/length table,
                                      // 10 distance table, 11..15 asm-run exits IX_SYM .. IX_MATCH
#endif
    uint8_t* out;     // + base + ob = position 0
    uint64_t base, ob, cap;   // cap: absolute output capacity
    uint32_t op, fl;  // produced / flushed (relative)
    uint32_t a, b;    // stream mode: Adler-32 of everything flushed
};
#define IRENORM (1u << 30)

__device__ __forceinline__ uint32_t io_caprel(const IOut& o) {
    const uint64_t c = o.cap - o.ob;
    return c > 0x80000000ull ? 0x80000000u : (uint32_t)c;
}

__device__ __forceinline__ uint64_t wave_sum64(uint64_t v) {
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// Write window bytes [fl, upto) to HBM (upto - fl <= W).  ADLER: fold them into (a, b).
// STORE = false (the batch decode's measure pass): the same walk without its stores.
// Cells: window positions [fl, upto) to the cell buffer (2 bytes a position), 8 cells (16
// bytes) per lane where the destination is 16-byte aligned.
template <uint32_t W>
__device__ __forceinline__ void io_flush_cells(InfLDS<W, uint16_t>& S, IOut& o, uint32_t upto, uint32_t lane) {
    constexpr uint32_t IM = W - 1;
    __syncthreads();
    uint16_t* dst = reinterpret_cast<uint16_t*>(o.out) + o.base + o.ob;
    uint32_t p = o.fl;
    const uint32_t head = min(upto - p, (uint32_t)(((16 - (((uintptr_t)(dst + p)) & 15)) & 15) >> 1));
    if (lane < head) dst[p + lane] = S.win[(p + lane) & IM];
    p += head;
    for (; p + 8 <= upto; p += 512) {
        const uint32_t q = p + lane * 8;
        if (q + 8 <= upto) {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                w[k] = (uint32_t)S.win[(q + 2 * k) & IM] | ((uint32_t)S.win[(q + 2 * k + 1) & IM] << 16);
            *(uint4*)&dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
        } else if (q < upto) {
            for (uint32_t t = q; t < upto; t++) dst[t] = S.win[t & IM];
        }
    }
    if (p < upto && lane == 0)
        for (uint32_t t = p; t < upto; t++) dst[t] = S.win[t & IM];
    o.fl = upto;
    __builtin_amdgcn_s_waitcnt(0);   // the stores are done: far-match reads see them
    if (o.fl >= IRENORM) {
        o.ob += IRENORM;
        o.op -= IRENORM;
        o.fl -= IRENORM;
    }
    __syncthreads();
}

template <bool ADLER, bool STORE = true, uint32_t W, typename TW>
__device__ __forceinline__ void io_flush(InfLDS<W, TW>& S, IOut& o, uint32_t upto, uint32_t lane) {
    if constexpr (sizeof(TW) == 2) {
        io_flush_cells<W>(S, o, upto, lane);
        return;
    } else {
    constexpr uint32_t IM = W - 1;
    [[maybe_unused]] const unsigned long long ts0 = IST_NOW();
    __syncthreads();
    uint8_t* dst = o.out + o.base + o.ob;
    const uint32_t n = upto - o.fl;
    uint64_t ss = 0, tt = 0;
    uint32_t p = o.fl;
    // byte head up to a 16-byte aligned destination
    const uint32_t head = min(n, (uint32_t)((16 - (((uintptr_t)dst + p) & 15)) & 15));
    if (lane < head) {
        const uint32_t x = S.win[(p + lane) & IM];
        if constexpr (STORE) dst[p + lane] = (uint8_t)x;
        if (ADLER) { ss += x; tt += (uint64_t)(n - lane) * x; }
    }
    p += head;
    // 16 bytes per lane
    for (; p + 16 <= upto; p += 1024) {
        const uint32_t q = p + lane * 16;
        if (q + 16 <= upto) {
            uint32_t w[4];
            const uint32_t wp = q & IM;
            if ((wp & 15) == 0) {
                const uint4 v = *(const uint4*)&S.win[wp];
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
                for (int k = 0; k < 4; k++) {
                    uint32_t x = 0;
                    for (int j = 0; j < 4; j++) x |= (uint32_t)S.win[(q + 4 * k + j) & IM] << (8 * j);
                    w[k] = x;
                }
            }
            if constexpr (STORE) *(uint4*)&dst[q] = make_uint4(w[0], w[1], w[2], w[3]);
            if (ADLER) {
                const uint32_t rem = upto - q;   // weight of the first byte
                for (int k = 0; k < 16; k++) {
                    const uint32_t x = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                    ss += x;
                    tt += (uint64_t)(rem - k) * x;
                }
            }
        } else if (q < upto) {   // the last partial stride: bytes
            for (uint32_t t = q; t < upto; t++) {
                const uint32_t x = S.win[t & IM];
                if constexpr (STORE) dst[t] = (uint8_t)x;
                if (ADLER) { ss += x; tt += (uint64_t)(upto - t) * x; }
            }
        }
    }
    if (p < upto && lane == 0) {   // fewer than 16 bytes left after the loop
        for (uint32_t t = p; t < upto; t++) {
            const uint32_t x = S.win[t & IM];
            if constexpr (STORE) dst[t] = (uint8_t)x;
            if (ADLER) { ss += x; tt += (uint64_t)(upto - t) * x; }
        }
    }
    if (ADLER) {
        ss = wave_sum64(ss);
        tt = wave_sum64(tt);
        // a' = a + S; b' = b + n * a + T  (mod 65521)
        const uint64_t b2 = (o.b + (uint64_t)(n % 65521) * o.a + tt % 65521) % 65521;
        o.a = rfl((uint32_t)((o.a + ss % 65521) % 65521));
        o.b = rfl((uint32_t)b2);
    }
    o.fl = upto;
    __builtin_amdgcn_s_waitcnt(0);   // the stores are done: far-match reads see them
    if (o.fl >= IRENORM) {   // keep relative positions small (ob stays a multiple of W)
        o.ob += IRENORM;
        o.op -= IRENORM;
        o.fl -= IRENORM;
    }
    __syncthreads();
    IST_ADD(o, 2, IST_NOW() - ts0);
    }
}

// LDS byte address of a __shared__ object (ds_* instructions address LDS from 0)
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void*)p;
}

// ---------------------------------------------------------------------------------------
// The symbol loop's common path, hand-scheduled.  Compiled code for this state machine spent
// ~100 instructions a token (the structurizer's branch flags, copies of the stream registers
// that waited for their prefetch); this one spends ~20 on a literal and ~60 on a match.
// In SGPRs: the 64-bit bit buffer (s[94:95]), bc, wi, op; the two tables come from HBM (the
// workgroup's table area, agent-scope loads) into v64..v79 (literal/length) and v80..v95
// (distance, bases in v96..v111) and are read by
// v_readlane under s_set_gpr_idx_on.  A literal is one ds_write_b8 (every lane stores the same
// byte); a match is 64 bytes a round (lane t: byte src + t, read before the round's writes,
// when distance >= length or >= 64; byte src + t mod distance for a shorter period; a
// source older than the ring from the flushed output in HBM).  Returns at the first event it
// leaves to the caller, with nothing of the current token consumed unless noted:
//   IX_SYM   a long, end-of-block or invalid literal/length code
//   IX_SEG   a refill at a token start that needs a stream segment it does not rotate into
//            (the segment after next is not wholly inside the stream)
//   IX_LIM   op >= lim at a literal or a length (a flush the run does not do itself, or the
//            capacity), or a length that does not fit the capacity
//   IX_DIST  length decoded into len and consumed; the distance code is long or invalid, or
//            the refill in front of it needs a stream segment the run does not rotate into
//            (then bc <= 32 and the caller's refill comes first)
//   IX_MATCH len and dist decoded: a distance before the output
// Both refills (at a token start, and between a length and its distance) rotate the stream
// segments when their word is the first of vnxt, so wi - wb <= 64 at every refill and at
// every exit, which is what ib_word's single rotation needs.  (Until the second one did,
// tokens of one size dividing 32 -- zlib's runs of 2-bit tokens for constant input, at odd bit
// offsets -- could place every refill of a stretch between length and distance: nothing
// rotated, and past wb + 128 v_readlane's lane select wrapped onto words already consumed.)
// Hazards: a lane select written by SALU is 4+ instructions old at each v_readlane (s_nop 3
// where it is not); the stream prefetch is waited for before it is read and before return;
// m0 (written by s_set_gpr_idx_on) is restored.
// ---------------------------------------------------------------------------------------
// diagnostic timing builds only (the output is wrong): DMX_INF_NOFAR copies far sources from
// the ring instead of HBM, DMX_INF_NOWAIT writes a copy round without waiting for its reads
#ifdef DMX_INF_NOFAR
#define IFAR_BRANCH "s_cbranch_scc1 L_cp%=\n"
#else
#define IFAR_BRANCH "s_cbranch_scc1 L_far%=\n"
#endif
#ifdef DMX_INF_NOWAIT
#define ICOPY_WAIT
#else
#define ICOPY_WAIT "s_waitcnt lgkmcnt(0)\n"
#endif
// table lookups: lane s94 & 63 of register v64 + (s94 >> 6 & 15) (v80 + for distances, their
// bases at v96 +), read by v_readlane under the index mode: the mode indexes the readlane's
// VGPR source too (tools/gpridx_test.hip checks it on the device), so a lookup is s_bfe,
// s_set_gpr_idx_on, v_readlane, s_set_gpr_idx_off -- no VGPR copy of the indexed register
#define ILOOK_LL "s_set_gpr_idx_on s98, gpr_idx(SRC0)\n" "v_readlane_b32 s99, v64, s94\n" "s_set_gpr_idx_off\n"
#define ILOOK_D "s_set_gpr_idx_on s98, gpr_idx(SRC0)\n" "v_readlane_b32 s99, v80, s94\n" \
                "v_readlane_b32 s90, v96, s94\n" "s_set_gpr_idx_off\n"
// A copy of one round (length <= 64) is left pending: its LDS read (or HBM load, for a source
// older than the ring) is issued and the wave goes on decoding the next token while it is in
// flight; the write (lanes in s[84:85], data v116 >> v118, address v117) is issued before
// the next read of the ring, the next copy, or the return.  Literal stores in between touch
// other positions.
#define IFLUSH_PENDING(N) \
    "s_cmp_eq_u64 s[84:85], 0\n" \
    "s_cbranch_scc1 L_nf" #N "%=\n" \
    "s_waitcnt vmcnt(0) lgkmcnt(0)\n" \
    "s_mov_b64 exec, s[84:85]\n" \
    "v_lshrrev_b32 v116, v118, v116\n" \
    IWR " v117, v116\n" \
    "s_mov_b64 exec, s[86:87]\n" \
    "s_mov_b64 s[84:85], 0\n" \
    "L_nf" #N "%=:\n"
#define IX_SYM 1u
#define IX_SEG 2u
#define IX_LIM 3u
#define IX_DIST 4u
#define IX_MATCH 5u

template <uint32_t W, bool CELL>
__device__ __forceinline__ uint32_t isym_run(IBits& r, uint32_t& op, uint32_t& lim, uint32_t& fl, uint32_t capr,
                                             uint32_t fok, uint64_t gfl, uint32_t dfl, uint32_t lta,
                                             uint64_t tgl, uint64_t tgd, uint32_t toff, uint32_t lane, uint64_t gpos0,
                                             uint32_t& len, uint32_t& dist) {
    uint32_t ex;
    const uint64_t galn = gpos0 & ~3ull;   // output position 0 in HBM, as an aligned base + 0..3
    const uint32_t gmis = (uint32_t)gpos0 & 3u;
    const int32_t wrl = (int32_t)r.wfast - 192;   // rotate while the new segment is wholly inside
    const uint64_t zb = (uint64_t)(uintptr_t)r.zb;
    if constexpr (!CELL) {
#define ISYM_CELL 0
#include "dmx_isym.inc"
#undef ISYM_CELL
    } else {
#define ISYM_CELL 1
#include "dmx_isym.inc"
#undef ISYM_CELL
    }
    return ex;
}

// ---------------------------------------------------------------------------------------
// One DEFLATE block at the reader.  Returns 0 / -E_*; last = BFINAL.
// ---------------------------------------------------------------------------------------
// RING: flush to HBM every half ring (ADLER: folding the Adler-32 sums; the stream mode);
// otherwise the whole output stays in the window.  W < 32 KiB: matches farther than the ring
// read their source from the output already flushed to HBM.
// CELL: the chained decode of dictionary streams -- the window and the output hold 16-bit
// cells; a match reaching before the sw block's first byte writes reference cells there.
// STORE = false: nothing is written to o.out, which may then be NULL -- only with ADLER and
// W == IW: the asm run then never flushes by itself (fok is 0), the far-source paths below are
// compiled out, and the run's own far branch needs dist > W, which no distance code spells
// (24 577 + 8 191 = 32 768).
template <bool RING, bool ADLER, uint32_t W, bool CELL = false, bool STORE = true>
__device__ __forceinline__ int iblock(InfLDS<W, typename std::conditional<CELL, uint16_t, uint8_t>::type>& S, IBits& r,
                                      IOut& o, uint32_t* __restrict__ gt, uint32_t lane, bool& last) {
    constexpr uint32_t IM = W - 1, FL = W / 2;
    constexpr uint32_t CS = CELL ? 2 : 1;   // bytes per output position
    static_assert(STORE || (RING && ADLER && W == IW && !CELL), "without stores: the stream mode's ring only");
    [[maybe_unused]] const unsigned long long ts0 = IST_NOW();
    IST_ADD(o, 6, 1);
    last = ib_bits(r, 1) != 0;
    const uint32_t bt = ib_bits(r, 2);
    if (bt == 0) {   // stored
        ib_drop(r, r.bc & 7);
        const uint32_t len = ib_bits(r, 16), nlen = ib_bits(r, 16);
        if (len != (~nlen & 0xFFFFu)) return -(int)E_ZNLEN;
        if (len > io_caprel(o) - o.op) return -(int)E_SZ;
        const uint64_t src = ib_bytepos(r);   // relative to z
        if (src + len + r.lo > r.hi) return -(int)E_LEN;
        gu8* zs = r.zb + r.lo + src;
        for (uint32_t c0 = 0; c0 < len; c0 += FL) {   // pieces the ring can hold
            if (RING && o.op - o.fl > W - FL) io_flush<ADLER, STORE>(S, o, o.op, lane);
            const uint32_t ce = min(len, c0 + FL);
            for (uint32_t j = c0 + lane; j < ce; j += 64) S.win[(o.op + (j - c0)) & IM] = zs[j];
            o.op += ce - c0;
        }
        __syncthreads();
        ib_seek(r, (src + len) * 8);
        return 0;
    }
    if (bt == 3) return -(int)E_ZBTYPE;
    int nlen = 288, ndist = 30;
    if (bt == 1) {   // fixed codes
        for (int s = (int)lane; s < 320; s += 64)
            S.seq[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
    } else {
        nlen = (int)ib_bits(r, 5) + 257;
        ndist = (int)ib_bits(r, 5) + 1;
        const int ncode = (int)ib_bits(r, 4) + 4;
        if (nlen > 286 || ndist > 30) return -(int)E_ZINV;
        if (lane < 19) S.len[lane] = 0;
        __syncthreads();
        for (int k = 0; k < ncode; k++) {
            const uint32_t v = ib_bits(r, 3);
            if (lane == 0) S.len[c_iclorder[k]] = (uint8_t)v;
        }
        __syncthreads();
        [[maybe_unused]] const unsigned long long tc0 = IST_NOW();
        if (itable_build<false>(S, S.lt, gt, 19, lane) != 0) return -(int)E_HUFAMB;
        [[maybe_unused]] const unsigned long long tc1 = IST_NOW();
        IST_ADD(o, 7, tc1 - tc0);
        uint32_t prev = 0;
        int idx = 0, err = 0;
        while (idx < nlen + ndist) {
            ib_refill(r);
            const uint32_t e = ientry_cl(r, S.lt, gt);
            if (e == ISLOW) { err = -(int)E_HUFINV; break; }
            ib_drop(r, e & 15u);
            const uint32_t sy = e >> 4;
            if (sy < 16) {
                if (lane == 0) S.seq[idx] = (uint8_t)sy;
                prev = sy;
                idx++;
            } else {
                uint32_t rep, v = 0;
                if (sy == 16) {
                    if (idx == 0) { err = -(int)E_ZINV; break; }
                    v = prev;
                    rep = 3 + ib_bits(r, 2);
                } else if (sy == 17) {
                    rep = 3 + ib_bits(r, 3);
                } else {
                    rep = 11 + ib_bits(r, 7);
                }
                if (idx + (int)rep > nlen + ndist) { err = -(int)E_ZINV; break; }
                for (uint32_t q = lane; q < rep; q += 64) S.seq[idx + q] = (uint8_t)v;
                prev = v;
                idx += (int)rep;
            }
        }
        if (err) return err;
        __syncthreads();
        if (rfl(S.seq[256]) == 0) return -(int)E_ZINV;
    }
    // literal/length table from seq[0, nlen), distance table from seq[nlen, nlen + ndist)
    for (int s = (int)lane; s < 288; s += 64) S.len[s] = s < nlen ? S.seq[s] : 0;
    __syncthreads();
    [[maybe_unused]] const unsigned long long tl0 = IST_NOW();
    IST_ADD(o, 8, tl0 - ts0);
    int e = itable_build<false>(S, S.lt, gt, nlen, lane);
    [[maybe_unused]] const unsigned long long tl1 = IST_NOW();
    IST_ADD(o, 9, tl1 - tl0);
    // an incomplete code is allowed only as a single code of length 1 (offs[15] + cnt[15]: the
    // number of codes); a distance table without any code is legal until a length needs it
    if (e < 0 || (e > 0 && bt == 2 && !(rfl(S.lt.offs[15] + S.lt.cnt[15]) == 1 && rfl(S.lt.cnt[1]) == 1)))
        return -(int)E_HUFAMB;
    for (int s = (int)lane; s < 32; s += 64) S.len[s] = s < ndist ? S.seq[nlen + s] : 0;
    __syncthreads();
    e = itable_build<true>(S, S.dt, gt + (1u << IFB), ndist, lane);
    IST_ADD(o, 10, IST_NOW() - tl1);
    if (e < 0 || (e > 0 && bt == 2 && rfl(S.dt.offs[15] + S.dt.cnt[15]) != 0 &&
                  !(rfl(S.dt.offs[15] + S.dt.cnt[15]) == 1 && rfl(S.dt.cnt[1]) == 1)))
        return -(int)E_HUFAMB;

    // symbols: the common path in isym_run (literals, lengths and distances with table codes,
    // matches inside the ring without overlap or with a period >= 64); the rest here.
    uint32_t op = o.op;
    uint32_t capr = io_caprel(o);
    int err = 0;
    [[maybe_unused]] const unsigned long long ts1 = IST_NOW();
    IST_ADD(o, 0, ts1 - ts0);
    if (lds_addr(S.win) != 0) return -(int)E_RANGE;   // isym_run addresses the ring from LDS 0
    const uint64_t tgl = (uint64_t)(uintptr_t)gt, tgd = tgl + 4 * (1u << IFB);   // the tables' words, 4 bytes a lane
    const uint32_t dfl = o.ob != 0 ? 0x40000000u : 0u;   // stream mode: sources before ob exist
    const uint64_t gpos0 = (uint64_t)(uintptr_t)(o.out + CS * (o.base + o.ob));
    // the run flushes half rings itself (no Adler sums; a 16-byte aligned output)
    const uint32_t fok = (uint32_t)__builtin_amdgcn_readfirstlane((RING && !ADLER && (gpos0 & 15) == 0) ? 1 : 0);
    // the literal/length table's canonical arrays (long codes inside the run; 16-byte aligned:
    // the ring before them is W positions)
    const uint32_t lta = (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_addr(&S.lt));
    static_assert((W * CS) % 16 == 0 && sizeof(ITable) == 672, "the run's ITable offsets (dmx_isym.inc)");
    for (;;) {
        // The input's end bounds the loop: the reader hands out zeros behind it, and where they
        // spell literals or matches only the capacity would end a cut stream -- never, with an
        // unlimited capacity under MEASURE.  The run returns here at least every half ring, so at
        // most FL + 258 positions are decoded from those zeros (ib_status: -E_LEN).  A valid
        // stream never has consumed more than it holds while a block is still open.
        if (ib_past(r)) { err = -(int)E_LEN; break; }
        uint32_t lim = RING ? min(capr, o.fl + FL) : capr, fl = o.fl;
        uint32_t len, dist;
        const uint32_t ex = isym_run<W, CELL>(r, op, lim, fl, capr, fok, gpos0, dfl, lta, tgl, tgd, lane * 4, lane, gpos0,
                                              len, dist);
        o.fl = fl;
        IST_ADD(o, 5, 1);
        IST_ADD(o, 11, ex == IX_SYM ? 1 : 0);
        IST_ADD(o, 12, ex == IX_SEG ? 1 : 0);
        IST_ADD(o, 13, ex == IX_LIM ? 1 : 0);
        IST_ADD(o, 14, ex == IX_DIST ? 1 : 0);
        IST_ADD(o, 15, ex == IX_MATCH ? 1 : 0);
        if (ex == IX_SEG) {   // a refill at a token start that the run does not rotate into
            ib_refill(r);
            continue;
        }
        if (ex == IX_LIM && RING && op - o.fl >= FL) {
            o.op = op;
            io_flush<ADLER, STORE>(S, o, o.fl + FL, lane);
            op = o.op;
            capr = io_caprel(o);
            continue;
        }
        uint32_t en = 0;
        if (ex == IX_SYM || ex == IX_LIM) {   // one symbol the general way (nothing consumed)
            ib_refill(r);
            en = rfl(gtab_ld(gt + ib_peek(r, IFB)));
            if (en == IVSLOW) {
                const uint32_t e16 = ientry_slow(r, S.lt);
                if (e16 == ISLOW) { err = -(int)E_HUFINV; break; }
                en = iv_ll(e16);
            }
            if (!(en & 0x8000u)) {   // a literal: at the capacity limit, or a long code
                ib_drop(r, en & 31u);
                if (op >= capr) { err = -(int)E_SZ; break; }
                S.win[op & IM] = (uint8_t)(en >> 16);   // (a byte value in a cell, too)
                op++;
                continue;
            }
            if (en & 0x4000u) {
                ib_drop(r, en & 31u);
                if (en & 0x2000u) err = -(int)E_HUFVAL;
                break;   // end of block
            }
            len = (en >> 23) + iv_extra(r.bb, en);
            ib_drop(r, (en >> 8) & 31u);
        }
        if (ex != IX_MATCH) {   // the distance the general way
            ib_refill(r);
            uint32_t ed = rfl(gtab_ld(gt + (1u << IFB) + ib_peek(r, IFB)));
            if (ed >= IVBAD) {
                // no code at the reader (an unused code of an incomplete table, a table without
                // codes, the fixed code's 30 and 31): -E_HUFINV; -E_HUFVAL is a decoded symbol
                // out of range, which no distance table of at most 30 symbols can produce
                const uint32_t e16 = ed == IVSLOW ? ientry_slow(r, S.dt) : ISLOW;
                if (e16 == ISLOW) { err = -(int)E_HUFINV; break; }
                ed = iv_d(e16);
                if (ed == IVBAD) { err = -(int)E_HUFVAL; break; }
            }
            dist = iv_dbase(ed) + iv_extra(r.bb, ed);
            ib_drop(r, (ed >> 8) & 31u);
        }
        if (o.ob == 0 && dist > op && (!CELL || dist - op > o.base)) { err = -(int)E_HUFDIS; break; }
        if (len > capr - op) { err = -(int)E_SZ; break; }
        if (RING && op - o.fl >= FL) {   // half the ring is due before this match
            o.op = op;
            io_flush<ADLER, STORE>(S, o, o.fl + FL, lane);
            op = o.op;
            capr = io_caprel(o);
        }
        const uint32_t src = op - dist;
        IST_ADD(o, 3, 1);
        if (CELL && dist > op) {   // (o.ob == 0 here) from before the sw block: reference cells
            const uintptr_t g = (uintptr_t)(o.out + CS * o.base);
            auto cell_at = [&](uint32_t t) -> uint32_t {   // output position op + t
                const int32_t sp = (int32_t)op - (int32_t)dist + (int32_t)t;
                if (sp < 0) return 0xFFu + (uint32_t)(-sp);   // 0x100 + (back - 1)
                if (t >= dist) return S.win[(op + t - dist) & IM];   // this match's own output
                if (W < IW && dist > W) {   // flushed: from the cell buffer
                    const uintptr_t a = g + CS * (uintptr_t)sp;
                    const uint32_t w = __hip_atomic_load((gu32*)(a & ~(uintptr_t)3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    return (w >> (8 * (a & 3))) & 0xFFFFu;
                }
                return S.win[(uint32_t)sp & IM];
            };
            if (len <= dist) {
                for (uint32_t t = lane; t < len; t += 64) S.win[(op + t) & IM] = cell_at(t);
            } else {   // the match overlaps itself (rare): in order, one lane
                if (lane == 0)
                    for (uint32_t t = 0; t < len; t++) S.win[(op + t) & IM] = cell_at(t);
            }
            __syncthreads();
        } else if (W < IW && dist > W) {
            IST_ADD(o, 4, 1);
            // older than the ring: from the output in HBM, flushed before this match (op - fl
            // stays below W / 2 + 258, so every source byte lies below fl).  Agent-scope loads
            // go to L2, past any vector-L1 copy of a line that was flushed in two pieces.
            const uintptr_t g = (uintptr_t)(o.out + CS * (o.base + o.ob));
            for (uint32_t t = lane; t < len; t += 64) {
                const uintptr_t a = g + CS * (uintptr_t)(src + t);
                const uint32_t w = __hip_atomic_load((gu32*)(a & ~(uintptr_t)3), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                S.win[(op + t) & IM] = CELL ? (w >> (8 * (a & 3))) & 0xFFFFu : (w >> (8 * (a & 3))) & 0xFFu;
            }
        } else if (dist >= 64 || dist >= len) {   // every read is of bytes written before its round
            for (uint32_t t = lane; t < len; t += 64) S.win[(op + t) & IM] = S.win[(src + t) & IM];
        } else {   // short period: byte t repeats byte t mod dist
            const float inv = 1.0f / (float)dist;
            for (uint32_t t = lane; t < len; t += 64) {
                int q = (int)((float)t * inv);
                int rm = (int)t - q * (int)dist;
                if (rm >= (int)dist) rm -= (int)dist;
                if (rm < 0) rm += (int)dist;
                S.win[(op + t) & IM] = S.win[(src + (uint32_t)rm) & IM];
            }
        }
        op += len;
    }
    o.op = op;
    IST_ADD(o, 1, IST_NOW() - ts1);
    return err;   // (the caller folds the end of the input in: ib_status)
}

// CELL: out is the cell buffer (2 bytes a position), out_cap in positions.  max_len: the largest
// out_len of an entry -- IW for dmx_inflate_async and for the cells (a reference cell holds a
// distance below IW, and the chained lists 16-bit offsets), DMX_BGZF_MAX_ISIZE for the members of
// dmx_inflate_members_async.  Nothing below depends on it (the audit): positions
// are 32-bit, the ring index is a mask, and sources older than the ring come from d_out.
// COUNTED (dmx_bgzf_read_ranges_async): the grid is a capacity the host knows, the number of entries
// the word *count that the planning kernels left in device memory.  A workgroup at or past it leaves
// at once, a uniform exit on one scalar load; without COUNTED count is not read (NULL).
template <bool CELL, bool COUNTED = false>
__global__ __launch_bounds__(64) void dmx_inflate_index_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                               const dmx_iblock* __restrict__ index,
                                                               uint8_t* __restrict__ out, uint64_t out_cap,
                                                               uint32_t* __restrict__ gtab, uint32_t max_len,
                                                               dmx_inflate_status* __restrict__ st,
                                                               const uint32_t* __restrict__ count) {
    if (COUNTED && blockIdx.x >= *count) return;
    // bytes: an 8 KiB ring, 10 KiB of LDS; cells: 4 096 cells, the same 10 KiB.  12 workgroups
    // per CU (151 VGPRs: 3 waves per SIMD), so 3 072 blocks decode at once
    constexpr uint32_t WR = CELL ? IWC : IWX;
    __shared__ InfLDS<WR, typename std::conditional<CELL, uint16_t, uint8_t>::type> S;
    uint32_t* gt = gtab + (uint64_t)blockIdx.x * ITAB_WORDS;
    const uint32_t lane = threadIdx.x;
    IBits r;
    ib_init(r, z, zbytes);
    const uint64_t bit = rfl64(index[blockIdx.x].bit);
    const uint64_t off = rfl64(index[blockIdx.x].out_off);
    const uint32_t olen = rfl(index[blockIdx.x].out_len);
    IOut o;
#ifdef DMX_INF_STAMPS
    for (int k = 0; k < INF_NST; k++) o.st[k] = 0;
#endif
    o.out = out;
    o.base = off;
    o.ob = 0;
    o.cap = olen;
    o.op = 0;
    o.fl = 0;
    o.a = 1;
    o.b = 0;
    int err = 0;
    if (olen > max_len || off > out_cap || olen > out_cap - off || (bit >> 3) >= zbytes) err = -(int)E_RANGE;
    if (!err) {
        ib_seek(r, bit);
        bool last = false;
        do {   // one sw block may be several DEFLATE blocks (DMX_F_SPLIT)
            err = ib_status(r, iblock<true, false, WR, CELL>(S, r, o, gt, lane, last));
        } while (!err && o.op < olen && !last);
        if (!err && o.op != olen) err = -(int)E_SZ;
        if (!err) io_flush<false>(S, o, o.op, lane);
    }
    if (lane == 0 && err) atomicCAS(&st->status, 0, err);
    if (lane == 0 && !err) atomicAdd((unsigned long long*)&st->out_len, (unsigned long long)o.op);
#ifdef DMX_INF_STAMPS
    if (lane < INF_NST && blockIdx.x < (1u << 16)) dmx_inf_st[blockIdx.x][lane] = o.st[lane];
#endif
}

__global__ __launch_bounds__(64) void dmx_inflate_stream_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                                uint8_t* __restrict__ out, uint64_t out_cap,
                                                                uint32_t* __restrict__ gtab,
                                                                dmx_inflate_status* __restrict__ st) {
    __shared__ InfLDS<IW> S;
    const uint32_t lane = threadIdx.x;
    IBits r;
    ib_init(r, z, zbytes);
    IOut o;
#ifdef DMX_INF_STAMPS
    for (int k = 0; k < INF_NST; k++) o.st[k] = 0;
#endif
    o.out = out;
    o.base = 0;
    o.ob = 0;
    o.cap = out_cap;
    o.op = 0;
    o.fl = 0;
    o.a = 1;
    o.b = 0;
    int err = 0;
    if (zbytes < 2) err = -(int)E_ZHEAD;   // (a header and nothing behind it: -E_LEN at the first block)
    if (!err) {
        const uint32_t cmf = z[0], flg = z[1];
        if ((cmf & 0x0F) != 8) err = -(int)E_ZCMPMT;
        else if ((cmf >> 4) > 7) err = -(int)E_ZSLWIN;
        else if (((cmf << 8) | flg) % 31) err = -(int)E_ZFCHCK;
        else if (flg & 0x20) err = -(int)E_ZPDICT;
    }
    if (!err) {
        ib_seek(r, 16);
        bool last = false;
        while (!err && !last) err = ib_status(r, iblock<true, true, IW>(S, r, o, gtab, lane, last));
    }
    if (!err) {
        io_flush<true>(S, o, o.op, lane);
        ib_drop(r, r.bc & 7);   // Adler-32 trailer, MSB first
        uint32_t want = 0;
        for (int k = 0; k < 4; k++) want = (want << 8) | ib_bits(r, 8);
        if (ib_past(r)) err = -(int)E_ZADL32;   // cut inside the trailer
        else if (((o.b << 16) | o.a) != want) err = -(int)E_ZADL32;
    }
    if (lane == 0) {
        if (err) atomicCAS(&st->status, 0, err);
        else st->out_len = o.ob + o.op;
    }
}

// ------------------------------------------------------------------------------------
// Batches of independent streams (dmx_inflate_batch_async, include/dmx.h): the stream kernel's
// body with per-stream parameters.  One wave per workgroup and the IW ring (34 KB of LDS: four
// workgroups per CU); the grid is what the device holds at once, and a workgroup claims streams
// from a device counter, in index order, until none is left -- its table area in d_work and its
// ring serve one stream after the other (a stream's matches never reach before its own first
// byte: o.ob == 0 and dist > op is -E_HUFDIS, so what the ring held before is never read).
// Everything per stream is wave-uniform: the descriptor, the framing (dmx_gz_head.h, the text of
// the host's header checks), the trailers.  The reader hands out zeros past in_len and never
// loads a byte behind the stream (ib_vload: whole aligned words that end inside it -- the first
// may begin up to 3 bytes in front, which are shifted out -- and single bytes at its end), so a
// stream that ends early is -E_LEN through ib_status, not a decode of its neighbour.
// MEASURE: no store to d_out (iblock / io_flush with STORE = false); out may be NULL, cap is only
// a limit.  A gzip member's CRC-32 needs the bytes: the decode leaves status 0 and, in reserved, a
// note of a wrong ISIZE for the CRC pass (dmx_crc_batch_kernel), which finalises the member and
// counts it in the summary; under MEASURE there is no such pass and a wrong ISIZE is -E_LEN here.
// ------------------------------------------------------------------------------------
#define IBATCH_MAX_WG 2048u   // the grid's fixed upper bound: d_work holds this many table areas at most

struct IBatchCtl {   // the first 256 bytes of d_work
    unsigned long long next;   // the claim counter
};

__global__ void dmx_inflate_batch_clear_kernel(IBatchCtl* __restrict__ ctl, dmx_batch_status* __restrict__ st) {
    ctl->next = 0;
    st->nfailed = 0;
    st->first_bad = 0xFFFFFFFFu;
    st->total_out = 0;
}

// Preset dictionaries (dmx_inflate_batch_dict_async; DICT).  A dictionary is output that was flushed
// before the stream began: its last dlen <= IW bytes go to win[0, dlen), the stream starts with
// op = fl = dlen, base = out_off - dlen (the first flushed byte lands at out_off; Adler-32 is folded
// over flushed bytes only) and cap = out_cap + dlen, and reports ob + op - dlen.  Nothing below that
// level knows: the too-far test is dist > op while ob == 0, the ring invariant, isym_run, the stored
// copy and the renormalisation see positions only, and with W == IW no distance exceeds the ring
// (dlen == IW fills it exactly; a first match at distance IW reads the slot it is about to write, as
// such a match does mid-stream).  A stream without a dictionary starts at op = 0 as before, so what
// the ring held for the stream before it -- primed bytes included -- is never read.
struct IBatchDict {   // by value; all zero (no dictionaries) for the instantiations without DICT
    const uint8_t* dict;       // d_dict
    uint64_t dict_bytes;
    const dmx_bdict* dicts;
    const uint32_t* dict_of;   // NULL: every stream uses dictionary 0
    const uint32_t* adler;     // in d_work: the Adler-32 of every dictionary (dmx_dict_adler_kernel)
    uint32_t ndicts;
};

// win[0, n) = src[0, n), n <= IW: 16-byte loads of the aligned groups inside the range, single bytes
// at its edges (no byte outside src[0, n) is loaded); everything is wave-uniform but the lane's share
__device__ __forceinline__ void iprime(uint8_t* win, const uint8_t* src, uint32_t n, uint32_t lane) {
    const uint32_t head = min(n, (uint32_t)((16 - ((uintptr_t)src & 15)) & 15));
    if (lane < head) win[lane] = src[lane];
    const uint32_t groups = (n - head) >> 4;
    for (uint32_t g = lane; g < groups; g += 64) {
        const uint32_t p = head + 16 * g;
        const uint4 v = *reinterpret_cast<const uint4*>(src + p);
        if (head == 0) {
            *reinterpret_cast<uint4*>(win + p) = v;
        } else if ((head & 3) == 0) {
            uint32_t* w = reinterpret_cast<uint32_t*>(win + p);
            w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        } else {
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 16; j++) win[p + j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
        }
    }
    const uint32_t tail = head + 16 * groups;   // fewer than 16 bytes behind the last group
    if (lane < n - tail) win[tail + lane] = src[tail + lane];
    __syncthreads();
}

// The Adler-32 of every dictionary of a call into adl[j] (0 for an entry outside the buffer: the
// decode refuses it before it looks), one block of 256 threads per dictionary.  A thread takes a
// slice whose edges are 16-byte aligned addresses and folds it in pieces of at most 4 096 bytes
// with position-weighted sums, as io_flush does (a' = a + S, b' = b + n a + T mod 65521, from
// a = b = 0); the slices combine by the same rule, and the leading 1 of Adler-32 adds len to b.
// the Adler-32 of src[0, n) into *adl, by the 256 threads of one block
__device__ __forceinline__ void dict_adler_block(const uint8_t* src, uint64_t n, uint32_t* adl) {
    __shared__ uint32_t sa[256], sb[256];
    constexpr uint32_t M = 65521u;
    const uint32_t t = threadIdx.x;
    const uintptr_t p = (uintptr_t)src, a0 = p & ~(uintptr_t)15;
    const uint8_t* q = reinterpret_cast<const uint8_t*>(a0);   // positions below are relative to a0
    const uint64_t pb = p - a0, pe = pb + n;
    const uint64_t sl = ((pe + 255) / 256 + 15) & ~15ull;
    uint64_t lo = (uint64_t)t * sl, hi = lo + sl;
    if (lo < pb) lo = pb;
    if (hi > pe) hi = pe;
    uint32_t a = 0, b = 0;
    for (uint64_t i = lo; i < hi;) {
        const uint64_t ce = hi - i > 4096 ? i + 4096 : hi;
        uint32_t cs = 0;
        uint64_t ct = 0;   // <= 4096 * 4096 * 255
        uint64_t x = i;
        for (; x < ce && (x & 15); x++) { cs += q[x]; ct += (ce - x) * q[x]; }
        for (; x + 16 <= ce; x += 16) {
            const uint4 v = *reinterpret_cast<const uint4*>(q + x);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t c = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                cs += c;
                ct += (ce - x - k) * c;
            }
        }
        for (; x < ce; x++) { cs += q[x]; ct += (ce - x) * q[x]; }
        b = (uint32_t)((b + (ce - i) * a + ct % M) % M);
        a = (a + cs) % M;
        i = ce;
    }
    // the slice's share of the whole: its bytes are added to b once more for every byte behind it
    sa[t] = a;
    sb[t] = lo < hi ? (uint32_t)((b + ((pe - hi) % M) * a) % M) : 0u;
    __syncthreads();
    if (t == 0) {
        uint64_t A = 1, B = n % M;
        for (int k = 0; k < 256; k++) { A += sa[k]; B += sb[k]; }
        *adl = ((uint32_t)(B % M) << 16) | (uint32_t)(A % M);
    }
}
__global__ __launch_bounds__(256) void dmx_dict_adler_kernel(const uint8_t* __restrict__ dict, uint64_t dict_bytes,
                                                             const dmx_bdict* __restrict__ dicts,
                                                             uint32_t* __restrict__ adl) {
    const uint32_t j = blockIdx.x;
    const uint64_t off = dicts[j].off, n = dicts[j].len;
    if (off > dict_bytes || n > dict_bytes - off) {   // (uniform)
        if (threadIdx.x == 0) adl[j] = 0;
        return;
    }
    dict_adler_block(dict + off, n, adl + j);
}
// one dictionary given by value: the DICTID of a DMX_F_FDICT encode (dmx_encode_async, dmx_kernels.hip)
__global__ __launch_bounds__(256) void dmx_dict_adler_one_kernel(const uint8_t* __restrict__ dict, uint64_t n,
                                                                 uint32_t* __restrict__ adl) {
    dict_adler_block(dict, n, adl);
}
int dmx_dict_adler_launch(const void* d_dict, uint64_t n, uint32_t* d_adl, hipStream_t s) {
    hipLaunchKernelGGL(dmx_dict_adler_one_kernel, dim3(1), dim3(256), 0, s, (const uint8_t*)d_dict, n, d_adl);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}
int dmx_dict_adler_batch_launch(const void* d_dict, uint64_t dict_bytes, const dmx_bdict* d_dicts, uint32_t ndicts,
                                uint32_t* d_adl, hipStream_t s) {
    hipLaunchKernelGGL(dmx_dict_adler_kernel, dim3(ndicts), dim3(256), 0, s, (const uint8_t*)d_dict, dict_bytes, d_dicts, d_adl);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

template <bool MEASURE, bool DICT = false>
__global__ __launch_bounds__(64) void dmx_inflate_batch_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                               const dmx_bstream* __restrict__ streams, uint32_t nstreams,
                                                               uint32_t fmt, uint8_t* out, uint64_t out_bytes,
                                                               dmx_bresult* __restrict__ res, uint32_t* __restrict__ gtab,
                                                               IBatchCtl* __restrict__ ctl,
                                                               dmx_batch_status* __restrict__ st, const IBatchDict dd) {
    __shared__ InfLDS<IW> S;   // the kernel's one __shared__ object: isym_run addresses the ring from LDS 0
    uint32_t* gt = gtab + (uint64_t)blockIdx.x * ITAB_WORDS;
    const uint32_t lane = threadIdx.x;
    for (;;) {
        unsigned long long claim = 0;
        if (lane == 0) claim = atomicAdd(&ctl->next, 1ull);
        const uint64_t k64 = rfl64(claim);
        if (k64 >= nstreams) break;
        const uint32_t k = (uint32_t)k64;
        const uint64_t in_off = rfl64(streams[k].in_off), in_len = rfl64(streams[k].in_len);
        const uint64_t out_off = rfl64(streams[k].out_off), out_cap = rfl64(streams[k].out_cap);
        int err = 0;
        uint32_t format = fmt;   // (0 under AUTO until the first two bytes are read)
        uint64_t body = 0, olen = 0, used = 0;
        uint32_t check = 0, note = 0;
        if (in_off > zbytes || in_len > zbytes - in_off || in_len > 0xFFFFFFF0ull) err = -(int)E_RANGE;
        if (!MEASURE && (out_off > out_bytes || out_cap > out_bytes - out_off)) err = -(int)E_RANGE;
        const uint8_t* zs = z + in_off;
        uint32_t dlen = 0;   // primed bytes (DICT)
        if constexpr (DICT) {
            // the stream's dictionary: its index, its range, its check value -- all wave-uniform
            const uint32_t di = rfl(dd.dict_of ? dd.dict_of[k] : dd.ndicts ? 0u : DMX_BATCH_NODICT);
            const uint8_t* dsrc = nullptr;
            uint32_t dadl = 0, dl = 0;
            bool have = false;
            if (!err && di != DMX_BATCH_NODICT) {
                if (di >= dd.ndicts) {
                    err = -(int)E_RANGE;
                } else {
                    const uint64_t doff = rfl64(dd.dicts[di].off), dn = rfl64(dd.dicts[di].len);
                    if (doff > dd.dict_bytes || dn > dd.dict_bytes - doff) {
                        err = -(int)E_RANGE;
                    } else {
                        have = true;
                        dadl = rfl(dd.adler[di]);
                        dl = dn < IW ? (uint32_t)dn : (uint32_t)IW;
                        dsrc = dd.dict + doff + (dn - dl);
                    }
                }
            }
            bool primed = false;
            if (!err) err = dmx_frame_head_dict(zs, in_len, fmt, have, dadl, &format, &body, &primed);
            err = (int)rfl((uint32_t)err);
            if (!err && rfl(primed ? 1u : 0u)) {
                dlen = dl;
                iprime(S.win, dsrc, dlen, lane);
            }
        } else {
            if (!err) err = dmx_frame_head(zs, in_len, fmt, &format, &body);
        }
        format = rfl(format);
        body = rfl64(body);
        err = (int)rfl((uint32_t)err);
        IBits r;
        IOut o;
#ifdef DMX_INF_STAMPS
        for (int q = 0; q < INF_NST; q++) o.st[q] = 0;
#endif
        o.out = out;
        // base lies below the window by the primed bytes.  The unsigned subtraction wraps when out_off <
        // dlen (always under MEASURE, where it is 0 - dlen on a NULL out): that is meant.  out + base is
        // only ever used with a position p >= fl >= dlen added (io_flush's dst + p), which is back inside
        // the window; the run's far-source base (gpos0) is dead code with W == IW.  Do not clamp it.
        o.base = (MEASURE ? 0 : out_off) - dlen;
        o.ob = 0;
        o.cap = out_cap > ~0ull - dlen ? ~0ull : out_cap + dlen;
        o.op = dlen;
        o.fl = dlen;
        o.a = 1;
        o.b = 0;
        if (!err) {
            ib_init(r, zs, in_len);
            ib_seek(r, body * 8);
            // the loop's exit is made uniform for the compiler too (readfirstlane): what the reader
            // holds in scalar registers is then one value behind the loop, not a value per lane
            for (;;) {
                bool last = false;
                const int e = ib_status(r, iblock<true, true, IW, false, !MEASURE>(S, r, o, gt, lane, last));
                err = (int)rfl((uint32_t)e);
                if (err || rfl(last ? 1u : 0u)) break;
            }
        }
        if (!err) {
            r.wi = rfl(r.wi);
            r.bc = rfl(r.bc);
            io_flush<true, !MEASURE>(S, o, o.op, lane);
            olen = o.ob + o.op - dlen;
            ib_drop(r, r.bc & 7);   // the trailer starts at the next byte; a raw stream ends there
            // in_used from the reader's position here, in front of the three-way branch, plus the
            // trailer's size: taken from the reader behind the branch (ib_bytepos), the raw path's
            // 64-bit word index came out of the compiler undefined (seen in the ISA and
            // as garbage in_used values; tests/test_gpu_inflate_batch.py checks in_used per format)
            used = rfl64(ib_used(r) / 8 - r.lo) + (format == DMX_BATCH_ZLIB ? 4u : format == DMX_BATCH_GZIP ? 8u : 0u);
            if (format == DMX_BATCH_ZLIB) {   // Adler-32, MSB first
                for (int q = 0; q < 4; q++) check = (check << 8) | ib_bits(r, 8);
                if (ib_past(r) || ((o.b << 16) | o.a) != check) err = -(int)E_ZADL32;
            } else if (format == DMX_BATCH_GZIP) {   // CRC-32 and ISIZE, little-endian
                uint32_t isize = 0;
                for (int q = 0; q < 4; q++) check |= ib_bits(r, 8) << (8 * q);
                for (int q = 0; q < 4; q++) isize |= ib_bits(r, 8) << (8 * q);
                if (ib_past(r)) err = -(int)E_CRC;   // cut inside the trailer
                else if (isize != (uint32_t)olen) {
                    if (MEASURE) err = -(int)E_LEN;
                    else note = 1;   // the CRC is checked first: the CRC pass reports it
                }
            }
        }
        if (lane == 0) {
            dmx_bresult v;
            v.status = err;
            v.format = format;
            v.out_len = err ? 0 : olen;
            v.in_used = err ? 0 : used;
            v.check = err ? 0 : check;
            v.reserved = err ? 0 : note;
            res[k] = v;
            if (err) {
                atomicAdd(&st->nfailed, 1u);
                atomicMin(&st->first_bad, k);
            } else if (MEASURE || format != DMX_BATCH_GZIP) {   // (a gzip member: the CRC pass counts it)
                atomicAdd((unsigned long long*)&st->total_out, (unsigned long long)olen);
            }
        }
        __syncthreads();   // the ring and the small arrays are the next stream's
    }
}

// ------------------------------------------------------------------------------------
// Seek points (dmx_inflate_points_async, include/dmx.h; DESIGN.md 3.1 "Seek points"): entries of
// the index dmx_zindex_build_host made of one foreign stream, a wave each, with the batch decode's
// geometry -- one wave per workgroup, the IW ring, workgroups claiming entries from the counter in
// d_work, the first-level tables behind it.  Entry e is point k = sel[e]: its window is output that
// was flushed before the point began, exactly a preset dictionary (the arithmetic above IBatchDict):
// the wlen = min(out_off, IW) bytes at the end of slot k prime win[0, wlen), op = fl = wlen,
// base = dst - wlen, cap = out_len + wlen.  A point with out_off forged to 0 starts at op = 0, so
// what the ring held for the entry before it is never read (dist > op is -E_HUFDIS).
// The reader is set up on the point's own bytes, z[bit >> 3, ceil(end_bit / 8)), and sought to
// bit & 7: zeros past them, an overrun is -E_LEN through ib_status, and only the extent of one point
// has to fit the reader's 32-bit positions.  Blocks are decoded until the bits consumed are exactly
// end_bit; a boundary beyond it, or BFINAL short of it, is -E_SZ, and so is an output that is not
// out_len at the end.  The capacity is always the finite out_len + wlen: the symbol loop ends by
// capacity, a block without output consumes input and the loop over blocks ends at end_bit, so every
// loop here is bounded, and iblock's symbol loop also ends with the input (ib_past), whatever the
// capacity.  Long zero-run streams (zlib's 4.2 MB blocks of two 1-bit codes) are in the GPU suite,
// whole and by ranges (tests/test_gpu_refill.py; the refill they starved: isym_run's header).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void dmx_inflate_points_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                                const dmx_zpoint* __restrict__ points,
                                                                const uint32_t* __restrict__ adler,
                                                                const uint8_t* __restrict__ windows, uint32_t npoints,
                                                                const uint32_t* __restrict__ sel,
                                                                const uint64_t* __restrict__ dst_off, uint32_t nsel,
                                                                uint8_t* out, uint64_t out_bytes,
                                                                dmx_bresult* __restrict__ res, uint32_t* __restrict__ gtab,
                                                                IBatchCtl* __restrict__ ctl,
                                                                dmx_batch_status* __restrict__ st) {
    __shared__ InfLDS<IW> S;   // the kernel's one __shared__ object: isym_run addresses the ring from LDS 0
    uint32_t* gt = gtab + (uint64_t)blockIdx.x * ITAB_WORDS;
    const uint32_t lane = threadIdx.x;
    for (;;) {
        unsigned long long claim = 0;
        if (lane == 0) claim = atomicAdd(&ctl->next, 1ull);
        const uint64_t e64 = rfl64(claim);
        if (e64 >= nsel) break;
        const uint32_t e = (uint32_t)e64;
        const uint32_t k = rfl(sel ? sel[e] : e);
        int err = 0;
        uint64_t bit = 0, end_bit = 0, out_off = 0, out_len = 0, dst = 0, first = 0, ext = 0;
        if (k >= npoints) {
            err = -(int)E_RANGE;
        } else {
            bit = rfl64(points[k].bit);
            end_bit = rfl64(points[k].end_bit);
            out_off = rfl64(points[k].out_off);
            out_len = rfl64(points[k].out_len);
            dst = dst_off ? rfl64(dst_off[e]) : out_off;
            first = bit >> 3;
            const uint64_t endb = (end_bit >> 3) + ((end_bit & 7) ? 1u : 0u);   // ceil(end_bit / 8)
            if (bit >= end_bit || endb > zbytes) err = -(int)E_RANGE;
            else if ((ext = endb - first) > 0xFFFFFFF0ull) err = -(int)E_RANGE;
            if (dst > out_bytes || out_len > out_bytes - dst) err = -(int)E_RANGE;
        }
        const uint32_t wlen = out_off < IW ? (uint32_t)out_off : (uint32_t)IW;
        uint64_t olen = 0;
        uint32_t check = 0;
        IBits r;
        IOut o;
#ifdef DMX_INF_STAMPS
        for (int q = 0; q < INF_NST; q++) o.st[q] = 0;
#endif
        o.out = out;
        o.base = dst - wlen;   // (wraps where dst < wlen: meant, as in the batch kernel -- only ever used with p >= fl >= wlen added)
        o.ob = 0;
        o.cap = out_len + wlen;
        o.op = wlen;
        o.fl = wlen;
        o.a = 1;
        o.b = 0;
        if (!err) {
            if (wlen) iprime(S.win, windows + (uint64_t)k * IW + (IW - wlen), wlen, lane);
            ib_init(r, z + first, ext);
            ib_seek(r, bit & 7);
            const uint64_t endrel = end_bit - 8 * first;   // in the reader's bits (relative to z + first)
            // the loop's exits are made uniform for the compiler too (readfirstlane), as in the batch kernel
            for (;;) {
                bool last = false;
                const int e2 = ib_status(r, iblock<true, true, IW, false, true>(S, r, o, gt, lane, last));
                err = (int)rfl((uint32_t)e2);
                if (err) break;
                const uint64_t used = (uint64_t)rfl(r.wi) * 32 - rfl(r.bc) - 8ull * r.lo;
                if (used == endrel) break;
                if (used > endrel || rfl(last ? 1u : 0u)) { err = -(int)E_SZ; break; }
            }
        }
        if (!err) {
            io_flush<true, true>(S, o, o.op, lane);
            olen = o.ob + o.op - wlen;
            check = (o.b << 16) | o.a;
            if (olen != out_len) err = -(int)E_SZ;
            else if (adler && rfl(adler[k]) != check) err = -(int)E_ZADL32;
        }
        if (lane == 0) {
            dmx_bresult v;
            v.status = err;
            v.format = DMX_BATCH_RAW;
            v.out_len = err ? 0 : olen;
            v.in_used = err ? 0 : ext;
            v.check = err ? 0 : check;
            v.reserved = 0;
            res[e] = v;
            if (err) {
                atomicAdd(&st->nfailed, 1u);
                atomicMin(&st->first_bad, e);
            } else {
                atomicAdd((unsigned long long*)&st->total_out, (unsigned long long)olen);
            }
        }
        __syncthreads();   // the ring and the small arrays are the next entry's
    }
}

// ------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------

// Table scratch of dmx_inflate_async: a stream-ordered allocation from a private memory pool
// per device, freed on the same stream after the launch.  The pool keeps what it was given
// (release threshold = no limit), so a steady stream of decodes allocates from the pool's
// reserve, not from the driver, and any number of streams (created and destroyed per
// request, or the per-thread default stream) is safe: no buffer is shared between calls.
// (Round 4 cached one buffer per (device, stream handle): it failed past 64 streams, never
// released a slot, and a reused handle shared a buffer with a destroyed stream's work.)
#define ITAB_DEVS 64
static hipMemPool_t g_itab_pool[ITAB_DEVS];
static pthread_mutex_t g_itab_mu = PTHREAD_MUTEX_INITIALIZER;
static hipMemPool_t itab_pool(int dev) {
    if (dev < 0 || dev >= ITAB_DEVS) return nullptr;
    pthread_mutex_lock(&g_itab_mu);
    if (!g_itab_pool[dev]) {
        hipMemPoolProps pp;
        memset(&pp, 0, sizeof(pp));
        pp.allocType = hipMemAllocationTypePinned;
        pp.handleTypes = hipMemHandleTypeNone;
        pp.location.type = hipMemLocationTypeDevice;
        pp.location.id = dev;
        hipMemPool_t p = nullptr;
        if (hipMemPoolCreate(&p, &pp) == hipSuccess) {
            uint64_t keep = ~0ull;
            (void)hipMemPoolSetAttribute(p, hipMemPoolAttrReleaseThreshold, &keep);
            g_itab_pool[dev] = p;
        }
    }
    hipMemPool_t r = g_itab_pool[dev];
    pthread_mutex_unlock(&g_itab_mu);
    return r;
}
static uint32_t* itab_scratch(hipStream_t s, uint64_t bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    void* p = nullptr;
    hipMemPool_t pool = itab_pool(dev);
    if (pool ? hipMallocFromPoolAsync(&p, bytes, pool, s) != hipSuccess : hipMallocAsync(&p, bytes, s) != hipSuccess)
        return nullptr;
    return (uint32_t*)p;
}
// the same pool for the scratch of dmx_bgzf_decode_device (dmx_bgzf_index.hip); hipFreeAsync on s frees it
void* dmx_itab_scratch(hipStream_t s, uint64_t bytes) { return itab_scratch(s, bytes); }

// The status record's reset.  A kernel, not hipMemsetAsync: captured into a graph (ROCm 7.2), the
// 16-byte memset node wrote zeros on the first replay only and other bytes on every later one.
__global__ void dmx_inflate_status_clear_kernel(dmx_inflate_status* __restrict__ st) {
    st->status = 0;
    st->reserved = 0;
    st->out_len = 0;
}

// the decode of dmx_inflate_async (d_index == NULL: the stream mode) and of
// dmx_inflate_members_async; max_len: the indexed kernel's bound on an entry's out_len
static int inflate_launch(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk, void* d_out,
                          uint64_t out_cap, uint32_t max_len, dmx_inflate_status* d_status, hipStream_t s) {
    if (zbytes > 0xFFFFFFF0ull) return -(int)E_RANGE;   // reader word indices are 32-bit
    hipLaunchKernelGGL(dmx_inflate_status_clear_kernel, dim3(1), dim3(1), 0, s, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    // the workgroups' first-level tables: scratch from the per-device stream-ordered pool
    // (hipMallocFromPoolAsync here, hipFreeAsync on the same stream after the launch)
    const uint64_t tb = (uint64_t)(d_index ? nblk : 1) * ITAB_WORDS * 4;
    uint32_t* gtab = itab_scratch(s, tb);
    if (!gtab) return -(int)E_MALLOC;
    if (d_index)
        hipLaunchKernelGGL(dmx_inflate_index_kernel<false>, dim3(nblk), dim3(64), 0, s, (const uint8_t*)d_z, zbytes,
                           d_index, (uint8_t*)d_out, out_cap, gtab, max_len, d_status, (const uint32_t*)nullptr);
    else
        hipLaunchKernelGGL(dmx_inflate_stream_kernel, dim3(1), dim3(64), 0, s, (const uint8_t*)d_z, zbytes,
                           (uint8_t*)d_out, out_cap, gtab, d_status);
    const hipError_t le = hipGetLastError();
    (void)hipFreeAsync(gtab, s);   // stream-ordered: after the decode
    if (le != hipSuccess) return -(int)E_DEVICE;
    return 0;
}

extern "C" int dmx_inflate_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk,
                                 void* d_out, uint64_t out_cap, dmx_inflate_status* d_status, void* stream) {
    if (!d_z || !d_out || !d_status || (d_index && !nblk)) return -(int)E_INVAL;
    return inflate_launch(d_z, zbytes, d_index, nblk, d_out, out_cap, IW, d_status, (hipStream_t)stream);
}

uint64_t dmx_itab_bytes(uint32_t slots) { return (uint64_t)slots * ITAB_WORDS * 4; }

int dmx_inflate_counted_launch(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t slots,
                               const uint32_t* d_count, void* d_out, uint64_t out_cap, void* d_gtab,
                               dmx_inflate_status* d_status, hipStream_t s) {
    if (zbytes > 0xFFFFFFF0ull) return -(int)E_RANGE;
    if (!slots) return 0;
    hipLaunchKernelGGL((dmx_inflate_index_kernel<false, true>), dim3(slots), dim3(64), 0, s, (const uint8_t*)d_z, zbytes,
                       d_index, (uint8_t*)d_out, out_cap, (uint32_t*)d_gtab, (uint32_t)DMX_BGZF_MAX_ISIZE, d_status, d_count);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

// The members of any BGZF file (include/dmx.h): the indexed decode with the format's own bound on
// a member, then the members' CRC-32s over the decoded ranges, compared on the device.  The CRC
// kernel ends at once after a failed decode and otherwise sets -E_CRC by compare-and-swap.
extern "C" int dmx_inflate_members_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk,
                                         void* d_out, uint64_t out_cap, const uint32_t* d_crc_want,
                                         dmx_inflate_status* d_status, void* stream) {
    if (!d_z || !d_out || !d_status || !d_index || !nblk) return -(int)E_INVAL;
    if ((reinterpret_cast<uintptr_t>(d_crc_want) & 3) != 0) return -(int)E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    const int r = inflate_launch(d_z, zbytes, d_index, nblk, d_out, out_cap, DMX_BGZF_MAX_ISIZE, d_status, s);
    if (r || !d_crc_want) return r;
    return dmx_crc32_ranges_launch(d_out, out_cap, d_index, nblk, NULL, d_crc_want, d_status, s);
}

// Batches of independent streams.  d_work: [IBatchCtl, 256 B][first-level tables, ITAB_WORDS per
// workgroup of the largest grid a batch of nstreams can get].
extern "C" uint64_t dmx_inflate_batch_work(uint32_t nstreams) {
    return 256 + 4ull * ITAB_WORDS * (nstreams < IBATCH_MAX_WG ? nstreams : IBATCH_MAX_WG);
}

// workgroups of the batch kernel the current device holds at once (the occupancy API's answer per
// CU times the CUs, at most IBATCH_MAX_WG), looked up once per device; 0: a device call failed
static uint32_t ibatch_resident(void) {
    static uint32_t wg[ITAB_DEVS];
    int dev = 0, ncu = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= ITAB_DEVS) return 0;
    uint32_t v = __atomic_load_n(&wg[dev], __ATOMIC_RELAXED);
    if (v) return v;
    // (all four instantiations have the same LDS, the limit, and one wave per SIMD fits their registers)
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, dmx_inflate_batch_kernel<false>, 64, 0) != hipSuccess ||
        hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || per < 1 || ncu < 1)
        return 0;
    const uint64_t n = (uint64_t)per * (uint64_t)ncu;
    v = n < IBATCH_MAX_WG ? (uint32_t)n : IBATCH_MAX_WG;
    __atomic_store_n(&wg[dev], v, __ATOMIC_RELAXED);
    return v;
}

extern "C" int dmx_inflate_batch_async(const void* d_z, uint64_t zbytes, const dmx_bstream* d_streams, uint32_t nstreams,
                                       uint32_t flags, void* d_out, uint64_t out_bytes, dmx_bresult* d_results,
                                       void* d_work, uint64_t work_bytes, dmx_batch_status* d_status, void* stream) {
    const bool measure = (flags & DMX_BATCH_MEASURE) != 0;
    if (!d_results || !d_status || !d_work || (!d_streams && nstreams) || (!d_z && zbytes) || (!d_out && !measure))
        return -(int)E_INVAL;
    if (((uintptr_t)d_streams & 7) || ((uintptr_t)d_results & 7) || ((uintptr_t)d_status & 7)) return -(int)E_INVAL;
    if (((uintptr_t)d_work & 255) || work_bytes < dmx_inflate_batch_work(nstreams)) return -(int)E_INVAL;
    const uint32_t fmt = flags & 15u;
    if ((flags & ~(15u | DMX_BATCH_MEASURE)) || fmt > DMX_BATCH_RAW) return -(int)E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    IBatchCtl* ctl = (IBatchCtl*)d_work;
    uint32_t* gtab = (uint32_t*)((uint8_t*)d_work + 256);
    hipLaunchKernelGGL(dmx_inflate_batch_clear_kernel, dim3(1), dim3(1), 0, s, ctl, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (!nstreams) return 0;
    const uint32_t resident = ibatch_resident();
    if (!resident) return -(int)E_DEVICE;
    const uint32_t grid = nstreams < resident ? nstreams : resident;
    const IBatchDict none = {nullptr, 0, nullptr, nullptr, nullptr, 0};
    if (measure)
        hipLaunchKernelGGL(dmx_inflate_batch_kernel<true>, dim3(grid), dim3(64), 0, s, (const uint8_t*)d_z, zbytes, d_streams,
                           nstreams, fmt, (uint8_t*)nullptr, 0ull, d_results, gtab, ctl, d_status, none);
    else
        hipLaunchKernelGGL(dmx_inflate_batch_kernel<false>, dim3(grid), dim3(64), 0, s, (const uint8_t*)d_z, zbytes, d_streams,
                           nstreams, fmt, (uint8_t*)d_out, out_bytes, d_results, gtab, ctl, d_status, none);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (measure || fmt == DMX_BATCH_ZLIB || fmt == DMX_BATCH_RAW) return 0;   // no gzip member to finish
    return dmx_crc32_batch_launch(d_out, out_bytes, d_streams, nstreams, d_results, d_status, s);
}

// The same with preset dictionaries.  d_work: dmx_inflate_batch_work(nstreams) bytes as above, then
// one Adler-32 word per dictionary (rounded up to 256 bytes), so the tables lie where they lay.
extern "C" uint64_t dmx_inflate_batch_dict_work(uint32_t nstreams, uint32_t ndicts) {
    return dmx_inflate_batch_work(nstreams) + ((4ull * ndicts + 255) & ~255ull);
}

extern "C" int dmx_inflate_batch_dict_async(const void* d_z, uint64_t zbytes, const dmx_bstream* d_streams, uint32_t nstreams,
                                            uint32_t flags, const void* d_dict, uint64_t dict_bytes,
                                            const dmx_bdict* d_dicts, uint32_t ndicts, const uint32_t* d_dict_of,
                                            void* d_out, uint64_t out_bytes, dmx_bresult* d_results, void* d_work,
                                            uint64_t work_bytes, dmx_batch_status* d_status, void* stream) {
    const bool measure = (flags & DMX_BATCH_MEASURE) != 0;
    if (!d_results || !d_status || !d_work || (!d_streams && nstreams) || (!d_z && zbytes) || (!d_out && !measure) ||
        (!d_dicts && ndicts) || (!d_dict && dict_bytes))
        return -(int)E_INVAL;
    if (((uintptr_t)d_streams & 7) || ((uintptr_t)d_results & 7) || ((uintptr_t)d_status & 7) || ((uintptr_t)d_dicts & 7) ||
        ((uintptr_t)d_dict_of & 3))
        return -(int)E_INVAL;
    if (((uintptr_t)d_work & 255) || work_bytes < dmx_inflate_batch_dict_work(nstreams, ndicts)) return -(int)E_INVAL;
    const uint32_t fmt = flags & 15u;
    if ((flags & ~(15u | DMX_BATCH_MEASURE)) || fmt > DMX_BATCH_RAW) return -(int)E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    IBatchCtl* ctl = (IBatchCtl*)d_work;
    uint32_t* gtab = (uint32_t*)((uint8_t*)d_work + 256);
    uint32_t* adl = (uint32_t*)((uint8_t*)d_work + dmx_inflate_batch_work(nstreams));
    hipLaunchKernelGGL(dmx_inflate_batch_clear_kernel, dim3(1), dim3(1), 0, s, ctl, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (!nstreams) return 0;
    const uint32_t resident = ibatch_resident();
    if (!resident) return -(int)E_DEVICE;
    if (ndicts) {
        hipLaunchKernelGGL(dmx_dict_adler_kernel, dim3(ndicts), dim3(256), 0, s, (const uint8_t*)d_dict, dict_bytes, d_dicts, adl);
        if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    }
    const uint32_t grid = nstreams < resident ? nstreams : resident;
    const IBatchDict dd = {(const uint8_t*)d_dict, dict_bytes, d_dicts, d_dict_of, adl, ndicts};
    if (measure)
        hipLaunchKernelGGL((dmx_inflate_batch_kernel<true, true>), dim3(grid), dim3(64), 0, s, (const uint8_t*)d_z, zbytes,
                           d_streams, nstreams, fmt, (uint8_t*)nullptr, 0ull, d_results, gtab, ctl, d_status, dd);
    else
        hipLaunchKernelGGL((dmx_inflate_batch_kernel<false, true>), dim3(grid), dim3(64), 0, s, (const uint8_t*)d_z, zbytes,
                           d_streams, nstreams, fmt, (uint8_t*)d_out, out_bytes, d_results, gtab, ctl, d_status, dd);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (measure || fmt == DMX_BATCH_ZLIB || fmt == DMX_BATCH_RAW) return 0;   // no gzip member to finish
    return dmx_crc32_batch_launch(d_out, out_bytes, d_streams, nstreams, d_results, d_status, s);
}

// The entries of a ZIP archive: the batch decode on its raw path, a copy kernel for stored entries
#include "dmx_zip_read.inc"

// Seek points: d_work as the batch decode's -- [IBatchCtl, 256 B][first-level tables].  The grid is
// the batch kernel's too: the same InfLDS<IW> is the limit per CU.
extern "C" uint64_t dmx_inflate_points_work(uint32_t nsel) { return dmx_inflate_batch_work(nsel); }

extern "C" int dmx_inflate_points_async(const void* d_z, uint64_t zbytes, const dmx_zpoint* d_points, const uint32_t* d_adler,
                                        const void* d_windows, uint32_t npoints, const uint32_t* d_sel,
                                        const uint64_t* d_dst_off, uint32_t nsel, void* d_out, uint64_t out_bytes,
                                        dmx_bresult* d_results, void* d_work, uint64_t work_bytes, dmx_batch_status* d_status,
                                        void* stream) {
    if (!d_results || !d_status || !d_work || ((!d_points || !d_windows || !d_out) && nsel) || (!d_z && zbytes))
        return -(int)E_INVAL;
    if (((uintptr_t)d_points & 7) || ((uintptr_t)d_dst_off & 7) || ((uintptr_t)d_results & 7) || ((uintptr_t)d_status & 7) ||
        ((uintptr_t)d_adler & 3) || ((uintptr_t)d_sel & 3))
        return -(int)E_INVAL;
    if (((uintptr_t)d_work & 255) || work_bytes < dmx_inflate_points_work(nsel)) return -(int)E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    IBatchCtl* ctl = (IBatchCtl*)d_work;
    uint32_t* gtab = (uint32_t*)((uint8_t*)d_work + 256);
    hipLaunchKernelGGL(dmx_inflate_batch_clear_kernel, dim3(1), dim3(1), 0, s, ctl, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (!nsel) return 0;
    const uint32_t resident = ibatch_resident();
    if (!resident) return -(int)E_DEVICE;
    const uint32_t grid = nsel < resident ? nsel : resident;
    hipLaunchKernelGGL(dmx_inflate_points_kernel, dim3(grid), dim3(64), 0, s, (const uint8_t*)d_z, zbytes, d_points, d_adler,
                       (const uint8_t*)d_windows, npoints, d_sel, d_dst_off, nsel, (uint8_t*)d_out, out_bytes, d_results, gtab,
                       ctl, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

// ------------------------------------------------------------------------------------
// One foreign stream in one pass (dmx_inflate_parallel_plan_async / _decode_async, include/dmx.h;
// DESIGN.md 3.1 "One foreign stream: the decode").  The plan is dmx_inflate_parallel_plan_host's on
// the device, four launches over d_plan = [head 256][live chunks 32 x nc][candidates 8 x nc]
// [measures 32 x nc][tables 8 KiB x workgroups] (dmx_pf_plan_bytes):
//   head     one thread: the framing (dmx_frame_head), the record's and the claim counter's reset
//   find     a wave per chunk: the first bit offset of the chunk dmx_pf_valid accepts.  A step tests
//            64 offsets: lanes 0..7 load the eight aligned words that hold them (whole words inside
//            the stream, single bytes at its ends, zeros past it), every lane takes its two views
//            from them by cross-lane reads, dmx_pf_filter_w runs on all 64, dmx_pf_header only in
//            the lanes the filter left, and the lowest accepted lane ends the search
//   measure  workgroups of one wave claim candidates from the counter and decode them for lengths
//            only (iblock without stores, the window taken as primed, capacity
//            DMX_PF_MAX_CHUNK_OUT + 1, the reader bounded by the input: every loop ends), with dmx_pf_land at every block boundary.  Every
//            candidate is measured, not only those the walk reaches: a dead one costs time, and
//            its record is never read
//   link     one thread: dmx_pf_link, the walk that keeps the live chunks, and the trailer
// The decode, over d_work = [control 256][tables 8 KiB x workgroups][cells 2 x out_len][piece index,
// unused][piece CRC-32 remainders 4 x np][piece Adler-32 sums 4 x np] (dmx_pf_work; every offset is
// computed on the device from the record's out_len and nlive):
//   begin    one thread: the plan's record into d_status, the capacity checks (-E_SZ), the reset
//   cells    a wave per live chunk, claimed from a counter: iblock into 16-bit cells (CELL) with
//            base = out_off and cap = out_len until exactly end_bit
//   tails    one workgroup of 1 024 threads walks the live chunks in order with the 32 KiB in front
//            of the current chunk in LDS (dmx_ptail.h)
//   pack     cells into bytes; what is still a reference reads a cell the tail pass resolved
//   check    (verify) per piece of 64 KiB the Adler-32 sums or the raw CRC-32 remainder
//   status   one thread: the first error by chunk order, the pieces combined, the trailer compared
// A workgroup beyond the device-side counts leaves at once; after a status no later stage runs.
// ------------------------------------------------------------------------------------
struct PPlanHead {   // the first 256 bytes of d_plan
    dmx_par_status st;         // 0: the record
    uint32_t chunk_bytes;      // 56
    uint32_t isize;            // 60: gzip's ISIZE
    uint64_t body_bit;         // 64
    uint64_t zbytes;           // 72
    unsigned long long next;   // 80: the measure pass's claim counter
};
static_assert(sizeof(dmx_par_status) == 56 && sizeof(PPlanHead) <= 256 && sizeof(dmx_pf_meas) == 32, "d_plan's layout");
struct PMPlanHead {   // a file of members: the 64-byte record (dmx_par_multi_status) in front
    dmx_par_status st;               // 0
    uint32_t nmembers, bad_member;   // 56, 60
    uint32_t chunk_bytes;            // 64
    uint32_t isize;                  // 68: the last member's ISIZE
    uint64_t body_bit;               // 72: 0, the first header
    uint64_t zbytes;                 // 80
    unsigned long long next;         // 88
};
static_assert(sizeof(dmx_par_multi_status) == 64 && offsetof(PMPlanHead, chunk_bytes) == 64 && sizeof(PMPlanHead) <= 256 &&
                  sizeof(dmx_pf_mside) == 16 && sizeof(dmx_pmember) == 32,
              "d_plan's layout, many members");
template <bool MULTI>
using PHead = typename std::conditional<MULTI, PMPlanHead, PPlanHead>::type;
// the sides in a plan of many members, behind the walks' member offsets (begin has checked plan_bytes)
__device__ __forceinline__ const dmx_pf_mside* pm_sides(const uint8_t* plan) {
    const uint32_t nc = reinterpret_cast<const PMPlanHead*>(plan)->st.nchunks;
    return reinterpret_cast<const dmx_pf_mside*>(plan + 256 + 2 * dmx_pf_a256(32ull * nc) + 2 * dmx_pf_a256(8ull * nc));
}

struct PDecCtl {   // the first 256 bytes of d_work
    unsigned long long next;   // the cell pass's claim counter
    unsigned long long err;    // chunk << 32 | status, an integer minimum: the first chunk's error
    uint64_t out_len;
    uint32_t go, nlive, format, check, isize;
    uint32_t nmembers;         // a file of members (dmx_inflate_parallel_multi_decode_async) from here on
    unsigned long long bad;    // member << 32 | status: the first member whose check fails
};
#define PDEC_NOERR (~0ull)
__device__ __forceinline__ void pdec_fail(PDecCtl* ctl, uint32_t chunk, int err) {
    atomicMin(&ctl->err, ((unsigned long long)chunk << 32) | (uint32_t)err);
}
__device__ __forceinline__ uint8_t* pdec_cells(uint8_t* work, uint32_t nlive) { return work + 256 + 8192 * dmx_pf_cell_wg(nlive); }
__device__ __forceinline__ uint32_t* pdec_crcs(uint8_t* work, uint64_t out_len, uint32_t nlive) {
    const uint64_t np = dmx_pf_pieces(out_len);
    return (uint32_t*)(pdec_cells(work, nlive) + dmx_pf_a256(2 * out_len) + dmx_pf_a256(24 * np));
}

__global__ void dmx_par_head_kernel(const uint8_t* __restrict__ z, uint64_t zbytes, uint32_t fmt, uint32_t chunk,
                                    uint32_t nc, PPlanHead* __restrict__ h, uint64_t* __restrict__ cand) {
    dmx_par_status st;
    uint64_t body = 0;
    uint32_t format = 0;
    st.status = dmx_frame_head(z, zbytes, fmt, &format, &body);
    st.format = format;
    st.out_len = st.in_used = st.work_len = 0;
    st.check = st.nlive = st.ndead = st.gave_up = 0;
    st.nchunks = nc;
    st.ncand = st.status ? 0u : 1u;
    h->st = st;
    h->chunk_bytes = chunk;
    h->isize = 0;
    h->body_bit = 8 * body;
    h->zbytes = zbytes;
    h->next = 0;
    cand[0] = 8 * body;
}

// word wi of the aligned view of z (zb = z rounded down to 4 bytes; the stream is bytes [mis, end)
// of it): a whole word inside the stream is one load, any other is assembled from the stream's bytes
__device__ __forceinline__ uint32_t par_word(const uint8_t* zb, uint32_t mis, uint64_t end, uint64_t wi) {
    if (4 * wi + 4 <= end) return reinterpret_cast<const uint32_t*>(zb)[wi];   // (the first may begin up to 3 bytes in front)
    uint32_t v = 0;
    for (uint32_t j = 0; j < 4; j++) {
        const uint64_t b = 4 * wi + j;
        if (b >= mis && b < end) v |= (uint32_t)zb[b] << (8 * j);
    }
    return v;
}

template <bool MULTI>
__global__ __launch_bounds__(64) void dmx_par_find_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                          PHead<MULTI>* __restrict__ h, uint64_t* __restrict__ cand) {
    const uint32_t c = blockIdx.x, lane = threadIdx.x;
    if (c == 0 || h->st.status) return;   // chunk 0 begins at the framing's bit
    uint64_t lo, hi;
    dmx_pf_range(c, h->chunk_bytes, zbytes, h->body_bit, &lo, &hi);
    const uintptr_t a = (uintptr_t)z;
    const uint8_t* zb = (const uint8_t*)(a & ~(uintptr_t)3);
    const uint32_t mis = (uint32_t)(a & 3);
    const uint64_t end = mis + zbytes;
    uint64_t found = DMX_PF_NONE;
    for (uint64_t b0 = lo; b0 < hi; b0 += 64) {
        const uint64_t w0 = ((b0 >> 3) + mis) >> 2;   // the first staged word
        const uint32_t wv = lane < 8 ? par_word(zb, mis, end, w0 + lane) : 0u;
        const uint64_t bit = b0 + lane;
        // the lane's 16 bytes begin rb <= 3 + 8 bytes into the staged words: words k .. k + 4, k <= 2
        const uint32_t rb = (uint32_t)(((bit >> 3) + mis) - 4 * w0), k = rb >> 2, sh = 8 * (rb & 3);
        uint32_t x[5];
#pragma unroll
        for (int q = 0; q < 5; q++) x[q] = (uint32_t)__shfl((int)wv, (int)(k + q), 64);
        uint32_t y[4];
#pragma unroll
        for (int q = 0; q < 4; q++) y[q] = (uint32_t)((((uint64_t)x[q + 1] << 32) | x[q]) >> sh);
        const uint64_t L = ((uint64_t)y[1] << 32) | y[0], H = ((uint64_t)y[3] << 32) | y[2];   // bytes p .. p + 7, p + 8 .. p + 15
        const uint32_t s = (uint32_t)bit & 7;
        const uint64_t w = L >> s, w2 = ((L >> 56) | (H << 8)) >> s;   // dmx_pf_peek at bit and at bit + 56
        uint64_t cl = 0;
        uint32_t hdr = 0;
        const bool pass = bit < hi && dmx_pf_filter_w(w, w2, zbytes, bit, &cl, &hdr);
        bool ok = false;
        if (__ballot(pass)) ok = pass && dmx_pf_header(z, zbytes, bit, cl, hdr);
        if constexpr (MULTI) {   // a member start, in the lanes whose bit is a byte's first: on the bytes already staged
            const bool mp = bit < hi && s == 0 && (bit >> 3) + 4 <= zbytes && dmx_pf_member_w((uint32_t)L);
            if (__ballot(mp)) ok = ok || (mp && dmx_pf_member_head(z, zbytes, bit >> 3));
        }
        const uint64_t am = __ballot(ok);
        if (am) {
            found = b0 + (uint32_t)__builtin_ctzll(am);
            break;
        }
    }
    if (lane == 0) {
        cand[c] = found;
        if (found != DMX_PF_NONE) atomicAdd(&h->st.ncand, 1u);
    }
}

template <bool MULTI>
__global__ __launch_bounds__(64) void dmx_par_measure_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                             PHead<MULTI>* __restrict__ h, const uint64_t* __restrict__ cand,
                                                             dmx_pf_meas* __restrict__ meas, uint32_t nc,
                                                             uint32_t* __restrict__ gtab, uint64_t* __restrict__ mloc) {
    __shared__ InfLDS<IW> S;   // the kernel's one __shared__ object: isym_run addresses the ring from LDS 0
    if (h->st.status) return;
    uint32_t* gt = gtab + (uint64_t)blockIdx.x * ITAB_WORDS;
    const uint32_t lane = threadIdx.x;
    for (;;) {
        unsigned long long claim = 0;
        if (lane == 0) claim = atomicAdd(&h->next, 1ull);
        const uint64_t k64 = rfl64(claim);
        if (k64 >= nc) break;
        const uint32_t k = (uint32_t)k64;
        const uint64_t start = rfl64(cand[k]);
        if (start == DMX_PF_NONE) continue;
        IBits r;
        IOut o;
#ifdef DMX_INF_STAMPS
        for (int q = 0; q < INF_NST; q++) o.st[q] = 0;
#endif
        // The window is taken as primed, as a preset dictionary of IW bytes primes it (the arithmetic
        // above IBatchDict) but without its bytes: nothing is stored and only lengths count, so no
        // distance is too far here -- chunk 0's included, as on the host: a distance before the
        // first output byte is the decode's to find.
        o.out = nullptr;
        o.base = 0;
        o.ob = 0;
        o.cap = DMX_PF_MAX_CHUNK_OUT + 1 + IW;
        o.op = IW;
        o.fl = IW;
        o.a = 1;
        o.b = 0;
        ib_init(r, z, zbytes);
        if constexpr (!MULTI) ib_seek(r, start);
        uint32_t t = k + 1, skipped = 0, flags = 0, next = 0xFFFFFFFFu;
        int status = 0;
        uint64_t out_len = 0;
        // a file of members (dmx_pfind.h; the host's measure_multi): nmem members begin in this walk,
        // the first and the last at the output offsets mfirst and mlast inside it
        [[maybe_unused]] uint32_t nmem = 0, mfirst = DMX_PF_NOMEM, mlast = DMX_PF_NOMEM;
        [[maybe_unused]] uint64_t stop = DMX_PF_NONE;   // where the walk ended other than at the reader's position
        [[maybe_unused]] bool walk = true;
        if constexpr (MULTI) {
            uint64_t at = start;
            if (dmx_pf_at_member(z, start)) {
                uint64_t body = 0;
                status = (int)rfl((uint32_t)dmx_gz_head(z + (start >> 3), zbytes - (start >> 3), &body));
                if (status) {
                    walk = false;
                    stop = start;
                } else {
                    nmem = 1;
                    mfirst = mlast = 0;
                    at = start + 8 * rfl64(body);
                    const int ld = (int)rfl((uint32_t)dmx_pf_land(cand, nc, &t, at, &skipped));
                    t = rfl(t);
                    skipped = rfl(skipped);
                    if (ld) {
                        if (ld == 1) next = t;
                        else flags = DMX_PF_LOST;
                        walk = false;
                        stop = at;
                    }
                }
            }
            ib_seek(r, at);
        }
        for (;;) {
            if constexpr (MULTI) {
                if (!walk) break;
            }
            bool last = false;
            const int e = ib_status(r, iblock<true, true, IW, false, false>(S, r, o, gt, lane, last));
            status = (int)rfl((uint32_t)e);
            out_len = rfl64(o.ob + o.op - IW);
            if (status == -(int)E_SZ || (!status && out_len > DMX_PF_MAX_CHUNK_OUT)) {   // too much for one chunk
                status = 0;
                flags = DMX_PF_LOST;
                break;
            }
            if (status) break;
            if constexpr (!MULTI) {
                if (rfl(last ? 1u : 0u)) {
                    flags = DMX_PF_LAST;
                    break;
                }
            }
            uint64_t pos = (uint64_t)rfl(r.wi) * 32 - rfl(r.bc) - 8ull * r.lo;
            if constexpr (MULTI) {
                if (rfl(last ? 1u : 0u)) {
                    uint64_t q = 0, body = 0;
                    uint32_t crc = 0, isize = 0;
                    const int e2 = (int)rfl((uint32_t)dmx_pf_member_end(z, zbytes, pos, &q, &body, &crc, &isize));
                    q = rfl64(q);
                    body = rfl64(body);
                    if (e2 < 0) { status = e2; break; }
                    if (e2 == 0) { flags = DMX_PF_LAST; break; }
                    const int l0 = (int)rfl((uint32_t)dmx_pf_land(cand, nc, &t, 8 * q, &skipped));   // at the member's first byte
                    t = rfl(t);
                    skipped = rfl(skipped);
                    if (l0 == 1) { next = t; stop = 8 * q; break; }
                    if (l0 == 2) { flags = DMX_PF_LOST; break; }
                    nmem++;
                    mlast = (uint32_t)out_len;
                    if (mfirst == DMX_PF_NOMEM) mfirst = mlast;
                    pos = 8 * (q + body);   // at its first block
                    ib_seek(r, pos);
                }
            }
            const int ld = (int)rfl((uint32_t)dmx_pf_land(cand, nc, &t, pos, &skipped));
            t = rfl(t);
            skipped = rfl(skipped);
            if (ld == 1) {
                next = t;
                break;
            }
            if (ld == 2) {
                flags = DMX_PF_LOST;
                break;
            }
        }
        if (lane == 0) {
            dmx_pf_meas m;
            m.end_bit = (uint64_t)rfl(r.wi) * 32 - rfl(r.bc) - 8ull * r.lo;
            if constexpr (MULTI) {
                if (stop != DMX_PF_NONE) m.end_bit = stop;
                mloc[k] = (uint64_t)mfirst | ((uint64_t)mlast << 32);
            }
            m.out_len = out_len;
            m.next = next;
            m.flags = flags;
            m.status = status;
            m.reserved = MULTI ? nmem : 0u;
            meas[k] = m;
        }
        __syncthreads();   // the ring and the small arrays are the next candidate's
    }
}

__global__ void dmx_par_link_kernel(const uint8_t* __restrict__ z, uint64_t zbytes, PPlanHead* __restrict__ h,
                                    const uint64_t* __restrict__ cand, const dmx_pf_meas* __restrict__ meas,
                                    dmx_pchunk* __restrict__ chunks, uint32_t nc) {
    if (h->st.status) return;
    dmx_par_status st = h->st;
    uint32_t isize = 0;
    dmx_pf_link(z, zbytes, cand, meas, chunks, nc, &st, &isize);
    h->st = st;
    h->isize = isize;
}

__global__ void dmx_par_begin_kernel(const PPlanHead* __restrict__ h, uint64_t plan_bytes, uint64_t zbytes, uint32_t max_live,
                                     uint64_t out_cap, uint64_t work_bytes, PDecCtl* __restrict__ ctl,
                                     dmx_par_status* __restrict__ d_status) {
    dmx_par_status st = h->st;
    ctl->next = 0;
    ctl->err = PDEC_NOERR;
    ctl->go = 0;
    if (!st.status) {
        // a plan of other bytes, or no plan at all: nothing below may trust its numbers
        if (h->zbytes != zbytes || !st.nlive || st.nlive > st.nchunks || plan_bytes < dmx_pf_plan_bytes(st.nchunks) ||
            st.out_len > DMX_PF_MAX_POS) {
            st.status = -(int32_t)E_INVAL;
            st.out_len = st.in_used = st.work_len = 0;
            st.check = 0;
        } else if (st.nlive > max_live || st.out_len > out_cap || work_bytes < dmx_pf_work(st.out_len, st.nlive)) {
            st.status = -(int32_t)E_SZ;   // the record holds the needed numbers
        } else {
            ctl->out_len = st.out_len;
            ctl->nlive = st.nlive;
            ctl->format = st.format;
            ctl->check = st.check;
            ctl->isize = h->isize;
            ctl->go = 1;
        }
    }
    *d_status = st;
}

// MULTI (a file of members): the wave crosses the member boundaries inside its chunk -- trailer,
// header, on at the next body -- and begins at a header when its bit names one.  Output position 0
// of the decoder is then the member's first byte, not the chunk's: in front of it (o.base = how far
// the chunk begins behind its member's start, so iblock's own -E_HUFDIS is the member's), and at a
// member start inside the chunk by flushing and starting over there, so no copy crosses it.  It
// writes the member records: the begin side of the members whose header it reads, the end side of
// those whose last block it decodes, at sides[i].mbase + the local count.
template <bool MULTI>
__global__ __launch_bounds__(64) void dmx_par_cells_kernel(const uint8_t* __restrict__ z, uint64_t zbytes,
                                                           const dmx_pchunk* __restrict__ chunks, uint8_t* __restrict__ work,
                                                           PDecCtl* __restrict__ ctl, const uint8_t* __restrict__ plan,
                                                           dmx_pmember* __restrict__ members, uint32_t max_members) {
    __shared__ InfLDS<IWC, uint16_t> S;   // the kernel's one __shared__ object
    if (!ctl->go) return;
    [[maybe_unused]] const dmx_pf_mside* sides = MULTI ? pm_sides(plan) : nullptr;
    const uint32_t nlive = ctl->nlive;
    if (blockIdx.x >= dmx_pf_cell_wg(nlive)) return;   // (no table area of its own)
    const uint64_t total = ctl->out_len;
    uint32_t* gt = (uint32_t*)(work + 256) + (uint64_t)blockIdx.x * ITAB_WORDS;
    uint8_t* cells = pdec_cells(work, nlive);
    const uint32_t lane = threadIdx.x;
    for (;;) {
        unsigned long long claim = 0;
        if (lane == 0) claim = atomicAdd(&ctl->next, 1ull);
        const uint64_t i64 = rfl64(claim);
        if (i64 >= nlive) break;
        const uint32_t i = (uint32_t)i64;
        const uint64_t bit = rfl64(chunks[i].bit), end_bit = rfl64(chunks[i].end_bit);
        const uint64_t off = rfl64(chunks[i].out_off), olen = rfl64(chunks[i].out_len);
        const uint64_t nxt = i + 1 < nlive ? rfl64(chunks[i + 1].out_off) : total;
        int err = 0;
        // the chunks tile [0, out_len) in order: the tail and pack passes rely on it
        if (bit >= end_bit || end_bit > 8 * zbytes || olen > DMX_PF_MAX_CHUNK_OUT || off > total || olen > total - off ||
            off + olen != nxt || (i == 0 && off != 0))
            err = -(int)E_RANGE;
        IBits r;
        IOut o;
#ifdef DMX_INF_STAMPS
        for (int q = 0; q < INF_NST; q++) o.st[q] = 0;
#endif
        o.out = cells;
        o.base = off;
        o.ob = 0;
        o.cap = olen;
        o.op = 0;
        o.fl = 0;
        o.a = 1;
        o.b = 0;
        uint64_t done = 0;   // MULTI: the chunk's output in front of the member the decoder stands in
        if constexpr (MULTI) {
            const uint64_t mst = rfl64(sides[i].mstart);
            if (!err && mst > off) err = -(int)E_RANGE;
            if (!err) {
                o.out = (uint8_t*)rfl64((uint64_t)(uintptr_t)(cells + 2 * mst));
                o.base = off - mst;
            }
        }
        if (!err) {
            ib_init(r, z, zbytes);
            uint64_t at = bit;
            bool walk = true;
            [[maybe_unused]] uint32_t cur = 0;      // members begun in front of the reader
            [[maybe_unused]] uint64_t mabs = 0;     // where the member the reader stands in began in the output
            if constexpr (MULTI) {
                cur = rfl(sides[i].mbase);
                mabs = rfl64(sides[i].mstart);
                if (dmx_pf_at_member(z, bit)) {
                    uint64_t body = 0;
                    err = (int)rfl((uint32_t)dmx_gz_head(z + (bit >> 3), zbytes - (bit >> 3), &body));
                    if (!err) {
                        if (lane == 0 && cur < max_members) {
                            members[cur].in_off = bit >> 3;
                            members[cur].out_off = off;
                        }
                        cur++;
                        mabs = off;
                        o.out = (uint8_t*)rfl64((uint64_t)(uintptr_t)(cells + 2 * off));
                        o.base = 0;
                        at = bit + 8 * rfl64(body);
                        if (at >= end_bit) {   // a header alone
                            walk = false;
                            if (at > end_bit) err = -(int)E_SZ;
                        }
                    } else {
                        walk = false;
                    }
                }
            }
            ib_seek(r, at);
            while (walk) {   // blocks until exactly end_bit, by the seek-point kernel's rules
                bool last = false;
                const int e = ib_status(r, iblock<true, false, IWC, true>(S, r, o, gt, lane, last));
                err = (int)rfl((uint32_t)e);
                if (err) break;
                const uint64_t used = (uint64_t)rfl(r.wi) * 32 - rfl(r.bc) - 8ull * r.lo;
                if constexpr (MULTI) {
                    if (rfl(last ? 1u : 0u)) {   // the member's end
                        io_flush<false>(S, o, o.op, lane);
                        const uint64_t loc = rfl64(done + o.ob + o.op);   // the chunk's output so far
                        uint64_t q = 0, body = 0;
                        uint32_t crc = 0, isize = 0;
                        const int e2 = (int)rfl((uint32_t)dmx_pf_member_end(z, zbytes, used, &q, &body, &crc, &isize));
                        q = rfl64(q);
                        body = rfl64(body);
                        if (e2 < 0) { err = e2; break; }
                        if (lane == 0 && cur >= 1 && cur - 1 < max_members) {
                            members[cur - 1].out_len = off + loc - mabs;
                            members[cur - 1].crc = crc;
                            members[cur - 1].isize = isize;
                        }
                        if (used == end_bit) {   // the file's end
                            if (e2 != 0) err = -(int)E_SZ;
                            break;
                        }
                        if (e2 == 0 || 8 * q > end_bit || loc > olen) { err = -(int)E_SZ; break; }
                        if (8 * q == end_bit) break;   // the next chunk begins at the header
                        if (lane == 0 && cur < max_members) {
                            members[cur].in_off = q;
                            members[cur].out_off = off + loc;
                        }
                        cur++;
                        mabs = off + loc;
                        done = loc;   // everything is flushed: the decoder starts over at the member's first byte
                        o.out = (uint8_t*)rfl64((uint64_t)(uintptr_t)(cells + 2 * (off + loc)));
                        o.base = 0;
                        o.ob = 0;
                        o.op = 0;
                        o.fl = 0;
                        o.cap = olen - loc;
                        const uint64_t nb = 8 * (q + body);
                        if (nb > end_bit) { err = -(int)E_SZ; break; }
                        ib_seek(r, nb);
                        if (nb == end_bit) break;
                        continue;
                    }
                }
                if (used == end_bit) break;
                if (used > end_bit || rfl(last ? 1u : 0u)) { err = -(int)E_SZ; break; }
            }
        }
        if (!err && done + o.ob + o.op != olen) err = -(int)E_SZ;
        if (!err) io_flush<false>(S, o, o.op, lane);
        if (err && lane == 0) pdec_fail(ctl, i, err);
        __syncthreads();   // the ring and the small arrays are the next chunk's
    }
}

#define PTAIL_T 1024u
#define PTAIL_Q (DMX_PT_WIN / PTAIL_T)   // window positions per thread
// MULTI: a reference may reach back to its member's first byte only -- the chunk's side says how far
// that is in front of the chunk, and from which of the chunk's positions on a member began inside it
// (the cell pass started over there: a reference behind it is before its member whatever it says).
template <bool MULTI>
__global__ __launch_bounds__(PTAIL_T) void dmx_par_tails_kernel(const dmx_pchunk* __restrict__ chunks,
                                                                uint8_t* __restrict__ work, PDecCtl* __restrict__ ctl,
                                                                const uint8_t* __restrict__ plan) {
    // two windows, not one ring: a reference is relative to the chunk's start, so any cell of a long
    // chunk's tail may name any of the 32 768 positions before the chunk
    __shared__ uint8_t win[2][DMX_PT_WIN];
    if (!ctl->go || ctl->err != PDEC_NOERR) return;
    [[maybe_unused]] const dmx_pf_mside* sides = MULTI ? pm_sides(plan) : nullptr;
    const uint32_t nlive = ctl->nlive, tid = threadIdx.x;
    uint16_t* cells = reinterpret_cast<uint16_t*>(pdec_cells(work, nlive));
    uint32_t cur = 0, bad = 0xFFFFFFFFu;
    for (uint32_t i = 0; i < nlive; i++) {
        const uint64_t off = chunks[i].out_off, len = chunks[i].out_len;
        uint16_t* tc = cells + off + len - dmx_pt_tail(len);   // the tail's cells
        [[maybe_unused]] uint64_t lim = off, mf = ~0ull;
        if constexpr (MULTI) {
            lim = off - sides[i].mstart;
            if (sides[i].mfirst != DMX_PF_NOMEM) mf = sides[i].mfirst;
        }
        const uint8_t* W = win[cur];
        uint8_t* N = win[cur ^ 1];
        // window position k = tid + PTAIL_T q of the next window: a tail entry or an old byte
        uint16_t c[PTAIL_Q];
#pragma unroll
        for (uint32_t q = 0; q < PTAIL_Q; q++) {   // all loads first: they fly together
            uint32_t idx;
            c[q] = dmx_pt_next(tid + PTAIL_T * q, len, &idx) ? tc[idx] : (uint16_t)0;
        }
#pragma unroll
        for (uint32_t q = 0; q < PTAIL_Q; q++) {
            uint32_t idx;
            int v;
            if (dmx_pt_next(tid + PTAIL_T * q, len, &idx)) {
                if constexpr (MULTI) v = dmx_pt_cell(c[q], W, len - dmx_pt_tail(len) + idx >= mf ? 0 : lim);
                else v = dmx_pt_cell(c[q], W, off);
                if (v < 0) {
                    bad = bad < i ? bad : i;
                    v = 0;
                }
                tc[idx] = (uint16_t)v;   // the byte, in place
            } else {
                v = W[idx];
            }
            N[tid + PTAIL_T * q] = (uint8_t)v;
        }
        __syncthreads();
        cur ^= 1;
    }
    if (bad != 0xFFFFFFFFu) pdec_fail(ctl, bad, -(int)E_HUFDIS);   // before output offset 0
}

#define PPACK_T 256u
#define PPACK_MAX_WG 4096u
template <bool MULTI>
__global__ __launch_bounds__(PPACK_T) void dmx_par_pack_kernel(const dmx_pchunk* __restrict__ chunks,
                                                               uint8_t* __restrict__ work, PDecCtl* __restrict__ ctl,
                                                               uint8_t* __restrict__ out, const uint8_t* __restrict__ plan) {
    if (!ctl->go || ctl->err != PDEC_NOERR) return;
    [[maybe_unused]] const dmx_pf_mside* sides = MULTI ? pm_sides(plan) : nullptr;
    const uint32_t nlive = ctl->nlive;
    const uint64_t n = ctl->out_len;   // <= out_cap (begin)
    const uint16_t* cells = reinterpret_cast<const uint16_t*>(pdec_cells(work, nlive));
    for (uint64_t q = 4 * ((uint64_t)blockIdx.x * PPACK_T + threadIdx.x); q < n; q += 4ull * PPACK_T * gridDim.x) {
        uint32_t lo = 0, hi = nlive;   // the last chunk that begins at or before q
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (chunks[mid].out_off <= q) lo = mid;
            else hi = mid;
        }
        uint32_t i = lo;
        uint64_t off = chunks[i].out_off, end = off + chunks[i].out_len;
        uint32_t b4 = 0;
        const uint32_t m = n - q < 4 ? (uint32_t)(n - q) : 4u;
        for (uint32_t j = 0; j < m; j++) {
            const uint64_t p = q + j;
            while (p >= end && i + 1 < nlive) {
                i++;
                off = chunks[i].out_off;
                end = off + chunks[i].out_len;
            }
            int v;
            if constexpr (MULTI) {
                const uint32_t mf = sides[i].mfirst;
                v = dmx_pt_pack_lim(cells, p, off, mf != DMX_PF_NOMEM && p - off >= mf ? 0 : off - sides[i].mstart);
            } else {
                v = dmx_pt_pack(cells, p, off);
            }
            if (v < 0) {
                pdec_fail(ctl, i, -(int)E_HUFDIS);
                v = 0;
            }
            b4 |= (uint32_t)v << (8 * j);
        }
        if (m == 4 && (((uintptr_t)out + q) & 3) == 0) {
            *reinterpret_cast<uint32_t*>(out + q) = b4;
        } else {
            for (uint32_t j = 0; j < m; j++) out[q + j] = (uint8_t)(b4 >> (8 * j));
        }
    }
}

// Per piece of DMX_PF_PIECE bytes of the packed output: zlib, the sums (a, b) of the piece from
// a = b = 0 with position weights (io_flush's fold: b counts a byte once for every byte from it to
// the piece's end), packed b << 16 | a; gzip, the piece's raw CRC-32 remainder (dmx_crc.h).  A thread
// takes 256 bytes; the slices combine by the same rules.
#define PCHK_T 256u
#define PCHK_MAX_WG 2048u
static_assert(PCHK_T * 256u == DMX_PF_PIECE, "a thread's slice");
__global__ __launch_bounds__(PCHK_T) void dmx_par_check_kernel(const uint8_t* __restrict__ out, uint8_t* __restrict__ work,
                                                               PDecCtl* __restrict__ ctl) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t ra[PCHK_T], rb[PCHK_T];
    if (!ctl->go || ctl->err != PDEC_NOERR || ctl->format == DMX_BATCH_RAW) return;
    constexpr uint32_t M = 65521u;
    const bool gz = ctl->format == DMX_BATCH_GZIP;
    const uint64_t n = ctl->out_len, np = dmx_pf_pieces(n);
    uint32_t* crcs = pdec_crcs(work, n, ctl->nlive);
    uint32_t* adls = crcs + dmx_pf_a256(4 * np) / 4;
    const uint32_t tid = threadIdx.x;
    uint32_t e = tid;
    for (int k = 0; k < 8; k++) e = (e >> 1) ^ ((0u - (e & 1u)) & DMX_CRC_POLY);
    tab[tid] = e;
    const uint32_t xfull = gz ? dmx_gf2_xpow((uint64_t)(PCHK_T - 1 - tid) * 256, 3) : 0u;   // the bytes behind the slice in a full piece
    __syncthreads();
    for (uint64_t pc = blockIdx.x; pc < np; pc += gridDim.x) {
        const uint64_t lo = pc * DMX_PF_PIECE, hi = n - lo < DMX_PF_PIECE ? n : lo + DMX_PF_PIECE;
        const uint64_t s0 = lo + 256ull * tid < hi ? lo + 256ull * tid : hi, s1 = hi - s0 < 256 ? hi : s0 + 256;
        uint32_t va = 0, vb = 0;
        if (gz) {
            uint32_t r = 0;
            for (uint64_t p = s0; p < s1; p++) r = tab[(r ^ out[p]) & 255u] ^ (r >> 8);
            if (s0 < s1) va = dmx_gf2_mulmod(r, hi - lo == DMX_PF_PIECE ? xfull : dmx_gf2_xpow(hi - s1, 3));
        } else {
            uint32_t sa = 0;
            uint64_t sb = 0;   // <= 256 x 65 536 x 255
            for (uint64_t p = s0; p < s1; p++) {
                const uint32_t x = out[p];
                sa += x;
                sb += (hi - p) * x;
            }
            va = sa;
            vb = (uint32_t)(sb % M);
        }
        ra[tid] = va;
        rb[tid] = vb;
        __syncthreads();
        if (tid == 0) {
            if (gz) {
                uint32_t r = 0;
                for (uint32_t k = 0; k < PCHK_T; k++) r ^= ra[k];
                crcs[pc] = r;
            } else {
                uint64_t A = 0, B = 0;
                for (uint32_t k = 0; k < PCHK_T; k++) { A += ra[k]; B += rb[k]; }
                adls[pc] = ((uint32_t)(B % M) << 16) | (uint32_t)(A % M);
            }
        }
        __syncthreads();
    }
}

__global__ void dmx_par_status_kernel(uint8_t* __restrict__ work, PDecCtl* __restrict__ ctl, int verify,
                                      dmx_par_status* __restrict__ st) {
    if (!ctl->go) return;   // the plan's status, -E_INVAL or -E_SZ: begin wrote it
    int err = ctl->err != PDEC_NOERR ? (int)(uint32_t)(ctl->err & 0xFFFFFFFFull) : 0;
    const uint64_t n = ctl->out_len, np = dmx_pf_pieces(n);
    if (!err && verify && ctl->format != DMX_BATCH_RAW) {
        const uint32_t* crcs = pdec_crcs(work, n, ctl->nlive);
        const uint32_t* adls = crcs + dmx_pf_a256(4 * np) / 4;
        if (ctl->format == DMX_BATCH_ZLIB) {
            constexpr uint64_t M = 65521u;
            uint64_t a = 1, b = 0;
            for (uint64_t pc = 0; pc < np; pc++) {   // a' = a + S, b' = b + len a + T
                const uint64_t len = pc + 1 < np ? DMX_PF_PIECE : n - pc * DMX_PF_PIECE;
                b = (b + (len % M) * a + (adls[pc] >> 16)) % M;
                a = (a + (adls[pc] & 0xFFFFu)) % M;
            }
            if ((uint32_t)((b << 16) | a) != ctl->check) err = -(int)E_ZADL32;
        } else {
            const uint32_t xp = dmx_gf2_xpow(DMX_PF_PIECE, 3);
            uint32_t r = 0;
            for (uint64_t pc = 0; pc < np; pc++) {   // R(A || B) = R(A) x^(8 |B|) xor R(B)
                const uint64_t len = pc + 1 < np ? DMX_PF_PIECE : n - pc * DMX_PF_PIECE;
                r = dmx_gf2_mulmod(r, len == DMX_PF_PIECE ? xp : dmx_gf2_xpow(len, 3)) ^ crcs[pc];
            }
            if ((r ^ dmx_crc32_affine(n)) != ctl->check) err = -(int)E_CRC;
            else if (ctl->isize != (uint32_t)n) err = -(int)E_LEN;
        }
    }
    if (err) {
        st->status = err;
        st->out_len = 0;
        st->in_used = 0;
        st->check = 0;
        st->work_len = 0;
    }
}

static inline uint32_t par_chunk(uint32_t chunk_bytes) { return chunk_bytes ? chunk_bytes : DMX_PF_DEF_CHUNK; }

extern "C" uint64_t dmx_inflate_parallel_plan_work(uint64_t zbytes, uint32_t chunk_bytes) {
    const uint32_t chunk = par_chunk(chunk_bytes);
    if (chunk < DMX_PF_MIN_CHUNK || chunk > DMX_PF_MAX_CHUNK || zbytes > DMX_PF_MAX_POS) return 0;
    return dmx_pf_plan_bytes(dmx_pf_nchunks(zbytes, chunk));
}

extern "C" int dmx_inflate_parallel_plan_async(const void* d_z, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                               void* d_plan, uint64_t plan_bytes, void* stream) {
    if (!d_plan || (!d_z && zbytes) || fmt > DMX_BATCH_RAW || ((uintptr_t)d_plan & 255)) return -(int)E_INVAL;
    const uint32_t chunk = par_chunk(chunk_bytes);
    if (chunk < DMX_PF_MIN_CHUNK || chunk > DMX_PF_MAX_CHUNK) return -(int)E_INVAL;
    if (zbytes > DMX_PF_MAX_POS) return -(int)E_RANGE;
    const uint32_t nc = dmx_pf_nchunks(zbytes, chunk);
    if (plan_bytes < dmx_pf_plan_bytes(nc)) return -(int)E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* P = (uint8_t*)d_plan;
    PPlanHead* h = (PPlanHead*)P;
    dmx_pchunk* chunks = (dmx_pchunk*)(P + 256);
    uint64_t* cand = (uint64_t*)(P + 256 + dmx_pf_a256(32ull * nc));
    dmx_pf_meas* meas = (dmx_pf_meas*)((uint8_t*)cand + dmx_pf_a256(8ull * nc));
    uint32_t* gtab = (uint32_t*)((uint8_t*)meas + dmx_pf_a256(32ull * nc));
    const uint8_t* z = (const uint8_t*)d_z;
    hipLaunchKernelGGL(dmx_par_head_kernel, dim3(1), dim3(1), 0, s, z, zbytes, fmt, chunk, nc, h, cand);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_find_kernel<false>, dim3(nc), dim3(64), 0, s, z, zbytes, h, cand);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_measure_kernel<false>, dim3((uint32_t)dmx_pf_meas_wg(nc)), dim3(64), 0, s, z, zbytes, h, cand,
                       meas, nc, gtab, (uint64_t*)nullptr);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_link_kernel, dim3(1), dim3(1), 0, s, z, zbytes, h, cand, meas, chunks, nc);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

extern "C" uint64_t dmx_inflate_parallel_work(uint64_t out_cap, uint32_t max_live) { return dmx_pf_work(out_cap, max_live); }

extern "C" int dmx_inflate_parallel_decode_async(const void* d_z, uint64_t zbytes, const void* d_plan, uint64_t plan_bytes,
                                                 uint32_t max_live, void* d_out, uint64_t out_cap, void* d_work,
                                                 uint64_t work_bytes, int verify, dmx_par_status* d_status, void* stream) {
    if (!d_plan || !d_work || !d_status || (!d_z && zbytes) || (!d_out && out_cap)) return -(int)E_INVAL;
    if (((uintptr_t)d_plan & 255) || ((uintptr_t)d_work & 255) || ((uintptr_t)d_status & 7)) return -(int)E_INVAL;
    if (plan_bytes < dmx_pf_plan_bytes(1) || work_bytes < 256) return -(int)E_INVAL;
    if (zbytes > DMX_PF_MAX_POS) return -(int)E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    const PPlanHead* h = (const PPlanHead*)d_plan;
    const dmx_pchunk* chunks = (const dmx_pchunk*)((const uint8_t*)d_plan + 256);
    uint8_t* work = (uint8_t*)d_work;
    PDecCtl* ctl = (PDecCtl*)work;
    const uint8_t* z = (const uint8_t*)d_z;
    hipLaunchKernelGGL(dmx_par_begin_kernel, dim3(1), dim3(1), 0, s, h, plan_bytes, zbytes, max_live, out_cap, work_bytes, ctl,
                       d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_cells_kernel<false>, dim3((uint32_t)dmx_pf_cell_wg(max_live)), dim3(64), 0, s, z, zbytes, chunks,
                       work, ctl, (const uint8_t*)nullptr, (dmx_pmember*)nullptr, 0u);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_tails_kernel<false>, dim3(1), dim3(PTAIL_T), 0, s, chunks, work, ctl, (const uint8_t*)nullptr);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    const uint64_t pw = (out_cap + 4 * PPACK_T - 1) / (4 * PPACK_T);
    hipLaunchKernelGGL(dmx_par_pack_kernel<false>, dim3(pw < PPACK_MAX_WG ? (pw ? (uint32_t)pw : 1u) : PPACK_MAX_WG),
                       dim3(PPACK_T), 0, s, chunks, work, ctl, (uint8_t*)d_out, (const uint8_t*)nullptr);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (verify) {
        const uint64_t np = dmx_pf_pieces(out_cap);
        hipLaunchKernelGGL(dmx_par_check_kernel, dim3(np < PCHK_MAX_WG ? (uint32_t)np : PCHK_MAX_WG), dim3(PCHK_T), 0, s,
                           (const uint8_t*)d_out, work, ctl);
        if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    }
    hipLaunchKernelGGL(dmx_par_status_kernel, dim3(1), dim3(1), 0, s, work, ctl, verify, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

// ------------------------------------------------------------------------------------
// One foreign file of many gzip members (dmx_inflate_parallel_multi_*, include/dmx.h; DESIGN.md 3.1
// "One foreign file of many members").  The plan and the decode above with MULTI: find also accepts
// member starts, measure walks over BFINAL, cells crosses the members inside a chunk and writes the
// member table, tails and pack bound a reference by its member's start.  d_plan = the single plan's
// parts, then [walks' member offsets 8 x nc][sides 16 x nc], then the tables (dmx_pf_mplan_bytes);
// d_work = [control][tables][cells] as above, then [segment bases 4 x (nm + 1)][segment CRC-32
// remainders 4 x (np + nm)] (dmx_pf_mwork).  Its own kernels: head, link, begin, and the segmented
// check -- segs (one workgroup scans ceil(out_len / 64 KiB) over the members), mcheck (a workgroup
// per segment: the slice code of dmx_par_check_kernel), mcombine (a thread per member) -- and status.
// ------------------------------------------------------------------------------------
__global__ void dmx_parm_head_kernel(const uint8_t* __restrict__ z, uint64_t zbytes, uint32_t chunk, uint32_t nc,
                                     PMPlanHead* __restrict__ h, uint64_t* __restrict__ cand) {
    dmx_par_status st;
    uint64_t body = 0;
    uint32_t format = 0;
    st.status = dmx_frame_head(z, zbytes, DMX_BATCH_GZIP, &format, &body);
    st.format = format;
    st.out_len = st.in_used = st.work_len = 0;
    st.check = st.nlive = st.ndead = st.gave_up = 0;
    st.nchunks = nc;
    st.ncand = st.status ? 0u : 1u;
    h->st = st;
    h->nmembers = 0;
    h->bad_member = 0xFFFFFFFFu;
    h->chunk_bytes = chunk;
    h->isize = 0;
    h->body_bit = 0;
    h->zbytes = zbytes;
    h->next = 0;
    cand[0] = 0;   // the first header
}

__global__ void dmx_parm_link_kernel(const uint8_t* __restrict__ z, uint64_t zbytes, PMPlanHead* __restrict__ h,
                                     const uint64_t* __restrict__ cand, const dmx_pf_meas* __restrict__ meas,
                                     const uint64_t* __restrict__ mloc, dmx_pchunk* __restrict__ chunks,
                                     dmx_pf_mside* __restrict__ sides, uint32_t nc) {
    if (h->st.status) return;
    dmx_par_multi_status ms;
    ms.st = h->st;
    uint32_t isize = 0;
    dmx_pf_link_multi(z, zbytes, cand, meas, mloc, chunks, sides, nc, &ms, &isize);
    h->st = ms.st;
    h->nmembers = ms.nmembers;
    h->bad_member = ms.bad_member;
    h->isize = isize;
}

__device__ __forceinline__ uint32_t* pdec_segbase(uint8_t* work, uint64_t out_len, uint32_t nlive) {
    return (uint32_t*)(pdec_cells(work, nlive) + dmx_pf_a256(2 * out_len));
}
__device__ __forceinline__ uint32_t* pdec_segcrc(uint8_t* work, uint64_t out_len, uint32_t nlive, uint32_t nmembers) {
    return pdec_segbase(work, out_len, nlive) + dmx_pf_a256(4 * ((uint64_t)nmembers + 1)) / 4;
}

__global__ void dmx_parm_begin_kernel(const PMPlanHead* __restrict__ h, uint64_t plan_bytes, uint64_t zbytes, uint32_t max_live,
                                      uint32_t max_members, uint64_t out_cap, uint64_t work_bytes, PDecCtl* __restrict__ ctl,
                                      dmx_par_multi_status* __restrict__ d_status) {
    dmx_par_multi_status ms;
    ms.st = h->st;
    ms.nmembers = h->nmembers;
    ms.bad_member = 0xFFFFFFFFu;
    dmx_par_status& st = ms.st;
    ctl->next = 0;
    ctl->err = PDEC_NOERR;
    ctl->bad = PDEC_NOERR;
    ctl->go = 0;
    if (!st.status) {
        if (h->zbytes != zbytes || !st.nlive || st.nlive > st.nchunks || plan_bytes < dmx_pf_mplan_bytes(st.nchunks) ||
            st.out_len > DMX_PF_MAX_POS || st.format != DMX_BATCH_GZIP || !ms.nmembers) {
            st.status = -(int32_t)E_INVAL;
            st.out_len = st.in_used = st.work_len = 0;
            st.check = 0;
            ms.nmembers = 0;
        } else if (st.nlive > max_live || ms.nmembers > max_members || st.out_len > out_cap ||
                   work_bytes < dmx_pf_mwork(st.out_len, st.nlive, ms.nmembers)) {
            st.status = -(int32_t)E_SZ;   // the record holds the needed numbers
        } else {
            ctl->out_len = st.out_len;
            ctl->nlive = st.nlive;
            ctl->format = st.format;
            ctl->check = st.check;
            ctl->isize = h->isize;
            ctl->nmembers = ms.nmembers;
            ctl->go = 1;
        }
    }
    *d_status = ms;
}

// segbase[m] = the segments of the members in front of m, segbase[nm] = all of them: one workgroup,
// tiles of PSEG_T members, a scan in LDS with the carry in a register.
#define PSEG_T 1024u
__global__ __launch_bounds__(PSEG_T) void dmx_parm_segs_kernel(const dmx_pmember* __restrict__ members, uint8_t* __restrict__ work,
                                                               PDecCtl* __restrict__ ctl) {
    __shared__ uint32_t sc[PSEG_T];
    if (!ctl->go || ctl->err != PDEC_NOERR) return;
    const uint32_t nm = ctl->nmembers, tid = threadIdx.x;
    uint32_t* segbase = pdec_segbase(work, ctl->out_len, ctl->nlive);
    uint32_t carry = 0;
    for (uint32_t m0 = 0; m0 < nm; m0 += PSEG_T) {
        const uint32_t m = m0 + tid;
        const uint32_t v = m < nm ? (uint32_t)((members[m].out_len + DMX_PF_PIECE - 1) / DMX_PF_PIECE) : 0u;
        sc[tid] = v;
        __syncthreads();
        for (uint32_t d = 1; d < PSEG_T; d <<= 1) {
            const uint32_t x = tid >= d ? sc[tid - d] : 0u;
            __syncthreads();
            sc[tid] += x;
            __syncthreads();
        }
        if (m < nm) segbase[m] = carry + sc[tid] - v;
        carry += sc[PSEG_T - 1];
        __syncthreads();
    }
    if (tid == 0) segbase[nm] = carry;
}

__global__ __launch_bounds__(PCHK_T) void dmx_parm_check_kernel(const uint8_t* __restrict__ out,
                                                                const dmx_pmember* __restrict__ members,
                                                                uint8_t* __restrict__ work, PDecCtl* __restrict__ ctl) {
    __shared__ uint32_t tab[256];
    __shared__ uint32_t ra[PCHK_T];
    if (!ctl->go || ctl->err != PDEC_NOERR) return;
    const uint64_t n = ctl->out_len;
    const uint32_t nm = ctl->nmembers;
    const uint32_t* segbase = pdec_segbase(work, n, ctl->nlive);
    uint32_t* segcrc = pdec_segcrc(work, n, ctl->nlive, nm);
    const uint32_t nseg = segbase[nm];
    if (nseg > dmx_pf_pieces(n) + nm) return;   // (a member table that is not the plan's: the combine reports it)
    const uint32_t tid = threadIdx.x;
    uint32_t e = tid;
    for (int k = 0; k < 8; k++) e = (e >> 1) ^ ((0u - (e & 1u)) & DMX_CRC_POLY);
    tab[tid] = e;
    const uint32_t xfull = dmx_gf2_xpow((uint64_t)(PCHK_T - 1 - tid) * 256, 3);   // the bytes behind the slice in a full segment
    __syncthreads();
    for (uint32_t sg = blockIdx.x; sg < nseg; sg += gridDim.x) {
        uint32_t lo_m = 0, hi_m = nm;   // the last member whose first segment is at or before sg
        while (hi_m - lo_m > 1) {
            const uint32_t mid = lo_m + ((hi_m - lo_m) >> 1);
            if (segbase[mid] <= sg) lo_m = mid;
            else hi_m = mid;
        }
        const uint64_t mo = members[lo_m].out_off, ml = members[lo_m].out_len;
        uint64_t lo = mo + (uint64_t)(sg - segbase[lo_m]) * DMX_PF_PIECE, hi = mo + ml;
        if (mo > n || ml > n - mo || lo > hi) lo = hi = 0;   // never outside out[0, out_len)
        if (hi - lo > DMX_PF_PIECE) hi = lo + DMX_PF_PIECE;
        const uint64_t s0 = lo + 256ull * tid < hi ? lo + 256ull * tid : hi, s1 = hi - s0 < 256 ? hi : s0 + 256;
        uint32_t r = 0, va = 0;
        for (uint64_t p = s0; p < s1; p++) r = tab[(r ^ out[p]) & 255u] ^ (r >> 8);
        if (s0 < s1) va = dmx_gf2_mulmod(r, hi - lo == DMX_PF_PIECE ? xfull : dmx_gf2_xpow(hi - s1, 3));
        ra[tid] = va;
        __syncthreads();
        if (tid == 0) {
            uint32_t x = 0;
            for (uint32_t k = 0; k < PCHK_T; k++) x ^= ra[k];
            segcrc[sg] = x;
        }
        __syncthreads();
    }
}

#define PCMB_T 256u
#define PCMB_MAX_WG 1024u
__global__ __launch_bounds__(PCMB_T) void dmx_parm_combine_kernel(const dmx_pmember* __restrict__ members, uint8_t* __restrict__ work,
                                                                  PDecCtl* __restrict__ ctl) {
    if (!ctl->go || ctl->err != PDEC_NOERR) return;
    const uint64_t n = ctl->out_len;
    const uint32_t nm = ctl->nmembers;
    const uint32_t* segbase = pdec_segbase(work, n, ctl->nlive);
    const uint32_t* segcrc = pdec_segcrc(work, n, ctl->nlive, nm);
    const bool sane = segbase[nm] <= dmx_pf_pieces(n) + nm;
    const uint32_t xp = dmx_gf2_xpow(DMX_PF_PIECE, 3);
    for (uint32_t m = blockIdx.x * PCMB_T + threadIdx.x; m < nm; m += gridDim.x * PCMB_T) {
        const uint64_t len = members[m].out_len;
        int err = 0;
        if (!sane) {
            err = -(int)E_RANGE;
        } else {
            uint32_t r = 0;
            uint64_t left = len;
            for (uint32_t sg = segbase[m]; sg < segbase[m + 1]; sg++) {   // R(A || B) = R(A) x^(8 |B|) xor R(B)
                const uint64_t l = left < DMX_PF_PIECE ? left : DMX_PF_PIECE;
                r = dmx_gf2_mulmod(r, l == DMX_PF_PIECE ? xp : dmx_gf2_xpow(l, 3)) ^ segcrc[sg];
                left -= l;
            }
            // (dmx_crc32_affine's two terms, spelled out: with a second caller in this file the compiler
            // stops inlining it into dmx_par_status_kernel, which is to stay the code it was)
            const uint32_t aff = dmx_gf2_mulmod(0xFFFFFFFFu, dmx_gf2_xpow(len, 3)) ^ 0xFFFFFFFFu;
            if ((r ^ aff) != members[m].crc) err = -(int)E_CRC;
            else if (members[m].isize != (uint32_t)len) err = -(int)E_LEN;
        }
        if (err) atomicMin(&ctl->bad, ((unsigned long long)m << 32) | (uint32_t)err);
    }
}

__global__ void dmx_parm_status_kernel(PDecCtl* __restrict__ ctl, dmx_par_multi_status* __restrict__ st) {
    if (!ctl->go) return;   // the plan's status, -E_INVAL or -E_SZ: begin wrote it
    int err = ctl->err != PDEC_NOERR ? (int)(uint32_t)(ctl->err & 0xFFFFFFFFull) : 0;
    if (!err && ctl->bad != PDEC_NOERR) {
        err = (int)(uint32_t)(ctl->bad & 0xFFFFFFFFull);
        st->bad_member = (uint32_t)(ctl->bad >> 32);
    }
    if (err) {
        st->st.status = err;
        st->st.out_len = 0;
        st->st.in_used = 0;
        st->st.check = 0;
        st->st.work_len = 0;
    }
}

extern "C" uint64_t dmx_inflate_parallel_multi_plan_work(uint64_t zbytes, uint32_t chunk_bytes) {
    const uint32_t chunk = par_chunk(chunk_bytes);
    if (chunk < DMX_PF_MIN_CHUNK || chunk > DMX_PF_MAX_CHUNK || zbytes > DMX_PF_MAX_POS) return 0;
    return dmx_pf_mplan_bytes(dmx_pf_nchunks(zbytes, chunk));
}

extern "C" int dmx_inflate_parallel_multi_plan_async(const void* d_z, uint64_t zbytes, uint32_t fmt, uint32_t chunk_bytes,
                                                     void* d_plan, uint64_t plan_bytes, void* stream) {
    if (!d_plan || (!d_z && zbytes) || ((uintptr_t)d_plan & 255)) return -(int)E_INVAL;
    if (fmt != DMX_BATCH_AUTO && fmt != DMX_BATCH_GZIP) return -(int)E_INVAL;
    const uint32_t chunk = par_chunk(chunk_bytes);
    if (chunk < DMX_PF_MIN_CHUNK || chunk > DMX_PF_MAX_CHUNK) return -(int)E_INVAL;
    if (zbytes > DMX_PF_MAX_POS) return -(int)E_RANGE;
    const uint32_t nc = dmx_pf_nchunks(zbytes, chunk);
    if (plan_bytes < dmx_pf_mplan_bytes(nc)) return -(int)E_INVAL;
    hipStream_t s = (hipStream_t)stream;
    uint8_t* P = (uint8_t*)d_plan;
    PMPlanHead* h = (PMPlanHead*)P;
    dmx_pchunk* chunks = (dmx_pchunk*)(P + 256);
    uint64_t* cand = (uint64_t*)(P + 256 + dmx_pf_a256(32ull * nc));
    dmx_pf_meas* meas = (dmx_pf_meas*)((uint8_t*)cand + dmx_pf_a256(8ull * nc));
    uint64_t* mloc = (uint64_t*)((uint8_t*)meas + dmx_pf_a256(32ull * nc));
    dmx_pf_mside* sides = (dmx_pf_mside*)((uint8_t*)mloc + dmx_pf_a256(8ull * nc));
    uint32_t* gtab = (uint32_t*)((uint8_t*)sides + dmx_pf_a256(16ull * nc));
    const uint8_t* z = (const uint8_t*)d_z;
    hipLaunchKernelGGL(dmx_parm_head_kernel, dim3(1), dim3(1), 0, s, z, zbytes, chunk, nc, h, cand);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_find_kernel<true>, dim3(nc), dim3(64), 0, s, z, zbytes, h, cand);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_measure_kernel<true>, dim3((uint32_t)dmx_pf_meas_wg(nc)), dim3(64), 0, s, z, zbytes, h, cand, meas,
                       nc, gtab, mloc);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_parm_link_kernel, dim3(1), dim3(1), 0, s, z, zbytes, h, cand, meas, mloc, chunks, sides, nc);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

extern "C" uint64_t dmx_inflate_parallel_multi_work(uint64_t out_cap, uint32_t max_live, uint32_t max_members) {
    return dmx_pf_mwork(out_cap, max_live, max_members);
}

extern "C" int dmx_inflate_parallel_multi_decode_async(const void* d_z, uint64_t zbytes, const void* d_plan, uint64_t plan_bytes,
                                                       uint32_t max_live, uint32_t max_members, void* d_out, uint64_t out_cap,
                                                       dmx_pmember* d_members, void* d_work, uint64_t work_bytes, int verify,
                                                       dmx_par_multi_status* d_status, void* stream) {
    if (!d_plan || !d_work || !d_status || (!d_z && zbytes) || (!d_out && out_cap) || (!d_members && max_members))
        return -(int)E_INVAL;
    if (((uintptr_t)d_plan & 255) || ((uintptr_t)d_work & 255) || ((uintptr_t)d_status & 7) || ((uintptr_t)d_members & 7))
        return -(int)E_INVAL;
    if (plan_bytes < dmx_pf_mplan_bytes(1) || work_bytes < 256) return -(int)E_INVAL;
    if (zbytes > DMX_PF_MAX_POS) return -(int)E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    const PMPlanHead* h = (const PMPlanHead*)d_plan;
    const dmx_pchunk* chunks = (const dmx_pchunk*)((const uint8_t*)d_plan + 256);
    uint8_t* work = (uint8_t*)d_work;
    PDecCtl* ctl = (PDecCtl*)work;
    const uint8_t* z = (const uint8_t*)d_z;
    hipLaunchKernelGGL(dmx_parm_begin_kernel, dim3(1), dim3(1), 0, s, h, plan_bytes, zbytes, max_live, max_members, out_cap,
                       work_bytes, ctl, d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    const uint8_t* plan = (const uint8_t*)d_plan;
    hipLaunchKernelGGL(dmx_par_cells_kernel<true>, dim3((uint32_t)dmx_pf_cell_wg(max_live)), dim3(64), 0, s, z, zbytes, chunks,
                       work, ctl, plan, d_members, max_members);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_par_tails_kernel<true>, dim3(1), dim3(PTAIL_T), 0, s, chunks, work, ctl, plan);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    const uint64_t pw = (out_cap + 4 * PPACK_T - 1) / (4 * PPACK_T);
    hipLaunchKernelGGL(dmx_par_pack_kernel<true>, dim3(pw < PPACK_MAX_WG ? (pw ? (uint32_t)pw : 1u) : PPACK_MAX_WG),
                       dim3(PPACK_T), 0, s, chunks, work, ctl, (uint8_t*)d_out, plan);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    if (verify) {
        hipLaunchKernelGGL(dmx_parm_segs_kernel, dim3(1), dim3(PSEG_T), 0, s, (const dmx_pmember*)d_members, work, ctl);
        if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
        const uint64_t ns = dmx_pf_pieces(out_cap) + max_members;
        hipLaunchKernelGGL(dmx_parm_check_kernel, dim3(ns < PCHK_MAX_WG ? (uint32_t)ns : PCHK_MAX_WG), dim3(PCHK_T), 0, s,
                           (const uint8_t*)d_out, (const dmx_pmember*)d_members, work, ctl);
        if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
        const uint32_t cw = (max_members + PCMB_T - 1) / PCMB_T;
        hipLaunchKernelGGL(dmx_parm_combine_kernel, dim3(cw < PCMB_MAX_WG ? (cw ? cw : 1u) : PCMB_MAX_WG), dim3(PCMB_T), 0, s,
                           (const dmx_pmember*)d_members, work, ctl);
        if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    }
    hipLaunchKernelGGL(dmx_parm_status_kernel, dim3(1), dim3(1), 0, s, ctl, d_status);
    return hipGetLastError() == hipSuccess ? 0 : -(int)E_DEVICE;
}

// ------------------------------------------------------------------------------------
// Chained decode (dictionary streams, DMX_F_DICT: a block's matches may reach into the block
// before it).  Three steps, all blocks in parallel:
//   1. dmx_inflate_index_kernel<true>: every sw block decodes on its own into 16-bit cells; a
//      byte it cannot know yet (a match source before the block's first output byte, or a
//      copy of such a cell) becomes a reference cell 0x100 + b - 1 = the byte b positions
//      before the block's start.  Copies inside the block copy cells, so a reference always
//      names a byte of an EARLIER block.
//   2. dmx_cells_prep_kernel: each reference becomes an absolute source position s; a source
//      that is already a byte is copied at once, otherwise P[j] = s, the cell is marked
//      unresolved (0xFFFF) and j goes on its block's list (as a 16-bit offset in the block).  The lists are per block -- block
//      b's entries sit in [out_off, out_off + count) of a list buffer, so a workgroup appends
//      with one LDS atomic per wave and no global atomic at all.
//      dmx_cells_jump_kernel, about log2(nblk) + 2 launches of one workgroup per block, each
//      over the list the one before it left: an unresolved j looks at s = P[j]: a resolved
//      cell is copied; otherwise it follows up to CHAIN_HOPS - 1 more links s <- P[s] in the
//      same launch, and if none reaches a byte, P[j] = P[s] and j goes on the next list (pointer jumping:
//      chains of references through many blocks -- a run carried across every block, say --
//      halve each launch).  In place: a stale read only delays resolution, never changes the
//      value (P moves along the chain, a resolved cell stays).  A block whose list is empty
//      returns at once.
//   3. dmx_cells_final_kernel: cells -> bytes; any cell still unresolved is an error.
// ------------------------------------------------------------------------------------
#define CHAIN_ROUNDS_MAX 40
#define CHAIN_WG 1024   // threads per block in prep and jump: a block's list is latency-bound
#ifndef CHAIN_HOPS
#define CHAIN_HOPS 3    // links followed per list entry and jump launch (1: 16.1, 2: 18.1, 3: 18.4, 4: 18.2 GB/s, `profiles/r03_h`)
#endif
#ifndef CHAIN_ILP
#define CHAIN_ILP 2     // list entries per jump thread in flight (two links each: 2 beat 4, `profiles/r03_d3`)
#endif

// Appends v at list[*lds_cnt ...] for every lane with want set; the whole wave calls it.
__device__ inline void chain_push(bool want, uint32_t v, uint16_t* __restrict__ list, uint32_t* lds_cnt) {
    const uint64_t m = __ballot(want);
    if (!m) return;
    const int lead = __ffsll((unsigned long long)m) - 1;
    const uint32_t lane = threadIdx.x & 63;
    uint32_t base = 0;
    if ((int)lane == lead) base = atomicAdd(lds_cnt, (uint32_t)__popcll(m));
    base = __shfl(base, lead);
    if (want) list[base + __popcll(m & ((1ull << lane) - 1))] = (uint16_t)v;
}

__global__ __launch_bounds__(CHAIN_WG) void dmx_cells_prep_kernel(const dmx_iblock* __restrict__ index, uint16_t* cells,
                                                            uint32_t* P, uint16_t* __restrict__ list,
                                                            uint32_t* __restrict__ count, uint32_t* __restrict__ total,
                                                            uint64_t cap, dmx_inflate_status* __restrict__ st) {
    __shared__ uint32_t nl;
    const uint64_t off = index[blockIdx.x].out_off;
    const uint32_t len = index[blockIdx.x].out_len;
    if (off > cap || len > cap - off || len > IW) {   // the decode already failed this index; read nothing
        if (threadIdx.x == 0) {
            count[blockIdx.x] = 0;
            atomicCAS(&st->status, 0, -(int32_t)E_RANGE);
        }
        return;
    }
    if (threadIdx.x == 0) nl = 0;
    __syncthreads();
    bool bad = false;
    for (uint32_t j0 = 0; j0 < len; j0 += CHAIN_WG) {   // uniform trip count: chain_push needs the whole wave
        const uint32_t j = j0 + threadIdx.x;
        bool want = false;
        if (j < len) {
            const uint32_t c = cells[off + j];
            if (c >= 0x100u) {
                const uint64_t back = (uint64_t)(c - 0xFFu) + j;   // positions before j
                if (back > off + j) {
                    bad = true;
                } else {
                    const uint32_t sp = (uint32_t)(off + j - back);
                    // a byte cell never changes; a reference (raw or already marked) waits
                    const uint16_t cs = cells[sp];
                    if (cs < 0x100u) {
                        cells[off + j] = cs;
                    } else {
                        P[off + j] = sp;
                        cells[off + j] = 0xFFFFu;
                        want = true;
                    }
                }
            }
        }
        chain_push(want, j, list + off, &nl);   // block-relative: 2 bytes an entry
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        count[blockIdx.x] = nl;
        if (nl) atomicAdd(total, nl);
    }
    if (bad) atomicCAS(&st->status, 0, -(int32_t)E_HUFDIS);
}

__global__ __launch_bounds__(CHAIN_WG) void dmx_cells_jump_kernel(const dmx_iblock* __restrict__ index, uint16_t* cells,
                                                                 uint32_t* P, const uint16_t* __restrict__ lin,
                                                                 uint16_t* __restrict__ lout, const uint32_t* __restrict__ cin,
                                                                 uint32_t* __restrict__ cout, uint32_t* __restrict__ total) {
    __shared__ uint32_t nl;
    const uint32_t cnt = cin[blockIdx.x];
    if (cnt == 0) {
        if (threadIdx.x == 0) cout[blockIdx.x] = 0;
        return;
    }
    const uint64_t off = index[blockIdx.x].out_off;
    if (threadIdx.x == 0) nl = 0;
    __syncthreads();
    // CHAIN_ILP entries per thread, their dependent loads (list, P, cell, P) interleaved
    for (uint32_t u0 = 0; u0 < cnt; u0 += CHAIN_ILP * CHAIN_WG) {
        uint32_t j[CHAIN_ILP], sp[CHAIN_ILP];
        uint16_t cs[CHAIN_ILP];
        bool act[CHAIN_ILP], want[CHAIN_ILP];
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++) {
            const uint32_t u = u0 + k * CHAIN_WG + threadIdx.x;
            act[k] = u < cnt;
            j[k] = act[k] ? (uint32_t)(off + lin[off + u]) : 0;
        }
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++) {
            sp[k] = act[k] ? P[j[k]] : 0;
            act[k] = act[k] && sp[k] < j[k];   // never otherwise from a well-formed prep: stays unresolved
        }
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++)
            cs[k] = act[k] ? cells[sp[k]] : 0;   // (plain loads: a stale copy is an older link of the chain)
#if CHAIN_HOPS > 1
        // more links in the same launch: while the source is unresolved, step to its own source
        // (P[s] < s on a well-formed chain); a byte found resolves j now, otherwise j jumps to
        // the last source's P (CHAIN_HOPS links a launch)
        uint32_t cur[CHAIN_ILP];
        bool ok[CHAIN_ILP];
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++) { cur[k] = sp[k]; ok[k] = true; }
#pragma unroll
        for (int h = 1; h < CHAIN_HOPS; h++) {
            uint32_t nx[CHAIN_ILP];
#pragma unroll
            for (int k = 0; k < CHAIN_ILP; k++) {
                nx[k] = (act[k] && ok[k] && cs[k] == 0xFFFFu) ? P[cur[k]] : 0u;
                if (act[k] && ok[k] && cs[k] == 0xFFFFu && nx[k] >= cur[k]) ok[k] = false;   // (malformed: stays)
            }
#pragma unroll
            for (int k = 0; k < CHAIN_ILP; k++)
                if (act[k] && ok[k] && cs[k] == 0xFFFFu) { cs[k] = cells[nx[k]]; cur[k] = nx[k]; }
        }
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++) {
            want[k] = false;
            if (act[k]) {
                if (cs[k] != 0xFFFFu) {
                    cells[j[k]] = cs[k];
                } else {
                    P[j[k]] = ok[k] ? P[cur[k]] : cur[k];
                    want[k] = true;
                }
            }
        }
#else
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++) {
            want[k] = false;
            if (act[k]) {
                if (cs[k] != 0xFFFFu) {
                    cells[j[k]] = cs[k];
                } else {
                    P[j[k]] = P[sp[k]];
                    want[k] = true;
                }
            }
        }
#endif
#pragma unroll
        for (int k = 0; k < CHAIN_ILP; k++) chain_push(want[k], (uint32_t)(j[k] - off), lout + off, &nl);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        cout[blockIdx.x] = nl;
        if (nl) atomicAdd(total, nl);
    }
}

// One workgroup per sw block: its own output range [out_off, out_off + out_len) of the index,
// cells -> bytes.  Positions of d_out the index does not cover are neither read nor written
// (out_cap is a capacity: the cell scratch past the decoded bytes was never initialised).
__global__ __launch_bounds__(256) void dmx_cells_final_kernel(const dmx_iblock* __restrict__ index,
                                                             const uint16_t* __restrict__ cells, uint8_t* __restrict__ out,
                                                             uint64_t cap, dmx_inflate_status* __restrict__ st) {
    const uint64_t off = index[blockIdx.x].out_off;
    const uint32_t len = index[blockIdx.x].out_len;
    if (off > cap || len > cap - off || len > IW) return;   // the decode already failed this index
    const uint64_t n = off + len;
    bool bad = false;
    // 16 positions per thread and step; the range's unaligned head and tail byte by byte
    const uint64_t a0 = min((off + 15) & ~15ull, n), a1 = max(a0, n & ~15ull);
    for (uint64_t j = off + threadIdx.x; j < a0; j += 256) {
        bad = bad || cells[j] > 0xFFu;
        out[j] = (uint8_t)cells[j];
    }
    for (uint64_t j = a1 + threadIdx.x; j < n; j += 256) {
        bad = bad || cells[j] > 0xFFu;
        out[j] = (uint8_t)cells[j];
    }
    if (((uintptr_t)out & 15) == 0) {
        for (uint64_t j0 = a0 + (uint64_t)threadIdx.x * 16; j0 < a1; j0 += 256 * 16) {
            const uint4 a = *reinterpret_cast<const uint4*>(cells + j0), b = *reinterpret_cast<const uint4*>(cells + j0 + 8);
            const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            uint32_t o[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint32_t lo = w[2 * k], hi = w[2 * k + 1];
                bad = bad || ((lo | hi) & 0xFF00FF00u) != 0;
                o[k] = (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi << 8) & 0xFF000000u);
            }
            *reinterpret_cast<uint4*>(out + j0) = make_uint4(o[0], o[1], o[2], o[3]);
        }
    } else {
        for (uint64_t j = a0 + threadIdx.x; j < a1; j += 256) {
            bad = bad || cells[j] > 0xFFu;
            out[j] = (uint8_t)cells[j];
        }
    }
    if (bad) atomicCAS(&st->status, 0, -(int32_t)E_HUFDIS);
}

// work layout: [list totals per round, 256 B][list lengths 2 x nblk, 256-aligned][tables ITAB_WORDS x nblk]
// [cells 2*cap, 256-aligned][P 4*cap][list A 2*cap][list B 2*cap] (list entries: 16-bit block-relative)
static inline uint64_t chain_a256(uint64_t x) { return (x + 255) & ~255ull; }

extern "C" uint64_t dmx_inflate_chained_work(uint64_t out_cap, uint32_t nblk) {
    return 256 + chain_a256(8ull * nblk) + 4ull * ITAB_WORDS * nblk + chain_a256(2 * out_cap) + 8 * out_cap;
}

// The reference lists' total lengths of the last chained decode on this work buffer: [0] after
// the prep kernel, [r + 1] after jump launch r (a diagnostic: how fast the chains resolve).
extern "C" int dmx_inflate_chained_lists(const void* d_work, uint32_t* host, uint32_t n, void* stream) {
    if (!d_work || !host || n > CHAIN_ROUNDS_MAX + 1) return -(int)E_INVAL;
    if (hipMemcpyAsync(host, d_work, 4ull * n, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess ||
        hipStreamSynchronize((hipStream_t)stream) != hipSuccess)
        return -(int)E_DEVICE;
    return 0;
}

extern "C" int dmx_inflate_chained_async(const void* d_z, uint64_t zbytes, const dmx_iblock* d_index, uint32_t nblk,
                                         void* d_out, uint64_t out_cap, void* d_work, uint64_t work_bytes,
                                         dmx_inflate_status* d_status, void* stream) {
    if (!d_z || !d_out || !d_status || !d_index || !nblk || !d_work) return -(int)E_INVAL;
    if (zbytes > 0xFFFFFFF0ull || out_cap > 0xFFFFFFF0ull) return -(int)E_RANGE;   // 32-bit positions
    if (work_bytes < dmx_inflate_chained_work(out_cap, nblk) || ((uintptr_t)d_work & 255)) return -(int)E_SZ;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* T = (uint32_t*)d_work;   // list totals per round
    uint32_t* C[2] = {T + 64, T + 64 + nblk};
    uint32_t* gtab = (uint32_t*)((uint8_t*)d_work + 256 + chain_a256(8ull * nblk));
    uint16_t* cells = (uint16_t*)(gtab + (uint64_t)ITAB_WORDS * nblk);
    uint32_t* P = (uint32_t*)((uint8_t*)cells + chain_a256(2 * out_cap));
    uint16_t* L[2] = {(uint16_t*)(P + out_cap), (uint16_t*)(P + out_cap) + out_cap};
    if (hipMemsetAsync(d_status, 0, sizeof(dmx_inflate_status), s) != hipSuccess) return -(int)E_DEVICE;
    if (hipMemsetAsync(T, 0, 256, s) != hipSuccess) return -(int)E_DEVICE;
    hipLaunchKernelGGL(dmx_inflate_index_kernel<true>, dim3(nblk), dim3(64), 0, s, (const uint8_t*)d_z, zbytes, d_index,
                       (uint8_t*)cells, out_cap, gtab, (uint32_t)IW, d_status, (const uint32_t*)nullptr);
    hipLaunchKernelGGL(dmx_cells_prep_kernel, dim3(nblk), dim3(CHAIN_WG), 0, s, d_index, cells, P, L[0], C[0], T, out_cap, d_status);
    uint32_t rounds = 2;   // pointer jumping: a chain through k blocks takes ~log2(k) + 1 rounds
    while ((1ull << (rounds - 2)) < (uint64_t)nblk && rounds < CHAIN_ROUNDS_MAX) rounds++;
    for (uint32_t rd = 0; rd < rounds; rd++)
        hipLaunchKernelGGL(dmx_cells_jump_kernel, dim3(nblk), dim3(CHAIN_WG), 0, s, d_index, cells, P, L[rd & 1],
                           L[(rd + 1) & 1], C[rd & 1], C[(rd + 1) & 1], T + rd + 1);
    hipLaunchKernelGGL(dmx_cells_final_kernel, dim3(nblk), dim3(256), 0, s, d_index, cells, (uint8_t*)d_out, out_cap,
                       d_status);
    if (hipGetLastError() != hipSuccess) return -(int)E_DEVICE;
    return 0;
}

#ifdef DMX_INF_STAMPS
// diagnostic builds: copy the per-workgroup phase totals of the last indexed launch
extern "C" int dmx_inflate_stamps(void* host, uint64_t bytes) {
    if (bytes > sizeof(dmx_inf_st)) bytes = sizeof(dmx_inf_st);
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(dmx_inf_st), bytes, 0, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif
