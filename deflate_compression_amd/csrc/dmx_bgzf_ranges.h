// dmx_bgzf_ranges.h -- batched range reads from a BGZF file in device memory
// (dmx_bgzf_read_ranges_async, DESIGN.md §3.5 "Reading ranges"), stage by stage: what one thread of
// every planning kernel and of the gather does, so that the kernels of dmx_bgzf_ranges.hip and the
// loops of the host twin (tests/c/bgzf_ranges_model.cpp) run the same text.  The collectives between
// the per-thread parts -- the exclusive scan over a workgroup -- are the caller's: LDS on the
// device, a loop in the twin.  Host and device, C++ only, internal.
#ifndef DMX_BGZF_RANGES_H
#define DMX_BGZF_RANGES_H

#include <stdint.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_bgzf_step.h"

// Scan tiles: a workgroup's share of the members / of the ranges, one element per thread.  The
// twin shrinks them (4 and 8) so that small inputs cross many tile edges.
#ifndef DMX_BRR_MTILE
#define DMX_BRR_MTILE 256u
#endif
#ifndef DMX_BRR_RTILE
#define DMX_BRR_RTILE 256u
#endif
// threads of the one workgroup that scans the tile sums (a contiguous share of the tiles each)
#ifndef DMX_BRR_STHREADS
#define DMX_BRR_STHREADS 1024u
#endif
#define DMX_BRR_GROUP 16u          // bytes of d_out per thread and step of the gather: an aligned 16-byte group
#define DMX_BRR_NOBAD 0xFFFFFFFFu

#if defined(__HIP_DEVICE_COMPILE__)
#define DMX_BRR_ADD(p, v) atomicAdd((p), (v))
#define DMX_BRR_MIN(p, v) atomicMin((p), (v))
#define DMX_BRR_OR(p, v) atomicOr((p), (v))
#else
#define DMX_BRR_ADD(p, v) (void)(*(p) += (v))
#define DMX_BRR_MIN(p, v) (void)(*(p) = *(p) < (v) ? *(p) : (v))
#define DMX_BRR_OR(p, v) (void)(*(p) |= (v))
#endif

// The head of d_work (256 bytes): what the stages hand to each other.
struct dmx_brr_head {
    uint32_t count;     // members the decode, the CRC pass and the gather work on: nmembers, or 0 with any status
    uint32_t bad;       // lowest index of a range that is -E_RANGE (an integer minimum), else DMX_BRR_NOBAD
    uint32_t invalid;   // != 0: an index entry failed dmx_brr_entry_ok
    uint32_t reserved;
    uint64_t out_len;   // the sum of the clipped lengths (saturating)
    uint64_t reserved2;
    dmx_inflate_status ist;   // the record of the decode and the CRC pass (its out_len counts decoded bytes)
};

// sums of clipped lengths saturate: len is any 64-bit value, 2^31 ranges of a file of 2^43 bytes
// pass 2^64, and a saturated sum is above every capacity (-E_SZ)
DMX_HD static inline uint64_t dmx_brr_sat(uint64_t a, uint64_t b) {
    const uint64_t s = a + b;
    return s < a ? ~0ull : s;
}
struct dmx_brr_op_add {
    template <typename T>
    DMX_HD T operator()(T a, T b) const { return a + b; }
};
struct dmx_brr_op_sat {
    DMX_HD uint64_t operator()(uint64_t a, uint64_t b) const { return dmx_brr_sat(a, b); }
};

// the last entry of idx[0..n), n >= 1, whose out_off (or bit) is <= x; 0 when there is none.
// Ends inside 0..n-1 whatever the entries hold.
DMX_HD static inline uint32_t dmx_brr_find_off(const dmx_iblock* idx, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (idx[mid].out_off <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}
DMX_HD static inline uint32_t dmx_brr_find_bit(const dmx_iblock* idx, uint32_t n, uint64_t x) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (idx[mid].bit <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- dmx_brr_plan_kernel: a thread per range q (nblk >= 1).  Clips the range as pread does
// against the decoded length of the file, finds the first and the last member it touches, adds +1 / -1 to the
// members' difference array (diff[0..nblk], integer atomics: any order gives the same sums), and
// stores the clipped length, the first member and the offset of the range's first byte in it.
// With DMX_RANGES_VIRTUAL off >> 16 is a member's file offset: the walk's own step
// (dmx_bgzf_step: bounds-checked, and FNAME / FCOMMENT / FHCRC behind the FEXTRA field count) gives
// the first bit of its DEFLATE data, 8 (offset + 12 + XLEN) for a member without those fields, and
// the entry with that bit is the member; none, or off & 0xFFFF at or past its out_len with
// len != 0, makes q a bad range.  Returns the clipped length.
DMX_HD static inline uint64_t dmx_brr_plan(const uint8_t* z, uint64_t zlen, const dmx_iblock* idx, uint32_t nblk,
                                           const dmx_brange* rg, uint32_t q, uint32_t flags, int32_t* diff,
                                           uint64_t* clen, uint32_t* rm0, uint32_t* rdelta, dmx_brr_head* head) {
    const uint64_t total = idx[nblk - 1].out_off + idx[nblk - 1].out_len;
    uint64_t off = rg[q].off;
    const uint64_t len = rg[q].len;
    uint32_t m0 = 0;
    bool have = false;
    if (flags & DMX_RANGES_VIRTUAL) {
        const uint64_t p = off >> 16;
        const uint32_t within = (uint32_t)(off & 0xFFFFu);
        dmx_bgzf_member mb;
        bool bad = p >= zlen || dmx_bgzf_step(z, zlen, p, DMX_BGZF_MAX_ISIZE, &mb) != 0;
        if (!bad) {
            const uint64_t bit = 8 * (p + mb.body);
            m0 = dmx_brr_find_bit(idx, nblk, bit);
            bad = idx[m0].bit != bit || (len && within >= idx[m0].out_len);
        }
        if (bad) {
            DMX_BRR_MIN(&head->bad, q);
            off = total;   // (nothing of it is read)
        } else {
            off = idx[m0].out_off + within;
            have = true;
        }
    }
    uint64_t c = 0;
    uint32_t delta = 0;
    if (off < total && len) {
        c = len < total - off ? len : total - off;
        if (!have) m0 = dmx_brr_find_off(idx, nblk, off);
        const uint32_t m1 = dmx_brr_find_off(idx, nblk, off + c - 1);
        DMX_BRR_ADD(&diff[m0], 1);
        DMX_BRR_ADD(&diff[m1 + 1], -1);
        delta = (uint32_t)(off - idx[m0].out_off);
    } else {
        m0 = 0;
    }
    clen[q] = c;
    rm0[q] = m0;
    rdelta[q] = delta;
    return c;
}

// ---- dmx_brr_msum_kernel, the index check: a thread per entry m.  File order, out_len in
// 1..65 536, every entry's bytes right behind those of the entry before it, the first at 0.
DMX_HD static inline bool dmx_brr_entry_ok(const dmx_iblock* idx, uint32_t m) {
    const uint32_t n = idx[m].out_len;
    if (n < 1 || n > DMX_BGZF_MAX_ISIZE) return false;
    if (m == 0) return idx[0].out_off == 0;
    return idx[m].out_off == idx[m - 1].out_off + idx[m - 1].out_len && idx[m].bit > idx[m - 1].bit;
}

// ---- dmx_brr_scan1_kernel / dmx_brr_scan2_kernel, the scan of the tile sums, by the one
// workgroup of DMX_BRR_STHREADS threads: thread t owns the tiles [a, b) of n, sums them (dmx_brr_chunk_sum), and -- given the sum over the threads
// before it -- replaces every one by the sum of the tiles before it (dmx_brr_chunk_apply).
DMX_HD static inline void dmx_brr_chunk(uint32_t n, uint32_t nth, uint32_t t, uint32_t* a, uint32_t* b) {
    const uint64_t per = ((uint64_t)n + nth - 1) / nth;
    const uint64_t lo = (uint64_t)t * per < n ? (uint64_t)t * per : n;
    *a = (uint32_t)lo;
    *b = (uint32_t)(lo + per < n ? lo + per : n);
}
template <typename T, typename Op>
DMX_HD static inline T dmx_brr_chunk_sum(const T* v, uint32_t n, uint32_t nth, uint32_t t, Op op) {
    uint32_t a, b;
    dmx_brr_chunk(n, nth, t, &a, &b);
    T s = 0;
    for (uint32_t k = a; k < b; k++) s = op(s, v[k]);
    return s;
}
template <typename T, typename Op>
DMX_HD static inline void dmx_brr_chunk_apply(T* v, uint32_t n, uint32_t nth, uint32_t t, T run, Op op) {
    uint32_t a, b;
    dmx_brr_chunk(n, nth, t, &a, &b);
    for (uint32_t k = a; k < b; k++) {
        const T c = v[k];
        v[k] = run;
        run = op(run, c);
    }
}

// ---- dmx_brr_need_kernel: need[m] = the prefix of the difference array at m is above 0 (the
// ranges that began at or before m and have not ended before it).  `before` = the sum of diff
// over the members before m.
DMX_HD static inline uint32_t dmx_brr_need(int32_t before, int32_t diff_m) { return before + diff_m > 0 ? 1u : 0u; }

// ---- dmx_brr_scan2_kernel, the decision, by one thread once the scans are done: the status by
// precedence (index check,
// bad range, capacities), the record, the device count and the decode's own record.
DMX_HD static inline void dmx_brr_decide(dmx_brr_head* head, uint32_t nmembers, uint64_t scratch_len, uint32_t max_members,
                                         uint64_t scratch_bytes, uint64_t out_cap, dmx_bgzf_ranges_status* rec) {
    dmx_bgzf_ranges_status r = {0, 0, 0, 0, DMX_BRR_NOBAD, 0};
    if (head->invalid) {
        r.status = -(int32_t)E_INVAL;
    } else if (head->bad != DMX_BRR_NOBAD) {
        r.status = -(int32_t)E_RANGE;
        r.bad = head->bad;
    } else {
        r.nmembers = nmembers;
        r.out_len = head->out_len;
        r.scratch_len = scratch_len;
        if (nmembers > max_members || scratch_len > scratch_bytes || head->out_len > out_cap) r.status = -(int32_t)E_SZ;
    }
    *rec = r;
    head->count = r.status ? 0 : nmembers;
    head->ist.status = r.status;   // a status here: the decode exits by the count, the CRC pass by this word
    head->ist.reserved = 0;
    head->ist.out_len = 0;
}

// ---- dmx_brr_emit_kernel.  A needed member m of rank `rank` whose bytes begin at `soff` of the scratch:
// its sub-index entry, its wanted CRC word (crc may be NULL), and its scratch offset for the gather.
DMX_HD static inline void dmx_brr_emit_member(const dmx_iblock* idx, const uint32_t* crc, uint32_t m, uint32_t rank,
                                              uint64_t soff, dmx_iblock* sub, uint32_t* subcrc, uint64_t* moff) {
    dmx_iblock e;
    e.bit = idx[m].bit;
    e.out_off = soff;
    e.out_len = idx[m].out_len;
    e.reserved = 0;
    sub[rank] = e;
    subcrc[rank] = crc ? crc[m] : 0u;
    moff[m] = soff;
}
// slot j of the sub-index at or past the count: an empty entry, whose CRC-32 is 0
DMX_HD static inline void dmx_brr_emit_slot(uint32_t j, dmx_iblock* sub, uint32_t* subcrc) {
    const dmx_iblock e = {0, 0, 0, 0};
    sub[j] = e;
    subcrc[j] = 0;
}

// ---- dmx_brr_gather_kernel: the aligned 16-byte group g of d_out (group 0 holds d_out[0], `head` bytes
// into it).  Its bytes are the positions [16 g - head, 16 g - head + 16) of the packed output, cut
// to [0, out_len): they belong to the range q found by binary search in out_off (the last one that
// starts at or before the first byte) and, where the group runs past its end, to the ranges behind
// it.  The bytes of range q are one piece of the scratch: they begin at
// moff[rm0[q]] + rdelta[q].  A whole group inside one range is one 16-byte load (any alignment)
// and one aligned 16-byte store; head, tail and groups across ranges go byte by byte.
DMX_HD static inline void dmx_brr_gather_group(uint64_t g, uint32_t head, uint64_t out_len, const uint64_t* out_off,
                                               uint32_t nranges, const uint32_t* rm0, const uint32_t* rdelta,
                                               const uint64_t* moff, const uint8_t* scratch, uint8_t* out) {
    const uint64_t lo = g * DMX_BRR_GROUP < head ? 0 : g * DMX_BRR_GROUP - head;
    uint64_t hi = g * DMX_BRR_GROUP + DMX_BRR_GROUP - head;
    if (hi > out_len) hi = out_len;
    if (lo >= hi) return;
    uint32_t q = 0, qh = nranges;   // out_off[0] = 0 <= lo
    while (qh - q > 1) {
        const uint32_t mid = q + (qh - q) / 2;
        if (out_off[mid] <= lo) q = mid;
        else qh = mid;
    }
    uint64_t p = lo;
    while (p < hi) {   // (out_off[nranges] = out_len >= hi: q stays below nranges)
        const uint64_t end = out_off[q + 1] < hi ? out_off[q + 1] : hi;
        if (end > p) {
            const uint8_t* src = scratch + moff[rm0[q]] + rdelta[q] + (p - out_off[q]);
            uint8_t* dst = out + p;
            if (end - p == DMX_BRR_GROUP) {
                memcpy(__builtin_assume_aligned(dst, DMX_BRR_GROUP), src, DMX_BRR_GROUP);
            } else {
                for (uint64_t k = 0; k < end - p; k++) dst[k] = src[k];
            }
            p = end;
        }
        q++;
    }
}

#endif
