// dmx_pfind.h -- the speculative parts of cutting one foreign stream for a parallel decode
// (dmx_inflate_parallel_plan_host, include/dmx.h; DESIGN.md 3.1 "One foreign stream"): the test
// whether a bit offset may be the start of a non-final dynamic block, the step from a block
// boundary to the next candidate, and the walk that keeps the chunks the stream really passes
// through.  One text for the host plan (dmx_inflate_par_host.cpp), the model under the
// sanitizers (tests/c/pfind_model.cpp) and the device plan (dmx_inflate_parallel_plan_async,
// dmx_inflate_dev.hip: no arrays that need scratch, no table build), where a lane tests an
// offset.  C++ only, internal.
#ifndef DMX_PFIND_H
#define DMX_PFIND_H

#include <stdint.h>
#include <string.h>

#include "../../include/dmx.h"
#include "dmx_gz_head.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_PF_HD __host__ __device__
#else
#define DMX_PF_HD
#endif

#define DMX_PF_NONE (~0ull)            // a chunk without a candidate
#define DMX_PF_MIN_CHUNK 1024u
#define DMX_PF_MAX_CHUNK (1u << 30)
#ifndef DMX_PF_DEF_CHUNK
#define DMX_PF_DEF_CHUNK 16384u        // profiles/inflate_parallel/README.md: the cut (profiles/inflate_parallel/README.md)
#endif
#define DMX_PF_MAX_SKIP 8u             // false candidates one measure walk passes before it is lost
// The most a chunk may produce.  Beyond it the measure walk is lost and a live one gives the stream
// up to the serial route: one wave decodes a chunk, twice, so a chunk that expands to tens of
// megabytes is a long single-wave kernel, and the cell decoder has been run on chunks up to this
// size only (it was bounded by 32 KiB entries before; its renormalisation at 2^30 would misread a
// reference).  Text at 16..128 KiB a chunk produces well under 1 MiB.
#define DMX_PF_MAX_CHUNK_OUT (4ull << 20)
#define DMX_PF_MAX_POS 0xFFFFFFF0ull   // 32-bit positions: zbytes and the output
#define DMX_PF_PIECE 65536u            // the check's pieces (a range of dmx_crc32_ranges_async)
#define DMX_PF_CELL_WG 2048u           // workgroups of the cell decode: table areas in d_work
#define DMX_PF_MEAS_WG 1024u           // workgroups of the measure pass: table areas in d_plan

#define DMX_PF_LAST 1u
#define DMX_PF_LOST 2u

// what the measure pass leaves per chunk that has a candidate
struct dmx_pf_meas {
    uint64_t end_bit;    // the block boundary it stopped at
    uint64_t out_len;    // bytes its blocks produce
    uint32_t next;       // the chunk whose candidate it landed on (only without LAST, LOST and status)
    uint32_t flags;      // DMX_PF_LAST: BFINAL reached; DMX_PF_LOST: more than DMX_PF_MAX_SKIP false candidates passed,
                         // or more than DMX_PF_MAX_CHUNK_OUT bytes produced
    int32_t status;      // 0 or -E_* of the block that failed
    uint32_t reserved;
};

static inline DMX_PF_HD uint64_t dmx_pf_a256(uint64_t x) { return (x + 255) & ~255ull; }

static inline DMX_PF_HD uint32_t dmx_pf_nchunks(uint64_t zbytes, uint32_t chunk_bytes) {
    const uint64_t n = (zbytes + chunk_bytes - 1) / chunk_bytes;
    return n ? (uint32_t)n : 1u;
}

// d_work of the decode: [control 256][tables 8 KiB x workgroups][cells 2 x out_len][piece index 24 x np,
// reserved: the check computes its pieces' ranges itself][piece CRC-32 remainders 4 x np][piece
// Adler-32 sums 4 x np], every part 256-byte aligned
static inline DMX_PF_HD uint64_t dmx_pf_pieces(uint64_t out_len) {
    const uint64_t np = (out_len + DMX_PF_PIECE - 1) / DMX_PF_PIECE;
    return np ? np : 1;
}
static inline DMX_PF_HD uint64_t dmx_pf_cell_wg(uint32_t nlive) {
    return nlive < DMX_PF_CELL_WG ? (nlive ? nlive : 1u) : DMX_PF_CELL_WG;
}
static inline DMX_PF_HD uint64_t dmx_pf_work(uint64_t out_len, uint32_t nlive) {
    const uint64_t np = dmx_pf_pieces(out_len);
    return 256 + 8192 * dmx_pf_cell_wg(nlive) + dmx_pf_a256(2 * out_len) + dmx_pf_a256(24 * np) + 2 * dmx_pf_a256(4 * np);
}
// d_plan: [head 256][live chunks 32 x nc][candidates 8 x nc][measures 32 x nc][tables 8 KiB x workgroups]
static inline DMX_PF_HD uint64_t dmx_pf_meas_wg(uint32_t nc) { return nc < DMX_PF_MEAS_WG ? nc : DMX_PF_MEAS_WG; }
static inline DMX_PF_HD uint64_t dmx_pf_plan_bytes(uint32_t nc) {
    return 256 + dmx_pf_a256(32ull * nc) + dmx_pf_a256(8ull * nc) + dmx_pf_a256(32ull * nc) + 8192 * dmx_pf_meas_wg(nc);
}

// 64 bits of z[0, n) from byte p on, little-endian; bytes at or past n read as zeros.  Never reads
// outside z[0, n).
static inline DMX_PF_HD uint64_t dmx_pf_load64(const uint8_t* z, uint64_t n, uint64_t p) {
    uint64_t v = 0;
    if (p + 8 <= n) {
        memcpy(&v, z + p, 8);
        return v;
    }
    for (uint32_t k = 0; k < 8 && p + k < n; k++) v |= (uint64_t)z[p + k] << (8 * k);
    return v;
}
// the 57 bits (at least) at bit offset `bit`
static inline DMX_PF_HD uint64_t dmx_pf_peek(const uint8_t* z, uint64_t n, uint64_t bit) {
    return dmx_pf_load64(z, n, bit >> 3) >> (bit & 7);
}

// The cheap filter: BFINAL = 0, BTYPE = 2, HLIT <= 29, HDIST <= 29, the code length code exactly
// complete (Kraft sum of its up to 19 three-bit lengths), and the header so far inside the input.
// *clp receives the 19 lengths, three bits each at 3 x symbol; *hdr the 17 header bits.
// dmx_pf_filter_w is the filter on bits the caller holds -- w the bits from `bit` on (57 at least),
// w2 those from bit + 56 on (18 at least; looked at only where the code length code has more than 13
// lengths): the device search stages its chunk as aligned words and hands every lane its two views.
static inline DMX_PF_HD bool dmx_pf_filter_w(uint64_t w, uint64_t w2, uint64_t n, uint64_t bit, uint64_t* clp, uint32_t* hdr) {
    if ((w & 7) != 4) return false;   // BFINAL 0, BTYPE 10b (the low bit first)
    const uint32_t hlit = (uint32_t)(w >> 3) & 31, hdist = (uint32_t)(w >> 8) & 31, ncode = ((uint32_t)(w >> 13) & 15) + 4;
    if (hlit > 29 || hdist > 29) return false;
    if (bit + 17 + 3 * ncode > 8 * n) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint64_t cl = 0;
    uint32_t kraft = 0;
    for (uint32_t k = 0; k < ncode; k++) {
        const uint32_t v = k < 13 ? (uint32_t)(w >> (17 + 3 * k)) & 7 : (uint32_t)(w2 >> (3 * (k - 13))) & 7;   // lengths 13..18: w2
        cl |= (uint64_t)v << (3 * order[k]);
        if (v) kraft += 128u >> v;
    }
    if (kraft != 128) return false;
    *clp = cl;
    *hdr = (uint32_t)w & 0x1FFFF;
    return true;
}
static inline DMX_PF_HD bool dmx_pf_filter(const uint8_t* z, uint64_t n, uint64_t bit, uint64_t* clp, uint32_t* hdr) {
    const uint64_t w = dmx_pf_peek(z, n, bit);
    if ((w & 7) != 4) return false;
    const uint64_t w2 = ((uint32_t)(w >> 13) & 15) + 4 > 13 ? dmx_pf_peek(z, n, bit + 56) : 0;
    return dmx_pf_filter_w(w, w2, n, bit, clp, hdr);
}

// The full test of a filter survivor, by the rules of the decoder's dynamic-block header (iblock,
// dmx_inflate_dev.hip; dynamic(), dmx_inflate.c): the code lengths decode (no repeat without a
// previous length, none past the end), there is an end-of-block code, the literal/length code is
// complete or a single code of length 1, the distance code is complete, empty or a single code of
// length 1, and all of the header lies inside the input.  Only sums are kept, no table is built.
static inline DMX_PF_HD bool dmx_pf_header(const uint8_t* z, uint64_t n, uint64_t bit, uint64_t cl, uint32_t hdr) {
    const uint32_t nlen = ((hdr >> 3) & 31) + 257, ndist = ((hdr >> 8) & 31) + 1, ncode = ((hdr >> 13) & 15) + 4;
    uint64_t cnt = 0;   // codes per length of the code length code, 8 bits each
    for (uint32_t s = 0; s < 19; s++) cnt += 1ull << (8 * ((cl >> (3 * s)) & 7));
    uint64_t pos = bit + 17 + 3 * ncode;
    const uint32_t tot = nlen + ndist;
    uint32_t idx = 0, prev = 0;
    uint32_t kl = 0, nl = 0, l1 = 0, kd = 0, nd = 0, d1 = 0;
    bool eob = false;
    while (idx < tot) {
        uint32_t v = (uint32_t)dmx_pf_peek(z, n, pos);
        // canonical decode by counts, one bit a step (the code is complete: it ends within 7 bits)
        uint32_t code = 0, first = 0, sym = 19, used = 0;
        for (uint32_t l = 1; l <= 7; l++) {
            code |= v & 1;
            v >>= 1;
            const uint32_t c = (uint32_t)(cnt >> (8 * l)) & 255;
            if (code < first + c) {
                uint32_t k = code - first;   // the k-th symbol of length l
                for (uint32_t s = 0; s < 19; s++) {
                    if (((cl >> (3 * s)) & 7) != l) continue;
                    if (k == 0) { sym = s; break; }
                    k--;
                }
                used = l;
                break;
            }
            first = (first + c) << 1;
            code <<= 1;
        }
        if (sym >= 19) return false;
        pos += used;
        uint32_t rep = 1, val = sym;
        if (sym == 16) {
            if (idx == 0) return false;
            val = prev;
            rep = 3 + (v & 3);
            pos += 2;
        } else if (sym == 17) {
            val = 0;
            rep = 3 + (v & 7);
            pos += 3;
        } else if (sym == 18) {
            val = 0;
            rep = 11 + (v & 127);
            pos += 7;
        }
        prev = val;
        if (idx + rep > tot) return false;
        if (val) {
            const uint32_t a = idx < nlen ? (idx + rep < nlen ? idx + rep : nlen) - idx : 0, b = rep - a;
            kl += a << (15 - val);
            nl += a;
            kd += b << (15 - val);
            nd += b;
            if (val == 1) { l1 += a; d1 += b; }
            if (idx <= 256 && 256 < idx + rep) eob = true;
        }
        idx += rep;
    }
    if (pos > 8 * n || !eob) return false;
    if (kl > 32768u || (kl < 32768u && !(nl == 1 && l1 == 1))) return false;
    if (kd > 32768u || (kd < 32768u && nd != 0 && !(nd == 1 && d1 == 1))) return false;
    return true;
}

// a non-final dynamic block may start at `bit`
static inline DMX_PF_HD bool dmx_pf_valid(const uint8_t* z, uint64_t n, uint64_t bit) {
    uint64_t cl;
    uint32_t hdr;
    return dmx_pf_filter(z, n, bit, &cl, &hdr) && dmx_pf_header(z, n, bit, cl, hdr);
}

// The search range of chunk c >= 1, in bits: its own bytes, behind the framing's start bit.
static inline DMX_PF_HD void dmx_pf_range(uint32_t c, uint32_t chunk_bytes, uint64_t zbytes, uint64_t body_bit, uint64_t* lo,
                                          uint64_t* hi) {
    uint64_t a = 8ull * c * chunk_bytes, b = a + 8ull * chunk_bytes;
    if (b > 8 * zbytes) b = 8 * zbytes;
    if (a <= body_bit) a = body_bit + 1;
    *lo = a;
    *hi = b > a ? b : a;
}

// A measure walk stands at the block boundary pos; *t is the first chunk it has not passed yet.
// Candidates below pos are false: they are passed and counted.  Returns 1 where a candidate is
// exactly pos (then *t is its chunk), 2 where more than DMX_PF_MAX_SKIP were passed, else 0 (go on
// decoding).
static inline DMX_PF_HD int dmx_pf_land(const uint64_t* cand, uint32_t nchunks, uint32_t* t, uint64_t pos, uint32_t* skipped) {
    uint32_t i = *t, k = *skipped;
    int r = 0;
    while (i < nchunks) {
        const uint64_t c = cand[i];
        if (c != DMX_PF_NONE && c >= pos) {
            r = c == pos ? 1 : 0;
            break;
        }
        if (c != DMX_PF_NONE && ++k > DMX_PF_MAX_SKIP) {
            r = 2;
            break;
        }
        i++;
    }
    *t = i;
    *skipped = k;
    return r;
}

// The walk from chunk 0 along `next`: a chunk is live iff the walk reaches it, so every live chunk
// began at a true block boundary (chunk 0 by the framing, the others because a live chunk's decode
// ended exactly there).  Writes the live chunks with the exclusive scan of their lengths (at most
// cap of them; all are counted) and the record: a live chunk's error is the stream's status; a
// lost one, or one that is too long for the cell decoder, sets gave_up with -E_RANGE; at BFINAL the
// trailer gives in_used and the stored check (zlib: Adler-32, a cut one is -E_ZADL32; gzip: CRC-32,
// a cut one is -E_CRC, and *isize).  format, nchunks, ncand are the caller's.
static inline DMX_PF_HD void dmx_pf_link(const uint8_t* z, uint64_t zbytes, const uint64_t* cand, const dmx_pf_meas* meas,
                                         dmx_pchunk* chunks, uint32_t cap, dmx_par_status* st, uint32_t* isize) {
    uint32_t i = 0, nlive = 0;
    uint64_t off = 0;
    int32_t status = 0;
    st->gave_up = 0;
    st->in_used = 0;
    st->check = 0;
    *isize = 0;
    for (;;) {
        const dmx_pf_meas m = meas[i];
        if (nlive < cap) {
            chunks[nlive].bit = cand[i];
            chunks[nlive].end_bit = m.end_bit;
            chunks[nlive].out_off = off;
            chunks[nlive].out_len = m.out_len;
        }
        nlive++;
        off += m.out_len;
        if (m.status) { status = m.status; break; }
        if ((m.flags & DMX_PF_LOST) || m.out_len > DMX_PF_MAX_CHUNK_OUT) {
            st->gave_up = 1;
            status = -(int32_t)E_RANGE;
            break;
        }
        if (off > DMX_PF_MAX_POS) { status = -(int32_t)E_RANGE; break; }
        if (m.flags & DMX_PF_LAST) {
            const uint64_t p = (m.end_bit + 7) >> 3;   // the trailer starts at the next byte
            const uint32_t tl = st->format == DMX_BATCH_ZLIB ? 4u : st->format == DMX_BATCH_GZIP ? 8u : 0u;
            if (p + tl > zbytes) {
                status = st->format == DMX_BATCH_ZLIB ? -(int32_t)E_ZADL32 : -(int32_t)E_CRC;
                break;
            }
            uint32_t c = 0, sz = 0;
            if (st->format == DMX_BATCH_ZLIB) {
                for (uint32_t k = 0; k < 4; k++) c = (c << 8) | z[p + k];
            } else if (st->format == DMX_BATCH_GZIP) {
                for (uint32_t k = 0; k < 4; k++) c |= (uint32_t)z[p + k] << (8 * k);
                for (uint32_t k = 0; k < 4; k++) sz |= (uint32_t)z[p + 4 + k] << (8 * k);
            }
            st->check = c;
            st->in_used = p + tl;
            *isize = sz;
            break;
        }
        i = m.next;
    }
    st->status = status;
    st->nlive = nlive;
    st->ndead = st->ncand - nlive;
    st->out_len = status ? 0 : off;
    if (status) { st->in_used = 0; st->check = 0; }
    st->work_len = status ? 0 : dmx_pf_work(off, nlive);
}

// ---- one file of many gzip members (dmx_inflate_parallel_multi_*, include/dmx.h; DESIGN.md 3.1
// "One foreign file of many members").  The text above serves it unchanged; what follows is the
// second kind of candidate, the step over a member's end, and the link that also scans the members.
#define DMX_PF_NOMEM 0xFFFFFFFFu   // a walk without a member start

// what the link leaves per live chunk besides its dmx_pchunk (16 bytes)
struct dmx_pf_mside {
    uint64_t mstart;   // the output offset at which the member the chunk begins in began
    uint32_t mbase;    // members that begin in front of the chunk: the index of the first that begins in it
    uint32_t mfirst;   // the output offset inside the chunk of its first member start, or DMX_PF_NOMEM
};

// d_plan: the single plan's parts, then [walks' member offsets 8 x nc][sides 16 x nc], then the tables
static inline DMX_PF_HD uint64_t dmx_pf_mplan_bytes(uint32_t nc) {
    return dmx_pf_plan_bytes(nc) + dmx_pf_a256(8ull * nc) + dmx_pf_a256(16ull * nc);
}
// d_work: [control 256][tables][cells 2 x out_len] as dmx_pf_work, then [segment bases 4 x (nm + 1)]
// [segment CRC-32 remainders 4 x (np + nm)]: a member of n bytes has ceil(n / DMX_PF_PIECE) segments
static inline DMX_PF_HD uint64_t dmx_pf_mwork(uint64_t out_len, uint32_t nlive, uint32_t nmembers) {
    return 256 + 8192 * dmx_pf_cell_wg(nlive) + dmx_pf_a256(2 * out_len) + dmx_pf_a256(4 * ((uint64_t)nmembers + 1)) +
           dmx_pf_a256(4 * (dmx_pf_pieces(out_len) + nmembers));
}

// A member may start at byte p: 1F 8B 08, no reserved flag bit (dmx_pf_member_w: on the four bytes
// the caller holds), a whole header, and a first block that is not of type 3.
static inline DMX_PF_HD bool dmx_pf_member_w(uint32_t w) { return (w & 0xE0FFFFFFu) == 0x00088B1Fu; }
static inline DMX_PF_HD bool dmx_pf_member_head(const uint8_t* z, uint64_t n, uint64_t p) {
    uint64_t body = 0;
    if (dmx_gz_head(z + p, n - p, &body) != 0) return false;
    return ((dmx_pf_peek(z, n, 8 * (p + body)) >> 1) & 3) != 3;
}
static inline DMX_PF_HD bool dmx_pf_member(const uint8_t* z, uint64_t n, uint64_t p) {
    return p + 4 <= n && dmx_pf_member_w((uint32_t)dmx_pf_load64(z, n, p)) && dmx_pf_member_head(z, n, p);
}
// the candidate at `bit` is a member start, not a block: 1F reads as BFINAL 1 / BTYPE 3, which the
// block filter refuses, so the two kinds never meet at one position.  Chunk 0's is bit 0, the first header.
static inline DMX_PF_HD bool dmx_pf_at_member(const uint8_t* z, uint64_t bit) { return (bit & 7) == 0 && z[bit >> 3] == 0x1F; }

// A measure walk's final block ended at bit e: the trailer and the rule behind it.  Returns 0 where
// the file ends (trailing data included), 1 where a member follows at byte *q with its data at
// *q + *body, or a status: -E_CRC for a trailer cut short, the next header's error.  *q is the
// byte behind the trailer, *crc and *isize what it stores.
static inline DMX_PF_HD int dmx_pf_member_end(const uint8_t* z, uint64_t zbytes, uint64_t e, uint64_t* q, uint64_t* body,
                                              uint32_t* crc, uint32_t* isize) {
    const uint64_t p = (e + 7) >> 3;
    *q = p;
    *body = 0;
    *crc = *isize = 0;
    if (p + 8 > zbytes) return -(int)E_CRC;
    uint32_t c = 0, sz = 0;
    for (uint32_t k = 0; k < 4; k++) c |= (uint32_t)z[p + k] << (8 * k);
    for (uint32_t k = 0; k < 4; k++) sz |= (uint32_t)z[p + 4 + k] << (8 * k);
    *crc = c;
    *isize = sz;
    *q = p + 8;
    if (p + 10 > zbytes || z[p + 8] != 0x1F || z[p + 9] != 0x8B) return 0;
    const int r = dmx_gz_head(z + p + 8, zbytes - (p + 8), body);
    return r ? r : 1;
}

// dmx_pf_link for a file of members: mloc[i] holds walk i's first (low half) and last (high half)
// member start as output offsets inside the walk, DMX_PF_NOMEM for none; meas[i].reserved the
// members that begin in it.  Writes the sides next to the chunks.  st->st.format is gzip.
static inline DMX_PF_HD void dmx_pf_link_multi(const uint8_t* z, uint64_t zbytes, const uint64_t* cand, const dmx_pf_meas* meas,
                                               const uint64_t* mloc, dmx_pchunk* chunks, dmx_pf_mside* sides, uint32_t cap,
                                               dmx_par_multi_status* ms, uint32_t* isize) {
    (void)zbytes;   // (a walk with DMX_PF_LAST has seen its whole trailer)
    dmx_par_status* st = &ms->st;
    uint32_t i = 0, nlive = 0, nmem = 0;
    uint64_t off = 0, mstart = 0;
    int32_t status = 0;
    st->gave_up = 0;
    st->in_used = 0;
    st->check = 0;
    *isize = 0;
    for (;;) {
        const dmx_pf_meas m = meas[i];
        const uint32_t first = (uint32_t)mloc[i], last = (uint32_t)(mloc[i] >> 32);
        if (nlive < cap) {
            chunks[nlive].bit = cand[i];
            chunks[nlive].end_bit = m.end_bit;
            chunks[nlive].out_off = off;
            chunks[nlive].out_len = m.out_len;
            sides[nlive].mstart = mstart;
            sides[nlive].mbase = nmem;
            sides[nlive].mfirst = first;
        }
        nlive++;
        if (last != DMX_PF_NOMEM) mstart = off + last;
        nmem += m.reserved;
        off += m.out_len;
        if (m.status) { status = m.status; break; }
        if ((m.flags & DMX_PF_LOST) || m.out_len > DMX_PF_MAX_CHUNK_OUT) {
            st->gave_up = 1;
            status = -(int32_t)E_RANGE;
            break;
        }
        if (off > DMX_PF_MAX_POS) { status = -(int32_t)E_RANGE; break; }
        if (m.flags & DMX_PF_LAST) {
            const uint64_t p = (m.end_bit + 7) >> 3;
            uint32_t c = 0, sz = 0;
            for (uint32_t k = 0; k < 4; k++) c |= (uint32_t)z[p + k] << (8 * k);
            for (uint32_t k = 0; k < 4; k++) sz |= (uint32_t)z[p + 4 + k] << (8 * k);
            st->check = c;
            st->in_used = p + 8;
            *isize = sz;
            break;
        }
        i = m.next;
    }
    st->status = status;
    st->nlive = nlive;
    st->ndead = st->ncand - nlive;
    st->out_len = status ? 0 : off;
    if (status) { st->in_used = 0; st->check = 0; }
    st->work_len = status ? 0 : dmx_pf_mwork(off, nlive, nmem);
    ms->nmembers = status ? 0 : nmem;
    ms->bad_member = 0xFFFFFFFFu;
}

#endif
