// dmx_bgzf_step.h -- one step of the BGZF member walk (dmx_bgzf_index_max, dmx_inflate.c), as a
// function of the offset alone, for the device index (dmx_bgzf_index.hip) and its host twin
// (tests/c/bgzf_dindex_model.cpp): both compile this text.  Host and device, C++ only, internal.
#ifndef DMX_BGZF_STEP_H
#define DMX_BGZF_STEP_H

#include <stdint.h>

#include "../../include/dmx.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DMX_HD __host__ __device__
#else
#define DMX_HD
#endif

// a member that parsed: its size, the offset of its DEFLATE data in it, ISIZE and the stored CRC-32
struct dmx_bgzf_member {
    uint32_t bsize;
    uint32_t body;
    uint32_t isize;
    uint32_t crc;
};

// What one iteration of dmx_bgzf_index_max's loop does at offset p < zlen of z[0..zlen): 0 and
// *m, or the status the walk returns there (-E_ZHEAD, -E_LEN, -E_RANGE).  Reads bytes of the
// member at p only, none at or behind zlen.  Every error of gzip_header is -E_ZHEAD in the walk,
// and its checks of ID / CM / reserved FLG bits have passed before it runs, so the skipping of
// FNAME / FCOMMENT / FHCRC is all that is left of it here.
DMX_HD static inline int dmx_bgzf_step(const uint8_t* z, uint64_t zlen, uint64_t p, uint32_t max_isize,
                                       dmx_bgzf_member* m) {
    const uint8_t* h = z + p;
    const uint64_t left = zlen - p;
    if (left < 12) {
        if (h[0] != 0x1F || (left > 1 && h[1] != 0x8B) || (left > 2 && h[2] != 8) || (left > 3 && !(h[3] & 4)))
            return -(int)E_ZHEAD;
        return -(int)E_LEN;
    }
    const uint32_t flg = h[3];
    if (h[0] != 0x1F || h[1] != 0x8B || h[2] != 8 || !(flg & 4) || (flg & 0xE0)) return -(int)E_ZHEAD;
    const uint64_t xlen = (uint64_t)h[10] | ((uint64_t)h[11] << 8);
    if (left < 12 + xlen) return -(int)E_LEN;
    uint64_t bsize = 0;
    for (uint64_t q = 12; q + 4 <= 12 + xlen;) {   // the subfields: SI1 SI2 SLEN(2) data
        const uint64_t slen = (uint64_t)h[q + 2] | ((uint64_t)h[q + 3] << 8);
        if (q + 4 + slen > 12 + xlen) break;
        if (h[q] == 'B' && h[q + 1] == 'C' && slen == 2) {
            bsize = ((uint64_t)h[q + 4] | ((uint64_t)h[q + 5] << 8)) + 1;
            break;
        }
        q += 4 + slen;
    }
    if (!bsize) return -(int)E_ZHEAD;
    if (left < bsize) return -(int)E_LEN;
    // gzip_header(h, bsize): FEXTRA, then FNAME and FCOMMENT (zero-terminated), then FHCRC
    if (bsize < 12 || bsize - 12 < xlen) return -(int)E_ZHEAD;
    uint64_t b = 12 + xlen;
    for (uint32_t f = 8; f <= 16; f <<= 1) {
        if (!(flg & f)) continue;
        while (b < bsize && h[b]) b++;
        if (b >= bsize) return -(int)E_ZHEAD;
        b++;
    }
    if (flg & 2) {
        if (bsize - b < 2) return -(int)E_ZHEAD;
        b += 2;
    }
    if (b + 8 > bsize) return -(int)E_ZHEAD;   // BSIZE leaves no room for the trailer
    const uint8_t* t = h + bsize - 8;
    const uint32_t crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
    const uint32_t isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
    if (isize > max_isize) return -(int)E_RANGE;
    m->bsize = (uint32_t)bsize;
    m->body = (uint32_t)b;
    m->isize = isize;
    m->crc = crc;
    return 0;
}

// The cheap test of a position's first four bytes (little-endian word): 1F 8B 08 and FLG with
// FEXTRA set and the reserved bits clear -- what dmx_bgzf_step asks of them.
DMX_HD static inline bool dmx_bgzf_magic(uint32_t w) { return (w & 0xE4FFFFFFu) == 0x04088B1Fu; }

// ---- the device index, stage by stage: what one thread does, so that the
// kernels of dmx_bgzf_index.hip and the loops of the host twin run the same text ----

// A candidate: a position where dmx_bgzf_step succeeds; err = the status of the walk behind this
// member (dmx_bgzf_step at off + bsize, when that is neither the end nor a candidate), else 0.
struct dmx_bgzf_cand {
    uint32_t off, bsize, body, isize, crc;
    int32_t err;
};
// Pointer doubling: after k rounds j = the 2^k-th successor (n = behind the end), c / s = the
// members with data / their bytes over the 2^k nodes from here.
struct dmx_bgzf_node {
    uint32_t j, c;
    uint64_t s;
};
// A node of the true chain once reached: round = 1 + the round that marked it (0 = not marked;
// node 0 starts with 1), c / s = the members with data / their bytes before it.
struct dmx_bgzf_mark {
    uint32_t round, c;
    uint64_t s;
};
#define DMX_BGZF_GROUP 16u   // bytes per aligned load of the scan

// Stage 2.  The candidates among the 16 positions of aligned group g of a file that starts `head`
// bytes into group 0 (position k is offset 16 g + k - head): w = the group's four words and the
// first word of the group behind it (anything where the file has no bytes: a position whose four
// bytes are not all in the file is skipped before they are looked at).  Returns their number; the
// first `room` of them go to out[] in offset order (err = 0).
DMX_HD static inline uint32_t dmx_bgzf_group(const uint8_t* z, uint64_t zlen, uint32_t max_isize, uint32_t head,
                                             uint64_t g, const uint32_t w[5], dmx_bgzf_cand* out, uint32_t room) {
    uint32_t n = 0, any = 0;
    for (uint32_t k = 0; k < 4; k++) {   // a byte 1F among the 16?  (the zero-byte test on w ^ 1F1F1F1F)
        const uint32_t x = w[k] ^ 0x1F1F1F1Fu;
        any |= (x - 0x01010101u) & ~x & 0x80808080u;
    }
    if (!any) return 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t k = 0; k < DMX_BGZF_GROUP; k++) {
        const uint64_t a = g * DMX_BGZF_GROUP + k;
        if (a < head || a - head + 4 > zlen) continue;
        const uint32_t v = (uint32_t)((((uint64_t)w[k / 4 + 1] << 32) | w[k / 4]) >> (8 * (k & 3)));
        if (!dmx_bgzf_magic(v)) continue;
        dmx_bgzf_member m;
        if (dmx_bgzf_step(z, zlen, a - head, max_isize, &m)) continue;
        if (n < room) {
            dmx_bgzf_cand c = {(uint32_t)(a - head), m.bsize, m.body, m.isize, m.crc, 0};
            out[n] = c;
        }
        n++;
    }
    return n;
}

// Stage 3 for node i of n candidates (sorted by offset) + the end node n: the link, the sums of
// one node, and the first mark.
DMX_HD static inline void dmx_bgzf_link(const uint8_t* z, uint64_t zlen, uint32_t max_isize, dmx_bgzf_cand* cand,
                                        uint32_t n, uint32_t i, dmx_bgzf_node* node, dmx_bgzf_mark* mark) {
    dmx_bgzf_mark mk = {i == 0 && n ? 1u : 0u, 0, 0};
    mark[i] = mk;
    dmx_bgzf_node x = {n, 0, 0};
    if (i < n) {
        const uint64_t q = (uint64_t)cand[i].off + cand[i].bsize;
        int32_t err = 0;
        if (q < zlen) {
            uint32_t lo = i + 1, hi = n;   // the first candidate at or behind q
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (cand[mid].off < q) lo = mid + 1;
                else hi = mid;
            }
            if (lo < n && cand[lo].off == q) x.j = lo;
            else {
                dmx_bgzf_member m;
                err = dmx_bgzf_step(z, zlen, q, max_isize, &m);
                if (!err) err = -(int)E_ZHEAD;   // (not reached: a position that steps is a candidate)
            }
        }
        cand[i].err = err;
        x.c = cand[i].isize ? 1u : 0u;
        x.s = cand[i].isize;
    }
    node[i] = x;
}

// Stage 4, round k = 0, 1, ... for node i <= n: a node marked before this round marks its 2^k-th
// successor, then the node doubles from a[] into b[].
DMX_HD static inline void dmx_bgzf_round(const dmx_bgzf_node* a, dmx_bgzf_node* b, dmx_bgzf_mark* mark, uint32_t n,
                                         uint32_t i, uint32_t k) {
    const dmx_bgzf_node x = a[i];
    const uint32_t r = mark[i].round;
    if (r && r <= k + 1 && x.j != n) {   // (a mark of this round has round k + 2: its c / s may not be there yet)
        dmx_bgzf_mark mk = {k + 2, mark[i].c + x.c, mark[i].s + x.s};
        mark[x.j] = mk;
    }
    const dmx_bgzf_node y = a[x.j];
    dmx_bgzf_node d = {y.j, x.c + y.c, x.s + y.s};
    b[i] = d;
}

// The status record of dmx_bgzf_index_async (include/dmx.h: dmx_bgzf_index_status, same layout).
struct dmx_bgzf_istat {
    int32_t status;
    uint32_t nblk;
    uint64_t out_len;
    uint32_t ncand;
    uint32_t reserved;
};

// Stage 5 for candidate i < n: a marked node writes its entry at its rank; the one whose walk
// ends -- at the end of the file or in an error -- writes the record.
DMX_HD static inline void dmx_bgzf_finish(const dmx_bgzf_cand* cand, const dmx_bgzf_mark* mark, uint32_t n, uint32_t i,
                                          uint64_t zlen, dmx_iblock* idx, uint32_t* crc, uint32_t cap,
                                          dmx_bgzf_istat* st) {
    const dmx_bgzf_mark mk = mark[i];
    if (!mk.round) return;
    const dmx_bgzf_cand c = cand[i];
    if (c.isize && mk.c < cap) {
        dmx_iblock e = {8 * ((uint64_t)c.off + c.body), mk.s, c.isize, 0};
        idx[mk.c] = e;
        if (crc) crc[mk.c] = c.crc;
    }
    if (c.err) {
        dmx_bgzf_istat r = {c.err, 0, 0, n, 0};
        *st = r;
    } else if ((uint64_t)c.off + c.bsize == zlen) {
        const uint32_t nb = mk.c + (c.isize ? 1u : 0u);
        dmx_bgzf_istat r = {nb > cap ? -(int)E_SZ : 0, nb, mk.s + c.isize, n, 0};
        *st = r;
    }
}

#endif
